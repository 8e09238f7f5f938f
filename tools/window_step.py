"""Window-net training step (yolo3_darknet53 with k=3, early join) vs the single-frame full step on the same B*k frames and
the heads step on B clips, ms per step at 416x416 and 16 clips by default: recorded forward + backward + Trainer.step,
timed with events over K steps after W warm-up steps, in a fresh child process.  With --stats, the same command runs a
second time under `rocprofv3 --kernel-trace --stats` and the window_pool / window_pool_bwd rows of its kernel statistics
are printed with the bytes each launch moves.

    python tools/window_step.py [--size 416] [--clips 16] [--k 3] [--join max] [--steps 20] [--warmup 5] [--stats]
"""
import argparse
import json
import sys

import _measure

sys.path.insert(0, _measure.ROOT)
CHILD_TIMEOUT_S = 900


def measure(args):
    import torch
    import videoyolo_amd as vy
    from videoyolo_amd import autograd, targets

    dev = torch.device("cuda", 0)
    classes = ["c%d" % i for i in range(20)]
    b, k, s = args.clips, args.k, args.size
    full = vy.yolo3_darknet53(classes, pretrained_base=False)
    full.initialize(init="synthetic", seed=233)
    params = {p.name: p.data() for p in full.collect_params().values()}
    full.collect_params().reset_ctx(dev)
    win = vy.yolo3_darknet53(classes, pretrained_base=False, k=k, k_join_type=args.join, k_join_pos="early")
    win.set_parameters(params)
    win.collect_params().reset_ctx(dev)
    heads = vy.yolo3_no_backbone(classes)
    heads.set_parameters({n: v for n, v in params.items() if not n.startswith("stages.")})
    heads.collect_params().reset_ctx(dev)
    x = torch.randn((b, k, 3, s, s), generator=torch.Generator().manual_seed(0)).to(dev)
    xf = x.view(b * k, 3, s, s)

    def tg(n):
        gt_boxes, gt_ids = targets.synthetic_gt(n, s, len(classes), m=8, seed=1)
        return torch.as_tensor(gt_boxes).to(dev), targets.YOLOV3PrefetchTargetGenerator(len(classes))(s, s, gt_boxes, gt_ids,
                                                                                                       device=dev)

    def timed(net, inputs, n):
        gt, fixed = tg(n)
        tr = vy.Trainer(net.collect_params(), "sgd", {"learning_rate": 1e-4, "wd": 5e-4, "momentum": 0.9})

        def step():
            with autograd.record():
                l = net(*inputs, gt, *fixed)
                autograd.backward([l[0] + l[1] + l[2] + l[3]])
            tr.step(n)
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    win_ms = timed(win, (x,), b)
    full_ms = timed(full, (xf,), b * k)
    heads_ms = timed(heads, full.extract_features(xf[:b]), b)
    return {"size": s, "clips": b, "k": k, "join": args.join, "steps": args.steps, "warmup": args.warmup,
            "window_step_ms": round(win_ms, 3), "full_step_ms_at_clips_x_k": round(full_ms, 3),
            "heads_step_ms_at_clips": round(heads_ms, 3),
            "window_over_full_plus_heads": round(win_ms / (full_ms + heads_ms), 3),
            "device": torch.cuda.get_device_name(0)}


def pool_bytes(args):
    """Bytes one window_pool / window_pool_bwd launch moves (fp32, interiors only)."""
    n = sum(c * (-(-args.size // d)) ** 2 for c, d in ((256, 8), (512, 16), (1024, 32)))  # floats per frame, three routes
    b, k = args.clips, args.k
    fwd = 4 * n * b * (k + 1)  # k frames read, the pooled route written
    bwd = 4 * n * b * ((2 * k + 2) if args.join == "max" else (k + 1))  # max: pooled g and x + k frames read, k written
    return fwd, bwd


def kernel_stats(args):
    found = _measure.kernel_rows(__file__, ["--child", "--size", str(args.size), "--clips", str(args.clips), "--k", str(args.k),
                                            "--join", args.join, "--steps", "2", "--warmup", "1"], CHILD_TIMEOUT_S, "window_step_")
    if isinstance(found, dict):
        return found
    rows = {}
    for r in found:
        if "window_pool" in r["name"]:
            rows["window_pool_bwd" if "bwd" in r["name"] else "window_pool"] = _measure.stats_of(r, ("calls", "mean_us", "min_us"))
    fwd, bwd = pool_bytes(args)
    for name, by in (("window_pool", fwd), ("window_pool_bwd", bwd)):
        if name in rows:
            rows[name]["bytes"] = by
            rows[name]["TB_per_s"] = round(by / (rows[name]["mean_us"] * 1e-6) / 1e12, 2)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--join", default="max", choices=("max", "mean"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--stats", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args)))
        return
    argv = [a for a in sys.argv[1:] if a != "--stats"]
    print(json.dumps(_measure.run_child(__file__, ["--child"] + argv, CHILD_TIMEOUT_S)))
    if args.stats:
        print(json.dumps(kernel_stats(args)))


if __name__ == "__main__":
    main()
