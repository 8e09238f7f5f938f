"""Windowed heads-only training step (yolo3_no_backbone with k=3) on a bank of stored per-frame routes, next to the plain
heads-only step on pre-pooled routes and the freeze_base=True window-net step on the frames, ms per step at 416x416 and 16
clips by default: recorded forward + backward + Trainer.step, timed with events over K steps after W warm-up steps, the
variants alternating over R rounds inside one fresh child process (the list per variant shows the spread).  The bank comes
twice: B*k frames with the identity table (233 MB at the defaults: fits the 256 MiB Infinity Cache) and 3*B*k frames with
three disjoint random tables used in turn (no frame is read again before 2 x 233 MB of other frames went by).

With --stats the kernels are timed in two further children under `rocprofv3 --kernel-trace --stats` (no counters), one per
bank: route_import_pool (max and mean), route_import of B frames and a float4 streaming copy of the same bytes as
route_import_pool moves, each with its bytes and TB/s.

    python tools/heads_window_step.py [--size 416] [--clips 16] [--k 3] [--steps 20] [--warmup 5] [--rounds 3] [--stats]
"""
import argparse
import json
import sys

import _measure

sys.path.insert(0, _measure.ROOT)

COPY_CALLS = 23  # a count of its own: the copy's row of the kernel statistics is found by it
CHILD_TIMEOUT_S = 900


def route_floats(size):
    """Floats of one frame's three routes."""
    return sum(c * (-(-size // d)) ** 2 for c, d in ((256, 8), (512, 16), (1024, 32)))


def setup(args, with_window):
    import numpy as np
    import torch
    import videoyolo_amd as vy

    dev = torch.device("cuda", 0)
    classes = ["c%d" % i for i in range(20)]
    b, k, s = args.clips, args.k, args.size
    full = vy.yolo3_darknet53(classes, pretrained_base=False)
    full.initialize(init="synthetic", seed=233)
    params = {p.name: p.data() for p in full.collect_params().values()}
    head_params = {n: v for n, v in params.items() if not n.startswith("stages.")}
    nets = {}
    nets["heads"] = vy.yolo3_no_backbone(classes)
    for join in ("max", "mean"):
        nets[join] = vy.yolo3_no_backbone(classes, k=k, k_join_type=join, k_join_pos="early")
    for net in nets.values():
        net.set_parameters(head_params)
        net.collect_params().reset_ctx(dev)
    if with_window:
        nets["window"] = vy.yolo3_darknet53(classes, pretrained_base=False, freeze_base=True, k=k, k_join_type="max",
                                            k_join_pos="early")
        nets["window"].set_parameters(params)
        nets["window"].collect_params().reset_ctx(dev)
    g = torch.Generator().manual_seed(0)
    frames = args.bank_frames or 3 * b * k
    h8 = -(-s // 8)
    bank = [torch.randn((frames, c, -(-h8 // d), -(-h8 // d)), generator=g).to(dev) for c, d in ((256, 1), (512, 2), (1024, 4))]
    perm = np.random.default_rng(0).permutation(frames)
    tables = [perm[i:i + b * k].reshape(b, k) for i in range(0, frames - b * k + 1, b * k)]
    ident = np.arange(b * k).reshape(b, k)
    pooled = [f[:b].contiguous() for f in bank]  # what the plain heads net imports: B frames
    return dev, nets, bank, tables, ident, pooled


def measure(args):
    import torch
    import videoyolo_amd as vy
    from videoyolo_amd import autograd, targets

    dev, nets, bank, tables, ident, pooled = setup(args, True)
    b, k, s = args.clips, args.k, args.size
    gt_boxes, gt_ids = targets.synthetic_gt(b, s, 20, m=8, seed=1)
    gt = torch.as_tensor(gt_boxes).to(dev)
    fixed = targets.YOLOV3PrefetchTargetGenerator(20)(s, s, gt_boxes, gt_ids, device=dev)
    x = torch.randn((b, k, 3, s, s), generator=torch.Generator().manual_seed(1)).to(dev)
    small = [f[:b * k] for f in bank]
    turn = [0]

    def rotating(net):
        turn[0] += 1
        return net.from_bank(*bank, tables[turn[0] % len(tables)], gt, *fixed)

    variants = [
        ("heads_step_ms_on_pooled_routes", nets["heads"], lambda n: n(*pooled, gt, *fixed)),
        ("window_heads_step_ms_max_bank_%d" % (b * k), nets["max"], lambda n: n.from_bank(*small, ident, gt, *fixed)),
        ("window_heads_step_ms_mean_bank_%d" % (b * k), nets["mean"], lambda n: n.from_bank(*small, ident, gt, *fixed)),
        ("window_heads_step_ms_max_bank_%d_random" % bank[0].shape[0], nets["max"], rotating),
        ("window_net_frozen_step_ms", nets["window"], lambda n: n(x, gt, *fixed)),
    ]
    trainers = {id(n): vy.Trainer(n.collect_params(), "sgd", {"learning_rate": 1e-4, "wd": 5e-4, "momentum": 0.9})
                for _, n, _ in variants}

    def timed(net, call, warmup):
        def step():
            with autograd.record():
                l = call(net)
                autograd.backward([l[0] + l[1] + l[2] + l[3]])
            trainers[id(net)].step(b)
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    ms = {name: [] for name, _, _ in variants}
    for r in range(args.rounds):
        for name, net, call in variants:
            ms[name].append(round(timed(net, call, args.warmup if r == 0 else 2), 3))
    mean = {name: sum(v) / len(v) for name, v in ms.items()}
    base = mean["heads_step_ms_on_pooled_routes"]
    out = {"size": s, "clips": b, "k": k, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds}
    out.update(ms)
    for name in ms:
        if name.startswith("window_heads"):
            out[name.replace("_step_ms", "") + "_minus_heads_us"] = round((mean[name] - base) * 1e3, 1)
    out["window_net_over_window_heads_max"] = round(mean["window_net_frozen_step_ms"] /
                                                    mean["window_heads_step_ms_max_bank_%d" % (b * k)], 2)
    out["device"] = torch.cuda.get_device_name(0)
    return out


def launch_kernels(args):
    """The child of the kernel statistics: inference calls, so that few other kernels run between the imports."""
    import torch
    dev, nets, bank, tables, ident, pooled = setup(args, False)
    n = route_floats(args.size) * args.clips * (args.k + 1) // 2  # the copy reads and writes what route_import_pool moves
    src = torch.randn(n, generator=torch.Generator().manual_seed(2)).to(dev)
    dst = torch.empty_like(src)
    for i in range(args.steps):
        for join in ("max", "mean"):
            nets[join].from_bank(*bank, tables[i % len(tables)])
        nets["heads"](*pooled)
    for _ in range(COPY_CALLS):
        torch.mul(src, 1.0, out=dst)
    torch.cuda.synchronize()
    return {"bank_frames": int(bank[0].shape[0]), "tables": len(tables), "calls": args.steps}


def kernel_stats(args, bank_frames):
    found = _measure.kernel_rows(__file__, ["--kernels-child", "--bank-frames", str(bank_frames), "--size", str(args.size),
                                            "--clips", str(args.clips), "--k", str(args.k), "--steps", str(args.steps)],
                                 CHILD_TIMEOUT_S, "heads_window_step_")
    if isinstance(found, dict):
        return found
    per_frame = 4 * route_floats(args.size)
    pool_bytes = per_frame * args.clips * (args.k + 1)  # k frames read, the pooled route written
    want = {"route_import_pool_kernel<0>": ("route_import_pool_max", pool_bytes),
            "route_import_pool_kernel<1>": ("route_import_pool_mean", pool_bytes),
            "route_xfer_kernel<true>": ("route_import_%d_frames" % args.clips, 2 * per_frame * args.clips)}
    want.update({"route_import_pool_kernelILi0E": want["route_import_pool_kernel<0>"],  # (should the names come mangled)
                 "route_import_pool_kernelILi1E": want["route_import_pool_kernel<1>"],
                 "route_xfer_kernelILb1E": want["route_xfer_kernel<true>"]})
    rows = {"bank_frames": bank_frames, "bank_MB": round(per_frame * bank_frames / 1e6, 1)}
    for r in found:
        kname = r["name"]
        hit = [v for key, v in want.items() if key in kname.replace(" ", "")]
        if not hit and r["calls"] == COPY_CALLS and "elementwise" in kname:
            hit = [("float4_copy", pool_bytes)]
            rows["float4_copy_kernel"] = kname[:100]
        for name, by in hit:
            rows[name] = dict(_measure.stats_of(r, ("calls", "mean_us", "min_us")), bytes=by,
                              TB_per_s=round(by / (r["mean_ns"] / 1e3 * 1e-6) / 1e12, 2))
    copy = rows.get("float4_copy", {}).get("TB_per_s")
    if copy:
        for name, v in rows.items():
            if isinstance(v, dict) and name != "float4_copy":
                v["of_copy_rate"] = round(v["TB_per_s"] / copy, 2)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--stats", action="store_true")
    ap.add_argument("--bank-frames", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--kernels-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child or args.kernels_child:
        print(json.dumps(measure(args) if args.child else launch_kernels(args)))
        return
    argv = [a for a in sys.argv[1:] if a != "--stats"]
    print(json.dumps(_measure.run_child(__file__, ["--child"] + argv, CHILD_TIMEOUT_S)))
    if args.stats:
        for frames in (args.clips * args.k, 3 * args.clips * args.k):
            print(json.dumps(kernel_stats(args, frames)))


if __name__ == "__main__":
    main()
