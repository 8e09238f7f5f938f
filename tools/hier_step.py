"""The hierarchical net (yolo3_darknet53 with new_model / hierarchical / h_join_type='max') next to the nets it competes
with, at 416x416 and 16 clips by default, in a fresh child process:

  * ms per training step (recorded forward + backward + Trainer.step) and per inference call for T = 3, 9 and 27 frames per
    clip (a T whose workspace does not fit is reported as such), device events over K steps after W warm-up steps;
  * the window net at k = 3 and the single-frame net on 16 frames, measured the same way in the same process;
  * every forward pool launch (hpool.i: device events around the launch, vy_net_profile_infer) with the bytes it moves
    (three frames read, one written, interiors) and its rate, beside a streaming copy of the same bytes timed the same way in
    the same rounds, alternating (same clocks); medians over the rounds.

With --stats the child for T = 9 runs once more under `rocprofv3 --kernel-trace --stats`: the kernels' own times of
hier_pool_kernel and hier_pool_bwd_kernel over all pool launches of the run, beside an elementwise copy kernel launched once
for every pool launch with that launch's bytes.  The table goes to --out.

With --join conv the hierarchical net is YOLOV3HierConv, the learned join (hier.hip's hier_join_* kernels), and every T is
measured next to the max net at the same T in the same process; the forward launches are hjoin.i (the same bytes as a pool:
three frames read, one written), and --stats times the two training kernels: hier_join_raw_kernel (three frames read, z
written: 16 bytes per pooled element, plus its statistics rows) and hier_join_bwd_kernel (dz and three frames read, three
gradients written: 28 bytes per pooled element, plus its weight-gradient rows).  The BatchNorm passes around them (finalize,
apply, backward reduce / apply: z read twice more and written once, the gradient read twice) are the kernels every cell
uses and are not listed.  There is no pass / fail bar: the rates are reported against the 0.7-of-copy target.  The table
goes to profiles/hier_conv_step.txt unless --out says otherwise; the default, --join max, is unchanged.

    python tools/hier_step.py [--join max|conv] [--stats] [--size 416] [--clips 16] [--frames 3,9,27] [--steps 5] [--warmup 2]
                              [--out PATH]
"""
import argparse
import json
import os
import sys

import _measure
from _measure import ROOT

sys.path.insert(0, ROOT)
CHILD_TIMEOUT_S = 900
POOL_PLANES = ((32, 1), (64, 2), (128, 4), (256, 8))  # (channels, stride) of the plane each pool point pools


def pool_floats(size, clips, frames, i):
    """floats of pooled plane i (interior) of a net with `frames` = 3^n frames per clip"""
    c, d = POOL_PLANES[i]
    return clips * (frames // 3 ** (i + 1)) * c * (-(-size // d)) ** 2


def measure(args):
    import numpy as np
    import torch
    import videoyolo_amd as vy
    from videoyolo_amd import autograd, targets

    dev = torch.device("cuda", 0)
    classes = ["c%d" % i for i in range(20)]
    b, s = args.clips, args.size
    base = vy.yolo3_darknet53(classes, pretrained_base=False)
    base.initialize(init="synthetic", seed=233)
    params = {p.name: p.data() for p in base.collect_params().values()}
    del base

    def tg(n):
        gt_boxes, gt_ids = targets.synthetic_gt(n, s, len(classes), m=8, seed=1)
        return torch.as_tensor(gt_boxes).to(dev), targets.YOLOV3PrefetchTargetGenerator(len(classes))(s, s, gt_boxes, gt_ids,
                                                                                                       device=dev)

    def step_and_infer(net, x, n):
        gt, fixed = tg(n)
        tr = vy.Trainer(net.collect_params(), "sgd", {"learning_rate": 1e-4, "wd": 5e-4, "momentum": 0.9})

        def step():
            with autograd.record():
                l = net(x, gt, *fixed)
                autograd.backward([l[0] + l[1] + l[2] + l[3]])
            tr.step(n)
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        step_ms = _measure.timed(torch, step, args.steps)
        for _ in range(args.warmup):
            net(x)
        torch.cuda.synchronize()
        return round(step_ms, 3), round(_measure.timed(torch, lambda: net(x), args.steps), 3)

    def make(**kw):
        net = vy.yolo3_darknet53(classes, pretrained_base=False, **kw)
        net.set_parameters(params)
        net.collect_params().reset_ctx(dev)
        return net

    def make_conv(hierarchical):  # the joins at the synthetic start (weights 1/3), the cells as every other net here
        net = vy.YOLOV3HierConv(classes, hierarchical=hierarchical)
        net.initialize(init="synthetic", seed=233)
        net.set_parameters(params, allow_missing=True)
        net.collect_params().reset_ctx(dev)
        return net

    conv = args.join == "conv"
    launch = "hjoin." if conv else "hpool."

    gen = torch.Generator().manual_seed(0)
    out = {"device": torch.cuda.get_device_name(0), "size": s, "clips": b, "steps": args.steps, "warmup": args.warmup,
           "rounds": args.rounds, "join": args.join, "hier": {}}
    for t in args.frames:
        n = {3: 1, 9: 2, 27: 3, 81: 4}[t]
        row = out["hier"][str(t)] = {"hierarchical": [3] * n + [1] * (5 - n)}
        try:
            x = torch.randn((b, t, 3, s, s), generator=gen).to(dev)
            net = make(new_model=True, hierarchical=row["hierarchical"], h_join_type="max")
            if conv:  # the max net first, then the conv-join net on the same clips
                row["max_step_ms"], row["max_infer_ms"] = step_and_infer(net, x, b)
                del net
                torch.cuda.empty_cache()
                net = make_conv(row["hierarchical"])
            row["step_ms"], row["infer_ms"] = step_and_infer(net, x, b)
            row["step_ms_per_frame"] = round(row["step_ms"] / (b * t), 4)
            row["infer_ms_per_frame"] = round(row["infer_ms"] / (b * t), 4)
            # the forward pool launches and copies of their bytes, alternating round by round
            pools = {"%s%d" % (launch, i): 16 * pool_floats(s, b, t, i) for i in range(n)}
            big = max(pools.values()) // 2
            src = torch.empty(big // 4, dtype=torch.float32, device=dev).normal_()
            dst = torch.empty_like(src)
            ms = {k: [] for k in pools}
            copy_ms = {k: [] for k in pools}
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for r in range(args.rounds + 1):
                prof = {name: v for name, v, _, _ in net.profile(x) if name.startswith(launch)}
                for k, by in pools.items():
                    e0.record()
                    dst[:by // 8].copy_(src[:by // 8])  # by / 2 bytes read, by / 2 written
                    e1.record()
                    torch.cuda.synchronize()
                    if r:  # (round 0 warms both up)
                        ms[k].append(prof[k])
                        copy_ms[k].append(e0.elapsed_time(e1))
            row["pools"] = {}
            for k, by in pools.items():
                m, c = float(np.median(ms[k])), float(np.median(copy_ms[k]))
                row["pools"][k] = {"bytes": by, "ms": round(m, 4), "TB_per_s": round(by / m / 1e9, 3), "copy_ms": round(c, 4),
                                   "copy_TB_per_s": round(by / c / 1e9, 3), "of_copy_rate": round(c / m, 3)}
            del net, x, src, dst
        except torch.cuda.OutOfMemoryError as e:  # the workspace of this T did not fit (any other error ends the tool)
            row["error"] = str(e).splitlines()[0][:200]
        torch.cuda.empty_cache()
    win = make(k=3, k_join_type="max", k_join_pos="early")
    x = torch.randn((b, 3, 3, s, s), generator=gen).to(dev)
    out["window_k3"] = dict(zip(("step_ms", "infer_ms"), step_and_infer(win, x, b)))
    del win
    single = make()
    out["single_frame"] = dict(zip(("step_ms", "infer_ms"), step_and_infer(single, x[:, 0].contiguous(), b)))
    return out


def stats_child(args):
    """T = 9: two training steps, and for every pool launch of them a torch elementwise copy kernel of that launch's bytes"""
    import torch
    import videoyolo_amd as vy
    from videoyolo_amd import autograd, targets

    dev = torch.device("cuda", 0)
    classes = ["c%d" % i for i in range(20)]
    b, s, t = args.clips, args.size, 9
    conv = args.join == "conv"
    if conv:
        net = vy.YOLOV3HierConv(classes, hierarchical=[3, 3, 1, 1, 1])
    else:
        net = vy.yolo3_darknet53(classes, pretrained_base=False, new_model=True, hierarchical=[3, 3, 1, 1, 1], h_join_type="max")
    net.initialize(init="synthetic", seed=233)
    net.collect_params().reset_ctx(dev)
    x = torch.randn((b, t, 3, s, s), generator=torch.Generator().manual_seed(0)).to(dev)
    gt_boxes, gt_ids = targets.synthetic_gt(b, s, len(classes), m=8, seed=1)
    gt = torch.as_tensor(gt_boxes).to(dev)
    fixed = targets.YOLOV3PrefetchTargetGenerator(len(classes))(s, s, gt_boxes, gt_ids, device=dev)
    fl = [pool_floats(s, b, t, i) for i in range(2)]
    src = torch.empty(16 * max(fl) // 4, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    for _ in range(2):
        with autograd.record():
            l = net(x, gt, *fixed)
            autograd.backward([l[0] + l[1] + l[2] + l[3]])
        for f in fl:
            # forward: 3 read + 1 written; backward: 5 read + 3 written (max), dz + 3 read + 3 written (conv)
            for units in (4, 7 if conv else 8):
                torch.neg(src[:units * f // 2], out=dst[:units * f // 2])
    torch.cuda.synchronize()
    return {"frames": t, "steps": 2, "pool_floats": fl}


def kernel_stats(args):
    rows = _measure.kernel_rows(__file__, ["--stats-child", "--size", str(args.size), "--clips", str(args.clips), "--join", args.join],
                                CHILD_TIMEOUT_S, "hier_step_")
    if isinstance(rows, dict):
        return rows
    fl = [pool_floats(args.size, args.clips, 9, i) for i in range(2)]
    found = {}
    conv = args.join == "conv"
    for r in rows:
        if "hier_join_bwd_kernel" in r["name"]:
            found["hier_join_bwd"] = dict(_measure.stats_of(r), bytes_per_step=28 * sum(fl))
        elif "hier_join_raw_kernel" in r["name"]:
            found["hier_join_raw"] = dict(_measure.stats_of(r), bytes_per_step=16 * sum(fl))
        elif "hier_pool_bwd_kernel" in r["name"]:
            found["hier_pool_bwd"] = dict(_measure.stats_of(r), bytes_per_step=32 * sum(fl))
        elif "hier_pool_kernel" in r["name"]:
            found["hier_pool"] = dict(_measure.stats_of(r), bytes_per_step=16 * sum(fl))
        elif "elementwise" in r["name"] and "neg" in r["name"].lower():  # torch.neg(src, out=dst): 8 launches in the run
            # (torch splits a launch whose byte offsets pass 2^31 in two: more than 8 calls, the same bytes)
            found["copy"] = dict(_measure.stats_of(r), bytes_per_step=(44 if conv else 48) * sum(fl), kernel=r["name"][:80])
    if "copy" not in found:
        found["elementwise_rows"] = [(r["name"][:80], r["calls"]) for r in rows if "elementwise" in r["name"]]
        return found
    for v in found.values():
        v["TB_per_s"] = round(v["bytes_per_step"] * 2 / (v["mean_us"] * v["calls"] * 1e-6) / 1e12, 3)
    return found


def table(res, stats):
    conv = res.get("join") == "conv"
    lines = ["Hierarchical net%s next to the window net and the single-frame net: %s, %d clips of %d x %d" % (
        " with the learned 'conv' join (YOLOV3HierConv), and the max net at the same T," if conv else "",
        res["device"], res["clips"], res["size"], res["size"]),
        "(device events, %d steps after %d warm-up steps, one process; tools/hier_step.py)" % (res["steps"], res["warmup"]), "",
        "%-34s %8s %12s %14s %12s %14s" % ("net", "frames", "step ms", "step ms/frame", "infer ms", "infer ms/frame")]
    b = res["clips"]
    for t, r in res["hier"].items():
        name = "hier %s" % r["hierarchical"]
        if "error" in r:
            lines.append("%-34s %8d   did not run: %s" % (name, b * int(t), r["error"]))
            continue
        if conv:
            name = "hier conv %s" % r["hierarchical"]
            lines.append("%-34s %8d %12.3f %14.4f %12.3f %14.4f" % ("hier max %s" % r["hierarchical"], b * int(t), r["max_step_ms"],
                                                                     r["max_step_ms"] / (b * int(t)), r["max_infer_ms"],
                                                                     r["max_infer_ms"] / (b * int(t))))
        lines.append("%-34s %8d %12.3f %14.4f %12.3f %14.4f" % (name, b * int(t), r["step_ms"], r["step_ms_per_frame"],
                                                                 r["infer_ms"], r["infer_ms_per_frame"]))
    for name, key, frames in (("window k=3 (max, early)", "window_k3", 3 * b), ("single frame", "single_frame", b)):
        r = res[key]
        lines.append("%-34s %8d %12.3f %14.4f %12.3f %14.4f" % (name, frames, r["step_ms"], r["step_ms"] / frames, r["infer_ms"],
                                                                 r["infer_ms"] / frames))
    lines += ["", "Forward %s launches (events around the launch; a copy of the same bytes alternating in the same rounds; "
              "medians of %d rounds; DESIGN's target for a streaming kernel: 0.7 of the copy rate)" % (
                  "join" if conv else "pool", res["rounds"]),
              "%-10s %-8s %12s %10s %8s %10s %8s %10s" % ("T", "launch", "MB", "ms", "TB/s", "copy ms", "TB/s", "of copy")]
    for t, r in res["hier"].items():
        for k, p in r.get("pools", {}).items():
            lines.append("%-10s %-8s %12.1f %10.4f %8.3f %10.4f %8.3f %10.3f%s" % (
                t, k, p["bytes"] / 1e6, p["ms"], p["TB_per_s"], p["copy_ms"], p["copy_TB_per_s"], p["of_copy_rate"],
                "   UNDER 0.7" if p["of_copy_rate"] < 0.7 else ""))
    if stats is not None:
        lines += ["", "rocprofv3 --kernel-trace --stats, T = 9, two training steps; the copy is one elementwise kernel per pool "
                  "launch with that launch's bytes: %s" % json.dumps(stats)]
        if conv:
            lines += ["(bytes_per_step: hier_join_raw 16 per pooled element — three frames read, z written; hier_join_bwd 28 — dz and "
                      "three frames read, three gradients written; their per-block partial rows and the BatchNorm passes around "
                      "them are not counted.  No bar: the target is 0.7 of the copy's TB_per_s.)"]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--frames", default="3,9,27")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--stats", action="store_true")
    ap.add_argument("--join", choices=("max", "conv"), default="max")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--stats-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.frames = [int(v) for v in str(args.frames).split(",")]
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "hier_conv_step.txt" if args.join == "conv" else "hier_step.txt")
    if any(t not in (3, 9, 27, 81) for t in args.frames):
        sys.exit("--frames: 3, 9, 27 or 81 frames per clip")
    if args.child:
        print(json.dumps(measure(args)))
        return
    if args.stats_child:
        print(json.dumps(stats_child(args)))
        return
    argv = ["--size", str(args.size), "--clips", str(args.clips), "--frames", ",".join(str(t) for t in args.frames), "--steps",
            str(args.steps), "--warmup", str(args.warmup), "--rounds", str(args.rounds), "--join", args.join]
    res = _measure.run_child(__file__, ["--child"] + argv, CHILD_TIMEOUT_S)
    text = table(res, kernel_stats(args) if args.stats else None)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
