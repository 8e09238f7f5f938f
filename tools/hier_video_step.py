"""A hierarchical net over a whole video (videoyolo_amd.hier_detect_video: every level once per frame position, the joins dilated)
next to the clip path it replaces, at 416x416 on a device-resident synthetic video of 256 frames by default, in a fresh
child process, device events, medians:

  * ms per emitted frame of hier_detect_video for T = 9, 27 and 81 frames per clip at frames_per_step 16 and 64;
  * the clip path, which is the reference: net(frames[window_indices(N, T, 1)[rows]]) in batches of 16 clips, the gather
    included (over --clip-batches batches from the middle of the video: every clip whole), and the same call on clips
    gathered beforehand — the infer column of profiles/hier_step.txt, which it must reproduce; a T whose clip workspace does
    not fit is reported as such;
  * the single-frame net on 16 frames;
  * every dilated join launch of a 16-centre chunk (hpool.i / hjoin.i: events around the launch, vy_net_profile_infer on the
    hier-video plan) in both forms — the chain walk a net launches, and three reads per destination frame (VY_HIER_CHAIN=0
    when the net is created) — beside a streaming copy of the launch's algorithmic bytes (the source plane once plus the destination once)
    timed the same way in the same rounds, alternating; medians over the rounds.  The target is DESIGN's 0.7 of the copy
    rate for a streaming kernel; a launch under it is marked.

With --stats a child runs hier_detect_video at T = 27 in both forms under `rocprofv3 --kernel-trace --stats`: the kernels' own
times over all dilated launches of the run, beside an elementwise copy kernel launched once per chunk with a chunk's bytes.

    python tools/hier_video_step.py [--join max|conv] [--stats] [--size 416] [--video 256] [--frames 9,27,81] [--steps 3]
                                    [--warmup 1] [--rounds 5] [--clip-batches 4] [--out profiles/hier_video_step.txt]
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
POOLS = {3: 1, 9: 2, 27: 3, 81: 4}


def join_bytes(size, centres, t, step, i):
    """algorithmic bytes of dilated join i of a chunk: the source plane's positions once plus the destination's once"""
    c, d = POOL_PLANES[i]
    src = centres + step * (t - 3 ** i)
    dst = centres + step * (t - 3 ** (i + 1))
    return 4 * (src + dst) * c * (-(-size // d)) ** 2


def _nets(args, dev):
    import videoyolo_amd as vy
    classes = ["c%d" % i for i in range(20)]
    base = vy.yolo3_darknet53(classes, pretrained_base=False)
    base.initialize(init="synthetic", seed=233)
    params = {p.name: p.data() for p in base.collect_params().values()}
    del base

    def single():
        net = vy.yolo3_darknet53(classes, pretrained_base=False)
        net.set_parameters(params)
        net.collect_params().reset_ctx(dev)
        return net

    def hier(t, chain=True):
        h = [3] * POOLS[t] + [1] * (5 - POOLS[t])
        old = os.environ.pop("VY_HIER_CHAIN", None)
        os.environ["VY_HIER_CHAIN"] = "1" if chain else "0"  # (read when the net is created)
        try:
            if args.join == "conv":  # the joins at the synthetic start (weights 1/3), the cells as every other net here
                net = vy.YOLOV3HierConv(classes, hierarchical=h)
                net.initialize(init="synthetic", seed=233)
                net.set_parameters(params, allow_missing=True)
            else:
                net = vy.yolo3_darknet53(classes, pretrained_base=False, new_model=True, hierarchical=h, h_join_type="max")
                net.set_parameters(params)
        finally:
            os.environ.pop("VY_HIER_CHAIN", None)
            if old is not None:
                os.environ["VY_HIER_CHAIN"] = old
        net.collect_params().reset_ctx(dev)
        return net

    return single, hier


def _median_ms(torch, np, fn, args):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    return float(np.median([_measure.timed(torch, fn, 1) for _ in range(args.steps)]))


def measure(args):
    import numpy as np
    import torch
    import videoyolo_amd as vy
    from videoyolo_amd import hier_detect_video

    dev = torch.device("cuda", 0)
    s, n = args.size, args.video
    single, hier = _nets(args, dev)
    frames = torch.randn((n, 3, s, s), generator=torch.Generator().manual_seed(0)).to(dev)
    launch = "hjoin." if args.join == "conv" else "hpool."
    out = {"device": torch.cuda.get_device_name(0), "size": s, "video": n, "steps": args.steps, "warmup": args.warmup,
           "rounds": args.rounds, "join": args.join, "clip_batches": args.clip_batches, "hier": {}}
    for t in args.frames:
        row = out["hier"][str(t)] = {}
        net = hier(t)
        for f in (16, 64):
            ms = _median_ms(torch, np, lambda: hier_detect_video(net, frames, frames_per_step=f), args)
            row["video_F%d_ms_per_frame" % f] = round(ms / n, 4)
        # the clip path on whole clips from the middle of the video
        idx = torch.from_numpy(vy.window_indices(n, t, 1)).to(dev)
        lo = max(0, n // 2 - 8 * args.clip_batches)
        rows = [idx[lo + 16 * k: lo + 16 * (k + 1)] for k in range(args.clip_batches)]
        try:
            def clip_path():
                for r in rows:
                    net(frames[r])
            row["clip_gather_ms_per_frame"] = round(_median_ms(torch, np, clip_path, args) / (16 * len(rows)), 4)
            x = frames[rows[0]].contiguous()
            row["clip_call_ms"] = round(_median_ms(torch, np, lambda: net(x), args), 3)
            row["clip_call_ms_per_frame"] = round(row["clip_call_ms"] / 16, 4)
            row["gather_MB_per_call"] = round(x.numel() * 4 / 1e6, 1)
            del x
        except torch.cuda.OutOfMemoryError as e:  # the clip workspace of this T did not fit (any other error ends the tool)
            row["clip_error"] = str(e).splitlines()[0][:200]
        torch.cuda.empty_cache()
        # the dilated launches of a 16-centre chunk in both forms, and copies of their bytes, alternating round by round
        base = hier(t, chain=False)
        chunk = frames[:16 + t - 1].contiguous()
        joins = {"%s%d" % (launch, i): join_bytes(s, 16, t, 1, i) for i in range(POOLS[t])}
        big = max(joins.values()) // 2
        src = torch.empty(big // 4, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        ms = {form: {k: [] for k in joins} for form in ("three_read", "chain_walk")}
        copy_ms = {k: [] for k in joins}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for r in range(args.rounds + 1):
            prof = {}
            for form, m in (("three_read", base), ("chain_walk", net)):
                got = {name: (v, by) for name, v, _, by in m._profile_video_chunk(chunk, 1) if name.startswith(launch)}
                assert {k: by for k, (_, by) in got.items()} == {k: float(v) for k, v in joins.items()}, (got, joins)
                prof[form] = got
            for k, by in joins.items():
                e0.record()
                dst[:by // 8].copy_(src[:by // 8])  # by / 2 bytes read, by / 2 written
                e1.record()
                torch.cuda.synchronize()
                if r:  # (round 0 warms everything up)
                    for form in ms:
                        ms[form][k].append(prof[form][k][0])
                    copy_ms[k].append(e0.elapsed_time(e1))
        row["joins"] = {}
        for k, by in joins.items():
            c = float(np.median(copy_ms[k]))
            row["joins"][k] = {"bytes": by, "copy_ms": round(c, 4), "copy_TB_per_s": round(by / c / 1e9, 3)}
            for form in ms:
                m = float(np.median(ms[form][k]))
                row["joins"][k][form] = {"ms": round(m, 4), "TB_per_s": round(by / m / 1e9, 3), "of_copy_rate": round(c / m, 3)}
        del net, base, src, dst, chunk
        torch.cuda.empty_cache()
    one = single()
    x = frames[:16].contiguous()
    out["single_frame_ms"] = round(_median_ms(torch, np, lambda: one(x), args), 3)
    return out


def stats_child(args):
    """T = 27: hier_detect_video over the video once per form (after a warm-up pass), then one elementwise copy of the bytes
    the dilated launches of a pass move"""
    import torch
    from videoyolo_amd import hier_detect_video
    dev = torch.device("cuda", 0)
    s, n, t = args.size, args.video, 27
    _, hier = _nets(args, dev)
    frames = torch.randn((n, 3, s, s), generator=torch.Generator().manual_seed(0)).to(dev)
    chunk = sum(join_bytes(s, 16, t, 1, i) for i in range(POOLS[t]))
    for chain in (False, True):
        net = hier(t, chain=chain)
        for _ in range(2):
            hier_detect_video(net, frames, frames_per_step=16)
        del net
    src = torch.empty(chunk // 8, dtype=torch.float32, device=dev).normal_()
    dst = torch.empty_like(src)
    for _ in range(2 * (n // 16)):  # one copy of a chunk's bytes per chunk of the two passes
        torch.neg(src, out=dst)
    torch.cuda.synchronize()
    return {"frames": t, "passes": 2, "bytes_per_pass": (n // 16) * chunk}


def kernel_stats(args):
    rows = _measure.kernel_rows(__file__, ["--stats-child", "--size", str(args.size), "--video", str(args.video), "--join", args.join],
                                CHILD_TIMEOUT_S, "hier_video_step_")
    if isinstance(rows, dict):
        return rows
    total = (args.video // 16) * sum(join_bytes(args.size, 16, 27, 1, i) for i in range(3))
    found = {}
    for r in rows:
        if "hier_dilated_chain_kernel" in r["name"]:
            found["chain_walk"] = dict(_measure.stats_of(r), bytes_per_pass=total)
        elif "hier_dilated_kernel" in r["name"]:
            found["three_read"] = dict(_measure.stats_of(r), bytes_per_pass=total)
        elif "elementwise" in r["name"] and "neg" in r["name"].lower():
            found["copy"] = dict(_measure.stats_of(r), bytes_per_pass=total, kernel=r["name"][:80])
    for v in found.values():
        v["TB_per_s"] = round(v["bytes_per_pass"] * 2 / (v["mean_us"] * v["calls"] * 1e-6) / 1e12, 3)
    return found


def table(res, stats):
    conv = res["join"] == "conv"
    n = res["video"]
    lines = ["Hierarchical net%s over a video of %d frames, every level once per frame position (hier_detect_video), next to the clip "
             "path: %s, %d x %d" % (" with the learned 'conv' join (YOLOV3HierConv)" if conv else "", n, res["device"], res["size"],
                                    res["size"]),
             "(device events, medians of %d runs after %d warm-up runs, one process; tools/hier_video_step.py; the clip path over "
             "%d batches of 16 whole clips)" % (res["steps"], res["warmup"], res["clip_batches"]), "",
             "ms per emitted frame",
             "%-6s %14s %14s %18s %18s %14s %12s %12s" % ("T", "video F=16", "video F=64", "clip path+gather", "clip call/16",
                                                         "clip call ms", "gather MB", "clip/video")]
    for t, r in res["hier"].items():
        if "clip_error" in r:
            lines.append("%-6s %14.4f %14.4f   the clip path did not run: %s" % (t, r["video_F16_ms_per_frame"],
                                                                               r["video_F64_ms_per_frame"], r["clip_error"]))
            continue
        lines.append("%-6s %14.4f %14.4f %18.4f %18.4f %14.3f %12.1f %12.2f" % (
            t, r["video_F16_ms_per_frame"], r["video_F64_ms_per_frame"], r["clip_gather_ms_per_frame"],
            r["clip_call_ms_per_frame"], r["clip_call_ms"], r["gather_MB_per_call"],
            r["clip_gather_ms_per_frame"] / r["video_F16_ms_per_frame"]))
    lines += ["%-6s %14.4f   (the single-frame net on 16 frames: %.3f ms)" % ("single", res["single_frame_ms"] / 16,
                                                                            res["single_frame_ms"]),
              "(clip/video: the clip path with its gather over hier_detect_video at frames_per_step 16.  clip call ms is the infer "
              "column of profiles/hier_step.txt.)", "",
              "Dilated %s launches of a 16-centre chunk, both forms (events around the launch; a copy of the launch's algorithmic "
              "bytes — source plane once, destination once — alternating in the same rounds; medians of %d rounds; DESIGN's target "
              "for a streaming kernel: 0.7 of the copy rate)" % ("join" if conv else "pool", res["rounds"]),
              "%-6s %-8s %10s %10s %8s | %10s %8s %8s | %10s %8s %8s" % ("T", "launch", "MB", "copy ms", "TB/s", "3-read ms", "TB/s",
                                                                        "of copy", "chain ms", "TB/s", "of copy")]
    for t, r in res["hier"].items():
        for k, p in r["joins"].items():
            a, b = p["three_read"], p["chain_walk"]
            lines.append("%-6s %-8s %10.1f %10.4f %8.3f | %10.4f %8.3f %8.3f | %10.4f %8.3f %8.3f%s" % (
                t, k, p["bytes"] / 1e6, p["copy_ms"], p["copy_TB_per_s"], a["ms"], a["TB_per_s"], a["of_copy_rate"], b["ms"],
                b["TB_per_s"], b["of_copy_rate"], "   UNDER 0.7 (3-read)" * (a["of_copy_rate"] < 0.7) +
                "   UNDER 0.7 (chain)" * (b["of_copy_rate"] < 0.7)))
    if stats is not None:
        lines += ["", "rocprofv3 --kernel-trace --stats, T = 27, two hier_detect_video passes per form at frames_per_step 16; the copy is "
                  "one elementwise kernel per chunk with the chunk's algorithmic bytes: %s" % json.dumps(stats)]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--video", type=int, default=256)
    ap.add_argument("--frames", default="9,27,81")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--clip-batches", type=int, default=4)
    ap.add_argument("--stats", action="store_true")
    ap.add_argument("--join", choices=("max", "conv"), default="max")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hier_video_step.txt"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--stats-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.frames = [int(v) for v in str(args.frames).split(",")]
    if any(t not in POOLS for t in args.frames):
        sys.exit("--frames: 3, 9, 27 or 81 frames per clip")
    if args.video < 16 * args.clip_batches + 82:
        sys.exit("--video: at least 16 * clip-batches + 82 frames, so that the timed clips are whole")
    if args.child:
        print(json.dumps(measure(args)))
        return
    if args.stats_child:
        print(json.dumps(stats_child(args)))
        return
    argv = ["--size", str(args.size), "--video", str(args.video), "--frames", ",".join(str(t) for t in args.frames), "--steps",
            str(args.steps), "--warmup", str(args.warmup), "--rounds", str(args.rounds), "--clip-batches", str(args.clip_batches),
            "--join", args.join]
    res = _measure.run_child(__file__, ["--child"] + argv, CHILD_TIMEOUT_S)
    text = table(res, kernel_stats(args) if args.stats else None)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
