"""A window net over a video, ms per emitted frame: the video path (VideoSession: Darknet-53 once per frame, routes in a
ring, clips pooled out of the ring) against the clip path of the same net (net(clips) on the materialised clips — every
frame through the backbone k times), in one run, alternating round by round, at 416x416, k = 3, step 1, 16 frames per
backbone call by default.  A round is one steady-state step: F new frames pushed and F clips detected (video), or F clips of
k frames detected (clip).  Timed with device events over --steps rounds after --warmup, in a fresh child process.  With
--stats the same command runs a second time under `rocprofv3 --kernel-trace --stats` (no counters) and the ring_push /
ring_pool rows of its kernel statistics are printed with the bytes each launch moves, computed from the shapes.

    python tools/video_step.py [--size 416] [--frames 16] [--k 3] [--step 1] [--join max] [--steps 100] [--warmup 5] [--stats]
"""
import argparse
import json
import sys

import _measure

sys.path.insert(0, _measure.ROOT)
CHILD_TIMEOUT_S = 900

COPY_TB_S = 6.3  # what a float4 copy reaches on this chip: the streaming bar is 0.7 of it


def measure(args):
    import torch
    import videoyolo_amd as vy

    dev = torch.device("cuda", 0)
    classes = ["c%d" % i for i in range(20)]
    f, k, s = args.frames, args.k, args.size
    win = vy.yolo3_darknet53(classes, pretrained_base=False, k=k, k_join_type=args.join, k_join_pos="early")
    win.initialize(init="synthetic", seed=233)
    win.collect_params().reset_ctx(dev)
    # two handles on the same parameters' values, one per path, so that alternating does not re-bind a workspace per round
    clipnet = vy.yolo3_darknet53(classes, pretrained_base=False, k=k, k_join_type=args.join, k_join_pos="early")
    clipnet.set_parameters({p.name: p.data() for p in win.collect_params().values()})
    clipnet.collect_params().reset_ctx(dev)
    frames = torch.randn((f, 3, s, s), generator=torch.Generator().manual_seed(0)).to(dev)
    idx = torch.from_numpy(vy.window_indices(f, k, args.step)).to(dev)
    clips = frames[idx].contiguous()  # (F, k, 3, s, s), materialised outside the timed region
    session = win.video(frames_per_step=f, step=args.step)

    def video_round():
        return session.push(frames)  # steady state: F frames in, F clips out

    def clip_round():
        return clipnet(clips)

    for _ in range(args.warmup):
        video_round()
        clip_round()
    torch.cuda.synchronize()
    ms = {"video": 0.0, "clip": 0.0}
    rounds = []
    for _ in range(args.steps):
        for name, fn in (("video", video_round), ("clip", clip_round)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            rounds.append((name, e0, e1, out[0].shape[0]))
    torch.cuda.synchronize()
    emitted = {"video": 0, "clip": 0}
    for name, e0, e1, n in rounds:
        ms[name] += e0.elapsed_time(e1)
        emitted[name] += n
    v, c = ms["video"] / emitted["video"], ms["clip"] / emitted["clip"]
    return {"size": s, "frames_per_step": f, "clips_per_step": session.clips_per_step, "ring": session.ring, "k": k,
            "step": args.step, "join": args.join, "steps": args.steps, "warmup": args.warmup,
            "video_ms_per_frame": round(v, 4), "clip_ms_per_frame": round(c, 4), "clip_over_video": round(c / v, 3),
            "flop_prediction": round((k * 49.0 + 16.4) / (49.0 + 16.4), 3),
            "timed_window_s": round((ms["video"] + ms["clip"]) / 1e3, 2), "device": torch.cuda.get_device_name(0)}


def ring_bytes(args):
    """Bytes one ring_push / ring_pool launch moves (fp32, interiors only)."""
    n = sum(c * (-(-args.size // d)) ** 2 for c, d in ((256, 8), (512, 16), (1024, 32)))  # floats per frame, three routes
    clips = min(args.frames, 512 // args.k)
    return 4 * n * args.frames * 2, 4 * n * clips * (args.k + 1)  # push: read + write; pool: k slots read, one write


def kernel_stats(args, video_ms_per_frame):
    found = _measure.kernel_rows(__file__, ["--child", "--size", str(args.size), "--frames", str(args.frames), "--k", str(args.k),
                                            "--step", str(args.step), "--join", args.join, "--steps", "4", "--warmup", "1"],
                                 CHILD_TIMEOUT_S, "video_step_")
    if isinstance(found, dict):
        return found
    rows = {}
    for r in found:
        for name in ("ring_push", "ring_pool"):
            if name in r["name"]:
                rows[name] = _measure.stats_of(r, ("calls", "mean_us", "min_us"))
    push, pool = ring_bytes(args)
    per_round_us = 0.0
    for name, by in (("ring_push", push), ("ring_pool", pool)):
        if name in rows:
            rows[name]["bytes"] = by
            rows[name]["TB_per_s"] = round(by / (rows[name]["mean_us"] * 1e-6) / 1e12, 2)
            rows[name]["of_copy_rate"] = round(rows[name]["TB_per_s"] / COPY_TB_S, 2)
            per_round_us += rows[name]["mean_us"]
    if per_round_us and video_ms_per_frame:
        rows["share_of_video_frame_time"] = round(per_round_us / args.frames / (video_ms_per_frame * 1e3), 5)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--frames", type=int, default=16, help="frames per backbone call = clips per heads call")
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--step", type=int, default=1)
    ap.add_argument("--join", default="max", choices=("max", "mean"))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--stats", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args)))
        return
    argv = [a for a in sys.argv[1:] if a != "--stats"]
    res = _measure.run_child(__file__, ["--child"] + argv, CHILD_TIMEOUT_S)
    print(json.dumps(res))
    if args.stats:
        print(json.dumps(kernel_stats(args, res.get("video_ms_per_frame"))))


if __name__ == "__main__":
    main()
