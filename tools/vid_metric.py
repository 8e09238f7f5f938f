"""Cost of the ImageNet-VID metric (videoyolo_amd/metrics.py VIDDetectionMetric, csrc/vid_metric.hip) next to the detecting it
scores.  Two sections, written to --out (default profiles/vid_metric.txt); each run replaces its own section and keeps the
other, since the two run on different machines:

  device (default)    in a fresh child process on the GPU: the device time of update() for 64 frames x 100 rows by events,
                      ALTERNATING with the batch-64 detect step at 416 x 416 and 608 x 608 of a single-frame net in the same
                      process (same clocks); then a VID-val-sized synthetic set (176 126 frames, 30 classes, 20 rows per
                      frame): every update() in batches of 64, and get().  With --stats a second child runs 20 updates
                      under `rocprofv3 --kernel-trace --stats` and the kernel's own mean time is added.
  --reference DIR     on a CPU, with the reference checkout at DIR: frames/s of the reference's own vid_eval_motion on a
                      2 000-frame synthetic set of the same make (20 rows, at most 4 ground truths per frame), run under the
                      stand-ins of tests/golden/make_vid_metric_golden.py, next to this metric's host path on the same set.

    python tools/vid_metric.py [--stats] [--frames 176126] [--out PATH]
    python tools/vid_metric.py --reference /path/to/VideoYOLO [--ref-frames 2000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

import _measure
from _measure import ROOT

sys.path.insert(0, ROOT)
CHILD_TIMEOUT_S = 900
SECTIONS = ["## reference on the CPU", "## device"]


class SyntheticVID(object):
    """n_frames frames, 0..max_gt integer ground-truth boxes each (a tenth of the frames have none), a motion IoU per
    ground truth; held as padded arrays, so building it is whole-array numpy."""

    def __init__(self, n_frames, n_cls=30, max_gt=4, seed=0):
        rng = np.random.default_rng(seed)
        self.n_frames, self.max_gt = n_frames, max_gt
        self.classes = self.wn_classes = ["n%02d" % c for c in range(n_cls)]
        self.count = rng.integers(1, max_gt + 1, n_frames) * (rng.random(n_frames) >= 0.1)
        xy = rng.integers(0, 400, (n_frames, max_gt, 2))
        wh = rng.integers(8, 260, (n_frames, max_gt, 2))
        self.gt = np.concatenate([xy, xy + wh - 1, rng.integers(0, n_cls, (n_frames, max_gt, 1))], 2).astype(np.float64)
        self.motion = np.round(rng.random((n_frames, max_gt)), 3)
        self.motion_ious = _MotionView(self)

    def get_sample_ids(self):
        return list(range(self.n_frames))

    def get_label(self, i):
        return self.gt[i, :self.count[i]]

    def detections(self, rows, seed=1, lo=0, hi=None):
        """(n, rows, 4), (n, rows, 1), (n, rows, 1) float32 for frames lo..hi: jittered copies of the frame's ground truths
        and clutter, a tenth of the rows below the score threshold, a tenth padding."""
        hi = self.n_frames if hi is None else hi
        rng = np.random.default_rng([seed, lo])
        n = hi - lo
        src = rng.integers(0, self.max_gt, (n, rows)) % np.maximum(self.count[lo:hi], 1)[:, None]
        picked = np.take_along_axis(self.gt[lo:hi], src[:, :, None], 1)
        boxes = picked[:, :, :4] + rng.normal(0, 5.0, (n, rows, 4))
        cls = picked[:, :, 4].copy()
        clutter = (rng.random((n, rows)) < 0.3) | (self.count[lo:hi] == 0)[:, None]
        rb = rng.uniform(0, 400, (n, rows, 2))
        boxes[clutter] = np.concatenate([rb, rb + rng.uniform(8, 260, (n, rows, 2))], 2)[clutter]
        cls[clutter] = rng.integers(0, len(self.classes), int(clutter.sum()))
        score = rng.random((n, rows))
        score[rng.random((n, rows)) < 0.1] *= 0.05
        pad = rng.random((n, rows)) < 0.1
        boxes[pad], cls[pad], score[pad] = -1, -1, -1
        return boxes.astype(np.float32), cls.astype(np.float32)[:, :, None], score.astype(np.float32)[:, :, None]


class _MotionView(object):
    def __init__(self, ds):
        self._ds = ds

    def __getitem__(self, key):
        i = int(key)
        return self._ds.motion[i, :self._ds.count[i]].tolist()


# ------------------------------------------------------------------------------------------------------- the device section
def measure(args):
    import torch
    import videoyolo_amd as vy
    dev = torch.device("cuda", 0)
    med = lambda v: float(np.median(v))  # noqa: E731
    out = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds}

    # ---- update() for 64 frames x 100 rows, alternating with the detect step
    batch, rows = 64, 100
    ds = SyntheticVID(batch * args.updates)
    metric = vy.VIDDetectionMetric(ds)
    dets = [tuple(torch.from_numpy(a).to(dev) for a in ds.detections(rows, lo=u * batch, hi=(u + 1) * batch))
            for u in range(args.updates)]
    state = {"u": 0}

    def update():
        u = state["u"] % args.updates
        if u == 0:
            metric.reset()
        metric.update(dets[u][0], dets[u][1], dets[u][2], sid=range(u * batch, (u + 1) * batch))
        state["u"] += 1

    for _ in range(args.updates):
        update()
    torch.cuda.synchronize()
    print("updates warmed up", file=sys.stderr, flush=True)
    if args.updates_only:
        return out
    net = _measure.detect_net(vy, ds.classes, dev)
    upd_ms, det_ms, host_ms = _measure.update_and_detect(torch, update, net, dev, batch, (416, 608), args)
    out["update"] = {"batch": batch, "rows": rows, "ms": round(med(upd_ms), 4), "ms_rounds": [round(v, 4) for v in upd_ms],
                     "host_ms_per_call": round(host_ms, 3),
                     "detect_ms": {str(s): round(med(v), 3) for s, v in det_ms.items()},
                     "detect_ms_rounds": {str(s): [round(t, 3) for t in v] for s, v in det_ms.items()}}
    del net, dets, metric
    print("update and detect steps timed: %s" % json.dumps(out["update"]), file=sys.stderr, flush=True)

    # ---- a VID-val-sized set
    rows = 20
    t0 = time.perf_counter()
    ds = SyntheticVID(args.frames)
    metric = vy.VIDDetectionMetric(ds)
    build_s = time.perf_counter() - t0
    chunk = 64 * 256
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    upd_dev_ms = upd_wall_s = 0.0
    for lo in range(0, args.frames, chunk):
        hi = min(lo + chunk, args.frames)
        b, l, s = (torch.from_numpy(a).to(dev) for a in ds.detections(rows, lo=lo, hi=hi))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for i in range(0, hi - lo, batch):
            j = min(i + batch, hi - lo)
            metric.update(b[i:j], l[i:j], s[i:j], sid=range(lo + i, lo + j))
        e1.record()
        torch.cuda.synchronize()
        upd_wall_s += time.perf_counter() - t0
        upd_dev_ms += e0.elapsed_time(e1)
    print("updates of the large set done", file=sys.stderr, flush=True)
    t0 = time.perf_counter()
    names, values = metric.get()
    get_s = time.perf_counter() - t0
    kept = len(metric.matches()[0])
    detect_fps = {s: 1e3 * batch / out["update"]["detect_ms"][str(s)] for s in (416, 608)}
    out["val"] = {"frames": args.frames, "rows": rows, "classes": len(ds.classes), "ground_truths": int(ds.count.sum()),
                  "kept_rows": kept, "tables_build_s": round(build_s, 2), "updates": -(-args.frames // batch),
                  "update_events_ms_total": round(upd_dev_ms, 1), "update_wall_s_total": round(upd_wall_s, 2),
                  "get_wall_s": round(get_s, 2), "detect_fps": {str(s): round(v, 1) for s, v in detect_fps.items()},
                  "mean_ap_all": values[0].split("\n")[1]}
    return out


def kernel_stats():
    rows = _measure.kernel_rows(__file__, ["--child", "--updates-only"], CHILD_TIMEOUT_S, "vid_metric_")
    if isinstance(rows, dict):
        return rows
    for r in rows:
        if "vid_match_kernel" in r["name"]:
            return _measure.stats_of(r)
    return {"error": "no vid_match_kernel row in the kernel statistics"}


def device_section(res, stats):
    u, v = res["update"], res["val"]
    d416, d608 = u["detect_ms"]["416"], u["detect_ms"]["608"]
    lines = ["%s; device events, median of %d rounds, update() and detect steps alternating in one process" % (
        res["device"], res["rounds"]), "",
        "update(), %d frames x %d rows (sort, casts, vy_vid_match; 4 x 4 slices): %.4f ms (rounds %s)" % (
            u["batch"], u["rows"], u["ms"], u["ms_rounds"]),
        "  the host's side of one call: %.3f ms (nothing waits for the device)" % u["host_ms_per_call"],
        "detect step, batch %d: 416 x 416 %.3f ms (%.0f frames/s), 608 x 608 %.3f ms (%.0f frames/s)" % (
            u["batch"], d416, 1e3 * u["batch"] / d416, d608, 1e3 * u["batch"] / d608),
        "  update / detect step at 416: %.2f%% (bar: 2%%) -> %s;   at 608: %.2f%%" % (
            100 * u["ms"] / d416, "within" if u["ms"] <= 0.02 * d416 else "MISSED", 100 * u["ms"] / d608), ""]
    if stats is not None:
        lines += ["rocprofv3 --kernel-trace --stats, vid_match_kernel alone over such updates: %s" % json.dumps(stats), ""]
    per_frame_us = 1e3 * v["update_events_ms_total"] / v["frames"]
    get_us = 1e6 * v["get_wall_s"] / v["frames"]
    lines += ["VID-val-sized synthetic set: %d frames, %d classes, %d rows per frame (%d kept), %d ground truths" % (
        v["frames"], v["classes"], v["rows"], v["kept_rows"], v["ground_truths"]),
        "  ground-truth tables at construction (host, once): %.2f s" % v["tables_build_s"],
        "  %d update() calls of 64 frames: %.1f ms of device time by events (%.2f us per frame), %.2f s wall" % (
            v["updates"], v["update_events_ms_total"], per_frame_us, v["update_wall_s_total"]),
        "  get() (one copy to the host, sorts, 16 x %d AP curves): %.2f s wall (%.2f us per frame)" % (
            v["classes"], v["get_wall_s"], get_us),
        "  %s" % v["mean_ap_all"]]
    for s in ("416", "608"):
        det_us = 1e6 / v["detect_fps"][s]
        wall_us = 1e6 * v["update_wall_s_total"] / v["frames"]
        lines.append("  per frame at %s: detect %.1f us; metric %.2f us on the device + %.2f us of get() = %.1f%% of detecting "
                     "(update by wall %.2f us: %.1f%% with get())" % (
                         s, det_us, per_frame_us, get_us, 100 * (per_frame_us + get_us) / det_us, wall_us,
                         100 * (wall_us + get_us) / det_us))
    return "\n".join(lines) + "\n"


# ---------------------------------------------------------------------------------------------------- the reference section
def reference_section(ref_dir, n_frames):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_vid_metric_golden as G
    G.REF = ref_dir
    G._install_stubs()
    import metrics.imgnetvid as ref
    ref.np = G._NumpyProxy()
    from videoyolo_amd.metrics import VIDDetectionMetric
    ds = SyntheticVID(n_frames)
    b, l, s = ds.detections(20)
    mine = VIDDetectionMetric(ds)
    t0 = time.perf_counter()
    mine.update(b, l, s, sid=range(n_frames))
    mine.get()
    mine_s = time.perf_counter() - t0
    m = ref.VIDDetectionMetric(ds)
    for i in range(n_frames):
        m.update(b[i:i + 1], l[i:i + 1, :, 0], s[i:i + 1, :, 0], None, None, None, sid=i)
    t0 = time.perf_counter()
    ap = ref.vid_eval_motion(ds, m._results, m._motion_ranges, m._area_ranges, iou_threshold=0.5)
    ref_s = time.perf_counter() - t0
    diff = float(np.abs(np.asarray(ap) - mine.ap).max())
    return ("the reference's vid_eval_motion on %d synthetic frames (30 classes, 20 rows, at most 4 ground truths per frame), "
            "one CPU core:\n  %.2f s = %.0f frames/s\nthis metric's host path (vid_match_host + get()) on the same set: %.2f s = "
            "%.0f frames/s\n  largest |AP difference| between the two: %.3g\n" % (
                n_frames, ref_s, n_frames / ref_s, mine_s, n_frames / mine_s, diff))


def write_section(path, header, body):
    parts = {h: "" for h in SECTIONS}
    if os.path.exists(path):
        cur = None
        for line in open(path).read().splitlines():
            if line in SECTIONS:
                cur = line
            elif cur:
                parts[cur] += line + "\n"
    parts[header] = body
    with open(path, "w") as f:
        f.write("ImageNet-VID motion / area mAP: cost of the metric (tools/vid_metric.py)\n\n")
        for h in SECTIONS:
            if parts[h].strip():
                f.write(h + "\n" + parts[h].strip("\n") + "\n\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=176126)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--stats", action="store_true")
    ap.add_argument("--reference", default=None)
    ap.add_argument("--ref-frames", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vid_metric.txt"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--updates-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args)))
        return
    if args.reference:
        text = reference_section(args.reference, args.ref_frames)
        write_section(args.out, SECTIONS[0], text)
        print(text)
        return
    res = _measure.run_child(__file__, ["--child", "--frames", str(args.frames), "--rounds", str(args.rounds), "--updates",
                                        str(args.updates), "--steps", str(args.steps)], CHILD_TIMEOUT_S)
    text = device_section(res, kernel_stats() if args.stats else None)
    write_section(args.out, SECTIONS[1], text)
    print(text)


if __name__ == "__main__":
    main()
