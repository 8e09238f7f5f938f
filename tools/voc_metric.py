"""Cost of the VOC metric's device path (videoyolo_amd/metrics.py VOCMApMetric.update on device tensors, csrc/voc_metric.hip)
next to the detecting it scores and next to the host path.  Written to --out (default profiles/voc_metric.txt).  In a
fresh child process on the GPU:

  (a) the device time of update() for 64 frames x 100 rows x 8 ground truths by events, ALTERNATING with the batch-64
      detect step at 416 x 416 and 608 x 608 of a single-frame net in the same process (same clocks), --rounds rounds;
  (c) the host path's update() on the same device tensors, by the wall clock, copy to the host included;
  (d) a synthetic validation set of --images images end to end (every update() in batches of 64, then get()) on both
      paths, by the wall clock, and that the two get() results are equal.
With --stats a second child runs such updates under `rocprofv3 --kernel-trace --stats` (no counters in that run) and
  (b) the kernel's own mean time is added.

    python tools/voc_metric.py [--stats] [--images 5000] [--out PATH]
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
CHILD_TIMEOUT_S = 600
N_CLS = 20


def synthetic(seed, images, rows=100, n_gt=8, size=416):
    """(images, rows, 4), (images, rows, 1), (images, rows, 1), (images, n_gt, 4), (images, n_gt, 1), (images, n_gt, 1)
    float32, the shapes validate() feeds: 1..n_gt ground truths per image (the rest -1 padding, a fifth difficult), rows
    that are jittered copies of them or clutter, a tenth of the rows padding."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, size * 0.6, (images, n_gt, 2))
    gb = np.concatenate([xy, xy + rng.uniform(16, size * 0.4, (images, n_gt, 2))], 2)
    gl = rng.integers(0, N_CLS, (images, n_gt)).astype(np.float64)
    gl[np.arange(n_gt)[None, :] >= rng.integers(1, n_gt + 1, (images, 1))] = -1
    gd = (rng.random((images, n_gt)) < 0.2).astype(np.float64)
    src = rng.integers(0, n_gt, (images, rows))
    boxes = np.take_along_axis(gb, src[:, :, None], 1) + rng.normal(0, 6.0, (images, rows, 4))
    labels = np.take_along_axis(gl, src, 1)
    clutter = (rng.random((images, rows)) < 0.3) | (labels < 0)
    cxy = rng.uniform(0, size * 0.6, (images, rows, 2))
    boxes[clutter] = np.concatenate([cxy, cxy + rng.uniform(16, size * 0.4, (images, rows, 2))], 2)[clutter]
    labels[clutter] = rng.integers(0, N_CLS, int(clutter.sum()))
    # distinct within an image, so the order of claims is defined on both paths
    scores = (rng.permuted(np.tile(np.arange(rows), (images, 1)), axis=1) + 0.5 * rng.random((images, rows))) / rows
    pad = rng.random((images, rows)) < 0.1
    boxes[pad], labels[pad], scores[pad] = -1, -1, -1
    f = np.float32
    return (boxes.astype(f), labels.astype(f)[:, :, None], scores.astype(f)[:, :, None], gb.astype(f), gl.astype(f)[:, :, None],
            gd.astype(f)[:, :, None])


def measure(args):
    import torch
    import videoyolo_amd as vy
    from videoyolo_amd.metrics import VOCMApMetric
    dev = torch.device("cuda", 0)
    med = lambda v: float(np.median(v))  # noqa: E731
    out = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds}
    classes = ["c%02d" % c for c in range(N_CLS)]

    # ---- (a) update() for 64 frames x 100 rows x 8 ground truths, alternating with the detect step
    batch = 64
    sets = [tuple(torch.from_numpy(a).to(dev) for a in synthetic(u, batch)) for u in range(args.updates)]
    metric = VOCMApMetric(class_names=classes)
    state = {"u": 0}

    def update():
        u = state["u"] % args.updates
        if u == 0:
            metric.reset()
        metric.update(*sets[u])
        state["u"] += 1

    for _ in range(args.updates):
        update()
    torch.cuda.synchronize()
    assert metric.device_updates == args.updates
    print("updates warmed up", file=sys.stderr, flush=True)
    if args.updates_only:
        return out
    net = _measure.detect_net(vy, classes, dev)
    upd_ms, det_ms, call_ms = _measure.update_and_detect(torch, update, net, dev, batch, (416, 608), args)
    del net

    # ---- (c) the host path on the same device tensors: copy, then numpy
    host = VOCMApMetric(class_names=classes)
    host_ms = []
    for _ in range(args.rounds):
        host.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for u in range(args.updates):
            host._update_host(*sets[u])
        host_ms.append((time.perf_counter() - t0) / args.updates * 1e3)
    metric.reset()
    for u in range(args.updates):
        metric.update(*sets[u])
    same_small = _equal(metric.get(), host.get())
    out["update"] = {"batch": batch, "rows": 100, "n_gt": 8, "ms": round(med(upd_ms), 4), "ms_rounds": [round(v, 4) for v in upd_ms],
                     "call_ms": round(call_ms, 3), "host_path_ms": round(med(host_ms), 2),
                     "host_path_ms_rounds": [round(v, 2) for v in host_ms], "equal": same_small,
                     "detect_ms": {str(s): round(med(v), 3) for s, v in det_ms.items()},
                     "detect_ms_rounds": {str(s): [round(t, 3) for t in v] for s, v in det_ms.items()}}
    print("update and detect steps timed: %s" % json.dumps(out["update"]), file=sys.stderr, flush=True)

    # ---- (d) a validation set end to end on both paths
    data = [torch.from_numpy(a).to(dev) for a in synthetic(99, args.images)]
    res = {}
    for path in ("device", "host"):
        m = VOCMApMetric(class_names=classes)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for lo in range(0, args.images, batch):
            part = [a[lo:lo + batch] for a in data]
            (m.update if path == "device" else m._update_host)(*part)
        t1 = time.perf_counter()
        res[path] = m.get()
        t2 = time.perf_counter()
        out["val_" + path] = {"update_s": round(t1 - t0, 4), "get_s": round(t2 - t1, 4), "launches": m.device_updates}
    out["val"] = {"images": args.images, "equal": _equal(res["device"], res["host"]), "mAP": res["device"][1][-1]}
    return out


def _equal(a, b):
    return a[0] == b[0] and all(x == y or (x != x and y != y) for x, y in zip(a[1], b[1]))


def kernel_stats():
    rows = _measure.kernel_rows(__file__, ["--child", "--updates-only"], CHILD_TIMEOUT_S, "voc_metric_")
    if isinstance(rows, dict):
        return rows
    for r in rows:
        if "voc_match_kernel" in r["name"]:
            return _measure.stats_of(r)
    return {"error": "no voc_match_kernel row in the kernel statistics"}


def report(res, stats):
    u, v = res["update"], res["val"]
    d416, d608 = u["detect_ms"]["416"], u["detect_ms"]["608"]
    lines = ["PASCAL-VOC mAP: cost of the metric's device path (tools/voc_metric.py)", "",
             "%s; device events, median of %d rounds, update() and detect steps alternating in one process" % (
                 res["device"], res["rounds"]), "",
             "(a) update(), %d frames x %d rows x %d ground truths (casts, vy_voc_match): %.4f ms (rounds %s)" % (
                 u["batch"], u["rows"], u["n_gt"], u["ms"], u["ms_rounds"]),
             "    the host's side of one call: %.3f ms (nothing waits for the device)" % u["call_ms"],
             "    detect step, batch %d: 416 x 416 %.3f ms (%.0f frames/s), 608 x 608 %.3f ms (%.0f frames/s)" % (
                 u["batch"], d416, 1e3 * u["batch"] / d416, d608, 1e3 * u["batch"] / d608),
             "    update / detect step at 416: %.3f%% (bar: 2%%) -> %s;   at 608: %.3f%%" % (
                 100 * u["ms"] / d416, "within" if u["ms"] <= 0.02 * d416 else "MISSED", 100 * u["ms"] / d608)]
    if stats is not None:
        lines.append("(b) rocprofv3 --kernel-trace --stats, voc_match_kernel alone over such updates: %s" % json.dumps(stats))
    lines += ["(c) the host path's update() on the same device tensors (copy to the host, then numpy), wall clock: %.2f ms per "
              "batch (rounds %s) = %.0f us per image; results equal: %s" % (
                  u["host_path_ms"], u["host_path_ms_rounds"], 1e3 * u["host_path_ms"] / u["batch"], u["equal"]),
              "    host path / device path per batch: %.0fx by device time, %.0fx by the caller's time" % (
                  u["host_path_ms"] / u["ms"], u["host_path_ms"] / u["call_ms"]),
              "(d) synthetic validation set, %d images x %d rows x %d ground truths in batches of %d, wall clock:" % (
                  v["images"], u["rows"], u["n_gt"], u["batch"])]
    for path in ("device", "host"):
        r = res["val_" + path]
        lines.append("    %-6s path: update() calls %.3f s, get() %.3f s, total %.3f s (%d launches)" % (
            path, r["update_s"], r["get_s"], r["update_s"] + r["get_s"], r["launches"]))
    lines.append("    get() results equal: %s (mAP %.6f)" % (v["equal"], v["mAP"]))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--stats", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voc_metric.txt"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--updates-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args)))
        return
    res = _measure.run_child(__file__, ["--child", "--images", str(args.images), "--rounds", str(args.rounds), "--updates",
                                        str(args.updates), "--steps", str(args.steps)], CHILD_TIMEOUT_S)
    text = report(res, kernel_stats() if args.stats else None)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    if not (res["update"]["equal"] and res["val"]["equal"]):
        sys.exit("device and host paths differ")


if __name__ == "__main__":
    main()
