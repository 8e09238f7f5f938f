"""Cost of the per-frame mAP's device path (videoyolo_amd/metrics.py FrameMApMetric.update on device tensors:
vy_voc_match + vy_voc_frame_ap, csrc/voc_metric.hip) next to the data-set metric on the same batch, next to the detecting
it scores and next to the host's per-frame loop.  Written to --out (default profiles/frame_metric.txt).  In a fresh child
process on the GPU:

  (a) the device time of FrameMApMetric.update() for 64 frames x 100 rows x 8 ground truths by events, ALTERNATING with
      the batch-64 detect step at 416 x 416 of a single-frame net in the same process (same clocks), --rounds rounds;
      VOCMApMetric.update() on the same batches, timed the same way;
  (c) the host's per-frame loop (frame_map_host: copy to the host, then reset / update / get per frame) on the same
      device tensors, by the wall clock;
  (d) the seeded batches the tests use (tests/voc_metric_cases.py, SHAPES with random_batch(7, ...)): the worst
      |device - frame_map_host| as a share of the derived bound 2 (rows + n_gt + 2) 2^-53, both modes.
With --stats a second child runs such updates under `rocprofv3 --kernel-trace --stats` (no counters in that run) and
  (b) the two kernels' own mean times are added.

    python tools/frame_metric.py [--stats] [--out PATH]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

import _measure
from _measure import ROOT
from voc_metric import N_CLS, synthetic

sys.path.insert(0, ROOT)
CHILD_TIMEOUT_S = 600


def accuracy(torch, dev):
    """(d): per mode, the worst |device - host| / bound over the tests' seeded shapes, and the shape it occurred at."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import voc_metric_cases as C
    from videoyolo_amd.metrics import FrameMApMetric, frame_map_host
    out = {}
    for mode in (False, True):
        worst = (0.0, "")
        for shape in C.SHAPES:
            batch, rows, n_gt, n_cls, difficult, class_map = shape
            arrays = C.random_batch(7, batch, rows, n_gt, n_cls, difficult, class_map)
            want = frame_map_host(*arrays, iou_thresh=0.5, class_map=class_map, use_07_metric=mode)
            m = FrameMApMetric(class_map=class_map, use_07_metric=mode)
            m.update(*[None if a is None else torch.from_numpy(a).to(dev) for a in arrays])
            assert m.device_updates == 1
            got = m.get()[1]
            if not np.array_equal(np.isnan(got), np.isnan(want)):
                return {"error": "NaN frames differ at %s" % C.shape_id(shape)}
            ok = ~np.isnan(want)
            if ok.any():
                ratio = float(np.abs(got[ok] - want[ok]).max()) / (2.0 * (rows + n_gt + 2) * 2.0 ** -53)
                worst = max(worst, (ratio, C.shape_id(shape)))
        out["use_07" if mode else "area"] = {"ratio": round(worst[0], 5), "shape": worst[1]}
    return out


def measure(args):
    import torch
    import videoyolo_amd as vy
    from videoyolo_amd.metrics import FrameMApMetric, VOCMApMetric, frame_map_host
    dev = torch.device("cuda", 0)
    med = lambda v: float(np.median(v))  # noqa: E731
    out = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds}
    classes = ["c%02d" % c for c in range(N_CLS)]

    batch = 64
    sets = [tuple(torch.from_numpy(a).to(dev) for a in synthetic(u, batch)) for u in range(args.updates)]
    frame_metric, set_metric = FrameMApMetric(class_names=classes), VOCMApMetric(class_names=classes)
    state = {"f": 0, "s": 0}

    def update_of(metric, slot):
        def update():
            u = state[slot] % args.updates
            if u == 0:
                metric.reset()
            metric.update(*sets[u])
            state[slot] += 1
        return update

    frame_update, set_update = update_of(frame_metric, "f"), update_of(set_metric, "s")
    for _ in range(args.updates):
        frame_update()
        set_update()
    torch.cuda.synchronize()
    assert frame_metric.device_updates == args.updates == set_metric.device_updates
    print("updates warmed up", file=sys.stderr, flush=True)
    if args.updates_only:
        return out
    net = _measure.detect_net(vy, classes, dev)
    upd_ms, det_ms, call_ms = _measure.update_and_detect(torch, frame_update, net, dev, batch, (416,), args)
    del net
    set_ms = [_measure.timed(torch, set_update, args.updates) for _ in range(args.rounds)]

    host_ms, want = [], None
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want = frame_map_host(*sets[0])
        host_ms.append((time.perf_counter() - t0) * 1e3)
    frame_metric.reset()
    frame_metric.update(*sets[0])
    got = frame_metric.get()[1]
    close = bool(np.array_equal(np.isnan(got), np.isnan(want)) and
                 np.nanmax(np.abs(got - want)) <= 2.0 * (100 + 8 + 2) * 2.0 ** -53)
    out["update"] = {"batch": batch, "rows": 100, "n_gt": 8, "ms": round(med(upd_ms), 4), "ms_rounds": [round(v, 4) for v in upd_ms],
                     "call_ms": round(call_ms, 3), "set_ms": round(med(set_ms), 4), "set_ms_rounds": [round(v, 4) for v in set_ms],
                     "host_loop_ms": round(med(host_ms), 2), "host_loop_ms_rounds": [round(v, 2) for v in host_ms],
                     "within_bound": close, "detect_ms": round(med(det_ms[416]), 3),
                     "detect_ms_rounds": [round(t, 3) for t in det_ms[416]]}
    print("update and detect steps timed: %s" % json.dumps(out["update"]), file=sys.stderr, flush=True)
    out["accuracy"] = accuracy(torch, dev)
    return out


def kernel_stats():
    rows = _measure.kernel_rows(__file__, ["--child", "--updates-only"], CHILD_TIMEOUT_S, "frame_metric_")
    if isinstance(rows, dict):
        return rows
    found = {k: _measure.stats_of(r) for r in rows for k in ("frame_ap_kernel", "voc_match_kernel") if k in r["name"]}
    return found or {"error": "no frame_ap_kernel row in the kernel statistics"}


def report(res, stats):
    u, acc = res["update"], res["accuracy"]
    lines = ["Per-frame mAP: cost of the metric's device path (tools/frame_metric.py)", "",
             "%s; device events, median of %d rounds, update() and detect steps alternating in one process" % (
                 res["device"], res["rounds"]), "",
             "(a) FrameMApMetric.update(), %d frames x %d rows x %d ground truths (casts, vy_voc_match, vy_voc_frame_ap): "
             "%.4f ms (rounds %s)" % (u["batch"], u["rows"], u["n_gt"], u["ms"], u["ms_rounds"]),
             "    the host's side of one call: %.3f ms (nothing waits for the device)" % u["call_ms"],
             "    VOCMApMetric.update() on the same batches (casts, vy_voc_match): %.4f ms (rounds %s)" % (
                 u["set_ms"], u["set_ms_rounds"]),
             "    detect step, batch %d at 416 x 416: %.3f ms (rounds %s); update / detect step: %.3f%%" % (
                 u["batch"], u["detect_ms"], u["detect_ms_rounds"], 100 * u["ms"] / u["detect_ms"])]
    if stats is not None:
        lines.append("(b) rocprofv3 --kernel-trace --stats over such updates: %s" % json.dumps(stats))
    lines += ["(c) the host's per-frame loop on the same device tensors (copy to the host, then reset / update / get per frame), "
              "wall clock: %.2f ms per batch (rounds %s) = %.0f us per frame; device scores within the bound of it: %s" % (
                  u["host_loop_ms"], u["host_loop_ms_rounds"], 1e3 * u["host_loop_ms"] / u["batch"], u["within_bound"]),
              "    host loop / device path per batch: %.0fx by device time, %.0fx by the caller's time" % (
                  u["host_loop_ms"] / u["ms"], u["host_loop_ms"] / u["call_ms"]),
              "(d) the tests' seeded batches, worst |device - frame_map_host| as a share of the bound 2 (rows + n_gt + 2) 2^-53: %s"
              % json.dumps(acc)]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--stats", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_metric.txt"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--updates-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args)))
        return
    res = _measure.run_child(__file__, ["--child", "--rounds", str(args.rounds), "--updates", str(args.updates), "--steps",
                                        str(args.steps)], CHILD_TIMEOUT_S)
    text = report(res, kernel_stats() if args.stats else None)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    if not res["update"]["within_bound"] or "error" in res["accuracy"]:
        sys.exit("device and host frame scores differ")


if __name__ == "__main__":
    main()
