"""Cases shared by tests/test_frame_map_host.py and tests/test_gpu_frame_map.py: the reference's recorded per-frame scores
(tests/golden/frame_map_golden.json), constructed frames with hand-derived answers, and the seeded batches of
voc_metric_cases with their host results, computed once."""
import json
import os

import numpy as np

import frame_map_model as M
import voc_metric_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
_golden = None
_refs = {}


def golden_cases():
    global _golden
    if _golden is None:
        with open(os.path.join(HERE, "golden", "frame_map_golden.json")) as f:
            _golden = json.load(f)
    return _golden


def golden_inputs(case):
    """(pred_bboxes, pred_labels, pred_scores, gt_bboxes, gt_labels, gt_difficults or None) float32, class_map, expected
    (frames,) float64 with NaN where the reference gave NaN."""
    a = {k: np.array(v, F32) for k, v in case["inputs"].items()}
    diff = a["gt_difficults"] if case["spec"]["difficult"] else None
    want = np.array([np.nan if e is None else e for e in case["expected"]], np.float64)
    return ((a["pred_bboxes"], a["pred_labels"], a["pred_scores"], a["gt_bboxes"], a["gt_labels"], diff),
            case["spec"]["class_map"], want)


def bound(rows, n_gt):
    """|device or model - frame_map_host| for a frame: each side sums at most `rows` non-negative terms totalling <= 1 per
    class, then averages at most n_gt classes, in float64, in its own order."""
    return 2.0 * (rows + n_gt + 2) * 2.0 ** -53


# ---------------------------------------------------------------------------------------------------------------------
# constructed frames, all at iou_thresh 0.5 with the dyadic boxes of voc_metric_cases: a detection A at place i matches the
# ground truth TALL at place i with IoU exactly 0.5; NOWHERE overlaps nothing.
def at(box, i):
    return [box[0] + 16 * i, box[1], box[2] + 16 * i, box[3]]


NOWHERE = [500, 500, 504, 504]
PAD = [-1, -1, -1, -1]


def seq11(values):
    """The 11-point sum in numpy's order: ap = 0; ap += v / 11.0 for every v."""
    ap = 0.0
    for v in values:
        ap += v / 11.0
    return ap


def _tps(m):
    """m true positives of one class with 10 ground truths: recall reaches exactly m / 10."""
    return ([at(C.A, i) for i in range(m)], [0] * m, [0.9 - 0.05 * i for i in range(m)],
            [at(C.TALL, i) for i in range(10)], [0] * 10, [0] * 10, [1] * m)


# name -> (boxes, labels, scores, gt_boxes, gt_labels, gt_difficults, flags, area score, 11-point score, classes, on host)
# `on host`: frame_map_host is defined on the case (no equal scores)
CONSTRUCTED = {
    # (a) score order TP FP TP, npos 2: prec 1, 1/2, 2/3 at rec 1/2, 1/2, 1.  Area: the first TP sees the envelope 1, the
    # second 2/3.  11-point: t = 0 .. 0.5 see prec 1, t = 0.6 .. 1.0 see 2/3.
    "a_tp_fp_tp": ([NOWHERE, at(C.A, 1), at(C.A, 0)], [0, 0, 0], [0.8, 0.7, 0.9], [at(C.TALL, 0), at(C.TALL, 1)], [0, 0], [0, 0],
                   [0, 1, 1], 0.5 * 1.0 + 0.5 * (2.0 / 3.0), seq11([1.0] * 6 + [2.0 / 3.0] * 5), 1, True),
    # (b) class 1 has a ground truth and no detection: AP 0 beside class 0's 1
    "b_class_without_detection": ([at(C.A, 0)], [0], [0.9], [at(C.TALL, 0), at(C.TALL, 1)], [0, 1], [0, 0],
                                  [1], (1.0 + 0.0) / 2, seq11([1.0] * 11) / 2, 2, True),
    # (c) class 1 has detections and no ground truth: it is not scored
    "c_class_without_ground_truth": ([at(C.A, 0), at(C.A, 1), NOWHERE], [0, 1, 1], [0.9, 0.95, 0.8], [at(C.TALL, 0)], [0], [0],
                                     [1, 0, 0], 1.0, seq11([1.0] * 11), 1, True),
    # (d) only a difficult ground truth: nothing to score
    "d_only_difficult": ([at(C.A, 0)], [0], [0.9], [at(C.TALL, 0)], [0], [1], [-1], float("nan"), float("nan"), 0, True),
    # (e) recall exactly m / 10 misses its own threshold 0.0 + m * 0.1 for m = 3, 6, 7 (0.30000000000000004,
    # 0.6000000000000001, 0.7000000000000001): thresholds 0 .. m - 1 see prec 1, the rest nothing
    "e_3_of_10": _tps(3) + (None, seq11([1.0] * 3), 1, True),
    "e_6_of_10": _tps(6) + (None, seq11([1.0] * 6), 1, True),
    "e_7_of_10": _tps(7) + (None, seq11([1.0] * 7), 1, True),
    # (f) a row matched to a difficult ground truth between two TPs: prec stays 1, npos is 2
    "f_ignored_between_tps": ([at(C.A, 0), at(C.A, 1), at(C.A, 2)], [0, 0, 0], [0.9, 0.8, 0.7],
                              [at(C.TALL, 0), at(C.TALL, 1), at(C.TALL, 2)], [0, 0, 0], [0, 1, 0],
                              [1, -1, 1], 1.0, seq11([1.0] * 11), 1, True),
    # (g) equal scores, the TP in the lower row: the device ranks it first, prec 1 then 1/2: AP 1 (the other order: 1/2)
    "g_equal_scores": ([at(C.A, 0), NOWHERE], [0, 0], [0.5, 0.5], [at(C.TALL, 0)], [0], [0],
                       [1, 0], 1.0, seq11([1.0] * 11), 1, False),
    # (h) padding rows anywhere, with the highest scores: they are no detections
    "h_padding_anywhere": ([PAD, at(C.A, 0), PAD, NOWHERE, PAD], [-1, 0, -1, 0, -1], [2.0, 0.9, 0.95, 0.8, -1.0], [at(C.TALL, 0)],
                           [0], [0], [-2, 1, -2, 0, -2], 1.0, seq11([1.0] * 11), 1, True),
    # (i) no rows at all and a ground truth: the class is scored, with AP 0
    "i_no_rows": ([], [], [], [at(C.TALL, 0), at(C.TALL, 1)], [0, 3], [0, 0], [], 0.0, 0.0, 2, True),
}


def constructed():
    """[(name, (boxes (1, R, 4), labels (1, R), scores (1, R), gt_boxes (1, M, 4), gt_labels (1, M), gt_difficults (1, M))
    float32, flags (R,) int8, area score or None, 11-point score, classes, on_host)]"""
    out = []
    for name, (b, l, s, gb, gl, gd, flags, area, eleven, classes, on_host) in CONSTRUCTED.items():
        arrays = (np.array(b, F32).reshape(1, -1, 4), np.array(l, F32).reshape(1, -1), np.array(s, F32).reshape(1, -1),
                  np.array(gb, F32).reshape(1, -1, 4), np.array(gl, F32).reshape(1, -1), np.array(gd, F32).reshape(1, -1))
        out.append((name, arrays, np.array(flags, np.int8), area, eleven, classes, on_host))
    return out


def same(a, b):
    return (a != a and b != b) or a == b


def ulps(a, b):
    return abs(a - b) / np.spacing(max(abs(a), abs(b)))


# ---------------------------------------------------------------------------------------------------------------------
def reference(shape):
    """The seeded batch of a shape of voc_metric_cases.SHAPES (random_batch(7, ...)), once: its arrays, the class-mapped
    ground-truth labels (B, M) int32, voc_match_host's flags (B, R), frame_map_host in both modes {use_07: (B,)} and the
    model's scores and class counts {use_07: ((B,), (B,))}.  Left unchanged by the tests."""
    from videoyolo_amd.metrics import frame_map_host, voc_match_host
    key = C.shape_id(shape)
    if key not in _refs:
        batch, rows, n_gt, n_cls, difficult, class_map = shape
        arrays = C.random_batch(7, batch, rows, n_gt, n_cls, difficult, class_map)
        pb, pl, ps, gb, gl, gd = arrays
        mapped = np.stack([C.mapped_labels(gl[i], class_map) for i in range(batch)]).reshape(batch, n_gt)
        mapped = np.where(mapped >= 0, mapped, -1).astype(np.int32)
        flags = np.zeros((batch, rows), np.int8)
        for i in range(batch):
            flags[i] = voc_match_host(pb[i], pl[i], ps[i], gb[i], mapped[i], None if gd is None else gd[i], 0.5)
        host = {m: frame_map_host(*arrays, iou_thresh=0.5, class_map=class_map, use_07_metric=m) for m in (False, True)}
        model = {m: M.batch_scores(pl.reshape(batch, rows), ps.reshape(batch, rows), flags, mapped,
                                   None if gd is None else gd.reshape(batch, n_gt), m) for m in (False, True)}
        _refs[key] = (arrays, mapped, flags, host, model)
    return _refs[key]
