"""Cases shared by tests/test_voc_metric_host.py and tests/test_gpu_voc_metric.py: the reference's recorded VOC cases
(tests/golden/voc_metric_golden.json), constructed images with known answers, and seeded random batches."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
_golden = None


def golden_cases():
    global _golden
    if _golden is None:
        with open(os.path.join(HERE, "golden", "voc_metric_golden.json")) as f:
            _golden = json.load(f)
    return _golden


def golden_updates(case):
    """The case's updates as float32 arrays: (pred_bboxes, pred_labels, pred_scores, gt_bboxes, gt_labels, gt_difficults
    or None), as tests/test_metrics_golden.py feeds them."""
    out = []
    for u in case["updates"]:
        a = {k: np.array(v, F32) for k, v in u.items()}
        diff = a["gt_difficults"] if case["spec"].get("difficult", True) else None
        out.append((a["pred_bboxes"], a["pred_labels"], a["pred_scores"], a["gt_bboxes"], a["gt_labels"], diff))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# constructed images: (name, boxes, labels, scores, gt_boxes, gt_labels, gt_difficults, want flags, want best), all at
# iou_thresh 0.5.  Every coordinate is dyadic, so every IoU below is exact in float32.
A = [0, 0, 4, 4]                       # area 16
TALL = [0, 0, 4, 8]                    # holds A: IoU 16 / 32 = 0.5 exactly
TALL_UP = [0, -4, 4, 4]                # the same, the other way
TALLER = [0, 0, 4, 8 + 2.0 ** -20]     # one float32 step taller: IoU 16 / (32 + 2^-18) = 0.5 - 2^-24
POINT = [1, 1, 1, 1]                   # no area: with itself 0 / 0
FAR = [50, 50, 60, 60]

CONSTRUCTED = [
    ("iou_equals_thresh", [A], [0], [0.9], [TALL], [0], [0], [1], [0]),
    ("iou_one_step_below", [A], [0], [0.9], [TALLER], [0], [0], [0], [-1]),
    # two rows on one ground truth, the higher score in the LATER row: it is the one that claims
    ("two_on_one", [A, A], [0, 0], [0.8, 0.9], [TALL], [0], [0], [0, 1], [0, 0]),
    ("equal_iou_first_index", [A], [0], [0.9], [FAR, TALL, TALL_UP], [0, 0, 0], [0, 0, 0], [1], [1]),
    ("difficult_claimed_twice", [A, A], [0, 0], [0.9, 0.8], [TALL], [0], [1], [-1, -1], [0, 0]),
    # a zero-area row on the same zero-area ground truth: 0 / 0 = NaN, the argmax, and NaN < thresh is false
    ("nan_branch", [POINT], [0], [0.9], [FAR, POINT, POINT], [0, 0, 0], [0, 0, 0], [1], [1]),
    ("padding_anywhere", [FAR, A, FAR, A, FAR], [-1, 0, -1, 0, -1], [-1, 0.9, -1, 0.8, -1], [TALL, FAR], [0, -1], [0, 0],
     [-2, 1, -2, 0, -2], [-1, 0, -1, 0, -1]),
    ("other_class_is_no_candidate", [A, A], [1, 0], [0.9, 0.8], [TALL], [0], [0], [0, 1], [-1, 0]),
    ("no_ground_truth", [A, FAR], [0, 3], [0.9, 0.8], [], [], [], [0, 0], [-1, -1]),
]


def constructed():
    """[(name, (boxes, labels, scores, gt_boxes, gt_labels, gt_difficults), want_flags, want_best)], float32 inputs."""
    out = []
    for name, b, l, s, gb, gl, gd, flags, best in CONSTRUCTED:
        arrays = (np.array(b, F32).reshape(-1, 4), np.array(l, F32), np.array(s, F32), np.array(gb, F32).reshape(-1, 4),
                  np.array(gl, F32), np.array(gd, F32))
        out.append((name, arrays, np.array(flags, np.int8), np.array(best, np.int64)))
    return out


def constructed_batch():
    """The constructed images as one padded batch (padding rows last): six (B, ...) float32 arrays, the wanted flags and
    best (B, R), and the wanted flags of the rows that are detections, image by image."""
    cases = constructed()
    n_rows = max(len(c[1][1]) for c in cases)
    n_gt = max(len(c[1][4]) for c in cases)
    B = len(cases)
    pb, pl, ps = np.zeros((B, n_rows, 4), F32), np.full((B, n_rows), -1, F32), np.full((B, n_rows), -1, F32)
    gb, gl, gd = np.zeros((B, n_gt, 4), F32), np.full((B, n_gt), -1, F32), np.zeros((B, n_gt), F32)
    flags, best = np.full((B, n_rows), -2, np.int8), np.full((B, n_rows), -1, np.int64)
    for i, (_, (b, l, s, g, glab, gdiff), f, bst) in enumerate(cases):
        pb[i, :len(l)], pl[i, :len(l)], ps[i, :len(l)] = b, l, s
        gb[i, :len(glab)], gl[i, :len(glab)], gd[i, :len(glab)] = g, glab, gdiff
        flags[i, :len(l)], best[i, :len(l)] = f, bst
    return (pb, pl, ps, gb, gl, gd), flags, best


# ---------------------------------------------------------------------------------------------------------------------
# seeded random batches
def random_batch(seed, batch, rows, n_gt, n_cls, difficult=True, class_map=None):
    """(pred_bboxes (B, R, 4), pred_labels (B, R, 1), pred_scores (B, R, 1), gt_bboxes (B, M, 4), gt_labels (B, M, 1),
    gt_difficults (B, M, 1) or None), float32.  Detections are jittered copies of the image's ground truths (several per
    ground truth, half of them on integer coordinates so that equal IoUs occur) and clutter; a sixth of the rows and of
    the ground truths are padding (label -1), anywhere; scores are distinct over the whole batch.  With a class_map the
    ground-truth labels are raw (indices into it) and the detections' labels mapped."""
    rng = np.random.default_rng(seed)
    n_raw = n_cls if class_map is None else len(class_map)
    xy = rng.integers(0, 300, (batch, n_gt, 2))
    wh = rng.integers(4, 120, (batch, n_gt, 2))
    gb = np.concatenate([xy, xy + wh], 2).astype(F32)
    gl = rng.integers(0, n_raw, (batch, n_gt)).astype(F32)
    gl[rng.random((batch, n_gt)) < 1 / 6] = -1
    gd = (rng.random((batch, n_gt)) < 0.25).astype(F32) if difficult else None
    if n_gt:
        src = rng.integers(0, n_gt, (batch, rows))
        boxes = np.take_along_axis(gb, src[:, :, None], 1).astype(np.float64)
        raw = np.take_along_axis(gl, src, 1)
        jitter = rng.normal(0, 6.0, (batch, rows, 4))
        whole = rng.random((batch, rows)) < 0.5
        jitter[whole] = np.round(jitter[whole] / 3.0)
        boxes = boxes + jitter
        if class_map is None:
            labels = raw.copy()
        else:
            labels = np.where(raw >= 0, np.asarray(class_map, np.float64)[np.maximum(raw, 0).astype(int)], -1.0)
        labels[labels < 0] = rng.integers(0, n_cls, int((labels < 0).sum()))
    else:
        boxes = np.zeros((batch, rows, 4))
        labels = rng.integers(0, n_cls, (batch, rows)).astype(np.float64)
    clutter = rng.random((batch, rows)) < 0.25
    cxy = rng.uniform(0, 300, (batch, rows, 2))
    boxes[clutter] = np.concatenate([cxy, cxy + rng.uniform(4, 120, (batch, rows, 2))], 2)[clutter]
    labels[clutter] = rng.integers(0, n_cls, int(clutter.sum()))
    scores = ((rng.permutation(batch * rows) + 1.0) / (batch * rows + 1.0)).reshape(batch, rows)
    pad = rng.random((batch, rows)) < 1 / 6
    if rows > 1:
        labels[pad], boxes[pad] = -1, -1
    pb, pl, ps = boxes.astype(F32), labels.astype(F32)[:, :, None], scores.astype(F32)[:, :, None]
    assert len(np.unique(ps)) == ps.size                       # distinct as float32: the order of claims is defined
    return pb, pl, ps, gb, gl[:, :, None], None if gd is None else gd[:, :, None]


DROPPING_MAP = [0, -1, 1, 2, -1, 3, 4, 5, 6, -1, 7, 8, 9, 10, 11, -1, 12, 13, 14, 15, 16, 17, -1, 18, 19]   # 25 raw -> 20

# (batch, rows, ground truths, classes, difficults, class_map): the smallest shapes that reach every piece of the kernel —
# one and several workgroups, 257 rows (the block-stride loop) and 1024 (the cap), no / one / many ground truths
SHAPES = [
    (1, 1, 0, 1, False, None),
    (1, 100, 1, 1, True, None),
    (5, 1, 300, 20, True, None),
    (5, 100, 70, 20, True, None),
    (5, 257, 300, 80, False, None),
    (5, 1024, 300, 20, True, DROPPING_MAP),
    (1, 1024, 70, 1, True, None),
    (67, 100, 70, 20, True, DROPPING_MAP),
    (67, 257, 1, 80, False, None),
    (67, 100, 0, 20, False, None),
]


def shape_id(s):
    return "B%d_R%d_M%d_C%d%s%s" % (s[0], s[1], s[2], s[3], "_diff" if s[4] else "", "_map" if s[5] else "")


def mapped_labels(gt_labels, class_map):
    """Ground-truth labels through the class map, as _update_image maps them; < 0: dropped."""
    gl = np.asarray(gt_labels).reshape(-1)
    if class_map is None:
        return gl
    return np.array([class_map[int(g)] for g in gl], np.float64).reshape(-1)
