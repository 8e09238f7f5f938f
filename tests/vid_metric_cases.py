"""Shared by the VID-metric tests: the golden cases (tests/golden/vid_metric_golden.json, written by the reference's own
metric, see tests/golden/make_vid_metric_golden.py), stand-in datasets and seeded random batches."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_cases = None


class StandInDataset(object):
    """The four attributes VIDDetectionMetric reads from a dataset."""

    def __init__(self, sample_ids, labels, motion_ious, wn_classes, classes):
        self._sample_ids, self._labels = sample_ids, labels
        self.motion_ious, self.wn_classes, self.classes = motion_ious, wn_classes, classes

    def get_sample_ids(self):
        return self._sample_ids

    def get_label(self, i):
        return self._labels[i]


def golden_cases():
    global _cases
    if _cases is None:
        with open(os.path.join(HERE, "golden", "vid_metric_golden.json")) as f:
            _cases = json.load(f)
    return _cases


def case_names():
    return [c["name"] for c in golden_cases()]


def case(name):
    return next(c for c in golden_cases() if c["name"] == name)


def case_dataset(c):
    d = c["dataset"]
    labels = {int(k): np.asarray(v, np.float64).reshape(-1, 5) for k, v in d["labels"].items()}
    return StandInDataset(d["sample_ids"], labels, d["motion_ious"], d["wn_classes"], d["classes"])


def case_frames(c):
    """(sid, boxes (N, 4), labels (N), scores (N)) float32, as the detector gives them."""
    return [(f["sid"], np.asarray(f["boxes"], np.float32).reshape(-1, 4), np.asarray(f["labels"], np.float32),
             np.asarray(f["scores"], np.float32)) for f in c["frames"]]


def expected_matches(c):
    """tp (n, 16) and fp (n, 16) of every kept detection in the golden order, with labels and scores."""
    e = c["expected"]
    n = len(e["det_scores"])
    tp = np.asarray([s["tp"] for s in e["slices"]], np.int64).reshape(len(e["slices"]), n).T
    fp = np.asarray([s["fp"] for s in e["slices"]], np.float64).reshape(len(e["slices"]), n).T
    return np.asarray(e["det_labels"], np.int64), np.asarray(e["det_scores"], np.float64), tp, fp


def check_against_golden(metric, c):
    """metric has seen every frame of c: its per-detection tp / fp equal the reference's exactly, ap within 1e-12, and the
    get() strings are the reference's."""
    names, values = metric.get()
    label, score, tp, fp = expected_matches(c)
    _, got_label, got_score, got_tp, got_fp = metric.matches()
    assert np.array_equal(got_label, label) and np.array_equal(got_score, score)
    assert got_tp.dtype == np.uint8 and got_fp.dtype == np.float64
    assert np.array_equal(got_tp, tp), np.argwhere(got_tp != tp)[:5]
    assert np.array_equal(got_fp, fp), np.argwhere(got_fp != fp)[:5]
    ap = np.asarray(c["expected"]["ap"], np.float64)
    assert metric.ap.shape == ap.shape
    assert np.abs(metric.ap - ap).max() <= 1e-12
    assert names == c["expected"]["names"] and values == c["expected"]["values"]


def random_set(seed, n_frames, n_cls=5, max_rows=100, max_gt=70, ties=True):
    """A stand-in dataset of n_frames frames and one (B, max_rows) batch of detections for it: 0..max_rows rows per frame,
    -1 padding, sub-threshold scores, 0..max_gt ground truths, frames without either, and (ties) repeated scores and
    detections that overlap two ground truths equally."""
    rng = np.random.default_rng(seed)
    labels, motion = {}, {}
    boxes = np.full((n_frames, max_rows, 4), -1.0, np.float32)
    cls = np.full((n_frames, max_rows), -1.0, np.float32)
    score = np.full((n_frames, max_rows), -1.0, np.float32)
    for i in range(n_frames):
        m = int(rng.integers(0, max_gt + 1)) if i % 5 else (0 if i % 2 else max_gt)
        xy = rng.integers(0, 400, (m, 2))
        wh = rng.integers(8, 260, (m, 2))
        labels[i] = np.concatenate([xy, xy + wh - 1, rng.integers(0, n_cls, (m, 1))], 1).astype(np.float64)
        if ties and m > 1:
            shift = int(wh[0, 0]) // 8
            labels[i][1, :4] = labels[i][0, :4] + [2 * shift, 0, 2 * shift, 0]    # a twin of ground truth 0, a little right
            labels[i][1, 4] = labels[i][0, 4]
        mo = np.round(rng.random(m), 2)
        mo[rng.random(m) < 0.2] = 0.7
        mo[rng.random(m) < 0.2] = 0.9
        motion[str(i)] = mo.tolist()
        k = int(rng.integers(0, max_rows + 1)) if i % 7 else (0 if i % 2 else max_rows)
        if not k:
            continue
        if m:
            src = rng.integers(0, m, k)
            b = labels[i][src, :4] + np.round(rng.normal(0, 4.0, (k, 4)))
            l = labels[i][src, 4].copy()
        else:
            b, l = np.zeros((k, 4)), np.zeros(k)
        clutter = (rng.random(k) < 0.3) | (m == 0)
        rb = rng.integers(0, 400, (k, 2))
        b[clutter] = np.concatenate([rb, rb + rng.integers(8, 260, (k, 2))], 1)[clutter]
        flip = rng.random(k) < 0.15
        l[flip] = rng.integers(0, n_cls, int(flip.sum()))
        s = rng.random(k)
        s[rng.random(k) < 0.1] *= 0.05
        if ties and k > 3:
            s[1] = s[0]
            if m > 1:   # halfway between ground truth 0 and its twin
                b[2] = labels[i][0, :4] + [shift, 0, shift, 0]
                l[2] = labels[i][0, 4]
        rows = rng.permutation(max_rows)[:k]                                      # padding anywhere, not only at the end
        boxes[i, rows], cls[i, rows], score[i, rows] = b, l, s
    names = ["n%02d" % c for c in range(n_cls)]
    ds = StandInDataset(list(range(n_frames)), labels, motion, names, ["class_" + n for n in names])
    return ds, boxes, cls, score
