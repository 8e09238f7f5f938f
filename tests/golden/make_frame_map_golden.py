"""Generates tests/golden/frame_map_golden.json by running THE REFERENCE's own VOCMApMetric
(/root/reference/metrics/pascalvoc.py) frame by frame, the way detect_yolo3.py:451-534 (add_metrics_to_predictions) does:
metric.reset(); metric.update(<one frame>); metric.get()[1][-1] — the mean AP of the frame, NaN recorded as null.

Runs only in the build container (needs /root/reference), with the stand-ins of make_voc_metric_golden.py for mxnet and
gluoncv.  The numeric body that produces the golden values is the reference's, unmodified.

Every coordinate is a multiple of 1/8 and every score a multiple of 1/64, so the file stays small; scores are distinct
within a frame, because the reference leaves the order among equal scores to an unstable argsort.

    python tests/golden/make_frame_map_golden.py
"""
import json
import math
import os
import warnings

import numpy as np

from make_voc_metric_golden import _install_stubs

HERE = os.path.dirname(os.path.abspath(__file__))
FRAMES = 4
DROPPING_MAP = [0, -1, 1, 2, -1, 3]          # 6 raw classes -> 4


def make_case(rng, n_pred, n_gt, n_cls, difficult, class_map, jitter):
    """FRAMES frames: detections are jittered copies of ground truths plus clutter, -1 padded like the detector's.  With a
    class_map the ground-truth labels are raw (indices into it) and the detections' labels mapped.  The last frame has
    nothing to score: only difficult ground truths, or only ground truths of dropped classes."""
    n_raw = n_cls if class_map is None else len(class_map)
    gt_b = np.full((FRAMES, n_gt, 4), -1.0, np.float32)
    gt_l = np.full((FRAMES, n_gt, 1), -1.0, np.float32)
    gt_d = np.zeros((FRAMES, n_gt, 1), np.float32)
    pr_b = np.full((FRAMES, n_pred, 4), -1.0, np.float32)
    pr_l = np.full((FRAMES, n_pred, 1), -1.0, np.float32)
    pr_s = np.full((FRAMES, n_pred, 1), -1.0, np.float32)
    for b in range(FRAMES):
        m = int(rng.integers(1, n_gt + 1))
        xy = rng.uniform(0, 300, (m, 2))
        wh = rng.uniform(20, 120, (m, 2))
        gt_b[b, :m] = np.round(np.concatenate([xy, xy + wh], 1) * 8) / 8
        gt_l[b, :m, 0] = rng.integers(0, n_raw, m)
        if difficult:
            gt_d[b, :m, 0] = rng.random(m) < 0.25
        if b == FRAMES - 1:
            if difficult:
                gt_d[b, :m, 0] = 1
            elif class_map is not None:
                gt_l[b, :m, 0] = rng.choice([i for i, v in enumerate(class_map) if v < 0], m)
        k = int(rng.integers(n_pred // 2, n_pred + 1))
        src = rng.integers(0, m, k)
        boxes = gt_b[b, src] + rng.normal(0, jitter, (k, 4))
        clutter = rng.random(k) < 0.3
        rb = rng.uniform(0, 300, (k, 2))
        boxes[clutter] = np.concatenate([rb, rb + rng.uniform(20, 120, (k, 2))], 1)[clutter]
        raw = gt_l[b, src, 0].copy()
        labels = raw if class_map is None else np.asarray(class_map, np.float64)[raw.astype(int)]
        flip = (rng.random(k) < 0.15) | (labels < 0)
        labels[flip] = rng.integers(0, n_cls, int(flip.sum()))
        pr_b[b, :k], pr_l[b, :k, 0] = np.round(boxes * 8) / 8, labels
        pr_s[b, :k, 0] = (rng.permutation(63)[:k] + 1) / 64.0
        assert len(np.unique(pr_s[b, :k, 0])) == k             # distinct within the frame
    return dict(pred_bboxes=pr_b, pred_labels=pr_l, pred_scores=pr_s, gt_bboxes=gt_b, gt_labels=gt_l, gt_difficults=gt_d)


def main():
    _install_stubs()
    from metrics.pascalvoc import VOCMApMetric
    rng = np.random.default_rng(20260451)
    specs = [dict(n_pred=40, n_gt=12, n_cls=4, difficult=True, class_map=None, jitter=6.0),
             dict(n_pred=40, n_gt=12, n_cls=4, difficult=False, class_map=None, jitter=6.0),
             dict(n_pred=24, n_gt=6, n_cls=3, difficult=True, class_map=None, jitter=20.0),
             dict(n_pred=10, n_gt=2, n_cls=2, difficult=False, class_map=None, jitter=6.0),
             dict(n_pred=40, n_gt=12, n_cls=4, difficult=True, class_map=DROPPING_MAP, jitter=6.0),
             dict(n_pred=30, n_gt=8, n_cls=4, difficult=False, class_map=DROPPING_MAP, jitter=10.0)]
    cases = []
    for spec in specs:
        n_raw = spec["n_cls"] if spec["class_map"] is None else len(spec["class_map"])
        names = ["class%d" % i for i in range(n_raw)]
        for _ in range(2):
            u = make_case(rng, **spec)
            metric = VOCMApMetric(iou_thresh=0.5, class_names=names, class_map=spec["class_map"])
            expected = []
            for b in range(FRAMES):
                metric.reset()
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore", RuntimeWarning)
                    metric.update(u["pred_bboxes"][b:b + 1], u["pred_labels"][b:b + 1], u["pred_scores"][b:b + 1],
                                  u["gt_bboxes"][b:b + 1], u["gt_labels"][b:b + 1],
                                  u["gt_difficults"][b:b + 1] if spec["difficult"] else None)
                    score = float(metric.get()[1][-1])
                expected.append(None if math.isnan(score) else score)
            cases.append(dict(spec=spec, class_names=names, iou_thresh=0.5,
                              inputs={k: v.tolist() for k, v in u.items()}, expected=expected))
    with open(os.path.join(HERE, "frame_map_golden.json"), "w") as f:
        json.dump(cases, f, separators=(",", ":"))
    scored = [e for c in cases for e in c["expected"]]
    print("wrote %d cases, %d frames, %d of them NaN" % (len(cases), len(scored), sum(e is None for e in scored)))


if __name__ == "__main__":
    main()
