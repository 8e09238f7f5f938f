"""Generates tests/golden/vid_metric_golden.json by running THE REFERENCE's own ImageNet-VID metric
(/root/reference/metrics/imgnetvid.py: VIDDetectionMetric.update / get, vid_eval_motion, calculate_ap) on small stand-in
datasets.

Runs only in the build container (needs /root/reference).  The reference's numeric body produces every expected value,
unmodified.  Three throw-away stand-ins make it run here:
  * the `mxnet` stub of make_voc_metric_golden.py (`mx.nd.NDArray` for isinstance checks, `mx.metric.EvalMetric` as base);
  * a proxy set as `metrics.imgnetvid.np`: numpy itself, except that `array` falls back to an object array for ragged lists
    (numpy >= 1.24 refuses them, imgnetvid.py:196,329) and that the removed alias `np.float` is `float` (:455,457);
  * a recorder wrapped round `calculate_ap` that stores each slice's tp_cell, fp_cell and npos before calling on.

Every case asserts that all its scores are distinct, within a frame and across frames: the reference's argsort leaves ties
to the sort's internals.  No case is left out.

    python tests/golden/make_vid_metric_golden.py
"""
import copy
import json
import os
import sys
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))


class _NumpyProxy(object):
    float = float

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def array(x, *args, **kwargs):
        try:
            return np.array(x, *args, **kwargs)
        except ValueError:
            out = np.empty(len(x), dtype=object)
            for i, v in enumerate(x):
                out[i] = v
            return out


def _install_stubs():
    mx = types.ModuleType("mxnet")
    mx.nd = types.ModuleType("mxnet.nd")
    mx.nd.NDArray = type("NDArray", (), {})
    mx.metric = types.ModuleType("mxnet.metric")

    class EvalMetric(object):
        def __init__(self, name, **kwargs):
            self.name = name
    mx.metric.EvalMetric = EvalMetric
    sys.modules.update({"mxnet": mx, "mxnet.nd": mx.nd, "mxnet.metric": mx.metric})
    sys.path.insert(0, REF)


class StandInDataset(object):
    """The four attributes the metric reads."""

    def __init__(self, sample_ids, labels, motion_ious, wn_classes, classes):
        self._sample_ids, self._labels = sample_ids, labels
        self.motion_ious, self.wn_classes, self.classes = motion_ious, wn_classes, classes

    def get_sample_ids(self):
        return self._sample_ids

    def get_label(self, i):
        return self._labels[i]


def _gt(boxes, classes):
    return np.concatenate([np.asarray(boxes, np.float64).reshape(-1, 4), np.asarray(classes, np.float64).reshape(-1, 1)], 1)


def random_case(rng, ids, n_cls, max_gt, max_det, det_classes=None, empty_gt=(), empty_det=(), crowd=None):
    """Integer ground-truth boxes (as annotations are), detections as float32 jittered copies plus clutter, -1 padded to
    max_det rows like the detector's output, with some scores below the 0.05 threshold."""
    labels, motion, frames = {}, {}, []
    n_det_cls = n_cls if det_classes is None else det_classes
    for i in ids:
        m = 0 if i in empty_gt else int(rng.integers(1, max_gt + 1))
        rows = max_det
        if crowd is not None and i == crowd[0]:
            m, rows = crowd[1], crowd[2]
        xy = rng.integers(0, 400, (m, 2))
        wh = rng.integers(8, 260, (m, 2))
        labels[i] = _gt(np.concatenate([xy, xy + wh - 1], 1), rng.integers(0, n_cls, m))
        mo = np.round(rng.random(m), 3)
        mo[rng.random(m) < 0.15] = 0.7
        mo[rng.random(m) < 0.15] = 0.9
        mo[rng.random(m) < 0.1] = 1.0
        motion[str(i)] = [float(v) for v in mo]
        k = 0 if i in empty_det else (rows if rows != max_det else int(rng.integers(1, max_det + 1)))
        b = np.full((rows, 4), -1.0, np.float32)
        l = np.full((rows,), -1.0, np.float32)
        s = np.full((rows,), -1.0, np.float32)
        if k:
            if m:
                src = rng.integers(0, m, k)
                boxes = labels[i][src, :4] + rng.normal(0, 5.0, (k, 4))
                cls = labels[i][src, 4].copy() % n_det_cls
            else:
                boxes, cls = np.zeros((k, 4)), np.zeros(k)
            clutter = (rng.random(k) < 0.3) | (m == 0)
            rb = rng.uniform(0, 400, (k, 2))
            boxes[clutter] = np.concatenate([rb, rb + rng.uniform(8, 260, (k, 2))], 1)[clutter]
            flip = rng.random(k) < 0.15
            cls[flip] = rng.integers(0, n_det_cls, int(flip.sum()))
            sc = rng.random(k)
            if rows == max_det:
                sc[rng.random(k) < 0.1] *= 0.05   # below conf_score_thresh
            else:
                sc = 0.06 + 0.94 * sc             # the crowded frame keeps all its rows
            b[:k], l[:k], s[:k] = boxes, cls, sc
        frames.append(dict(sid=i, boxes=b, labels=l, scores=s))
    return labels, motion, frames


def edge_case():
    """Hand-built integer boxes, one situation per frame.  Classes 0..2."""
    labels, motion, frames = {}, {}, []

    def frame(i, gts, mo, dets):
        labels[i] = _gt([g[:4] for g in gts], [g[4] for g in gts]) if gts else np.zeros((0, 5))
        motion[str(i)] = list(mo)
        d = np.asarray(dets, np.float32).reshape(-1, 6)
        frames.append(dict(sid=i, boxes=d[:, :4].copy(), labels=d[:, 4].copy(), scores=d[:, 5].copy()))

    # ov == thr exactly: ground truth 100 x 100, detection its upper half: ov = 5000 / 10000 = 0.5 = thr
    frame(0, [[0, 0, 99, 99, 0]], [0.5], [[0, 0, 99, 49, 0, 0.91]])
    # two detections on one ground truth: the second is a miss
    frame(1, [[10, 10, 109, 109, 1]], [0.8], [[10, 10, 109, 109, 1, 0.92], [12, 12, 111, 111, 1, 0.83]])
    # one detection overlapping two ground truths equally: the lower index wins; the next one takes the other
    # (ov = 9000 / 11000 with both)
    frame(2, [[0, 0, 99, 99, 2], [20, 0, 119, 99, 2]], [0.95, 0.3],
          [[10, 0, 109, 99, 2, 0.94], [10, 0, 109, 99, 2, 0.74]])
    # a small object: 10 x 10 gives thr = 100 / 400 = 0.25; the detection's ov = 60 / 140 = 0.43 is below 0.5 and matches
    frame(3, [[200, 200, 209, 209, 0]], [0.75], [[200, 200, 209, 205, 0, 0.88], [300, 300, 309, 309, 0, 0.52]])
    # areas on the range ends: 50 x 50 = 2500 and 150 x 150 = 22500, ground truths and detections
    frame(4, [[0, 0, 49, 49, 1], [100, 100, 249, 249, 1]], [0.7, 0.9],
          [[0, 0, 49, 49, 1, 0.97], [100, 100, 249, 249, 1, 0.96], [300, 0, 349, 49, 1, 0.41], [300, 100, 449, 249, 1, 0.42]])
    # motion IoU on the range ends, same label, overlapping boxes, and a wrong-label detection on top
    frame(5, [[0, 0, 199, 199, 2], [20, 20, 219, 219, 2]], [0.9, 0.7],
          [[0, 0, 199, 199, 2, 0.81], [20, 20, 219, 219, 2, 0.79], [10, 10, 209, 209, 0, 0.78]])
    # no ground truth at all: empty_weight
    frame(6, [], [], [[5, 5, 80, 80, 0, 0.67], [0, 0, 30, 30, 1, 0.31]])
    # no detections: padding only, and a row below the score threshold
    frame(7, [[30, 30, 90, 90, 0]], [0.2], [[-1, -1, -1, -1, -1, -1], [30, 30, 90, 90, 0, 0.01]])
    return labels, motion, frames


def run_case(name, labels, motion, frames, wn_classes, sample_ids=None, **kwargs):
    import metrics.imgnetvid as ref
    ids = [f["sid"] for f in frames]
    sample_ids = ids if sample_ids is None else sample_ids
    classes = ["class_%s" % c for c in wn_classes]
    ds = StandInDataset(sample_ids, labels, motion, wn_classes, classes)

    kept = np.concatenate([f["scores"][(f["labels"] >= 0) & (f["scores"].astype(np.float64) >= 0.05)] for f in frames])
    assert len(kept) and len(np.unique(kept)) == len(kept), "%s: equal scores" % name

    recorded = []
    real = ref.calculate_ap

    def recorder(tp_cell, fp_cell, gt_img_ids, obj_labels_cell, obj_confs_cell, classname_map, npos, class_map=None):
        recorded.append(dict(tp=copy.deepcopy(tp_cell), fp=copy.deepcopy(fp_cell), labels=copy.deepcopy(obj_labels_cell),
                             confs=copy.deepcopy(obj_confs_cell), ids=list(gt_img_ids), npos=[float(v) for v in npos]))
        return real(tp_cell, fp_cell, gt_img_ids, obj_labels_cell, obj_confs_cell, classname_map, npos, class_map)

    ref.calculate_ap = recorder
    try:
        m = ref.VIDDetectionMetric(ds, **kwargs)
        for f in frames:
            m.update(f["boxes"][None], f["labels"][None], f["scores"][None], None, None, None, sid=f["sid"])
        ap = ref.vid_eval_motion(ds, m._results, m._motion_ranges, m._area_ranges, iou_threshold=m._iou_thresh,
                                 class_map=m._class_map, agnostic=m._agnostic, offset=m._offset)
        first = recorded[:]
        names, values = m.get()
    finally:
        ref.calculate_ap = real
    assert len(first) == 16 and len(recorded) == 32

    def flat(cells, order, dtype):
        parts = [np.asarray(cells[i]) for i in order if cells[i] is not None and len(cells[i])]
        return np.concatenate(parts).astype(dtype).tolist() if parts else []

    order = first[0]["ids"]
    # frames without detections have labels None and tp zeros(0): both drop out
    with_dets = [i for i in order if first[0]["labels"][i] is not None]
    slices = [dict(tp=flat(r["tp"], with_dets, np.int64), fp=flat(r["fp"], with_dets, np.float64), npos=r["npos"])
              for r in first]
    return dict(name=name, kwargs=kwargs,
                dataset=dict(sample_ids=sample_ids, wn_classes=list(wn_classes), classes=classes,
                             labels={str(k): v.tolist() for k, v in labels.items()}, motion_ious=motion),
                frames=[dict(sid=f["sid"], boxes=f["boxes"].astype(np.float64).tolist(),
                             labels=f["labels"].astype(np.float64).tolist(),
                             scores=f["scores"].astype(np.float64).tolist()) for f in frames],
                expected=dict(order=[int(i) for i in with_dets], det_labels=flat(first[0]["labels"], with_dets, np.int64),
                              det_scores=flat(first[0]["confs"], with_dets, np.float64), slices=slices,
                              ap=np.asarray(ap).tolist(), names=names, values=values))


def main():
    _install_stubs()
    import metrics.imgnetvid as ref
    ref.np = _NumpyProxy()
    rng = np.random.default_rng(20260917)
    cases = []
    wn6 = ["n%02d" % c for c in range(6)]

    ids = [11, 3, 7, 0, 5, 2, 9, 14, 4, 8, 1, 6]           # the dataset's order, not sorted
    lab, mo, fr = random_case(rng, ids, 6, 4, 20, empty_gt=(7, 14), empty_det=(5, 14))
    cases.append(run_case("random", lab, mo, fr, wn6))
    cases.append(run_case("random_iou75_conf30", lab, mo, fr, wn6, iou_thresh=0.75, conf_score_thresh=0.3))

    lab, mo, fr = random_case(rng, [0, 1, 2], 5, 6, 30, crowd=(1, 70, 100))
    cases.append(run_case("crowd_70gt_100det", lab, mo, fr, wn6[:5]))

    lab, mo, fr = edge_case()
    cases.append(run_case("edges", lab, mo, fr, wn6[:3]))

    # class maps: dataset class -> model class, -1 drops it.  One drops the last dataset class, one a middle one only.
    ids = list(range(10))
    lab, mo, fr = random_case(rng, ids, 6, 5, 20, det_classes=4, empty_gt=(4,), empty_det=(8,))
    cases.append(run_case("class_map_drops_last", lab, mo, fr, wn6, class_map=[0, 2, -1, 1, 3, -1]))
    cases.append(run_case("class_map_drops_middle", lab, mo, fr, wn6, class_map=[3, -1, 0, 1, 1, 2]))

    lab, mo, fr = random_case(rng, ids, 6, 4, 20, empty_gt=(2,), empty_det=(3,))
    cases.append(run_case("agnostic", lab, mo, fr, wn6, agnostic=True))
    cases.append(run_case("agnostic_class_map", lab, mo, fr, wn6, agnostic=True, class_map=[0, 0, -1, 0, 0, 0]))

    # offset-style ids: [video, frame, id at offset 0, id at offset 1]
    lab, mo, fr = random_case(rng, [20, 21, 22, 23, 24], 6, 4, 20, empty_gt=(22,))
    cases.append(run_case("offset_list_ids", lab, mo, fr, wn6, sample_ids=[[0, j, 20 + j, 99] for j in range(5)], offset=0))

    path = os.path.join(HERE, "vid_metric_golden.json")
    with open(path, "w") as f:
        json.dump(cases, f)
    print("wrote %d cases, %d bytes" % (len(cases), os.path.getsize(path)))


if __name__ == "__main__":
    main()
