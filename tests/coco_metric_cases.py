"""Shared by the COCO metric's host and GPU tests: a stand-in dataset, the issue's known-answer cases and seeded sets that
carry every constructed condition of the rule (crowds, areas on the range ends, IoUs exactly on thresholds, score ties, an
annotation id 0, more than 100 rows of a category, empty images, unmapped labels, data_shape)."""
import json
import os
import tempfile

import numpy as np

import coco_eval_ref as REF

U = 0.9999999999999998
V = 0.9999999999999999


class Dataset(object):
    """What COCODetectionMetric reads of a dataset: sample_ids, classes, image_size, build_coco_json (or .coco.dataset),
    optionally contiguous_id_to_json."""

    def __init__(self, images, annotations, cat_ids, sizes=None, id_map=None, as_file=False):
        self.data = {'images': [{'id': i} for i in images], 'annotations': annotations,
                     'categories': [{'id': c, 'name': 'c%d' % c} for c in cat_ids]}
        self.sample_ids = list(images)
        self.classes = ['c%d' % c for c in sorted(cat_ids)]
        self._sizes = sizes or {}
        if id_map is not None:
            self.contiguous_id_to_json = dict(id_map)
        self.json_path = None
        if not as_file:
            self.coco = type('Coco', (), {'dataset': self.data})()

    def image_size(self, i):
        return self._sizes[i]

    def build_coco_json(self):
        fd, self.json_path = tempfile.mkstemp(suffix='.json')
        with os.fdopen(fd, 'w') as f:
            json.dump(self.data, f)
        return self.json_path


def ann(img, cat, box, idx, crowd=0, area=None):
    return {'image_id': img, 'category_id': cat, 'bbox': [float(v) for v in box], 'id': idx, 'iscrowd': crowd,
            'area': float(box[2] * box[3] if area is None else area)}


def corners(box):
    """xywh -> the corner row whose w = x2 - (x1 - 1) gives the box back."""
    x, y, w, h = box
    return [x, y, x + w - 1, y + h - 1]


B40 = [0, 0, 40, 40]


def known_cases():
    """name -> (n_images, n_cats, gts [(img, cat, xywh, id, crowd)], dets [(img, cat, xywh, score)], {stat index: value})"""
    full = lambda v: dict(enumerate(v))   # noqa: E731
    cases = {
        'A': (1, 1, [(0, 0, [10, 10, 20, 20], 1, 0)], [(0, 0, [10, 10, 20, 20], .9)],
              full([U, V, V, U, -1, -1, 1, 1, 1, 1, -1, -1])),
        'B': (1, 1, [(0, 0, [10, 10, 20, 20], 1, 0)], [(0, 0, [100, 100, 20, 20], .9), (0, 0, [10, 10, 20, 20], .8)],
              full([.5, .5, .5, .5, -1, -1, 0, 1, 1, 1, -1, -1])),
        'E': (1, 1, [(0, 0, [10, 10, 20, 20], 0, 0)], [(0, 0, [10, 10, 20, 20], .9)],
              full([0, 0, 0, 0, -1, -1, 0, 0, 0, 0, -1, -1])),
        'D': (1, 1, [(0, 0, [0, 0, 100, 100], 1, 1), (0, 0, [200, 200, 40, 40], 2, 0)],
              [(0, 0, [10, 10, 20, 20], .9), (0, 0, [30, 30, 20, 20], .8), (0, 0, [200, 200, 40, 40], .7),
               (0, 0, [400, 400, 40, 40], .6)], full([U, V, V, -1, U, -1, 0, 1, 1, -1, 1, -1])),
        'G': (1, 1, [(0, 0, [0, 0, 32, 32], 1, 0)], [(0, 0, [0, 0, 32, 32], .9)],
              full([U, V, V, U, U, -1, 1, 1, 1, 1, 1, -1])),
        'G2': (1, 1, [(0, 0, B40, 1, 0)], [(0, 0, [500, 500, 10, 10], .9), (0, 0, B40, .5)],
               full([.5, .5, .5, -1, U, -1, 0, 1, 1, -1, 1, -1])),
        'H_miss_first': (1, 1, [(0, 0, B40, 1, 0)], [(0, 0, [500, 500, 40, 40], .5), (0, 0, B40, .5)],
                         full([.5, .5, .5, -1, .5, -1, 0, 1, 1, -1, 1, -1])),
        'H_hit_first': (1, 1, [(0, 0, B40, 1, 0)], [(0, 0, B40, .5), (0, 0, [500, 500, 40, 40], .5)],
                        full([U, V, V, -1, U, -1, 1, 1, 1, -1, 1, -1])),
        'I': (1, 1, [(0, 0, B40, 1, 0), (0, 0, [10, 0, 40, 40], 2, 0)], [(0, 0, [8, 0, 40, 40], .9), (0, 0, B40, .8)],
              {0: 0.9252475247524753, 1: 1, 6: .45, 7: .95}),
        'J': (2, 2, [(0, 0, B40, 1, 0), (1, 0, B40, 2, 0), (1, 1, B40, 3, 0)], [(0, 0, B40, .9)],
              {0: 0.2524752475247524, 6: .25, 7: .25, 8: .25}),
        'F': (2, 2, [(0, 0, B40, 1, 0), (0, 0, [100, 0, 40, 40], 2, 0), (1, 0, [0, 0, 120, 120], 3, 0),
                     (1, 1, [0, 0, 50, 50], 4, 0)],
              [(0, 0, B40, .9), (0, 0, [100, 0, 40, 36], .8), (0, 0, [300, 300, 40, 40], .95), (1, 0, [0, 0, 120, 100], .5),
               (1, 1, [5, 0, 50, 50], .4), (1, 1, [300, 0, 20, 20], .3)],
              full([0.6651402640264026, .875, .875, -1, 0.6626237623762375, 0.6999999999999998, 0.4666666666666666,
                    0.7833333333333333, 0.7833333333333333, -1, .825, .7])),
    }
    for h, ap in ((5, 0.09999999999999999), (6, 0.29999999999999993), (7, 0.49999999999999994), (8, 0.6999999999999998),
                  (9, 0.8999999999999999)):
        cases['C%d' % h] = (1, 1, [(0, 0, [0, 0, 10, 10], 1, 0)], [(0, 0, [0, 0, 10, h], .9)], {0: ap})
    return cases


def build_case(case, as_file=False):
    """(dataset, results list for coco_eval_ref, (boxes, labels, scores) float64 arrays (images, rows, ..) for update)"""
    n_images, n_cats, gts, dets, _ = case
    ds = Dataset(list(range(n_images)), [ann(*g) for g in gts], list(range(n_cats)), as_file=as_file)
    results = [{'image_id': i, 'category_id': c, 'bbox': [float(v) for v in b], 'score': s} for i, c, b, s in dets]
    rows = max(max([sum(1 for d in dets if d[0] == i) for i in range(n_images)]), 1)
    boxes, labels = np.full((n_images, rows, 4), -1.0), np.full((n_images, rows), -1.0)
    scores = np.full((n_images, rows), -1.0)
    for i in range(n_images):
        for r, d in enumerate([d for d in dets if d[0] == i]):
            boxes[i, r], labels[i, r], scores[i, r] = corners(d[2]), d[1], d[3]
    return ds, results, (boxes, labels, scores)


def results_of(ds, arrays, score_thresh=0.05, data_shape=None):
    """The reference's update (metrics/mscoco.py:190-225), row by row: the results list COCOeval would load."""
    boxes, labels, scores = arrays
    ids = sorted(ds.sample_ids)
    out = []
    for b in range(len(boxes)):
        ws, hs = 1.0, 1.0
        if data_shape is not None:
            ow, oh = ds.image_size(ids[b])
            hs, ws = float(oh) / data_shape[0], float(ow) / data_shape[1]
        for box, label, score in zip(boxes[b].astype(np.float64), labels[b].reshape(-1), scores[b].reshape(-1).astype(np.float64)):
            if not label >= 0:
                continue
            label = int(label)
            if hasattr(ds, 'contiguous_id_to_json'):
                if label not in ds.contiguous_id_to_json:
                    continue
                label = ds.contiguous_id_to_json[label]
            if score < score_thresh:
                continue
            box = box.copy()
            box[[0, 2]] *= ws
            box[[1, 3]] *= hs
            box[2:4] -= (box[:2] - 1)
            out.append({'image_id': ids[b], 'category_id': label, 'bbox': box.tolist(), 'score': float(score)})
    return out


def seeded_set(seed, n_images, rows, n_gt, n_cats, use_map=True, data_shape=None, as_file=False):
    """A dataset and float32 prediction arrays (images, rows, 4), (images, rows), (images, rows) built to carry every
    condition of the rule.  Boxes lie on a grid of 8 with sides 8..128 (areas 1024 and 9216 among them), detections are
    ground truths kept whole, cut to a half or three quarters of their height (IoU exactly 0.5 and 0.75), shifted, or
    clutter; scores are twentieths.  Image 1 has no ground truth and image 2 no detection (when there are that many);
    image 0 gives its first 120 rows to one category when rows allow.  Annotation ids count from 0.  With data_shape the
    images are 0.5x, 1x or 2x that shape."""
    rng = np.random.default_rng(seed)
    json_of = (lambda c: 2 * c + 1) if use_map else (lambda c: c)     # noqa: E731
    cat_ids = [json_of(c) for c in range(n_cats)]
    sides = np.array([8, 16, 32, 64, 96, 128])
    anns, per_image = [], []
    for i in range(n_images):
        n = 0 if (i == 1 and n_images > 1) else n_gt
        xy = 8 * rng.integers(0, 40, (n, 2))
        wh = sides[rng.integers(0, len(sides), (n, 2))]
        wh[: n // 4, 1] = wh[: n // 4, 0]                        # squares: 32 x 32 and 96 x 96 sit on the range ends
        cats = rng.integers(0, n_cats, n)
        if i == 0:
            cats[: max(1, n // 3)] = 0
        crowd = rng.random(n) < 0.15
        per_image.append((np.concatenate([xy, wh], 1), cats))
        for g in range(n):
            anns.append(ann(i, json_of(int(cats[g])), np.concatenate([xy[g], wh[g]]), len(anns), int(crowd[g])))
    scale = {}
    sizes = {}
    for i in range(n_images):
        s = (0.5, 1.0, 2.0)[i % 3] if data_shape is not None else 1.0
        scale[i] = s
        if data_shape is not None:
            sizes[i] = (int(data_shape[1] * s), int(data_shape[0] * s))
    id_map = {c: json_of(c) for c in range(n_cats)} if use_map else None
    ds = Dataset(list(range(n_images)), anns, cat_ids, sizes, id_map, as_file)
    boxes = np.zeros((n_images, rows, 4))
    labels = np.full((n_images, rows), -1.0)
    scores = np.zeros((n_images, rows))
    for i in range(n_images):
        g_box, g_cat = per_image[i]
        for r in range(rows):
            kind = rng.integers(0, 6)
            if len(g_box) and kind < 4:
                g = rng.integers(0, len(g_box))
                x, y, w, h = g_box[g]
                cat = g_cat[g]
                if kind == 1:
                    h = h // 2
                elif kind == 2:
                    h = 3 * h // 4
                elif kind == 3:
                    x = x + 8 * rng.integers(-1, 2)
            else:
                x, y = 8 * rng.integers(0, 40, 2)
                w, h = sides[rng.integers(0, len(sides), 2)]
                cat = rng.integers(0, n_cats + 1)                # n_cats: a label the dataset does not have
            if i == 0 and r < 120 and rows > 120:
                cat = 0
            boxes[i, r] = np.array(corners([x, y, w, h])) / scale[i]
            labels[i, r] = cat
            scores[i, r] = rng.integers(0, 21) / 20.0
        pad = rng.random(rows) < 0.1
        if i == 2 and n_images > 2:
            pad[:] = True
        labels[i, pad], scores[i, pad], boxes[i, pad] = -1, -1, -1
    f = np.float32
    return ds, (boxes.astype(f), labels.astype(f), scores.astype(f))


def conditions(ds, arrays, data_shape=None):
    """Which constructed conditions a seeded set really carries, counted from its results and ground truths."""
    res = results_of(ds, arrays, data_shape=data_shape)
    anns = ds.data['annotations']
    cats = set(c['id'] for c in ds.data['categories'])
    by_cell = {}
    for d in res:
        by_cell.setdefault((d['image_id'], d['category_id']), []).append(d)
    ious = set()
    for g in anns:
        for d in by_cell.get((g['image_id'], g['category_id']), []):
            ious.add(float(REF._iou(d['bbox'], g['bbox'], g['iscrowd'])))
    scores = [d['score'] for d in res]
    labels = arrays[1]
    with_dets = set(d['image_id'] for d in res)
    with_gts = set(g['image_id'] for g in anns)
    tie_inside = any(len(set(d['score'] for d in cell)) < len(cell) for cell in by_cell.values())
    return {
        'crowd': any(g['iscrowd'] for g in anns), 'area_1024': any(g['area'] == 1024 for g in anns),
        'area_9216': any(g['area'] == 9216 for g in anns), 'iou_0.5': 0.5 in ious, 'iou_0.75': 0.75 in ious,
        'tie_inside': tie_inside, 'tie_across': len(set(scores)) < len(scores), 'id_0': any(g['id'] == 0 for g in anns),
        'over_100': any(len(cell) > 100 for cell in by_cell.values()),
        'no_dets': len(with_dets) < len(ds.sample_ids), 'no_gts': len(with_gts) < len(ds.sample_ids),
        'unknown_label': bool((labels >= len(cats)).any()), 'dropped_score': bool(((labels >= 0) & (arrays[2] < 0.05)).any()),
    }
