"""The COCO bbox evaluation, loop for loop as pycocotools' COCOeval performs it (iouType 'bbox', useCats 1): _prepare,
computeIoU, evaluateImg, accumulate, summarize.  [UPSTREAM-RECALLED]: pycocotools cannot be run here, so this transcription
— dicts and lists, one (image, category, area range) cell at a time, nothing shared with the product's row-wise code — is
what videoyolo_amd.metrics.COCODetectionMetric is held to.

    evaluate(dataset, results) -> dict(precision, recall, stats, summary)

``dataset``: the COCO-style ground-truth dict (images, annotations, categories).  ``results``: a list of
{image_id, category_id, bbox [x, y, w, h], score} in append order.
"""
from collections import defaultdict

import numpy as np

IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(0, 1, 101)
MAX_DETS = [1, 10, 100]
AREA_RANGES = [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]
AREA_LABELS = ['all', 'small', 'medium', 'large']


def _by_score(scores):
    return [int(i) for i in np.argsort(-np.asarray(scores, np.float64), kind='mergesort')]


def _iou(d, g, crowd):
    w = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
    if w <= 0:
        w = 0.0
    h = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
    if h <= 0:
        h = 0.0
    i = w * h
    da, ga = d[2] * d[3], g[2] * g[3]
    u = da if crowd else da + ga - i
    return np.float64(i) / np.float64(u)


def _outside(area, rng):
    return area < rng[0] or area > rng[1]


def _prepare(dataset, results):
    img_ids = sorted(im['id'] for im in dataset['images'])
    cat_ids = sorted(c['id'] for c in dataset['categories'])
    img_set, cat_set = set(img_ids), set(cat_ids)
    gts, dts = defaultdict(list), defaultdict(list)
    for ann in dataset['annotations']:
        if ann['image_id'] in img_set and ann['category_id'] in cat_set:
            g = dict(ann)
            g['ignore'] = 1 if g.get('iscrowd', 0) else 0      # an 'ignore' key of the file is overwritten
            gts[g['image_id'], g['category_id']].append(g)
    for n, res in enumerate(results):
        d = dict(res)
        d['id'] = n + 1
        d['area'] = d['bbox'][2] * d['bbox'][3]
        d['iscrowd'] = 0
        if d['image_id'] in img_set and d['category_id'] in cat_set:
            dts[d['image_id'], d['category_id']].append(d)
    return img_ids, cat_ids, gts, dts


def _compute_iou(gt, dt, max_det):
    if len(gt) == 0 and len(dt) == 0:
        return []
    dt = [dt[i] for i in _by_score([d['score'] for d in dt])][:max_det]
    with np.errstate(divide='ignore', invalid='ignore'):
        return [[_iou(d['bbox'], g['bbox'], int(g['iscrowd'])) for g in gt] for d in dt]


def _evaluate_img(gt, dt, ious, rng, max_det, iou_thrs):
    if len(gt) == 0 and len(dt) == 0:
        return None
    ignore = [1 if g['ignore'] or _outside(g['area'], rng) else 0 for g in gt]
    gtind = [int(i) for i in np.argsort(ignore, kind='mergesort')]
    gt = [gt[i] for i in gtind]
    gt_ig = [ignore[i] for i in gtind]
    dt = [dt[i] for i in _by_score([d['score'] for d in dt])][:max_det]
    iscrowd = [int(g['iscrowd']) for g in gt]
    ious = [[row[i] for i in gtind] for row in ious]
    n_t, n_g, n_d = len(iou_thrs), len(gt), len(dt)
    gtm = [[0] * n_g for _ in range(n_t)]
    dtm = [[0] * n_d for _ in range(n_t)]
    dt_ig = [[0] * n_d for _ in range(n_t)]
    if n_g and n_d:
        for tind, t in enumerate(iou_thrs):
            for dind, d in enumerate(dt):
                iou = min([t, 1 - 1e-10])
                m = -1
                for gind in range(n_g):
                    if gtm[tind][gind] > 0 and not iscrowd[gind]:
                        continue
                    if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:
                        break
                    if ious[dind][gind] < iou:
                        continue
                    iou = ious[dind][gind]
                    m = gind
                if m == -1:
                    continue
                dt_ig[tind][dind] = gt_ig[m]
                dtm[tind][dind] = gt[m]['id']
                gtm[tind][m] = d['id']
    for tind in range(n_t):
        for dind, d in enumerate(dt):
            if dtm[tind][dind] == 0 and _outside(d['area'], rng):
                dt_ig[tind][dind] = 1
    return {'dtMatches': dtm, 'dtScores': [d['score'] for d in dt], 'gtIgnore': gt_ig, 'dtIgnore': dt_ig}


def _accumulate(eval_imgs, n_i, n_k, n_a, iou_thrs, rec_thrs, max_dets):
    n_t, n_r, n_m = len(iou_thrs), len(rec_thrs), len(max_dets)
    precision = -np.ones((n_t, n_r, n_k, n_a, n_m))
    recall = -np.ones((n_t, n_k, n_a, n_m))
    for k in range(n_k):
        for a in range(n_a):
            for m, max_det in enumerate(max_dets):
                cells = [eval_imgs[k][a][i] for i in range(n_i)]
                cells = [e for e in cells if e is not None]
                if len(cells) == 0:
                    continue
                scores = [s for e in cells for s in e['dtScores'][:max_det]]
                inds = _by_score(scores)
                gt_ig = [g for e in cells for g in e['gtIgnore']]
                npig = sum(1 for g in gt_ig if g == 0)
                if npig == 0:
                    continue
                for t in range(n_t):
                    dtm = [v for e in cells for v in e['dtMatches'][t][:max_det]]
                    dt_ig = [v for e in cells for v in e['dtIgnore'][t][:max_det]]
                    dtm, dt_ig = [dtm[i] for i in inds], [dt_ig[i] for i in inds]
                    tps = [1 if (v != 0 and not g) else 0 for v, g in zip(dtm, dt_ig)]
                    fps = [1 if (v == 0 and not g) else 0 for v, g in zip(dtm, dt_ig)]
                    tp = np.cumsum(tps).astype(dtype=float)
                    fp = np.cumsum(fps).astype(dtype=float)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((n_r,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr, q = pr.tolist(), q.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    where = np.searchsorted(rc, rec_thrs, side='left')
                    try:
                        for ri, pi in enumerate(where):
                            q[ri] = pr[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)
    return precision, recall


def _summarize(precision, recall, iou_thrs, max_dets, area_labels):
    lines = []

    def one(ap, iou_thr, area, max_det):
        template = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'
        title = 'Average Precision' if ap == 1 else 'Average Recall'
        kind = '(AP)' if ap == 1 else '(AR)'
        iou_str = '{:0.2f}:{:0.2f}'.format(iou_thrs[0], iou_thrs[-1]) if iou_thr is None else '{:0.2f}'.format(iou_thr)
        aind = [i for i, lab in enumerate(area_labels) if lab == area]
        mind = [i for i, md in enumerate(max_dets) if md == max_det]
        s = precision if ap == 1 else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == iou_thrs)[0]]
        s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
        mean = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        lines.append(template.format(title, kind, iou_str, area, max_det, mean))
        return mean

    last = max_dets[-1]
    stats = [one(1, None, 'all', last), one(1, .5, 'all', last), one(1, .75, 'all', last), one(1, None, 'small', last),
             one(1, None, 'medium', last), one(1, None, 'large', last), one(0, None, 'all', max_dets[0]),
             one(0, None, 'all', max_dets[1]), one(0, None, 'all', max_dets[2]), one(0, None, 'small', last),
             one(0, None, 'medium', last), one(0, None, 'large', last)]
    return np.array(stats, np.float64), '\n'.join(lines)


def evaluate(dataset, results, iou_thrs=IOU_THRS, rec_thrs=REC_THRS, max_dets=MAX_DETS, area_ranges=AREA_RANGES):
    iou_thrs, rec_thrs = np.asarray(iou_thrs, np.float64), np.asarray(rec_thrs, np.float64)
    img_ids, cat_ids, gts, dts = _prepare(dataset, results)
    eval_imgs = [[[None] * len(img_ids) for _ in area_ranges] for _ in cat_ids]
    for k, cat in enumerate(cat_ids):
        for i, img in enumerate(img_ids):
            gt, dt = gts[img, cat], dts[img, cat]
            ious = _compute_iou(gt, dt, max_dets[-1])
            for a, rng in enumerate(area_ranges):
                eval_imgs[k][a][i] = _evaluate_img(gt, dt, ious, rng, max_dets[-1], iou_thrs)
    precision, recall = _accumulate(eval_imgs, len(img_ids), len(cat_ids), len(area_ranges), iou_thrs, rec_thrs, max_dets)
    stats, summary = _summarize(precision, recall, iou_thrs, max_dets, AREA_LABELS[:len(area_ranges)])
    return {'precision': precision, 'recall': recall, 'stats': stats, 'summary': summary}
