"""PASCAL-VOC detection mAP for the detector's outputs.

Host-side mirror (numpy, like the reference) of ``VOCMApMetric`` — the area-under-curve AP both
drivers instantiate (train_yolov3.py:181, detect_yolo3.py:183) — and ``VOC07MApMetric`` (11-point AP),
metrics/pascalvoc.py:12-259,523-560 in /root/reference.  Same ``update(pred_bboxes, pred_labels,
pred_scores, gt_bboxes, gt_labels, gt_difficults)`` / ``get()`` / ``reset()`` contract and the same
conventions: label < 0 rows are padding, difficult ground truths are ignored (neither TP nor FP), a
ground truth can be matched once, IoU without the +1 pixel offset, classes with no ground truth give
NaN.  Unlike the hot path this row IS pinned by the reference itself: tests/golden/voc_metric_*.json
were produced by running the reference's own class (mxnet stubbed out) — see
tests/golden/make_voc_metric_golden.py.

Accepts numpy arrays, torch tensors (any device) or lists of them (one per device, concatenated
along the batch axis like utils/general.py:6-17 ``as_numpy``).  float32 tensors on a GPU are matched there
(``voc_match_host`` states the rule, csrc/voc_metric.hip applies it) and copied once, by ``get()``.

After them: the per-frame mean AP and the worst-clip ranking (``frame_map_host``, ``FrameMApMetric``), scored on the
device from the same match.

Further down: the ImageNet-VID motion / area mAP (``VIDDetectionMetric``) and the COCO detection metric
(``COCODetectionMetric``), each with its matching rule stated on the host and applied on the device the same way.
"""
import ctypes

import numpy as np


def _to_numpy(a):
    if isinstance(a, (list, tuple)):
        parts = [_to_numpy(x) for x in a]
        try:
            return np.concatenate(parts, axis=0)
        except ValueError:
            return np.array(parts)
    if hasattr(a, "detach"):  # torch tensor
        return a.detach().cpu().numpy()
    return np.asarray(a)


def pairwise_iou(a, b):
    """IoU of every box of a (N,4) with every box of b (M,4), corner format, no +1 offset."""
    lo = np.maximum(a[:, None, :2], b[None, :, :2])
    hi = np.minimum(a[:, None, 2:4], b[None, :, 2:4])
    inter = np.prod(hi - lo, axis=2) * (lo < hi).all(axis=2)
    area_a = np.prod(a[:, 2:4] - a[:, :2], axis=1)
    area_b = np.prod(b[:, 2:4] - b[:, :2], axis=1)
    return inter / (area_a[:, None] + area_b[None, :] - inter)


def voc_match_host(boxes, labels, scores, gt_boxes, gt_labels, gt_difficults, iou_thresh, return_best=False):
    """The matching rule of the VOC metric for ONE image, row by row: ``VOCMApMetric._update_image`` restated per input
    row, and the definition the device kernel (csrc/voc_metric.hip, vy_voc_match) is held to, value for value.

    boxes (R, 4), labels (R), scores (R): the image's rows in any order, label < 0 = padding.  gt_boxes (M, 4), gt_labels
    (M) already class-mapped, gt_difficults (M) or None.  Returns one int8 per row, in row order: 1 true positive, 0 false
    positive, -1 ignored (matched a difficult ground truth), -2 not a detection (label < 0); with ``return_best`` also the
    candidate of every row, an index into the M ground truths given, or -1.

      rows kept: ground truths with label >= 0
      candidate: g = argmax of pairwise_iou over the kept ground truths of the row's own label; the first index wins a
        tie, a NaN IoU counts as the maximum (np.argmax); g = -1 when that maximum < iou_thresh, which is false for NaN
      flag: g < 0 gives 0; a difficult g gives -1; else 1 if no row of the image with the same g comes before this one,
        0 if one does.  Before = a higher score; at equal scores the lower row (``_update_image`` leaves equal scores to
        an unstable argsort).
      dtype: the arithmetic runs in the arrays' own dtype, as pairwise_iou does; iou_thresh is rounded to that dtype.
    """
    boxes, gt_boxes = np.asarray(boxes).reshape(-1, 4), np.asarray(gt_boxes).reshape(-1, 4)
    labels, scores = np.asarray(labels).reshape(-1), np.asarray(scores).reshape(-1)
    gt_labels = np.asarray(gt_labels).reshape(-1)
    gdiff = np.zeros(len(gt_labels), bool) if gt_difficults is None else np.asarray(gt_difficults).reshape(-1) != 0
    flags = np.full(len(labels), -2, np.int8)
    best = np.full(len(labels), -1, np.int64)
    det = np.flatnonzero(labels >= 0)
    flags[det] = 0
    dl = labels[det].astype(int)
    gkeep = np.flatnonzero(gt_labels >= 0)
    gl = gt_labels[gkeep].astype(int)
    for c in np.unique(dl):
        rows, gts = det[dl == c], gkeep[gl == c]
        if len(gts) == 0:
            continue
        with np.errstate(divide='ignore', invalid='ignore'):
            iou = pairwise_iou(boxes[rows], gt_boxes[gts])
        g = iou.argmax(axis=1)
        g[iou.max(axis=1) < iou.dtype.type(iou_thresh)] = -1
        best[rows] = np.where(g >= 0, gts[g], -1)
    hit = np.flatnonzero(best >= 0)
    flags[hit[gdiff[best[hit]]]] = -1
    claim = hit[~gdiff[best[hit]]]
    claim = claim[np.lexsort((claim, -scores[claim].astype(np.float64)))]   # before first: higher score, then lower row
    first = claim[np.unique(best[claim], return_index=True)[1]]              # the first claimant of every ground truth
    flags[first] = 1
    return (flags, best) if return_best else flags


def _is_gpu_f32(t):
    import torch
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32


# what the three device paths below share: a list of per-device tensors joined along the batch on the first one's device
def _gather(x):
    if isinstance(x, (list, tuple)) and len(x) and all(hasattr(t, "is_cuda") for t in x):
        import torch
        return torch.cat([t.to(x[0].device) for t in x], 0)
    return x


def _upload(cache, dev, **arrays):
    """The named numpy arrays as tensors on dev, once per device (cache); an empty one padded to one element: a valid pointer."""
    t = cache.get(dev)
    if t is None:
        import torch
        pad = lambda a: a if a.size else np.zeros((1,) + a.shape[1:], a.dtype)  # noqa: E731
        t = cache[dev] = {n: torch.from_numpy(pad(a)).to(dev) for n, a in arrays.items()}
    return t


# ctypes arguments of the vy_*_match entries: a device tensor's pointer, a host array's, a device's current stream
def _devp(t):
    return ctypes.c_void_p(t.data_ptr())


def _hostp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _streamp(dev):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _chunks_to_host(chunks):
    """``chunks``: one tuple of tensors per update, the same kinds at each position.  Returns the same structure as numpy
    arrays of the tensors' shapes, after ONE copy to the host: every tensor goes to the first chunk's device and is viewed
    as bytes, the bytes are joined kind by kind and split back on the host."""
    if not chunks:
        return []
    import torch
    dev = chunks[0][0].device
    # kind by kind, the widest item size first: every host view below is aligned
    kinds = sorted(range(len(chunks[0])), key=lambda k: -chunks[0][k].element_size())
    raw = torch.cat([torch.cat([c[k].to(dev).reshape(-1) for c in chunks]).view(torch.uint8) for k in kinds]).cpu().numpy()
    host, at = [[None] * len(c) for c in chunks], 0
    for k in kinds:
        dtype = torch.empty(0, dtype=chunks[0][k].dtype).numpy().dtype
        for i, c in enumerate(chunks):
            size = c[k].numel() * dtype.itemsize
            host[i][k] = raw[at:at + size].view(dtype).reshape(tuple(c[k].shape))
            at += size
    return [tuple(h) for h in host]


class _VocDeviceBatch(object):
    """A batch the VOC matching accepts on the device, as vy_voc_match takes it: contiguous tensors of one GPU."""
    __slots__ = ("dev", "batch", "rows", "n_gt", "boxes", "labels", "scores", "gt_boxes", "mapped", "diff")


def _voc_device_batch(class_map, luts, pred_bboxes, pred_labels, pred_scores, gt_bboxes, gt_labels, gt_difficults):
    """The acceptance test of the VOC metrics' device path (VOCMApMetric, FrameMApMetric): float32 tensors of one GPU
    (predictions and ground-truth boxes; labels and difficults of any numeric dtype there), at most VY_VOC_ROWS_MAX rows
    per image, ``class_map`` None or a sequence.  Returns the batch ready for the kernels — ground-truth labels through
    the class map (``luts``: its upload per device), difficults as bytes — or None: the call is the host path's."""
    cm = class_map
    if not (cm is None or isinstance(cm, (list, tuple, np.ndarray))):
        return None
    args = [_gather(x) for x in (pred_bboxes, pred_labels, pred_scores, gt_bboxes, gt_labels, gt_difficults)]
    if not all(hasattr(x, "is_cuda") for x in args[:5]):
        return None
    import torch
    pb, pl, ps, gb, gl, gd = args
    if not all(_is_gpu_f32(x) for x in (pb, pl, ps, gb)):
        return None
    others = [gl] if gd is None else [gl, gd]
    if not all(isinstance(x, torch.Tensor) and not x.is_complex() for x in others):
        return None
    dev = pb.device
    if any(x.device != dev for x in (pl, ps, gb) + tuple(others)):
        return None
    from . import _lib
    batch = int(pb.shape[0])
    rows = int(np.prod(pl.shape[1:])) if batch else 0
    n_gt = int(np.prod(gl.shape[1:])) if batch else 0
    if rows > _lib.VY_VOC_ROWS_MAX or pb.numel() != batch * rows * 4 or ps.numel() != batch * rows or \
            gb.numel() != batch * n_gt * 4 or gl.shape[0] != batch or (gd is not None and gd.numel() != batch * n_gt):
        return None
    d = _VocDeviceBatch()
    d.dev, d.batch, d.rows, d.n_gt = dev, batch, rows, n_gt
    d.boxes = d.labels = d.scores = d.gt_boxes = d.mapped = d.diff = None
    if batch == 0:
        return d
    gl = gl.reshape(batch, n_gt)
    if cm is None:
        mapped = torch.where(gl >= 0, gl.to(torch.int32), -1)
    else:
        lut = luts.get(dev)
        if lut is None:
            lut = luts[dev] = torch.tensor([int(v) for v in cm], dtype=torch.int32).to(dev)
        n = len(lut)
        idx = gl.to(torch.int64)                                  # a negative label counts from the end, as on the host
        inside = (idx >= -n) & (idx < n)
        if n:
            mapped = torch.where(inside, lut[torch.where(inside, idx, 0)], -1)
        else:
            mapped = torch.full_like(idx, -1, dtype=torch.int32)
    d.mapped = mapped.contiguous()
    d.diff = None if gd is None else (gd.reshape(batch, n_gt) != 0).to(torch.uint8).contiguous()
    d.labels, d.scores = pl.reshape(batch, rows).contiguous(), ps.reshape(batch, rows).contiguous()
    d.boxes, d.gt_boxes = pb.reshape(batch, rows, 4).contiguous(), gb.reshape(batch, n_gt, 4).contiguous()
    return d


def _voc_match_device(d, iou_thresh):
    """vy_voc_match on an accepted batch, on the current stream: the (batch, rows) int8 flags, a device tensor.  No rows:
    no launch."""
    import torch
    flags = torch.empty((d.batch, d.rows), dtype=torch.int8, device=d.dev)
    if d.rows:
        from . import _lib
        lib = _lib.load()
        best = torch.empty((d.batch, d.rows), dtype=torch.int32, device=d.dev)
        devp = lambda t: _devp(t if t.numel() else best)          # noqa: E731  a valid address for arrays without elements
        with torch.cuda.device(d.dev):
            _lib.check(lib.vy_voc_match(d.batch, d.rows, d.n_gt, devp(d.boxes), devp(d.labels), devp(d.scores),
                                        devp(d.gt_boxes), devp(d.mapped), None if d.diff is None else devp(d.diff),
                                        float(iou_thresh), devp(best), devp(flags), _streamp(d.dev)))
    return flags


class VOCMApMetric(object):
    """Mean average precision, area under the monotone precision envelope (VOC 2010+ style).

    ``update`` on float32 tensors of one GPU (predictions and ground-truth boxes; labels and difficults of any numeric
    dtype there; at most 1024 rows per image; ``class_map`` None or a sequence) matches them on the device (vy_voc_match)
    on the current stream: nothing is copied to the host and nothing synchronises, the flags stay device tensors until
    ``get()`` copies them once.  Everything else — numpy, other dtypes, tensors of several devices outside a list, more
    rows, a dict ``class_map`` — takes the host path below, unchanged; both may feed one metric.
    ``device_updates`` counts the launches since construction.  The one stated difference between the paths: among EQUAL
    scores the device takes the lower row first, the host path's unstable argsort whatever the sort gives.  (And a
    ground-truth label outside a sequence ``class_map`` is skipped on the device; on the host it is an IndexError.)"""

    def __init__(self, iou_thresh=0.5, class_names=None, class_map=None):
        self.iou_thresh = iou_thresh
        self.class_names = list(class_names) if class_names is not None else None
        self.class_map = class_map
        self.name = 'VOCMeanAP' if class_names is None else self.class_names + ['mAP']
        self.device_updates = 0
        self._class_luts = {}
        self.reset()

    def reset(self):
        self._n_pos = {}     # class -> number of non-difficult ground truths
        self._scores = {}    # class -> list of detection scores
        self._flags = {}     # class -> list of +1 (TP) / 0 (FP) / -1 (ignored: matched a difficult gt)
        self._chunks = []    # per device update: (labels, scores, mapped gt labels, flags, gt difficults or None, rows)

    # ------------------------------------------------------------------ accumulation
    def update(self, pred_bboxes, pred_labels, pred_scores, gt_bboxes, gt_labels, gt_difficults=None):
        if self._update_device(pred_bboxes, pred_labels, pred_scores, gt_bboxes, gt_labels, gt_difficults):
            return
        self._fold()         # keep the order of arrival
        self._update_host(pred_bboxes, pred_labels, pred_scores, gt_bboxes, gt_labels, gt_difficults)

    def _update_host(self, pred_bboxes, pred_labels, pred_scores, gt_bboxes, gt_labels, gt_difficults=None):
        pb, pl, ps, gb, gl = [_to_numpy(x) for x in (pred_bboxes, pred_labels, pred_scores, gt_bboxes, gt_labels)]
        gd = _to_numpy(gt_difficults) if gt_difficults is not None else None
        for i in range(len(pb)):
            self._update_image(pb[i], pl[i], ps[i], gb[i], gl[i], None if gd is None else gd[i])

    def _update_image(self, boxes, labels, scores, gboxes, glabels, gdiff):
        labels = np.asarray(labels).reshape(-1)
        keep = np.flatnonzero(labels >= 0)
        boxes, scores, labels = boxes[keep], np.asarray(scores).reshape(-1)[keep], labels[keep].astype(int)
        glabels = np.asarray(glabels).reshape(-1)
        if self.class_map is not None:
            glabels = np.array([self.class_map[int(g)] for g in glabels])
        gkeep = np.flatnonzero(glabels >= 0)
        gboxes, glabels = gboxes[gkeep], glabels[gkeep].astype(int)
        gdiff = np.zeros(len(gkeep)) if gdiff is None else np.asarray(gdiff).reshape(-1)[gkeep]
        for c in np.unique(np.concatenate([labels, glabels]).astype(int)):
            c = int(c)
            sel = labels == c
            order = scores[sel].argsort()[::-1]
            cb, cs = boxes[sel][order], scores[sel][order]
            gsel = glabels == c
            cg, cd = gboxes[gsel], gdiff[gsel]
            self._n_pos[c] = self._n_pos.get(c, 0) + int(np.logical_not(cd).sum())
            self._scores.setdefault(c, []).extend(cs)
            flags = self._flags.setdefault(c, [])
            if len(cb) == 0:
                continue
            if len(cg) == 0:
                flags.extend([0] * len(cb))
                continue
            iou = pairwise_iou(cb, cg)
            best = iou.argmax(axis=1)
            best[iou.max(axis=1) < self.iou_thresh] = -1
            taken = np.zeros(len(cg), dtype=bool)
            for g in best:  # detections in descending score order claim ground truths greedily
                if g < 0:
                    flags.append(0)
                elif cd[g]:
                    flags.append(-1)
                    taken[g] = True
                else:
                    flags.append(0 if taken[g] else 1)
                    taken[g] = True

    # ------------------------------------------------------------------ accumulation on the device
    def _update_device(self, pred_bboxes, pred_labels, pred_scores, gt_bboxes, gt_labels, gt_difficults):
        """Matches the batch on the device and returns True, or returns False: the call is the host path's."""
        d = _voc_device_batch(self.class_map, self._class_luts, pred_bboxes, pred_labels, pred_scores, gt_bboxes, gt_labels,
                              gt_difficults)
        if d is None:
            return False
        if d.batch == 0:
            return True
        flags = _voc_match_device(d, self.iou_thresh)
        self.device_updates += 1 if d.rows else 0
        self._chunks.append((d.labels.reshape(-1), d.scores.reshape(-1), d.mapped.reshape(-1), flags.reshape(-1),
                             None if d.diff is None else d.diff.reshape(-1), d.rows))
        return True

    def _fold(self):
        """Folds the device chunks into _scores / _flags / _n_pos: one copy to the host, then whole-array numpy.  A class
        gets its entries as _update_image makes them: image after image, a class's rows by descending score."""
        if not self._chunks:
            return
        import torch
        chunks, self._chunks = self._chunks, []
        # labels, scores, gt labels, flags, gt difficults (none given: none is difficult)
        host = _chunks_to_host([c[:4] + (torch.zeros_like(c[2], dtype=torch.uint8) if c[4] is None else c[4],) for c in chunks])
        for c, (labels, scores, glabels, flags, gdiff) in zip(chunks, host):
            det = np.flatnonzero(flags != -2)
            dl = labels[det].astype(int)
            order = np.lexsort((-scores[det].astype(np.float64), det // max(c[5], 1), dl))   # class, image, score
            det, dl = det[order], dl[order]
            gkeep = glabels >= 0
            counts = np.bincount(glabels[gkeep & (gdiff == 0)])
            for cls in np.unique(np.concatenate([dl, glabels[gkeep]]).astype(int)):
                cls = int(cls)
                lo, hi = np.searchsorted(dl, cls, 'left'), np.searchsorted(dl, cls, 'right')
                self._n_pos[cls] = self._n_pos.get(cls, 0) + (int(counts[cls]) if cls < len(counts) else 0)
                self._scores.setdefault(cls, []).extend(scores[det[lo:hi]])
                self._flags.setdefault(cls, []).extend(flags[det[lo:hi]].tolist())

    # ------------------------------------------------------------------ evaluation
    def _curves(self):
        self._fold()
        n_cls = max(self._n_pos) + 1 if self._n_pos else 0
        rec, prec = [None] * n_cls, [None] * n_cls
        for c in self._n_pos:
            s = np.array(self._scores[c])
            f = np.array(self._flags[c], dtype=np.int32)[s.argsort()[::-1]]
            tp, fp = np.cumsum(f == 1), np.cumsum(f == 0)
            with np.errstate(divide='ignore', invalid='ignore'):
                prec[c] = tp / (fp + tp)
            if self._n_pos[c] > 0:
                rec[c] = tp / self._n_pos[c]
        return rec, prec

    def _average_precision(self, rec, prec):
        if rec is None or prec is None:
            return np.nan
        r = np.concatenate([[0.0], rec, [1.0]])
        p = np.concatenate([[0.0], np.nan_to_num(prec), [0.0]])
        p = np.maximum.accumulate(p[::-1])[::-1]          # monotone envelope from the right
        step = np.flatnonzero(r[1:] != r[:-1])
        return float(np.sum((r[step + 1] - r[step]) * p[step + 1]))

    def get(self):
        rec, prec = self._curves()
        aps = [self._average_precision(r, p) for r, p in zip(rec, prec)]
        with np.errstate(all='ignore'):
            mean_ap = float(np.nanmean(aps)) if len(aps) else float('nan')
        if self.class_names is None:
            return self.name, mean_ap
        n = len(self.class_names)
        per_class = [aps[c] if c < len(aps) and c in self._n_pos else float('nan') for c in range(n)]
        if self.class_map:
            per_class = [float('nan') if self.class_map[c] < 0 else
                         (aps[self.class_map[c]] if self.class_map[c] < len(aps) and self.class_map[c] in self._n_pos
                          else float('nan')) for c in range(n)]
        return list(self.name), per_class + [mean_ap]


class VOC07MApMetric(VOCMApMetric):
    """Mean AP with the VOC2007 11-point interpolation (max precision at recall >= 0, 0.1, ..., 1)."""

    def _average_precision(self, rec, prec):
        if rec is None or prec is None:
            return np.nan
        p = np.nan_to_num(prec)
        ap = 0.0
        for t in np.arange(0.0, 1.1, 0.1):
            hit = rec >= t
            ap += (np.max(p[hit]) if hit.any() else 0.0) / 11.0
        return float(ap)


# ====================================================================================================================
# The per-frame mAP and the worst-clip ranking: detect_yolo3.py --per_frame_metric (add_metrics_to_predictions, :451-534,
# built at :855-862), which runs metric.reset(); metric.update(<one frame>); metric.get() on a VOCMApMetric for every
# frame, writes the mean AP as an eighth column beside the frame's predictions and ranks frames, or videos by their mean,
# worst first (summary.txt, what --worst_video_path renders from).
# ====================================================================================================================
def frame_map_host(pred_bboxes, pred_labels, pred_scores, gt_bboxes, gt_labels, gt_difficults=None, iou_thresh=0.5,
                   class_map=None, use_07_metric=False):
    """The per-frame mean AP, (B,) float64: for image b exactly what a fresh ``VOCMApMetric`` (``VOC07MApMetric`` with
    ``use_07_metric``) gives for ``update(<image b alone>); get()``, NaN for a frame with nothing to score.  This is the
    definition the device kernel (csrc/voc_metric.hip, vy_voc_frame_ap) is held to.  Spelled out per frame:

      detections: the rows with label >= 0; voc_match_host's flags say what each is (1 TP, 0 FP, -1 neither)
      class c: npos = its mapped ground truths that are not difficult.  Only classes with npos > 0 enter the mean: one
        with detections and no such ground truth is NaN and drops out of the nanmean, one with ground truth and no
        detection enters with AP 0
      rank: a class's rows by score descending (among equal scores the device takes the lower row first, the host what its
        unstable argsort gives); at a row tp / fp count the flag-1 / flag-0 rows at or ahead of it;
        prec = tp / (tp + fp) (0 / 0 -> 0), rec = tp / npos, float64
      area AP: the sum over the class's TP rows of (tp / npos - (tp - 1) / npos) * the largest prec at or behind the row
      11-point AP: for k = 0..10, t = 0.0 + k * 0.1: ap += (the largest prec over rows with rec >= t, else 0) / 11.0
      frame score: the sum of the classes' APs / the number of classes with npos > 0; NaN when there is none
    """
    import warnings
    arrays = [_to_numpy(x) for x in (pred_bboxes, pred_labels, pred_scores, gt_bboxes, gt_labels)]
    gd = _to_numpy(gt_difficults) if gt_difficults is not None else None
    cls = VOC07MApMetric if use_07_metric else VOCMApMetric
    out = np.full(len(arrays[0]), np.nan, np.float64)
    for b in range(len(out)):
        m = cls(iou_thresh=iou_thresh, class_map=class_map)
        m._update_host(*[a[b:b + 1] for a in arrays], gt_difficults=None if gd is None else gd[b:b + 1])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)           # nanmean of nothing but NaN: the frame is NaN
            out[b] = m.get()[1]
    return out


def frame_metric_lines(img_path, rows, score):
    """The reference's per-frame metric file format (detect_yolo3.py:517): ``path,class,score,x1,y1,x2,y2,frame_score``
    per detection, ``rows`` as transforms.prediction_lines takes them, ``score`` the frame's mean AP."""
    return ["{},{},{},{},{},{},{},{}\n".format(img_path, int(r[0]), r[1], r[2], r[3], r[4], r[5], score) for r in rows]


class FrameMApMetric(object):
    """The mean AP of every frame on its own, and the ranking of the worst frames and videos by it.

    ``update`` takes what ``VOCMApMetric.update`` takes, and ``keys``: one hashable per image (a sample id, a path, a
    ``(video, frame)`` pair); default the running index since ``reset``.  On the input ``VOCMApMetric`` matches on the
    device — float32 tensors of one GPU, at most 1024 rows per image, ``class_map`` None or a sequence — it launches
    vy_voc_match and vy_voc_frame_ap on the current stream and keeps the (B,) scores as a device tensor: nothing is
    copied and nothing synchronises until ``get()`` copies all of them at once.  Everything else takes
    ``frame_map_host``; both may feed one metric, in arrival order.  ``device_updates`` counts the launched updates.

    Where this differs from the reference, on purpose: there a frame with nothing to score is NaN, poisons its video's
    mean and leaves the sort undefined.  Here NaN frames are left out of ``worst`` and of the videos' means and frame
    counts and are reported in ``unscored``; a video without a scored frame comes last, its mean NaN.  Among equal scores
    the device ranks the lower row first (``VOCMApMetric``'s stated rule)."""

    def __init__(self, iou_thresh=0.5, class_names=None, class_map=None, use_07_metric=False):
        self.iou_thresh = iou_thresh
        self.class_names = list(class_names) if class_names is not None else None
        self.class_map = class_map
        self.use_07_metric = bool(use_07_metric)
        self.name = 'FrameMeanAP'
        self.device_updates = 0
        self._class_luts = {}
        self.reset()

    def reset(self):
        self._keys = []
        self._chunks = []    # per update, in arrival order: the (B,) scores, a float64 numpy array or a device tensor

    def update(self, pred_bboxes, pred_labels, pred_scores, gt_bboxes, gt_labels, gt_difficults=None, keys=None):
        d = _voc_device_batch(self.class_map, self._class_luts, pred_bboxes, pred_labels, pred_scores, gt_bboxes, gt_labels,
                              gt_difficults)
        if d is None:
            scores = frame_map_host(pred_bboxes, pred_labels, pred_scores, gt_bboxes, gt_labels, gt_difficults,
                                    self.iou_thresh, self.class_map, self.use_07_metric)
            batch = len(scores)
        else:
            batch = d.batch
        if keys is None:
            keys = range(len(self._keys), len(self._keys) + batch)
        keys = list(keys)
        if len(keys) != batch:
            raise ValueError("%d keys for a batch of %d frames" % (len(keys), batch))
        if d is not None and batch:
            scores = self._frame_ap_device(d)[0]
            self.device_updates += 1
        if batch:
            self._keys.extend(keys)
            self._chunks.append(scores)

    def _frame_ap_device(self, d):
        """vy_voc_match, then vy_voc_frame_ap on its flags, on the current stream: (scores (B,) float64, classes (B,)
        int32), device tensors."""
        import torch
        from . import _lib
        lib = _lib.load()
        flags = _voc_match_device(d, self.iou_thresh)
        ap = torch.empty(d.batch, dtype=torch.float64, device=d.dev)
        n_cls = torch.empty(d.batch, dtype=torch.int32, device=d.dev)
        devp = lambda t: _devp(t if t.numel() else ap)            # noqa: E731  a valid address for arrays without elements
        with torch.cuda.device(d.dev):
            _lib.check(lib.vy_voc_frame_ap(d.batch, d.rows, d.n_gt, devp(d.labels), devp(d.scores), devp(flags),
                                           devp(d.mapped), None if d.diff is None else devp(d.diff),
                                           int(self.use_07_metric), devp(ap), devp(n_cls), _streamp(d.dev)))
        return ap, n_cls

    def get(self):
        """``(keys, scores)``: the keys in arrival order and their frames' mean AP, a float64 numpy array (NaN: nothing to
        score).  The device results are copied here, all at once."""
        on_dev = [i for i, c in enumerate(self._chunks) if not isinstance(c, np.ndarray)]
        if on_dev:
            for i, (h,) in zip(on_dev, _chunks_to_host([(self._chunks[i],) for i in on_dev])):
                self._chunks[i] = h.copy()
        scores = np.concatenate(self._chunks) if self._chunks else np.zeros(0, np.float64)
        return list(self._keys), scores

    @property
    def unscored(self):
        """The keys of the frames with nothing to score (NaN), in arrival order."""
        keys, scores = self.get()
        return [k for k, s in zip(keys, scores) if s != s]

    def worst(self, n=None):
        """``[(key, score)]`` of the scored frames, the lowest score first (equal scores in arrival order), the first
        ``n`` of them."""
        keys, scores = self.get()
        scored = [(k, float(s)) for k, s in zip(keys, scores) if s == s]
        scored.sort(key=lambda ks: ks[1])
        return scored if n is None else scored[:n]

    def by_video(self, video_of=lambda key: key[0]):
        """``[(video, mean, frames)]`` sorted by ``(mean, -frames)`` — the order of the reference's summary.txt
        (detect_yolo3.py:521-527): the lowest mean first, among equal means the video with more frames.  ``mean`` and
        ``frames`` are over the video's scored frames; a video without one comes last with NaN and 0."""
        keys, scores = self.get()
        per_video = {}
        for k, s in zip(keys, scores):
            per_video.setdefault(video_of(k), []).extend([float(s)] if s == s else [])
        ranked = sorted(((v, sum(s) / len(s), len(s)) for v, s in per_video.items() if s), key=lambda r: (r[1], -r[2]))
        return ranked + [(v, float('nan'), 0) for v, s in per_video.items() if not s]


# ====================================================================================================================
# ImageNet-VID motion / area mAP: metrics/imgnetvid.py in the reference, the metric its detect
# driver builds for its main dataset (detect_yolo3.py:181-195) and its model README reports.  mAP over motion-IoU ranges
# x box-area ranges; a frame's detections claim ground truths greedily in score order, separately in every slice.
# Pinned by the reference's own vid_eval_motion: tests/golden/make_vid_metric_golden.py.
# ====================================================================================================================
VID_MOTION_RANGES = ((0.0, 1.0), (0.0, 0.7), (0.7, 0.9), (0.9, 1.0))
VID_AREA_RANGES = ((0, 1e5 * 1e5), (0, 50 * 50), (50 * 50, 150 * 150), (150 * 150, 1e5 * 1e5))


def vid_match_host(det_boxes, det_labels, gt_boxes, gt_labels, gt_thr, gt_motion, motion_ranges, area_ranges,
                   empty_weight, n_ig_motion=None):
    """The matching rule of the VID metric for ONE frame, every (motion range, area range) slice at once: the definition
    the device kernel (csrc/vid_metric.hip, vy_vid_match) is held to, value for value.

    det_boxes (D, 4) / det_labels (D): the frame's kept detections in descending score order.  gt_boxes (G, 4),
    gt_labels (G), gt_thr (G) the IoU a match needs, gt_motion (G) motion IoU.  motion_ranges (M, 2), area_ranges (A, 2):
    [lo, hi], both ends inside.  empty_weight (M): the weight of a miss in a frame without ground truth.  n_ig_motion (M):
    how many of the frame's ground truths lie outside each motion range (default: counted from gt_motion; the metric
    passes the count over the frame's unmapped list, which a class map makes longer than G).  Returns ``tp`` (D, M * A)
    uint8 and ``fp`` (D, M * A) float64, slice = motion * A + area.

    All float64, in this order (pixel boxes, both corners inside):
      iw = min(b2, g2) - max(b0, g0) + 1, ih likewise; both > 0: ov = iw * ih / ((bw * bh + gw * gh) - iw * ih), else 0
      per detection, ground truths in index order: a candidate has ov >= thr, is not yet detected in the slice and has
      the detection's label; the largest ov wins, the lowest index on a tie
      match: the ground truth is detected; tp = 1 unless it is outside the motion or the area range; fp = 0
      miss: fp = 0 if the detection's own area is outside the area range; else 1 if its best overlap with an in-range
      ground truth exceeds that with an out-of-range one, 0 if the reverse; else (equal, -1 when there is none)
      empty_weight if G == 0, else n_ig_motion / G
    """
    db = np.asarray(det_boxes, np.float64).reshape(-1, 4)
    dl = np.asarray(det_labels).reshape(-1).astype(np.int64)
    gb = np.asarray(gt_boxes, np.float64).reshape(-1, 4)
    gl = np.asarray(gt_labels).reshape(-1).astype(np.int64)
    thr = np.asarray(gt_thr, np.float64).reshape(-1)
    mo = np.asarray(gt_motion, np.float64).reshape(-1)
    mr = np.asarray(motion_ranges, np.float64).reshape(-1, 2)
    ar = np.asarray(area_ranges, np.float64).reshape(-1, 2)
    n_m, n_a = len(mr), len(ar)
    m0, m1 = np.repeat(mr[:, 0], n_a), np.repeat(mr[:, 1], n_a)
    a0, a1 = np.tile(ar[:, 0], n_m), np.tile(ar[:, 1], n_m)
    n_d, n_g, n_s = len(db), len(gb), n_m * n_a
    tp = np.zeros((n_d, n_s), np.uint8)
    fp = np.zeros((n_d, n_s), np.float64)
    ig_m = (mo[None, :] < m0[:, None]) | (mo[None, :] > m1[:, None])              # (S, G)
    gw, gh = gb[:, 2] - gb[:, 0] + 1, gb[:, 3] - gb[:, 1] + 1
    g_area = gh * gw
    ig_a = (g_area[None, :] < a0[:, None]) | (g_area[None, :] > a1[:, None])
    if n_g == 0:
        miss = np.repeat(np.asarray(empty_weight, np.float64).reshape(-1), n_a)
    else:
        n_ig = ig_m.sum(axis=1) if n_ig_motion is None else np.repeat(np.asarray(n_ig_motion).reshape(-1), n_a)
        miss = n_ig / float(n_g)
    detected = np.zeros((n_s, n_g), bool)
    rows = np.arange(n_s)
    for j in range(n_d):   # the chain: sequential in the detections, whole-array in ground truths and slices
        b = db[j]
        if n_g:
            iw = np.minimum(b[2], gb[:, 2]) - np.maximum(b[0], gb[:, 0]) + 1
            ih = np.minimum(b[3], gb[:, 3]) - np.maximum(b[1], gb[:, 1]) + 1
            ua = (b[2] - b[0] + 1) * (b[3] - b[1] + 1) + gw * gh - iw * ih
            with np.errstate(divide='ignore', invalid='ignore'):
                ov = np.where((iw > 0) & (ih > 0), iw * ih / ua, 0.0)
            cand = ((ov >= thr) & (gl == dl[j]))[None, :] & ~detected
            kmax = np.where(cand, ov[None, :], -1.0).argmax(axis=1)                 # first index of the largest
            hit = cand.any(axis=1)
            ov_ig = np.where(ig_m, ov[None, :], -1.0).max(axis=1)
            ov_nig = np.where(ig_m, -1.0, ov[None, :]).max(axis=1)
            detected[rows[hit], kmax[hit]] = True
            tp[j] = hit & ~ig_m[rows, kmax] & ~ig_a[rows, kmax]
        else:
            hit = np.zeros(n_s, bool)
            ov_ig = ov_nig = np.full(n_s, -1.0)
        b_area = (b[3] - b[1] + 1) * (b[2] - b[0] + 1)
        outside = (b_area < a0) | (b_area > a1)
        f = np.where(ov_nig > ov_ig, 1.0, np.where(ov_ig > ov_nig, 0.0, miss))
        fp[j] = np.where(hit | outside, 0.0, f)
    return tp, fp


def _vid_ap(rec, prec):
    """Area under the monotone precision envelope (imgnetvid.py:40-65), whole-array."""
    mrec = np.concatenate(([0.], rec, [1.]))
    mpre = np.concatenate(([0.], prec, [0.]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    i = np.flatnonzero(mrec[1:] != mrec[:-1])
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


class VIDDetectionMetric(object):
    """ImageNet-VID mean AP by motion-IoU range x box-area range: the reference's ``VIDDetectionMetric``
    (metrics/imgnetvid.py:357-472), same constructor, ``update`` / ``get`` / ``reset`` and ``get()`` strings.

    ``dataset`` is duck-typed: ``get_sample_ids()`` (with ``offset`` the entries are lists and the id is
    ``w[offset + 2]``), ``get_label(id)`` -> (n, >= 5) rows ``[x1, y1, x2, y2, cls, ...]``, ``wn_classes``, ``classes``
    and ``motion_ious[str(id)]``, one value per ground truth.  The ground-truth tables of the whole dataset are built here,
    once.  ``update``'s ground-truth arguments are accepted and ignored, as in the reference: ground truth comes from the
    dataset.  ``sid`` is the frame's id for a batch of 1, or a sequence of B ids.

    When the predictions are device tensors ``update`` matches them on the device (vy_vid_match): the per-frame sort and
    the float64 casts are torch calls, nothing is copied to the host and nothing synchronises; the outputs stay device
    tensors until ``get()`` copies them once.  Host arrays go through ``vid_match_host``.  Both give the same values.

    Where this differs from the reference, on purpose:
      * a ``sid`` the dataset does not have, or one seen before (since ``reset``), raises ``ValueError``.  The reference
        silently drops the rows of an unknown id and merges the rows of a repeated one into one frame.
      * equal scores keep their order (stable sorts; frames in the dataset's sample-id order).  The reference's
        ``argsort`` leaves ties to the sort's internals.
      * the ranges are constructor keywords (defaults: the reference's hard-set ones).
    ``class_map`` / ``agnostic`` compute what the reference computes, including that with a class map a frame's ``thr``,
    motion IoU and out-of-range count come from its unmapped label list (imgnetvid.py:204-220, :265) and that a dropped
    class reads the positives of the last one (:347).

    After ``get()``, ``metric.ap`` is the (motion ranges, area ranges, classes) array; -1: no positives in the slice.
    """

    def __init__(self, dataset, conf_score_thresh=0.05, iou_thresh=0.5, class_map=None, agnostic=False, offset=None,
                 motion_ranges=VID_MOTION_RANGES, area_ranges=VID_AREA_RANGES):
        self.name = 'ImgNetVIDMeanAP'
        self.dataset = dataset
        self._conf_score_thresh = float(conf_score_thresh)
        self._iou_thresh = iou_thresh
        self._class_map = class_map
        self._agnostic = agnostic
        self._offset = offset
        self._motion_ranges = [list(r) for r in motion_ranges]
        self._area_ranges = [list(r) for r in area_ranges]
        self._mr = np.asarray(self._motion_ranges, np.float64).reshape(-1, 2)
        self._ar = np.asarray(self._area_ranges, np.float64).reshape(-1, 2)
        if not (1 <= len(self._mr) <= 8 and 1 <= len(self._ar) <= 8):
            raise ValueError("between 1 and 8 motion ranges and area ranges")
        if (self._mr[:, 0] > self._mr[:, 1]).any() or (self._ar[:, 0] > self._ar[:, 1]).any():
            raise ValueError("a range with lo > hi")
        self._build_tables()
        self._device_tables = {}
        self.reset()

    # ------------------------------------------------------------------ the dataset's ground truth, once
    def _build_tables(self):
        ds = self.dataset
        ids = list(ds.get_sample_ids())
        if len(ids) and isinstance(ids[0], list):
            ids = [w[self._offset + 2] for w in ids]
        self._ids = ids
        self._row = {}
        for r, i in enumerate(ids):
            if i in self._row:
                raise ValueError("sample id %r appears twice in the dataset" % (i,))
            self._row[i] = r
        self._names = ['agnostic'] if self._agnostic else list(ds.wn_classes)
        cm = self._class_map
        n_pos = len(self._names) if cm is None else max(cm) + 1
        boxes, labels, thrs, motions, counts, all_motion, all_count = [], [], [], [], [], [], []
        for i in ids:
            lab = np.asarray(ds.get_label(i), np.float64)
            lab = lab.reshape(-1, lab.shape[-1] if lab.ndim == 2 else 5)
            box, raw = lab[:, :4], lab[:, 4].astype(np.int64)
            w, h = box[:, 2] - box[:, 0] + 1, box[:, 3] - box[:, 1] + 1
            thr = np.minimum((w * h) / ((w + 10) * (h + 10)), self._iou_thresh)
            mo = np.asarray(ds.motion_ious[str(i)], np.float64).reshape(-1)
            if len(mo) != len(lab):
                raise ValueError("sample %r: %d motion IoUs for %d ground truths" % (i, len(mo), len(lab)))
            if cm is not None:
                raw = np.array([cm[int(l)] for l in raw], np.int64).reshape(-1)
                valid = np.flatnonzero(raw >= 0)
                box, raw = box[valid], raw[valid]
            if self._agnostic:
                raw = raw * 0
            n = len(raw)
            boxes.append(box), labels.append(raw), thrs.append(thr[:n]), motions.append(mo[:n]), counts.append(n)
            all_motion.append(mo), all_count.append(len(mo))
        cat = lambda parts, shape, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(shape, dt)  # noqa: E731
        self._gt_box = np.ascontiguousarray(cat(boxes, (0, 4), np.float64).reshape(-1, 4))
        self._gt_label = cat(labels, (0,), np.int32)
        self._gt_thr = cat(thrs, (0,), np.float64)
        self._gt_motion = cat(motions, (0,), np.float64)
        self._gt_off = np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]).astype(np.int64)
        if self._gt_label.size and (self._gt_label.min() < 0 or self._gt_label.max() >= n_pos):
            raise ValueError("a ground-truth label outside the %d classes" % n_pos)
        n_m, n_a = len(self._mr), len(self._ar)
        # per frame and motion range: ground truths of the UNMAPPED list outside the range; the share inside it, dataset-wide
        am = cat(all_motion, (0,), np.float64)
        frame_of = np.repeat(np.arange(len(ids)), np.asarray(all_count, np.int64))
        self._gt_nig = np.zeros((len(ids), n_m), np.int32)
        self._empty_weight = np.zeros(n_m, np.float64)
        for m in range(n_m):
            out = (am < self._mr[m, 0]) | (am > self._mr[m, 1])
            self._gt_nig[:, m] = np.bincount(frame_of[out], minlength=len(ids))
            if len(am):
                self._empty_weight[m] = int((~out).sum()) / float(len(am))
        # positives per slice and class: the dataset's count minus the ground truths ignored in the slice
        base = np.bincount(self._gt_label, minlength=n_pos).astype(np.float64)
        area = (self._gt_box[:, 3] - self._gt_box[:, 1] + 1) * (self._gt_box[:, 2] - self._gt_box[:, 0] + 1)
        self._npos = np.zeros((n_m * n_a, n_pos), np.float64)
        for m in range(n_m):
            ig_m = (self._gt_motion < self._mr[m, 0]) | (self._gt_motion > self._mr[m, 1])
            for a in range(n_a):
                ig = ig_m | (area < self._ar[a, 0]) | (area > self._ar[a, 1])
                self._npos[m * n_a + a] = base - np.bincount(self._gt_label[ig], minlength=n_pos)

    def reset(self):
        self._chunks = []     # per update: (rows, labels, scores, tp, fp), numpy or device tensors
        self._seen = set()
        self.ap = None

    # ------------------------------------------------------------------ accumulation
    def _rows_of(self, sid, batch):
        if sid is None:
            raise ValueError("update needs sid: the frame's id, or one id per frame of the batch")
        if hasattr(sid, "tolist"):
            sid = sid.tolist()
        sids = list(sid) if isinstance(sid, (list, tuple, range)) else [sid]
        if len(sids) != batch:
            raise ValueError("%d ids for a batch of %d frames" % (len(sids), batch))
        rows = []
        for s in sids:
            if s not in self._row:
                raise ValueError("sid %r is not one of the dataset's sample ids" % (s,))
            if s in self._seen or self._row[s] in rows:
                raise ValueError("sid %r was given before" % (s,))
            rows.append(self._row[s])
        return sids, np.asarray(rows, np.int64)

    def update(self, pred_bboxes, pred_labels, pred_scores, gt_bboxes=None, gt_ids=None, gt_difficults=None, sid=None):
        """pred_bboxes (B, N, 4), pred_labels and pred_scores (B, N) or (B, N, 1): numpy, torch, or lists of them (one per
        device, joined along the batch).  Rows with label < 0 or score < conf_score_thresh are dropped."""
        pb, pl, ps = (_gather(x) for x in (pred_bboxes, pred_labels, pred_scores))
        on_device = all(getattr(x, "is_cuda", False) for x in (pb, pl, ps))
        if not on_device:
            pb, pl, ps = (np.asarray(_to_numpy(x)) for x in (pb, pl, ps))
        batch = int(pb.shape[0])
        sids, rows = self._rows_of(sid, batch)
        n = int(np.prod(pl.shape[1:])) if batch else 0
        if batch and n:
            pb, pl, ps = pb.reshape(batch, n, 4), pl.reshape(batch, n), ps.reshape(batch, n)
            self._chunks.append(self._update_device(pb, pl, ps, rows) if on_device else self._update_host(pb, pl, ps, rows))
        self._seen.update(sids)

    def _update_host(self, pb, pl, ps, rows):
        out = [[], [], [], [], []]
        for b, r in enumerate(rows):
            score = ps[b].astype(np.float64)
            keep = np.flatnonzero((pl[b] >= 0) & (score >= self._conf_score_thresh))
            keep = keep[np.argsort(-score[keep], kind='stable')]
            label = pl[b][keep].astype(np.int64) * (0 if self._agnostic else 1)
            g0, g1 = self._gt_off[r], self._gt_off[r + 1]
            tp, fp = vid_match_host(pb[b][keep].astype(np.float64), label, self._gt_box[g0:g1], self._gt_label[g0:g1],
                                    self._gt_thr[g0:g1], self._gt_motion[g0:g1], self._mr, self._ar, self._empty_weight,
                                    self._gt_nig[r])
            for o, v in zip(out, (np.full(len(keep), r, np.int64), label.astype(np.int32), score[keep], tp, fp)):
                o.append(v)
        return tuple(np.concatenate(o) for o in out)

    def _update_device(self, pb, pl, ps, rows):
        import torch
        from . import _lib
        lib = _lib.load()
        dev = pb.device
        batch, n = pl.shape
        n_s = len(self._mr) * len(self._ar)
        score = ps.to(torch.float64)
        order = torch.sort(score, dim=1, descending=True, stable=True).indices
        score = score.gather(1, order).contiguous()
        lab = pl.gather(1, order)
        lab_i = lab.to(torch.int32)
        label = torch.where(lab >= 0, torch.zeros_like(lab_i) if self._agnostic else lab_i, torch.full_like(lab_i, -1))
        box = pb.to(torch.float64).gather(1, order[:, :, None].expand(batch, n, 4)).contiguous()
        tp = torch.empty((batch * n, n_s), dtype=torch.uint8, device=dev)
        fp = torch.empty((batch * n, n_s), dtype=torch.float64, device=dev)
        flag_bytes = int((self._gt_off[rows + 1] - self._gt_off[rows]).sum()) * n_s
        flags = torch.empty(max(flag_bytes, 1), dtype=torch.uint8, device=dev)
        t = _upload(self._device_tables, dev, box=self._gt_box, label=self._gt_label, thr=self._gt_thr,
                    motion=self._gt_motion, nig=self._gt_nig)
        det_off = np.arange(batch + 1, dtype=np.int64) * n
        gt_frame = rows.astype(np.int32)
        with torch.cuda.device(dev):
            _lib.check(lib.vy_vid_match(
                batch, _hostp(det_off), _devp(box), _devp(label), _devp(score), self._conf_score_thresh, _hostp(gt_frame),
                len(self._ids), _hostp(self._gt_off), _devp(t['box']), _devp(t['label']), _devp(t['thr']), _devp(t['motion']),
                _devp(t['nig']), len(self._mr), _hostp(self._mr), len(self._ar), _hostp(self._ar),
                _hostp(self._empty_weight), _devp(flags), flag_bytes, _devp(tp), _devp(fp), _streamp(dev)))
        return np.repeat(rows, n), label.reshape(-1), score.reshape(-1), tp, fp

    # ------------------------------------------------------------------ evaluation
    def matches(self):
        """Every kept detection so far as ``(row, label, score, tp, fp)`` numpy arrays: frames in the dataset's sample-id
        order (``row`` indexes it), a frame's detections by descending score; tp (n, slices) uint8, fp (n, slices)
        float64, slice = motion range * area ranges + area range.  Device results are copied here, once."""
        n_s = len(self._mr) * len(self._ar)
        parts = [[], [], [], [], []]
        dev_chunks = [c for c in self._chunks if not isinstance(c[3], np.ndarray)]
        if dev_chunks:
            import torch
            dev = dev_chunks[0][3].device
            # joined on the device first: thousands of chunks cost more to split on the host than they cost to join there
            joined = _chunks_to_host([tuple(torch.cat([c[k].to(dev) for c in dev_chunks], 0) for k in range(1, 5))])[0]
            keep = np.flatnonzero((joined[0] >= 0) & (joined[1] >= self._conf_score_thresh))
            parts[0].append(np.concatenate([c[0] for c in dev_chunks])[keep])
            for k in range(4):
                parts[k + 1].append(joined[k][keep])
        for c in self._chunks:
            if isinstance(c[3], np.ndarray):
                for k in range(5):
                    parts[k].append(c[k])
        empty = (np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float64), np.zeros((0, n_s), np.uint8),
                 np.zeros((0, n_s), np.float64))
        out = [np.concatenate(p) if p else e for p, e in zip(parts, empty)]
        order = np.argsort(out[0], kind='stable')
        return tuple(a[order] for a in out)

    def _average_precisions(self):
        _, label, score, tp, fp = self.matches()
        n_m, n_a, n_c = len(self._mr), len(self._ar), len(self._names)
        by_score = np.argsort(-score, kind='stable')
        by_class = np.argsort(label[by_score], kind='stable')
        idx = by_score[by_class]                      # class by class, descending score inside a class
        sorted_label = label[idx]
        tp, fp = np.ascontiguousarray(tp[idx].T), np.ascontiguousarray(fp[idx].T)
        cm = self._class_map if self._class_map is not None else list(range(n_c))
        eps = np.finfo(np.float64).eps
        ap = np.zeros((n_m * n_a, n_c))
        for c in range(n_c):
            lo, hi = np.searchsorted(sorted_label, cm[c], 'left'), np.searchsorted(sorted_label, cm[c], 'right')
            for s in range(n_m * n_a):
                npos = self._npos[s][cm[c]]
                if npos <= 0:
                    ap[s, c] = -1
                    continue
                tpc = np.cumsum(tp[s, lo:hi], dtype=np.float64)
                fpc = np.cumsum(fp[s, lo:hi])
                ap[s, c] = _vid_ap(tpc / npos, tpc / np.maximum(tpc + fpc, eps))
        return ap.reshape(n_m, n_a, n_c)

    def get(self):
        """``(names, values)`` with the reference's strings (imgnetvid.py:402-426): the summary of every slice's mean AP
        over the classes with positives, then AP x 100 of every class in the first slice."""
        ap = self.ap = self._average_precisions()
        names, values = ['~~~~ Summary metrics ~~~~\n'], []
        info_str = ''
        for mi, mr in enumerate(self._motion_ranges):
            for ai, ar in enumerate(self._area_ranges):
                lo, hi = np.sqrt(ar[0]), np.sqrt(ar[1])
                info_str += 'motion [{0:.1f} {1:.1f}], area [{2} {3} {4} {5}]\n'.format(mr[0], mr[1], lo, lo, hi, hi)
                scored = ap[mi, ai][ap[mi, ai] >= 0]
                mean = np.mean(scored) if len(scored) else float('nan')
                info_str += 'Mean AP@{:.1f} = {:.4f}\n\n'.format(self._iou_thresh, mean)
        values.append(info_str)
        if self._agnostic:
            names.append('agnostic')
            values.append('{:.1f}'.format(100 * ap[0, 0, 0]))
            return names, values
        for c, cls_name in enumerate(self.dataset.classes):
            names.append(cls_name)
            values.append('{:.1f}'.format(100 * ap[0, 0, c]))
        return names, values


# ====================================================================================================================
# COCO detection metric: metrics/mscoco.py in the reference, the second metric its detect driver builds by
# default (detect_yolo3.py:53, :185) on every dataset, each of which writes a COCO-style ground-truth file for it
# (build_coco_json).  The reference hands the evaluation to pycocotools' COCOeval (iouType 'bbox', useCats 1), which
# cannot be run here: everything below that restates COCOeval is [UPSTREAM-RECALLED] — evaluateImg in coco_match_host,
# accumulate in coco_accumulate, summarize in COCODetectionMetric._summarize.  tests/golden/make_coco_metric_golden.py
# records the real COCOeval's values on a machine that has it.
# ====================================================================================================================
COCO_IOU_THRS = np.linspace(.5, .95, 10)
COCO_REC_THRS = np.linspace(0, 1, 101)
COCO_MAX_DETS = (1, 10, 100)
COCO_AREA_RANGES = ((0, 1e10), (0, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e10))
COCO_AREA_NAMES = ('all', 'small', 'medium', 'large')
_COCO_LUT_MAX = 1 << 20


def _coco_iou(d, g, crowd):
    """[UPSTREAM-RECALLED] maskUtils.iou on xywh boxes: one detection against (G, 4) ground truths, float64."""
    w = np.minimum(d[0] + d[2], g[:, 0] + g[:, 2]) - np.maximum(d[0], g[:, 0])
    h = np.minimum(d[1] + d[3], g[:, 1] + g[:, 3]) - np.maximum(d[1], g[:, 1])
    w, h = np.where(w <= 0, 0.0, w), np.where(h <= 0, 0.0, h)
    inter = w * h
    da = d[2] * d[3]
    with np.errstate(divide='ignore', invalid='ignore'):
        return inter / np.where(crowd, da, (da + g[:, 2] * g[:, 3]) - inter)


def coco_match_host(det_xywh, det_cat, det_score, gt_xywh, gt_cat, gt_area, gt_crowd, gt_id, iou_thrs, area_ranges,
                    max_det):
    """[UPSTREAM-RECALLED] The matching rule of the COCO metric for ONE image, row by row: ``COCOeval.evaluateImg``
    (iouType 'bbox') for every category, area range and IoU threshold at once, and the definition the device kernel
    (csrc/coco_metric.hip, vy_coco_match) is held to, value for value.

    det_xywh (R, 4), det_cat (R) category index, < 0 = the row takes no part, det_score (R): the image's rows in any
    order.  gt_xywh (G, 4), gt_cat (G), gt_area (G) the file's area, gt_crowd (G), gt_id (G) the annotations' ids.
    iou_thrs (T), area_ranges (A, 2) [lo, hi], both ends inside.  Returns, in input row order, ``rank`` (R) int32 — the
    row's position among the image's kept rows of its category in the stable descending score order
    (``argsort(-score, kind='mergesort')``), -1 for a row that takes no part or a position >= max_det — and ``flags``
    (R, A, T) uint8: bit 0 ``dtm != 0``, bit 1 ``dtIg``; 0 where rank is -1.

    All float64:
      iou: w = min(dx + dw, gx + gw) - max(dx, gx), 0 if w <= 0, h likewise; i = w * h; u = dw * dh for a crowd, else
        (dw * dh + gw * gh) - i; iou = i / u
      per (category, area range): a ground truth is ignored when it is a crowd or its area < lo or > hi; the ones that are
        not ignored come first (stable)
      per threshold t, the category's first max_det rows in score order: best = min(t, 1 - 1e-10), m = none; over the
        ground truths in that order: one taken at this (range, t) that is no crowd is passed over; with m set and not
        ignored, the first ignored one ends the walk; iou < best is passed over; else best = iou, m = it.  With m set the
        row's dtIg is m's, its dtm is m's ID, and m is taken
      afterwards dtIg |= dtm == 0 and the row's own area dw * dh < lo or > hi
    ``dtm == 0`` is COCOeval's test for "unmatched": a row matched to the annotation whose id is 0 takes that ground truth
    and its ignore flag, and counts as unmatched from then on.
    """
    d = np.asarray(det_xywh, np.float64).reshape(-1, 4)
    dc = np.asarray(det_cat).reshape(-1).astype(np.int64)
    ds = np.asarray(det_score, np.float64).reshape(-1)
    g = np.asarray(gt_xywh, np.float64).reshape(-1, 4)
    gc = np.asarray(gt_cat).reshape(-1).astype(np.int64)
    ga = np.asarray(gt_area, np.float64).reshape(-1)
    gcrowd = np.asarray(gt_crowd).reshape(-1) != 0
    gid = np.asarray(gt_id).reshape(-1).astype(np.int64)
    thr = np.asarray(iou_thrs, np.float64).reshape(-1)
    ar = np.asarray(area_ranges, np.float64).reshape(-1, 2)
    n_r, n_a, n_t = len(dc), len(ar), len(thr)
    rank = np.full(n_r, -1, np.int32)
    flags = np.zeros((n_r, n_a, n_t), np.uint8)
    kept = np.flatnonzero(dc >= 0)
    kept = kept[np.argsort(-ds[kept], kind='mergesort')]
    start = np.minimum(thr, 1 - 1e-10)
    floor = start.min() if n_t else 0.0
    g_ig = gcrowd[None, :] | (ga[None, :] < ar[:, :1]) | (ga[None, :] > ar[:, 1:])               # (A, G)
    d_area = d[:, 2] * d[:, 3]
    for c in np.unique(dc[kept]):
        rows = kept[dc[kept] == c][:max_det]
        rank[rows] = np.arange(len(rows))
        gs = np.flatnonzero(gc == c)
        ig, crowd, named = g_ig[:, gs], gcrowd[gs], gid[gs] != 0
        taken = np.zeros((n_a, n_t, len(gs)), bool)
        for r in rows:   # the chain: sequential in rows and ground truths, whole-array in (range, threshold)
            iou = _coco_iou(d[r], g[gs], crowd)
            best = np.tile(start, (n_a, 1))
            m = np.full((n_a, n_t), -1, np.int64)
            for second in (False, True):
                still = m < 0        # the walk reaches the ignored ones only where none of the others matched
                for j in np.flatnonzero(~(iou < floor)):
                    cond = (ig[:, j] == second)[:, None] & still & ~(iou[j] < best) & (~taken[:, :, j] | crowd[j])
                    best[cond], m[cond] = iou[j], j
            hit = m >= 0
            mm = np.where(hit, m, 0)
            a_idx = np.arange(n_a)[:, None]
            dt_ig = hit & ig[a_idx, mm] if len(gs) else np.zeros((n_a, n_t), bool)
            matched = hit & named[mm] if len(gs) else np.zeros((n_a, n_t), bool)
            if len(gs):
                aa, tt = np.nonzero(hit)
                taken[aa, tt, m[aa, tt]] = True
            outside = (d_area[r] < ar[:, 0]) | (d_area[r] > ar[:, 1])
            dt_ig = dt_ig | (~matched & outside[:, None])
            flags[r] = matched.astype(np.uint8) | (dt_ig.astype(np.uint8) << 1)
    return rank, flags


def coco_accumulate(image, cat, score, rank, flags, npig, rec_thrs, max_dets):
    """[UPSTREAM-RECALLED] ``COCOeval.accumulate`` over whole arrays.  One entry per detection row that took part
    (rank >= 0): image (N) its image's position among the evaluated images, cat (N) category index, score (N), rank (N)
    and flags (N, A, T) as coco_match_host gives them; npig (K, A) the ground truths not ignored per category and range.
    Returns ``precision`` (T, R, K, A, M) and ``recall`` (T, K, A, M), -1 where npig is 0.

    Per category, range and max_dets entry md: the rows with rank < md — image after image, by rank inside an image —
    sorted by -score (stable); tp = dtm != 0 and not dtIg, fp = dtm == 0 and not dtIg, summed cumulatively as float;
    rc = tp / npig, pr = tp / (fp + tp + spacing(1)); recall = rc[-1] (0 without rows); pr made non-increasing from the
    right; precision[r] = pr[searchsorted(rc, rec_thrs[r], 'left')], the assignment stopping at the first index past the
    end and leaving zeros."""
    image, cat, rank = np.asarray(image), np.asarray(cat), np.asarray(rank)
    score = np.asarray(score, np.float64)
    rec_thrs = np.asarray(rec_thrs, np.float64)
    n_k, n_a = npig.shape
    n_t, n_r, n_m = flags.shape[2], len(rec_thrs), len(max_dets)
    precision = -np.ones((n_t, n_r, n_k, n_a, n_m))
    recall = -np.ones((n_t, n_k, n_a, n_m))
    order = np.lexsort((rank, image, -score, cat))       # category; then -score, ties by image and rank: the stable sort
    cat_s, rank_s = cat[order], rank[order]
    eps = np.spacing(1)
    for k in range(n_k):
        if not npig[k].any():
            continue
        idx = order[np.searchsorted(cat_s, k, 'left'):np.searchsorted(cat_s, k, 'right')]
        rk = rank[idx]
        for mi, md in enumerate(max_dets):
            sel = idx[rk < md]
            f = flags[sel]                               # (n, A, T)
            n = len(sel)
            for a in range(n_a):
                if npig[k, a] == 0:
                    continue
                tp = np.cumsum(f[:, a, :] == 1, axis=0).astype(np.float64)        # matched and not ignored
                fp = np.cumsum(f[:, a, :] == 0, axis=0).astype(np.float64)        # unmatched and not ignored
                rc = tp / npig[k, a]
                pr = tp / (fp + tp + eps)
                pr = np.maximum.accumulate(pr[::-1], axis=0)[::-1]
                for t in range(n_t):
                    recall[t, k, a, mi] = rc[-1, t] if n else 0
                    q = np.zeros(n_r)
                    inds = np.searchsorted(rc[:, t], rec_thrs, side='left')
                    past = np.flatnonzero(inds >= n)
                    stop = past[0] if len(past) else n_r
                    q[:stop] = pr[inds[:stop], t]
                    precision[t, :, k, a, mi] = q
    return precision, recall


class COCODetectionMetric(object):
    """The COCO bbox metric: the reference's ``COCODetectionMetric`` (metrics/mscoco.py), same ``update`` / ``get`` /
    ``reset`` and ``get()`` strings, with the evaluation pycocotools does for the reference restated here
    ([UPSTREAM-RECALLED]: coco_match_host, coco_accumulate, _summarize).

    ``dataset`` is duck-typed: ``sample_ids``, ``classes``, ``build_coco_json()`` -> the path of a COCO-style ground-truth
    file (or ``dataset.coco.dataset``, the loaded dict), ``image_size(id)`` -> (width, height) when ``data_shape`` is
    given, and optionally ``contiguous_id_to_json``.  The ground-truth tables are built once, here.  Per annotation
    ``image_id``, ``category_id``, ``bbox`` (xywh), ``area`` (the file's), ``iscrowd`` and ``id`` are read; an ``ignore``
    key has no effect.  All images of the file are evaluated, in sorted id order; category k is the k-th of the file's
    sorted category ids.

    ``update`` takes a batch's images in ``sorted(dataset.sample_ids)`` order by a running counter, as the reference does;
    ``sid`` (one id per image) names them instead.  Rows with label < 0, a label outside ``contiguous_id_to_json`` or
    score < score_thresh are dropped; with ``data_shape`` (h, w) boxes are scaled to the image's own size; then
    w = x2 - (x1 - 1), h likewise (the reference's +1).  float32 tensors of one GPU with at most 1024 rows per image are
    matched on the device (vy_coco_match) on the current stream: the casts, the scale gather, the xywh step and the label
    lookup are torch calls, nothing is copied to the host and nothing synchronises; the outputs stay device tensors until
    ``get()`` copies them once.  Everything else takes the host path (coco_match_host).  Both may feed one metric, in any
    order, and give identical results: every order in the rule is a stable one.  ``device_updates`` counts the launches.

    Where this differs from the reference, on purpose: ``save_prefix`` may be None (nothing is written); a ``sid`` or a
    sample id the ground-truth file does not have, a repeated one, or more images than the dataset has raise
    ``ValueError``; thresholds, ranges and max_dets are constructor keywords (defaults: COCO's); category ids and label
    keys lie in [0, 2**20).

    After ``get()``: ``metric.stats`` (12), ``metric.precision`` (T, 101, K, A, M), ``metric.recall`` (T, K, A, M).
    """

    def __init__(self, dataset, save_prefix=None, use_time=True, cleanup=False, score_thresh=0.05, data_shape=None,
                 iou_thrs=COCO_IOU_THRS, area_ranges=COCO_AREA_RANGES, max_dets=COCO_MAX_DETS):
        self.name = 'COCOMeanAP'
        self.dataset = dataset
        self._img_ids = sorted(dataset.sample_ids)
        self._cleanup = cleanup
        self._score_thresh = float(score_thresh)
        if isinstance(data_shape, (tuple, list)):
            assert len(data_shape) == 2, "Data shape must be (height, width)"
        elif not data_shape:
            data_shape = None
        else:
            raise ValueError("data_shape must be None or tuple of int as (height, width)")
        self._data_shape = data_shape
        self._thr = np.array(iou_thrs, np.float64).reshape(-1)
        self._ar = np.array([list(r) for r in area_ranges], np.float64).reshape(-1, 2)
        self._max_dets = [int(m) for m in max_dets]
        self._rec_thrs = COCO_REC_THRS
        if not (1 <= len(self._thr) <= 16 and 1 <= len(self._ar) <= 8):
            raise ValueError("between 1 and 16 IoU thresholds and 1 and 8 area ranges")
        if not np.isfinite(self._thr).all() or not (self._ar[:, 0] <= self._ar[:, 1]).all():
            raise ValueError("a threshold that is not finite or a range with lo > hi")
        if not self._max_dets or min(self._max_dets) < 0 or sorted(self._max_dets) != self._max_dets:
            raise ValueError("max_dets must ascend")
        self._filename = None
        if save_prefix is not None:
            import datetime
            import os
            t = datetime.datetime.now().strftime('_%Y_%m_%d_%H_%M_%S') if use_time else ''
            self._filename = os.path.abspath(os.path.expanduser(save_prefix) + t + '.json')
            try:
                open(self._filename, 'w').close()
            except IOError as e:
                raise RuntimeError("Unable to open json file to dump. What(): {}".format(str(e)))
        self._build_tables()
        self._device_tables = {}
        self._scales = None
        self.device_updates = 0
        self.stats = self.precision = self.recall = None
        self.reset()

    def __del__(self):
        if getattr(self, '_cleanup', False) and getattr(self, '_filename', None):
            import os
            try:
                os.remove(self._filename)
            except OSError:
                pass

    # ------------------------------------------------------------------ the dataset's ground truth, once
    def _build_tables(self):
        ds = self.dataset
        if hasattr(ds, 'coco'):
            data = ds.coco.dataset
        else:
            import json
            with open(ds.build_coco_json()) as f:
                data = json.load(f)
        self._eval_ids = sorted(im['id'] for im in data.get('images', []))
        self._row = {i: r for r, i in enumerate(self._eval_ids)}
        if len(self._row) != len(self._eval_ids):
            raise ValueError("an image id appears twice in the ground-truth file")
        for i in self._img_ids:
            if i not in self._row:
                raise ValueError("sample id %r is not an image of the ground-truth file" % (i,))
        self._cat_ids = sorted(c['id'] for c in data.get('categories', []))
        cat_k = {c: k for k, c in enumerate(self._cat_ids)}
        per_image = [[] for _ in self._eval_ids]
        for ann in data.get('annotations', []):
            r = self._row.get(ann['image_id'])
            if r is not None:
                per_image[r].append(ann)
        anns = [a for lst in per_image for a in lst]
        self._gt_off = np.concatenate([[0], np.cumsum([len(lst) for lst in per_image], dtype=np.int64)]).astype(np.int64)
        self._gt_xywh = np.array([a['bbox'] for a in anns], np.float64).reshape(-1, 4)
        self._gt_cat = np.array([cat_k.get(a['category_id'], -1) for a in anns], np.int32).reshape(-1)
        self._gt_area = np.array([a['area'] for a in anns], np.float64).reshape(-1)
        self._gt_crowd = np.array([1 if a.get('iscrowd', 0) else 0 for a in anns], np.uint8).reshape(-1)
        self._gt_id = np.array([a['id'] for a in anns], np.int64).reshape(-1)
        n_k, n_a = len(self._cat_ids), len(self._ar)
        self._npig = np.zeros((n_k, n_a), np.int64)
        named = self._gt_cat >= 0
        for a in range(n_a):
            ok = named & (self._gt_crowd == 0) & ~((self._gt_area < self._ar[a, 0]) | (self._gt_area > self._ar[a, 1]))
            self._npig[:, a] = np.bincount(self._gt_cat[ok], minlength=n_k)
        # label -> category id of the file and category index, as tables: the same lookup on the host and on the device
        to_json = getattr(ds, 'contiguous_id_to_json', None)
        self._has_map = to_json is not None
        pairs = [(int(k), int(v)) for k, v in to_json.items()] if self._has_map else [(c, c) for c in self._cat_ids]
        if any(not (0 <= k < _COCO_LUT_MAX) for k, _ in pairs) or any(not (0 <= c < _COCO_LUT_MAX) for c in self._cat_ids):
            raise ValueError("category ids and label keys must lie in [0, %d)" % _COCO_LUT_MAX)
        size = max([k for k, _ in pairs] + [0]) + 1
        self._lut_json = np.zeros(size, np.int64)
        self._lut_k = np.full(size, -1, np.int32)
        self._lut_has = np.zeros(size, bool)
        for k, v in pairs:
            self._lut_json[k], self._lut_k[k], self._lut_has[k] = v, cat_k.get(v, -1), True

    def _scale_table(self):
        """(images of the file, 4) float64 [width, height, width, height] scales of data_shape, once."""
        if self._scales is None:
            s = np.ones((len(self._eval_ids), 4), np.float64)
            for i in self._img_ids:
                orig_width, orig_height = self.dataset.image_size(i)
                ws, hs = float(orig_width) / self._data_shape[1], float(orig_height) / self._data_shape[0]
                s[self._row[i]] = (ws, hs, ws, hs)
            self._scales = s
        return self._scales

    def _tables_on(self, dev):
        names = ('_gt_xywh', '_gt_cat', '_gt_area', '_gt_crowd', '_gt_id', '_lut_json', '_lut_k', '_lut_has')
        scale = {} if self._data_shape is None else {'scale': self._scale_table()}
        return _upload(self._device_tables, dev, **{n: getattr(self, n) for n in names}, **scale)

    def reset(self):
        self._current_id = 0
        self._chunks = []     # per update: (image rows, category index, score, rank, flags, file category, xywh)
        self._seen = set()

    # ------------------------------------------------------------------ accumulation
    def _rows_of(self, sid, batch):
        if sid is None:
            if self._current_id + batch > len(self._img_ids):
                raise ValueError("%d images after %d: the dataset has %d" % (batch, self._current_id, len(self._img_ids)))
            sids = self._img_ids[self._current_id:self._current_id + batch]
        else:
            if hasattr(sid, "tolist"):
                sid = sid.tolist()
            sids = list(sid) if isinstance(sid, (list, tuple, range)) else [sid]
            if len(sids) != batch:
                raise ValueError("%d ids for a batch of %d images" % (len(sids), batch))
        rows = []
        for s in sids:
            if s not in self._row:
                raise ValueError("sid %r is not an image of the ground-truth file" % (s,))
            if self._row[s] in self._seen or self._row[s] in rows:
                raise ValueError("sid %r was given before" % (s,))
            rows.append(self._row[s])
        if sid is None:
            self._current_id += batch
        return np.asarray(rows, np.int64)

    def update(self, pred_bboxes, pred_labels, pred_scores, *args, **kwargs):
        """pred_bboxes (B, N, 4) corners, pred_labels and pred_scores (B, N) or (B, N, 1): numpy, torch, or lists of them
        (one per device, joined along the batch).  Further positional arguments are accepted and ignored, as in the
        reference; ``sid=`` names the images."""
        sid = kwargs.pop('sid', None)
        pb, pl, ps = (_gather(x) for x in (pred_bboxes, pred_labels, pred_scores))
        on_device = all(hasattr(x, "is_cuda") and _is_gpu_f32(x) for x in (pb, pl, ps)) and \
            pb.device == pl.device == ps.device
        if not on_device:
            pb, pl, ps = (np.asarray(_to_numpy(x)) for x in (pb, pl, ps))
        batch = int(pb.shape[0])
        n = int(np.prod(pl.shape[1:])) if batch else 0
        if on_device and n > 1024:
            on_device = False
            pb, pl, ps = (np.asarray(_to_numpy(x)) for x in (pb, pl, ps))
        rows = self._rows_of(sid, batch)
        if batch and n:
            pb, pl, ps = pb.reshape(batch, n, 4), pl.reshape(batch, n), ps.reshape(batch, n)
            self._chunks.append((self._update_device if on_device else self._update_host)(pb, pl, ps, rows))
        self._seen.update(rows.tolist())

    def _update_host(self, pb, pl, ps, rows):
        batch, n = pl.shape
        n_a, n_t = len(self._ar), len(self._thr)
        size = len(self._lut_k)
        valid = pl >= 0
        with np.errstate(invalid='ignore'):
            li = np.where(valid, pl, 0).astype(np.float64)
            file_cat = li.astype(np.int64)
            li = np.minimum(li, size).astype(np.int64)
        inside = li < size
        lic = np.where(inside, li, 0)
        k = np.where(inside, self._lut_k[lic], -1)
        has = valid
        if self._has_map:
            has, file_cat = valid & inside & self._lut_has[lic], self._lut_json[lic]
        score = ps.astype(np.float64)
        keep = has & ~(score < self._score_thresh)
        box = pb.astype(np.float64)
        if self._data_shape is not None:
            box = box * self._scale_table()[rows][:, None, :]
        xywh = np.concatenate([box[..., :2], box[..., 2:] - (box[..., :2] - 1)], -1)
        cat = np.where(keep, k, -1).astype(np.int32)
        file_cat = np.where(keep, file_cat, -1)
        rank = np.zeros((batch, n), np.int32)
        flags = np.zeros((batch, n, n_a, n_t), np.uint8)
        for b, r in enumerate(rows):
            g0, g1 = self._gt_off[r], self._gt_off[r + 1]
            rank[b], flags[b] = coco_match_host(xywh[b], cat[b], score[b], self._gt_xywh[g0:g1], self._gt_cat[g0:g1],
                                                self._gt_area[g0:g1], self._gt_crowd[g0:g1], self._gt_id[g0:g1], self._thr,
                                                self._ar, self._max_dets[-1])
        return rows, cat, score, rank, flags, keep, file_cat, xywh

    def _update_device(self, pb, pl, ps, rows):
        import torch
        from . import _lib
        lib = _lib.load()
        dev = pb.device
        batch, n = pl.shape
        n_a, n_t = len(self._ar), len(self._thr)
        t = self._tables_on(dev)
        size = len(self._lut_k)
        valid = pl >= 0
        li = torch.where(valid, pl, torch.zeros_like(pl)).to(torch.float64)
        file_cat = li.to(torch.int64)
        li = li.clamp(max=size).to(torch.int64)
        inside = li < size
        lic = torch.where(inside, li, torch.zeros_like(li))
        k = torch.where(inside, t['_lut_k'][lic], torch.full_like(lic, -1, dtype=torch.int32))
        has = valid
        if self._has_map:
            has, file_cat = valid & inside & t['_lut_has'][lic], t['_lut_json'][lic]
        score = ps.to(torch.float64).contiguous()
        keep = has & ~(score < self._score_thresh)
        box = pb.to(torch.float64)
        if self._data_shape is not None:
            if len(rows) and (np.diff(rows) == 1).all():
                scale = t['scale'][int(rows[0]):int(rows[0]) + batch]
            else:
                scale = t['scale'][torch.from_numpy(rows).to(dev)]
            box = box * scale[:, None, :]
        xywh = torch.cat([box[..., :2], box[..., 2:] - (box[..., :2] - 1)], -1).contiguous()
        cat = torch.where(keep, k, torch.full_like(k, -1)).contiguous()
        file_cat = torch.where(keep, file_cat, torch.full_like(file_cat, -1))
        rank = torch.empty((batch, n), dtype=torch.int32, device=dev)
        flags = torch.empty((batch, n, n_a, n_t), dtype=torch.uint8, device=dev)
        taken_bytes = int((self._gt_off[rows + 1] - self._gt_off[rows]).sum()) * n_a * n_t
        taken = torch.empty(max(taken_bytes, 1), dtype=torch.uint8, device=dev)
        gt_image = rows.astype(np.int32)
        with torch.cuda.device(dev):
            _lib.check(lib.vy_coco_match(
                batch, n, _devp(xywh), _devp(cat), _devp(score), _hostp(gt_image), len(self._eval_ids), _hostp(self._gt_off),
                _devp(t['_gt_xywh']), _devp(t['_gt_cat']), _devp(t['_gt_area']), _devp(t['_gt_crowd']), _devp(t['_gt_id']), n_t,
                _hostp(self._thr), n_a, _hostp(np.ascontiguousarray(self._ar)), self._max_dets[-1], _devp(taken), taken_bytes,
                _devp(rank), _devp(flags), _streamp(dev)))
        self.device_updates += 1
        return rows, cat, score, rank, flags, keep, file_cat, xywh

    # ------------------------------------------------------------------ evaluation
    def _fold(self, with_boxes):
        """Every row so far, update after update: image row, category index, score, rank, flags (and kept, file category,
        xywh for the results file) as numpy arrays.  Device results are copied here, once."""
        n_a, n_t = len(self._ar), len(self._thr)
        kinds = range(1, 8 if with_boxes else 5)
        dev_chunks = [i for i, c in enumerate(self._chunks) if not isinstance(c[1], np.ndarray)]
        host = dict(zip(dev_chunks, _chunks_to_host([tuple(self._chunks[i][k] for k in kinds) for i in dev_chunks])))
        parts = {}
        for k in kinds:
            tail = (4,) if k == 7 else (n_a, n_t) if k == 4 else ()
            parts[k] = [(host[i][k - 1] if i in host else c[k]).reshape((-1,) + tail) for i, c in enumerate(self._chunks)]
        empty = {1: np.zeros(0, np.int32), 2: np.zeros(0, np.float64), 3: np.zeros(0, np.int32),
                 4: np.zeros((0, n_a, n_t), np.uint8), 5: np.zeros(0, bool), 6: np.zeros(0, np.int64),
                 7: np.zeros((0, 4), np.float64)}
        out = [np.concatenate([np.repeat(c[0], c[1].shape[1]) for c in self._chunks]) if self._chunks
               else np.zeros(0, np.int64)]
        for k in kinds:
            out.append(np.concatenate(parts[k]) if self._chunks else empty[k])
        return out

    def _write_results(self, image, keep, file_cat, xywh, score):
        """The results file the reference writes: one entry per kept row in the order of arrival (a dummy one if none)."""
        import json
        results = [{'image_id': self._eval_ids[image[i]], 'category_id': int(file_cat[i]), 'bbox': xywh[i].tolist(),
                    'score': float(score[i])} for i in np.flatnonzero(keep)]
        if not results and self._img_ids:
            results.append({'image_id': self._img_ids[0], 'category_id': 0, 'bbox': [0, 0, 0, 0], 'score': 0})
        try:
            with open(self._filename, 'w') as f:
                json.dump(results, f)
        except IOError as e:
            raise RuntimeError("Unable to dump json file, ignored. What(): {}".format(str(e)))

    def _summarize(self):
        """[UPSTREAM-RECALLED] ``COCOeval.summarize``: the twelve numbers and their printed lines."""
        thr, names = self._thr, COCO_AREA_NAMES
        template = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'

        def one(ap, iou_thr, area, md):
            a = names.index(area)
            m = [i for i, v in enumerate(self._max_dets) if v == md]
            if ap:
                s = self.precision
                if iou_thr is not None:
                    s = s[np.where(iou_thr == thr)[0]]
                s = s[:, :, :, a:a + 1 if a < len(self._ar) else 0, m]
            else:
                s = self.recall
                if iou_thr is not None:
                    s = s[np.where(iou_thr == thr)[0]]
                s = s[:, :, a:a + 1 if a < len(self._ar) else 0, m]
            mean = np.mean(s[s > -1]) if len(s[s > -1]) else -1
            iou_str = '{:0.2f}:{:0.2f}'.format(thr[0], thr[-1]) if iou_thr is None else '{:0.2f}'.format(iou_thr)
            line = template.format('Average Precision' if ap else 'Average Recall', '(AP)' if ap else '(AR)', iou_str,
                                   area, md, mean)
            return mean, line

        md = self._max_dets
        last = md[-1]
        ask = [(1, None, 'all', last), (1, .5, 'all', last), (1, .75, 'all', last), (1, None, 'small', last),
               (1, None, 'medium', last), (1, None, 'large', last), (0, None, 'all', md[0]),
               (0, None, 'all', md[min(1, len(md) - 1)]), (0, None, 'all', md[min(2, len(md) - 1)]),
               (0, None, 'small', last), (0, None, 'medium', last), (0, None, 'large', last)]
        got = [one(*q) for q in ask]
        self.stats = np.array([g[0] for g in got], np.float64)
        return '\n'.join(g[1] for g in got)

    def get(self):
        """``(names, values)`` with the reference's strings (mscoco.py:117-162): COCOeval's summary block, AP x 100 of every
        class of ``dataset.classes`` over all thresholds at the first area range and the last max_dets, and the mean."""
        if len(self._seen) != len(self._img_ids):
            import warnings
            warnings.warn('Recorded {} out of {} validation images, incomplete results'.format(
                len(self._seen), len(self._img_ids)))
        with_boxes = self._filename is not None
        folded = self._fold(with_boxes)
        image, cat, score, rank, flags = folded[:5]
        if with_boxes:
            self._write_results(image, folded[5], folded[6], folded[7], score)
        part = rank >= 0
        self.precision, self.recall = coco_accumulate(image[part], cat[part], score[part], rank[part], flags[part],
                                                      self._npig, self._rec_thrs, self._max_dets)
        summary = self._summarize()
        near = lambda v: np.flatnonzero((self._thr > v - 1e-5) & (self._thr < v + 1e-5))   # noqa: E731
        lo, hi = near(0.5), near(0.95)
        ind_lo, ind_hi = (lo[0] if len(lo) else 0), (hi[0] if len(hi) else len(self._thr) - 1)

        def mean_ap(p):
            p = p[p > -1]
            return float(np.mean(p)) if len(p) else float('nan')

        names, values = ['~~~~ Summary metrics ~~~~\n'], [summary.strip()]
        for cls_ind, cls_name in enumerate(self.dataset.classes):
            ap = mean_ap(self.precision[ind_lo:ind_hi + 1, :, cls_ind, 0, -1]) if cls_ind < len(self._cat_ids) else float('nan')
            names.append(cls_name)
            values.append('{:.1f}'.format(100 * ap))
        names.append('~~~~ MeanAP @ IoU=[{:.2f},{:.2f}] ~~~~\n'.format(0.5, 0.95))
        values.append('{:.1f}'.format(100 * mean_ap(self.precision[ind_lo:ind_hi + 1, :, :, 0, -1])))
        return names, values
