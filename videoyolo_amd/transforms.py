"""The steps either side of the model call in the reference's drivers, and the training transform.

  before  YOLO3VideoInferenceTransform.__call__  models/definitions/yolo/transforms.py:316-350
          (resize -> to_tensor -> normalize) as ONE HIP kernel (csrc/preproc.hip): imresize(interp=9) =
          OpenCV area (shrink) / bicubic (enlarge) / bilinear (mixed) on the uint8 frame, restated from memory
          (no OpenCV offline: the CPU checker restates every rounding step and is cross-checked against torch / exact area definitions),
          fused with to_tensor + normalize; frames already at the network size skip the resize.
  train   YOLO3VideoTrainTransform.__call__  models/definitions/yolo/transforms.py:199-294: the random draws on the
          host in the reference's order from the reference's two generators (`draw`), the frames of a whole batch of
          clips in ONE HIP launch (csrc/augment.hip), the targets through targets.YOLOV3PrefetchTargetGenerator.
  mixup   gluoncv.data.MixupDetection as train_yolov3.py:227-229, 571-581 uses it: the wrapper's draws on the host
          (MixupDetection), the two sources unblended (MixedClip), the blend inside the transform's launch.
  after   detect_yolo3.py:226 (clip to the image), :256-265 (drop id < 0 rows, boxes / image size,
          one [id, score, x1, y1, x2, y2] row per detection), :327-330 (the prediction txt line).
"""
import ctypes
import random

import numpy as np

from . import _lib

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


class YOLO3VideoInferenceTransform(object):
    def __init__(self, width, height, mean=MEAN, std=STD):
        self._width, self._height = width, height
        self._mean = np.asarray(mean, np.float32)
        self._std = np.asarray(std, np.float32)

    def __call__(self, frames, device="cuda:0"):
        """frames: (B,h,w,3) or (h,w,3) uint8 (numpy or torch), any size -> (B,3,height,width) fp32 normalised
        torch tensor on `device` (resized like timage.imresize(frame, width, height, interp=9))."""
        import torch
        lib = _lib.load()
        x = frames if isinstance(frames, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(frames))
        if x.dtype != torch.uint8:
            raise TypeError("frames must be uint8 (decoded images), got %s" % x.dtype)
        if x.dim() == 3:
            x = x[None]
        b, h, w, c = x.shape
        if c != 3:
            raise ValueError("expected (B,h,w,3) frames, got %s" % (tuple(x.shape),))
        x = x.to(device).contiguous()
        out = torch.empty((b, 3, self._height, self._width), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.vy_preprocess_resize_frames(
                ctypes.c_void_p(x.data_ptr()), h, w, ctypes.c_void_p(out.data_ptr()), b, self._height, self._width,
                self._mean.ctypes.data_as(ctypes.c_void_p), self._std.ctypes.data_as(ctypes.c_void_p),
                ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)))
        return out


# ---------------------------------------------------------------------------------------------------------------------
# The label's way through the transform.  What the reference's box helpers (models/transforms/bbox.py) compute is restated
# here in the project's own form: a label is one (N, 4+) array or a list of T of them (per-frame labels), every step
# returns copies, and x and y are handled as the strided column views [:, 0:4:2] and [:, 1:4:2].  What has to agree
# with the reference is each value's sequence of float operations and the sequence of generator calls — pinned by
# tests/golden/train_transform_golden.json, which was recorded from the reference's own module.


def _frames_of(label):
    return label if isinstance(label, list) else [label]


def _on_axes(label, fn):
    """Copies of the label's arrays with fn(xs, ys) applied in place to the (N, 2) views of their x and y columns."""
    out = []
    for boxes in _frames_of(label):
        boxes = boxes.copy()
        fn(boxes[:, 0:4:2], boxes[:, 1:4:2])
        out.append(boxes)
    return out if isinstance(label, list) else out[0]


def _shift(label, dx, dy):
    def fn(xs, ys):
        xs += dx
        ys += dy
    return _on_axes(label, fn)


def _into_window(label, window):
    """Boxes clipped to the window (x0, y0, w, h) and expressed in its coordinates.  As in the reference's crop with
    allow_outside_center=False, NOTHING is dropped: there the mask of boxes whose centre left the crop is applied to a
    local that is then discarded (bbox.py:192), so a box outside the window comes out with x2 < x1 or y2 < y1."""
    x0, y0, w, h = window

    def fn(xs, ys):
        for v, lo, hi in ((xs, x0, x0 + w), (ys, y0, y0 + h)):
            np.maximum(v[:, 0], lo, out=v[:, 0])
            np.minimum(v[:, 1], hi, out=v[:, 1])
            v -= lo
    return _on_axes(label, fn)


def _scaled(label, fx, fy):
    def fn(xs, ys):
        xs *= fx
        ys *= fy
    return _on_axes(label, fn)


def _mirrored(label, width):
    def fn(xs, ys):
        xs[:] = width - xs[:, ::-1]
    return _on_axes(label, fn)


def _iou_with_window(boxes, window):
    """IoU of every box with the pixel rectangle (x0, y0, w, h), float64.  The boxes' own areas are formed in the
    label's dtype (as the reference's are) before they meet the integer rectangle."""
    x0, y0, w, h = window
    f64 = boxes[:, :4].astype(np.float64)
    iw = np.minimum(f64[:, 2], x0 + w) - np.maximum(f64[:, 0], x0)
    ih = np.minimum(f64[:, 3], y0 + h) - np.maximum(f64[:, 1], y0)
    inter = np.where((iw > 0) & (ih > 0), iw * ih, 0.0)
    own = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    return inter / ((own.astype(np.float64) + float(w * h)) - inter)


# the SSD sampling thresholds on the IoU of every box with the crop: at least 0.1 / 0.3 / 0.5 / 0.7 / 0.9, or at most 1
_IOU_BANDS = [(lo, np.inf) for lo in (0.1, 0.3, 0.5, 0.7, 0.9)] + [(-np.inf, 1)]
_TRIALS_PER_BAND = 50


def _trial_window(R, w, h):
    """One trial of the constrained crop, four draws from `random`: a scale in [0.3, 1], an aspect ratio in
    [max(1/2, scale^2), min(2, 1/scale^2)], then the top and the left edge."""
    s = R.uniform(0.3, 1)
    s2 = s * s
    root = np.sqrt(R.uniform(max(0.5, s2), min(2, 1 / s2)))
    ch, cw = int(h * s / root), int(w * s * root)
    y0 = R.randrange(h - ch)
    x0 = R.randrange(w - cw)
    return x0, y0, cw, ch


def _constrained_crop(label, w, h, R, N):
    """The crop window of a (w, h) canvas and the label inside it (bbox.py:13-128 by behaviour).  For each IoU band up to
    50 trial windows are drawn until one keeps every box of every frame inside the band; one of the windows found, or
    the whole canvas, is then picked with np.random.randint.  Three behaviours of the reference are kept: with no box
    in any frame the very first trial window is the crop and the label comes back as it was; otherwise an array label
    comes back as a one-element list; and the first pick is final (its retry on an emptied frame never triggers)."""
    frames = _frames_of(label)
    nothing = all(len(f) == 0 for f in frames)
    found = [(0, 0, w, h)]
    for lo, hi in _IOU_BANDS:
        for _ in range(_TRIALS_PER_BAND):
            window = _trial_window(R, w, h)
            if nothing:
                return label, window
            ious = [_iou_with_window(f, window) for f in frames]
            if not any(lo > i.min() or i.max() > hi for i in ious):
                found.append(window)
                break
    window = found.pop(N.randint(0, len(found)))
    return _into_window(frames, window), window


# RGB <-> YIQ, the coefficients of the reference's hue distortion (models/transforms/video.py:133-138)
_TYIQ = np.array([[0.299, 0.587, 0.114], [0.596, -0.274, -0.321], [0.211, -0.523, 0.311]])
_ITYIQ = np.array([[1.0, 0.956, 0.621], [1.0, -0.272, -0.647], [1.0, -1.107, 1.705]])


def hue_matrix(alpha):
    """The float32 matrix t of a hue distortion by alpha half-turns, applied as pixel . t: a rotation of the I-Q plane
    between the two YIQ conversions, formed in double."""
    theta = alpha * np.pi
    rot = np.eye(3)
    rot[1:, 1:] = [[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]]
    return (_ITYIQ @ rot @ _TYIQ).T.astype(np.float32)


def _clip4(src, what):
    """A (k, h, w, 3) uint8 view of a clip or of one (h, w, 3) image (numpy or torch)."""
    if not hasattr(src, "shape"):
        src = np.asarray(src)
    if len(src.shape) == 3:
        src = src[None]
    if len(src.shape) != 4 or src.shape[3] != 3:
        raise ValueError("%s: expected (k, h, w, 3) or (h, w, 3) frames, got %s" % (what, tuple(src.shape)))
    if str(src.dtype).split(".")[-1] != "uint8":
        raise TypeError("%s: frames must be uint8 (decoded images), got %s" % (what, src.dtype))
    return src


class MixedClip(object):
    """Two uint8 clips and the ratio `lambd` of their mixup, NOT blended: what MixupDetection.__getitem__ returns for
    lambd < 1 and what YOLO3VideoTrainTransform takes wherever it takes a clip.  The blend happens in the transform's
    launch (vy_train_transform_mix), pixel by pixel as the kernel reads them.

    first, second: (k, h, w, 3) uint8 with the same k (an (h, w, 3) image is a clip of k = 1), numpy or torch, of any two
    sizes.  Both sit at the origin of a canvas of the larger height and width: ``shape`` is (k, max h, max w, 3).
    ``l1`` = float32(lambd) weighs the first, ``l2`` = float32(1.0 - lambd) — subtracted in double, then cast — the second.
    """

    def __init__(self, first, second, lambd):
        self.first, self.second = _clip4(first, "first source"), _clip4(second, "second source")
        if self.first.shape[0] != self.second.shape[0]:
            raise ValueError("a clip of %d frames cannot be mixed with one of %d: frame t is blended with frame t" % (
                self.first.shape[0], self.second.shape[0]))
        self.lambd = float(lambd)
        if not 0.0 <= self.lambd <= 1.0:
            raise ValueError("lambd must lie in [0, 1], got %r" % (lambd,))
        self.l1, self.l2 = np.float32(self.lambd), np.float32(1.0 - self.lambd)

    @property
    def shape(self):
        a, b = self.first.shape, self.second.shape
        return (int(a[0]), int(max(a[1], b[1])), int(max(a[2], b[2])), 3)

    def numpy(self):
        """The mixed clip as gluoncv materialises it, (k, max h, max w, 3) uint8 on the host — the slow path the launch
        replaces, kept for callers that want the image and as the statement of the arithmetic: a float32 canvas of
        zeros, ``canvas[:h1, :w1] = p1 * l1``, ``canvas[:h2, :w2] += p2 * l2`` (each product rounded to float32, then
        added), and astype(uint8), which truncates toward zero."""
        a, b = [s.cpu().numpy() if hasattr(s, "cpu") else np.asarray(s) for s in (self.first, self.second)]
        canvas = np.zeros(self.shape, np.float32)
        canvas[:, :a.shape[1], :a.shape[2]] = a.astype(np.float32) * self.l1
        canvas[:, :b.shape[1], :b.shape[2]] += b.astype(np.float32) * self.l2
        return canvas.astype(np.uint8)


class MixupDetection(object):
    """gluoncv.data.MixupDetection, the wrapper the reference puts round its training set (train_yolov3.py:227-229) and
    switches per epoch (:571-581): ``set_mixup(np.random.beta, 1.5, 1.5)`` turns mixing on, ``set_mixup(None)`` off
    [UPSTREAM-RECALLED: gluoncv is not available here; restated from memory, DESIGN.md §18].

    ``self[idx]`` draws in gluoncv's order — ``dataset[idx]``; ``lambd = max(0, min(1, mixup(*args)))`` (1 without a
    mixup callable); for lambd >= 1 nothing more is drawn and the first sample is returned itself, its label with a ratio
    column of ones; otherwise ``idx2 = choice(delete(arange(len(self)), idx))`` and ``dataset[idx2]`` — and returns
    (MixedClip, label): the two sources and lambd, unblended, and ``vstack(hstack(label1, lambd), hstack(label2,
    1 - lambd))``.  Boxes are not moved: both sources sit at the canvas origin.

    rng=None draws idx2 from the global ``np.random``, as gluoncv does; rng=(random.Random, np.random.RandomState), the
    pair YOLO3VideoTrainTransform takes, draws it from the RandomState (pass that RandomState's ``beta`` as the mixup
    callable to keep the global generator untouched).

    Two departures from gluoncv, both on purpose.  Clips: gluoncv reads shape[0] as the height and breaks on
    (k, h, w, 3); here frame t is blended with frame t, both samples must have the same k (ValueError otherwise), and
    (h, w, 3) is k = 1.  Label columns: a label is (N, 5) [x1, y1, x2, y2, class] or (N, 6) with the reference's
    ``difficult`` column, and comes back as (N1 + N2, 6) [x1, y1, x2, y2, class, ratio] — ``difficult`` is dropped
    rather than widening the label to seven columns, which YOLO3VideoTrainTransform.draw refuses."""

    def __init__(self, dataset, mixup=None, *args, rng=None):
        self._dataset = dataset
        self._rng = rng
        self._mixup, self._mixup_args = mixup, args

    def set_mixup(self, mixup=None, *args):
        self._mixup, self._mixup_args = mixup, args

    def __len__(self):
        return len(self._dataset)

    @staticmethod
    def _with_ratio(label, ratio):
        label = np.asarray(label)
        if label.ndim != 2 or label.shape[1] not in (5, 6):
            raise ValueError("labels are (N, 5) [x1, y1, x2, y2, class] or (N, 6) [..., difficult] arrays, got %s" % (
                label.shape,))
        return np.hstack((label[:, :5], np.full((label.shape[0], 1), ratio)))

    def __getitem__(self, idx):
        N = self._rng[1] if self._rng is not None else np.random
        img1, label1 = self._dataset[idx]
        lambd = 1
        if self._mixup is not None:
            lambd = max(0, min(1, self._mixup(*self._mixup_args)))
        if lambd >= 1:
            return img1, self._with_ratio(label1, 1.0)
        idx2 = N.choice(np.delete(np.arange(len(self)), idx))
        img2, label2 = self._dataset[idx2]
        mixed = MixedClip(img1, img2, lambd)
        return mixed, np.vstack((self._with_ratio(label1, lambd), self._with_ratio(label2, 1. - lambd)))


class YOLO3VideoTrainTransform(object):
    """The reference's training transform (models/definitions/yolo/transforms.py:167-294) for k-frame clips.

    ``draw`` makes the random draws on the host; the frames are transformed by one HIP launch per batch
    (vy_train_transform, csrc/augment.hip) and the targets by targets.YOLOV3PrefetchTargetGenerator's kernel.  The
    targets need only ``net.classes`` and the size: no forward of a copied net is run for anchors (:185-193).

    rng=None draws from the global ``random`` / ``np.random`` modules, as the reference does, so equal seeds give equal
    draws; rng=(random.Random, np.random.RandomState) uses private generators.  num_classes is accepted for the
    reference's signature: there it only sizes the one-hot slice of multi-class labels (:265), which `draw` refuses.
    """

    def __init__(self, k, width, height, net=None, mean=MEAN, std=STD, mixup=False, num_classes=-1, rng=None):
        self._k, self._width, self._height = int(k), int(width), int(height)
        self._mean = np.asarray(mean, np.float32)
        self._std = np.asarray(std, np.float32)
        self._fill = np.asarray([m * 255 for m in mean], np.float32)  # random_expand(fill=[m * 255 for m in mean])
        self._mixup = mixup
        self._rng = rng
        self._target_generator = None
        if net is not None:
            from . import targets
            self._target_generator = targets.YOLOV3PrefetchTargetGenerator(num_class=len(net.classes))

    # -- the draw -------------------------------------------------------------------------------------------------------
    def draw(self, src_h, src_w, label):
        """The random draws of one __call__ for a (src_h, src_w) source, in the reference's order, and the label's
        way through them.  label: one (N, 5+) array or a list of T arrays (per-frame labels; both take the same crop).

        Returns (aug, boxes).  aug is a dict: ``order`` (np.random.randint(0, 2): 1 = contrast, saturation, hue; 0 =
        saturation, hue, contrast), ``ops`` (the applied colour ops in order, (code, a, b) with float32 arguments:
        brightness delta / contrast alpha / saturation (alpha, 1 - alpha)), ``hue`` (the float32 3x3 matrix or None),
        ``expand`` ((off_x, off_y, ow, oh) or None), ``crop`` ((x0, y0, w, h) in the canvas), ``interp`` (0..4),
        ``flip``, ``src`` ((h, w)) and ``steps`` (the boxes after expand / crop / resize / flip).  boxes is the
        transformed label: a list (one element for an array label) unless every label is empty."""
        R, N = self._rng if self._rng is not None else (random, np.random)
        for b in _frames_of(label):
            if np.ndim(b) != 2 or np.shape(b)[-1] not in (5, 6):
                raise NotImplementedError("labels are (N, 5) [x1, y1, x2, y2, class] or (N, 6) [..., mix ratio] arrays; "
                                          "multi-class one-hot labels are not supported")
        f32 = np.float32
        ops, hue_t = [], None
        # random_color_distort (models/transforms/video.py:68-158)
        if N.uniform(0, 1) > 0.5:
            ops.append((_lib.VY_AUG_BRIGHTNESS, f32(N.uniform(-32, 32)), f32(0)))

        def contrast():
            if N.uniform(0, 1) > 0.5:
                ops.append((_lib.VY_AUG_CONTRAST, f32(N.uniform(0.5, 1.5)), f32(0)))

        def saturation():
            if N.uniform(0, 1) > 0.5:
                alpha = N.uniform(0.5, 1.5)
                ops.append((_lib.VY_AUG_SATURATION, f32(alpha), f32(1.0 - alpha)))

        def hue():
            if N.uniform(0, 1) > 0.5:
                ops.append((_lib.VY_AUG_HUE, f32(0), f32(0)))
                return hue_matrix(R.uniform(-18, 18))
            return None

        order = int(N.randint(0, 2))
        if order:
            contrast()
            saturation()
            hue_t = hue()
        else:
            saturation()
            hue_t = hue()
            contrast()
        steps = {}
        # random_expand with probability 0.5 (video.py:12-65), keep_ratio
        h, w = int(src_h), int(src_w)
        expand, bbox = None, label
        if N.uniform(0, 1) > 0.5:
            ratio = R.uniform(1, 4)
            oh, ow = int(h * ratio), int(w * ratio)
            off_y = R.randint(0, oh - h)
            off_x = R.randint(0, ow - w)
            expand = (off_x, off_y, ow, oh)
            bbox = _shift(label, off_x, off_y)
            h, w = oh, ow
        steps["expand"] = bbox
        bbox, crop = _constrained_crop(bbox, w, h, R, N)
        steps["crop"] = bbox
        interp = int(N.randint(0, 5))
        bbox = _scaled(bbox, self._width / crop[2], self._height / crop[3])
        steps["resize"] = bbox
        flip = bool(N.uniform(0, 1) > 0.5)
        if flip:
            bbox = _mirrored(bbox, self._width)
        steps["flip"] = bbox
        aug = dict(src=(int(src_h), int(src_w)), order=order, ops=ops, hue=hue_t, expand=expand,
                   crop=tuple(int(c) for c in crop), interp=interp, flip=flip, steps=steps)
        return aug, bbox

    @staticmethod
    def descriptor(aug, src_offset=0):
        """The vy_train_aug of a draw."""
        d = _lib.TrainAug()
        d.src_offset = int(src_offset)
        d.src_h, d.src_w = aug["src"]
        if aug["expand"] is not None:
            d.paste_x, d.paste_y, d.canvas_w, d.canvas_h = aug["expand"]
        else:
            d.paste_x, d.paste_y, d.canvas_w, d.canvas_h = 0, 0, d.src_w, d.src_h
        d.crop_x, d.crop_y, d.crop_w, d.crop_h = aug["crop"]
        d.interp, d.flip = int(aug["interp"]), int(bool(aug["flip"]))
        d.num_ops = len(aug["ops"])
        for i, (code, a, b) in enumerate(aug["ops"]):
            d.op[i], d.a[i], d.b[i] = int(code), float(a), float(b)
        if aug["hue"] is not None:
            for j in range(3):
                for c in range(3):
                    d.hue[j][c] = float(aug["hue"][j][c])
        return d

    # -- the frames -----------------------------------------------------------------------------------------------------
    def transform_frames(self, srcs, augs, device="cuda:0"):
        """One launch sequence for a batch: srcs is a list of (k, h, w, 3) uint8 clips (numpy or torch, sizes may differ
        between samples, k is the same for all) or MixedClips, augs their draws (a MixedClip's for its canvas size) ->
        (B, k, 3, height, width) fp32 on `device`.  Every source, both of a MixedClip, goes into the one packed buffer;
        the batch goes out through vy_train_transform_mix if any sample is mixed, else through vy_train_transform."""
        import torch
        lib = _lib.load()
        dev = torch.device(device)
        flat, off = [], 0
        k = int(srcs[0].shape[0])

        def pack(s):
            nonlocal off
            t = s if isinstance(s, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(s))
            if t.dtype != torch.uint8:
                raise TypeError("frames must be uint8 (decoded images), got %s" % t.dtype)
            if t.dim() != 4 or t.shape[0] != k or t.shape[3] != 3:
                raise ValueError("expected (%d,h,w,3) frames, got %s" % (k, tuple(t.shape)))
            flat.append(t.reshape(-1))
            at = off
            off += t.numel()
            return at

        offs, mixes = [], []
        for s in srcs:
            m = _lib.TrainMix()
            if isinstance(s, MixedClip):
                offs.append(pack(s.first))
                m.src2_offset = pack(s.second)
                (m.h1, m.w1), (m.h2, m.w2) = s.first.shape[1:3], s.second.shape[1:3]
                m.l1, m.l2 = float(s.l1), float(s.l2)
            else:
                offs.append(pack(s))
                m.src2_offset = -1
                m.h1, m.w1 = m.h2, m.w2 = s.shape[1:3]
                m.l1, m.l2 = 1.0, 0.0
            mixes.append(m)
        if len({f.device for f in flat}) == 1 and flat[0].device == dev:
            buf = torch.cat(flat)
        else:  # one buffer on the host, one copy
            buf = torch.cat([f.cpu() for f in flat]).to(dev)
        for s, a in zip(srcs, augs):  # the kernel reads k frames of the draw's size from the sample's offset
            if tuple(s.shape[1:3]) != tuple(a["src"]):
                raise ValueError("a draw for a %s source was given %s frames" % (a["src"], tuple(s.shape[1:3])))
        descs = (_lib.TrainAug * len(srcs))(*[self.descriptor(a, o) for a, o in zip(augs, offs)])
        out = torch.empty((len(srcs), k, 3, self._height, self._width), dtype=torch.float32, device=dev)
        tail = (len(srcs), k, ctypes.c_void_p(out.data_ptr()), self._height, self._width,
                self._fill.ctypes.data_as(ctypes.c_void_p), self._mean.ctypes.data_as(ctypes.c_void_p),
                self._std.ctypes.data_as(ctypes.c_void_p))
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            if any(isinstance(s, MixedClip) for s in srcs):
                _lib.check(lib.vy_train_transform_mix(ctypes.c_void_p(buf.data_ptr()), descs,
                                                      (_lib.TrainMix * len(srcs))(*mixes), *tail, stream))
            else:
                _lib.check(lib.vy_train_transform(ctypes.c_void_p(buf.data_ptr()), descs, *tail, stream))
        return out

    # -- the targets ----------------------------------------------------------------------------------------------------
    def _gt(self, box_lists):
        """Rows of (M_i, 5+) transformed labels -> gt_boxes (R, M, 4), gt_ids (R, M, 1), mix ratio (R, M, 1) or None,
        fp32, padded with -1 to the longest row (the reference's batchify pads the same way)."""
        m = max([len(b) for b in box_lists] + [0])
        gb = np.full((len(box_lists), m, 4), -1, np.float32)
        gi = np.full((len(box_lists), m, 1), -1, np.float32)
        gm = np.full((len(box_lists), m, 1), -1, np.float32) if self._mixup else None
        for r, b in enumerate(box_lists):
            gb[r, :len(b)] = b[:, :4]
            gi[r, :len(b)] = b[:, 4:5]
            if gm is not None:
                gm[r, :len(b)] = b[:, -1:]
        return gb, gi, gm

    def __call__(self, src, label, device="cuda:0"):
        """One sample.  src: (k, h, w, 3) or (h, w, 3) uint8, or a MixedClip (drawn for its canvas size).  net=None: the image, (k, 3, H, W) or (3, H, W) fp32 on
        `device`.  With a net: (img, objectness, center_targets, scale_targets, weights, class_targets, gt_boxes) as the
        reference returns them — for an array label one set ((N, 1) ... (M, 4)); for a list label stacked per frame,
        (T, N, 1) ... and gt_boxes (T, M, 4), M the longest frame's box count (at most 100), shorter frames padded
        with -1.  NOT (T, 100, 4): the reference fills a (T, 100, 4) buffer of -1 (:253) and returns
        ``gt_bboxes_t[:, :max_boxes, :]`` (:294); this returns that slice, since the contract is what the reference's
        call returns."""
        import torch
        t = src if isinstance(src, (torch.Tensor, MixedClip)) else torch.as_tensor(np.ascontiguousarray(src))
        was_three = len(t.shape) == 3
        if was_three:
            t = t[None]
        aug, bbox = self.draw(t.shape[1], t.shape[2], label)
        img = self.transform_frames([t], [aug], device)[0]
        if was_three:
            img = img[0]
        if self._target_generator is None:
            return img
        rows = bbox if isinstance(bbox, list) else [bbox]
        if any(len(b) > 100 for b in rows):
            raise ValueError("more than 100 boxes in a frame (transforms.py:253)")
        gb, gi, gm = self._gt(rows)
        fixed = self._target_generator(self._height, self._width, gb, gi, gm, device=device)
        gt = torch.as_tensor(gb).to(device)
        if len(rows) == 1:
            return (img,) + tuple(f[0] for f in fixed) + (gt[0],)
        return (img,) + tuple(fixed) + (gt,)

    def batch(self, srcs, labels, device="cuda:0"):
        """A training batch: one draw per sample, the sources packed into one device buffer, ONE vy_train_transform call
        and ONE vy_prefetch_targets call.  srcs: B clips (k, h, w, 3) uint8 (or (h, w, 3) with k = 1) of any sizes, or
        MixedClips as MixupDetection returns them (drawn for their canvas size; the call is then vy_train_transform_mix);
        labels: B (N_i, 5+) arrays, one label set per clip.  Returns (x, gt_boxes, objectness, center_targets,
        scale_targets, weights, class_targets): x (B, k, 3, H, W) — (B, 3, H, W) for k = 1 — and the six training
        inputs of net(x, gt_boxes, obj_t, centers_t, scales_t, weights_t, clas_t)."""
        import torch
        if self._target_generator is None:
            raise ValueError("batch() builds targets: construct the transform with net=")
        if len(srcs) != len(labels) or not len(srcs):
            raise ValueError("one label per clip")
        clips, augs, rows = [], [], []
        for s, label in zip(srcs, labels):
            if isinstance(label, list):
                raise ValueError("batch() takes one label array per clip (the nets train on one label set per sample)")
            t = s if isinstance(s, (torch.Tensor, MixedClip)) else torch.as_tensor(np.ascontiguousarray(s))
            if len(t.shape) == 3:
                t = t[None]
            if len(t.shape) != 4 or t.shape[0] != self._k:
                raise ValueError("expected clips of %d frames, got %s" % (self._k, tuple(t.shape)))
            aug, bbox = self.draw(t.shape[1], t.shape[2], label)
            clips.append(t)
            augs.append(aug)
            rows.append(bbox[0] if isinstance(bbox, list) else bbox)
        x = self.transform_frames(clips, augs, device)
        if self._k == 1:
            x = x[:, 0]
        gb, gi, gm = self._gt(rows)
        fixed = self._target_generator(self._height, self._width, gb, gi, gm, device=device)
        return (x, torch.as_tensor(gb).to(device)) + tuple(fixed)


def postprocess(ids, scores, bboxes, size):
    """detect_yolo3.py:226,256-265 for one batch: clip boxes to [0, size], keep rows with id >= 0,
    normalise boxes by size.  Returns a list (per image) of float arrays (k, 6): id, score, x1, y1, x2, y2."""
    to_np = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    ids, scores, bboxes = to_np(ids), to_np(scores), to_np(bboxes)
    bboxes = np.clip(bboxes, 0, size)
    out = []
    for i in range(ids.shape[0]):
        valid = np.where(ids[i].flat >= 0)[0]
        box = bboxes[i][valid, :] / size
        out.append(np.concatenate([ids[i].flat[valid].astype(int)[:, None].astype(np.float64),
                                   scores[i].flat[valid][:, None].astype(np.float64),
                                   box.astype(np.float64)], axis=1))
    return out


def prediction_lines(img_path, rows):
    """The reference's prediction file format (detect_yolo3.py:327-330):
    ``path,class,score,x1,y1,x2,y2`` per detection, class printed as an int."""
    return ["{},{},{},{},{},{},{}\n".format(img_path, int(r[0]), r[1], r[2], r[3], r[4], r[5]) for r in rows]
