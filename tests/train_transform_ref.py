"""CPU restatement of the frames side of the training transform (csrc/augment.hip).  TEST INFRASTRUCTURE ONLY.

Reference: YOLO3VideoTrainTransform.__call__ (models/definitions/yolo/transforms.py:199-245) — random_color_distort,
random_expand, crop, imresize with interp 0..4 on the FLOAT32 frames the colour step leaves, flip, to_tensor, normalize.
Unlike the kernel, which walks back from a destination pixel to its taps, this file does what the reference does, one
whole image after another: distort the source, paste it on a filled canvas, slice the crop, resize it, mirror it.

PARITY UNPINNED, like oracle/resize_oracle.py: mxnet's operators and OpenCV's cv::resize on CV_32FC3 are not available
here, so every step is restated from memory [UPSTREAM-RECALLED], op by op in float32 (DESIGN.md §13 lists the choices),
and tests/test_train_transform_host.py cross-checks the resize against torch's nearest / bilinear / bicubic, exact block
means, and float64 sinc weights where the definitions coincide.  The Lanczos-4 weights come from the library's host
export of include/vy_math.h (vy_math_lanczos4): the one piece that is shared with the kernel rather than restated.
"""
import ctypes

import numpy as np

from oracle.resize_oracle import area_tab

F = np.float32
BRIGHTNESS, CONTRAST, SATURATION, HUE = 1, 2, 3, 4
MEAN = np.array((0.485, 0.456, 0.406), F)
STD = np.array((0.229, 0.224, 0.225), F)
FILL = np.array([m * 255 for m in (0.485, 0.456, 0.406)], F)  # random_expand(fill=[m * 255 for m in mean]) -> float32


def colour(frames, ops, hue):
    """random_color_distort's arithmetic for drawn ops [(code, a, b)]: (..., 3) uint8 -> float32."""
    v = np.asarray(frames).astype(F)
    for code, a, b in ops:
        a, b = F(a), F(b)
        if code == BRIGHTNESS:
            v = v + a
        elif code == CONTRAST:
            v = v * a
        elif code == SATURATION:
            gray = (v[..., 0] * F(0.299) + v[..., 1] * F(0.587)) + v[..., 2] * F(0.114)
            gray = (gray * b)[..., None]
            v = v * a + gray
        elif code == HUE:
            t = np.asarray(hue, F)
            v = np.stack([(v[..., 0] * t[0, c] + v[..., 1] * t[1, c]) + v[..., 2] * t[2, c] for c in range(3)], -1)
        else:
            raise ValueError(code)
        assert v.dtype == F
    return v


def lanczos4_weights(x):
    from videoyolo_amd import _lib
    w = (ctypes.c_float * 8)()
    _lib.load().vy_math_lanczos4(float(x), w)
    return np.array(w[:], F)


def _src_coord(dsize, ssize):
    scale = float(ssize) / float(dsize)
    f = ((np.arange(dsize, dtype=np.float64) + 0.5) * scale - 0.5).astype(F)
    s = np.floor(f).astype(np.int64)
    return s, (f - s.astype(F)).astype(F)


def _linear_clamp(s, f, ssize):
    lo = s < 0
    f = np.where(lo, F(0), f)
    s = np.where(lo, 0, s)
    hi = s >= ssize - 1
    f = np.where(hi, F(0), f)
    s = np.where(hi, ssize - 1, s)
    idx = np.stack([s, np.minimum(s + 1, ssize - 1)], 1)
    return idx, np.stack([F(1) - f, f], 1).astype(F)


def taps(mode, dsize, ssize):
    """(index (dsize, N), float32 weight (dsize, N)) of one axis; mode: 'nearest', 'linear', 'cubic', 'lanczos',
    'area_linear' (INTER_AREA's coordinates when a side is enlarged)."""
    scale = float(ssize) / float(dsize)
    d = np.arange(dsize, dtype=np.float64)
    if mode == "nearest":
        s = np.minimum(np.floor(d * scale).astype(np.int64), ssize - 1)
        return s[:, None], np.ones((dsize, 1), F)
    if mode == "linear":
        s, f = _src_coord(dsize, ssize)
        return _linear_clamp(s, f, ssize)
    if mode == "area_linear":
        inv_scale = float(dsize) / float(ssize)
        s = np.floor(d * scale).astype(np.int64)
        f = ((d + 1) - (s + 1) * inv_scale).astype(F)
        f = np.where(f <= 0, F(0), f - np.floor(f)).astype(F)
        return _linear_clamp(s, f, ssize)
    s, x = _src_coord(dsize, ssize)
    if mode == "cubic":
        A, one = F(-0.75), F(1)
        c0 = ((A * (x + one) - F(5) * A) * (x + one) + F(8) * A) * (x + one) - F(4) * A
        c1 = ((A + F(2)) * x - (A + F(3))) * x * x + one
        c2 = ((A + F(2)) * (one - x) - (A + F(3))) * (one - x) * (one - x) + one
        c3 = one - c0 - c1 - c2
        w = np.stack([c0, c1, c2, c3], 1)
        assert w.dtype == F
        return np.clip(s[:, None] + np.arange(-1, 3)[None, :], 0, ssize - 1), w
    if mode == "lanczos":
        w = np.stack([lanczos4_weights(v) for v in x])
        return np.clip(s[:, None] + np.arange(-3, 5)[None, :], 0, ssize - 1), w
    raise ValueError(mode)


def _separable(img, nh, nw, mode):
    """rows first: r = (S0 * a0 + S1 * a1) + ..., then columns: (R0 * b0 + R1 * b1) + ..."""
    xi, xw = taps(mode, nw, img.shape[1])
    yi, yw = taps(mode, nh, img.shape[0])
    rows = img[:, xi[:, 0], :] * xw[None, :, 0, None]
    for t in range(1, xi.shape[1]):
        rows = rows + img[:, xi[:, t], :] * xw[None, :, t, None]
    out = rows[yi[:, 0]] * yw[:, 0, None, None]
    for t in range(1, yi.shape[1]):
        out = out + rows[yi[:, t]] * yw[:, t, None, None]
    assert out.dtype == F
    return out


def _area_int(img, nh, nw, iy, ix):
    """one running float sum over the block, row-major, times 1.f / area"""
    c = img.shape[2]
    blocks = img[:nh * iy, :nw * ix].reshape(nh, iy, nw, ix, c)
    acc = np.zeros((nh, nw, c), F)
    for yy in range(iy):
        for xx in range(ix):
            acc = acc + blocks[:, yy, :, xx, :]
    return acc * (F(1.0) / F(ix * iy))


def _area_frac(img, nh, nw):
    """computeResizeAreaTab's weights; along x a float running sum from 0 in table order, along y the first row
    assigns beta * buf and the later rows add (the loop of OpenCV's ResizeArea_Invoker)."""
    h, w, c = img.shape

    def passes(tab, dsize):
        per = [[] for _ in range(dsize)]
        for di, si, alpha in tab:
            per[di].append((si, alpha))
        depth = max(len(p) for p in per)
        idx = np.zeros((depth, dsize), np.int64)
        wgt = np.zeros((depth, dsize), F)
        for d, p in enumerate(per):
            for k, (si, alpha) in enumerate(p):
                idx[k, d], wgt[k, d] = si, alpha
        return idx, wgt, np.array([len(p) for p in per])

    xi, xw, xcnt = passes(area_tab(w, nw), nw)
    buf = np.zeros((h, nw, c), F)
    for k in range(xi.shape[0]):
        live = (k < xcnt)[None, :, None]
        buf = np.where(live, buf + img[:, xi[k], :] * xw[k][None, :, None], buf)
    yi, yw, ycnt = passes(area_tab(h, nh), nh)
    out = yw[0][:, None, None] * buf[yi[0]]
    for k in range(1, yi.shape[0]):
        live = (k < ycnt)[:, None, None]
        out = np.where(live, out + yw[k][:, None, None] * buf[yi[k]], out)
    assert out.dtype == F
    return out


def imresize(img, nw, nh, interp):
    """cv::resize of one float32 (h, w, 3) image with OpenCV's flag `interp` (0 nearest, 1 linear, 2 cubic, 3 area,
    4 Lanczos-4).  Nothing is rounded or clamped."""
    img = np.asarray(img)
    assert img.dtype == F and img.ndim == 3
    h, w, _ = img.shape
    if (h, w) == (nh, nw):
        return img.copy()
    if interp == 3:
        sx, sy = float(w) / nw, float(h) / nh
        if sx >= 1 and sy >= 1:
            ix, iy = int(round(sx)), int(round(sy))
            eps = np.finfo(np.float64).eps
            if abs(sx - ix) < eps and abs(sy - iy) < eps:
                return _area_int(img, nh, nw, iy, ix)
            return _area_frac(img, nh, nw)
        return _separable(img, nh, nw, "area_linear")
    return _separable(img, nh, nw, {0: "nearest", 1: "linear", 2: "cubic", 4: "lanczos"}[interp])


def transform(src, aug, width, height, mean=MEAN, std=STD, fill=FILL):
    """The frames of one sample: src (k, h, w, 3) uint8, aug a draw of YOLO3VideoTrainTransform.draw (ops, hue, expand,
    crop, interp, flip) -> (k, 3, height, width) float32."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 4
    mean, std = np.asarray(mean, F), np.asarray(std, F)
    img = colour(src, aug["ops"], aug["hue"])
    k, h, w, c = img.shape
    if aug["expand"] is not None:
        off_x, off_y, ow, oh = aug["expand"]
        fill = np.asarray(fill, F)
        canvas = np.tile(fill.reshape(1, c), (k * oh * ow, 1)).reshape(k, oh, ow, c)
        canvas[:, off_y:off_y + h, off_x:off_x + w, :] = img
        img = canvas
    x0, y0, cw, ch = aug["crop"]
    img = img[:, y0:y0 + ch, x0:x0 + cw, :]
    assert img.shape[1:3] == (ch, cw), "the crop leaves the canvas"
    out = np.stack([imresize(f, width, height, aug["interp"]) for f in img])
    if aug["flip"]:
        out = out[:, :, ::-1, :]
    x = out / F(255.0)
    x = (x - mean) / std
    assert x.dtype == F
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2))
