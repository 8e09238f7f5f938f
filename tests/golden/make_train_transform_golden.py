"""Generates tests/golden/train_transform_golden.json by running THE REFERENCE's own augmentation code on seeded inputs.

    python tests/golden/make_train_transform_golden.py <path to the reference checkout>

What runs unmodified: models/transforms/bbox.py (numpy and utils/bbox.py only) — translate, random_crop_with_constraints,
crop, resize, flip — and models/transforms/video.py's random_color_distort / random_expand.  The latter two need mxnet,
which is not installable: a throw-away numpy stand-in for the few `nd` calls they make is injected before the import
(the way make_voc_metric_golden.py does it for the metric).  The stand-in logs each call, which is how the drawn colour
ops and their arguments are recorded; where mxnet's own summation order is not pinned it uses the project's
(gray = (r + g) + b products, dot = (s0 t0 + s1 t1) + s2 t2).  The call sequence below is
YOLO3VideoTrainTransform.__call__'s (models/definitions/yolo/transforms.py:208-237), which itself cannot be imported
(gluoncv).  np.random.randint is wrapped (not replaced) to log what it returns: the colour order, the candidate pick
and the interpolation.

Recorded per seed: the label, the draws (colour order, ops and arguments, hue matrix, expand, crop, interp, flip), the
boxes after every step, and the float32 result of the colour step on a 4 x 5 frame.
"""
import json
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MEAN = (0.485, 0.456, 0.406)
LOG = []


class ND(object):
    """The few NDArray operations random_color_distort / random_expand touch."""

    def __init__(self, a, gray=False):
        self.a, self.gray, self.context = np.asarray(a), gray, None

    shape = property(lambda self: self.a.shape)
    dtype = property(lambda self: self.a.dtype)
    size = property(lambda self: self.a.size)

    def astype(self, dt):
        return ND(self.a.astype(dt))

    def reshape(self, shape):
        return ND(self.a.reshape(shape))

    def __iadd__(self, o):
        if isinstance(o, ND):
            LOG.append(("add_gray",))
            self.a = self.a + o.a
        else:
            LOG.append(("add", o))
            self.a = self.a + np.float32(o)  # a scalar op computes in the array's type
        return self

    def __imul__(self, o):
        LOG.append(("gray_mul" if self.gray else "mul", o))
        self.a = self.a * np.float32(o)
        return self

    def __mul__(self, o):
        return ND(self.a * o.a)

    def __setitem__(self, key, val):
        self.a[key] = val.a


def _install_stand_in(ref):
    mx = types.ModuleType("mxnet")
    nd = types.ModuleType("mxnet.nd")
    base = types.ModuleType("mxnet.base")
    base.numeric_types = (float, int, np.generic)
    nd.array = lambda x, dtype=None, ctx=None: ND(np.asarray(x, dtype or np.float32))
    nd.full = lambda shape, val, dtype=None: ND(np.full(shape, val, dtype or np.float32))
    nd.tile = lambda x, reps: ND(np.tile(x.a, reps))

    def nd_sum(x, axis, keepdims):
        assert axis == 3 and keepdims and x.a.shape[3] == 3
        return ND(((x.a[..., 0] + x.a[..., 1]) + x.a[..., 2])[..., None], gray=True)

    def nd_dot(s, t):
        LOG.append(("dot", t.a.copy()))
        assert t.a.dtype == np.float32 and s.a.dtype == np.float32
        v, m = s.a, t.a
        return ND(np.stack([(v[..., 0] * m[0, c] + v[..., 1] * m[1, c]) + v[..., 2] * m[2, c] for c in range(3)], -1))

    nd.sum, nd.dot = nd_sum, nd_dot
    mx.nd, mx.base = nd, base
    sys.modules.update({"mxnet": mx, "mxnet.nd": nd, "mxnet.base": base})
    sys.path.insert(0, ref)


def _ops_from_log(log):
    """[(name, a, b)] with float32 arguments, in application order, and the hue matrix."""
    ops, hue, i = [], None, 0
    while i < len(log):
        e = log[i]
        if e[0] == "add":
            ops.append(("brightness", np.float32(e[1]), np.float32(0)))
        elif e[0] == "gray_mul":
            assert log[i + 1][0] == "mul" and log[i + 2][0] == "add_gray"
            ops.append(("saturation", np.float32(log[i + 1][1]), np.float32(e[1])))
            i += 2
        elif e[0] == "mul":
            ops.append(("contrast", np.float32(e[1]), np.float32(0)))
        elif e[0] == "dot":
            ops.append(("hue", np.float32(0), np.float32(0)))
            hue = e[1]
        else:
            raise AssertionError(e)
        i += 1
    return ops, hue


def _label(rng, kind, h, w, dtype):
    def boxes(n):
        xy = rng.uniform(0, [w * 0.8, h * 0.8], (n, 2))
        wh = rng.uniform([w * 0.05, h * 0.05], [w * 0.5, h * 0.5], (n, 2))
        x2y2 = np.minimum(xy + wh, [w - 1, h - 1])
        cls = rng.integers(0, 20, (n, 1))
        return np.concatenate([xy, x2y2, cls], 1).astype(dtype)
    if kind == "array":
        return boxes(int(rng.integers(1, 6)))
    if kind == "list":
        return [boxes(int(rng.integers(1, 4))) for _ in range(3)]
    if kind == "empty_array":
        return np.zeros((0, 5), dtype)
    return [np.zeros((0, 5), dtype) for _ in range(3)]


def _tolist(b):
    return [x.tolist() for x in b] if isinstance(b, list) else b.tolist()


def main(ref):
    _install_stand_in(ref)
    from models.transforms import bbox as tbbox
    from models.transforms import video as tvideo

    real_randint = np.random.randint
    randints = []

    def logged_randint(*a, **k):
        r = real_randint(*a, **k)
        randints.append(int(r))
        return r
    np.random.randint = logged_randint

    kinds = ["array", "array", "list", "array", "list", "array", "empty_array", "array", "list", "empty_list"]
    sizes = [(90, 120), (37, 53), (120, 160), (64, 96), (75, 50)]
    outs = [(416, 416), (96, 64), (64, 64)]
    cases = []
    for seed in range(40):
        rng = np.random.default_rng(1000 + seed)
        kind = kinds[seed % len(kinds)]
        h, w = sizes[seed % len(sizes)]
        width, height = outs[seed % len(outs)]
        dtype = np.float32 if seed % 2 == 0 else np.float64
        label = _label(rng, kind, h, w, dtype)
        frame = rng.integers(0, 256, (1, 4, 5, 3), dtype=np.uint8)
        random.seed(seed)
        np.random.seed(seed)
        del LOG[:], randints[:]
        # transforms.py:208-237
        img = tvideo.random_color_distort(ND(frame))
        ops, hue = _ops_from_log(LOG)
        steps = {}
        expand = None
        if np.random.uniform(0, 1) > 0.5:
            _, expand = tvideo.random_expand(ND(np.zeros((1, h, w, 3), np.float32)), fill=[m * 255 for m in MEAN])
            bbox = tbbox.translate(label, x_offset=expand[0], y_offset=expand[1])
            ch, cw = expand[3], expand[2]
        else:
            bbox, ch, cw = label, h, w
        steps["expand"] = _tolist(bbox)
        bbox, crop = tbbox.random_crop_with_constraints(bbox, (cw, ch))
        steps["crop"] = _tolist(bbox)
        interp = np.random.randint(0, 5)
        bbox = tbbox.resize(bbox, (crop[2], crop[3]), (width, height))
        steps["resize"] = _tolist(bbox)
        flip = bool(np.random.uniform(0, 1) > 0.5)
        if flip:
            bbox = tbbox.flip(bbox, (width, height), flip_x=True)
        steps["flip"] = _tolist(bbox)
        assert img.a.dtype == np.float32
        cases.append(dict(
            seed=seed, kind=kind, dtype=np.dtype(dtype).name, src=[h, w], out=[width, height], label=_tolist(label),
            frame=frame.tolist(), order=randints[0], ops=[[n, float(a), float(b)] for n, a, b in ops],
            hue=None if hue is None else [float(v) for v in hue.reshape(-1)],
            expand=None if expand is None else [int(v) for v in expand], crop=[int(v) for v in crop],
            interp=int(interp), flip=flip, boxes_is_list=isinstance(bbox, list), steps=steps,
            colour=[float(v) for v in img.a.reshape(-1)]))
    np.random.randint = real_randint

    # the coverage the tests rely on
    def degenerate(c):
        rows = c["steps"]["crop"]
        rows = rows if c["boxes_is_list"] else [rows]
        return any(b[2] < b[0] or b[3] < b[1] for r in rows for b in r)
    assert {c["kind"] for c in cases} == {"array", "list", "empty_array", "empty_list"}
    assert {c["expand"] is None for c in cases} == {True, False}
    assert {c["interp"] for c in cases} == {0, 1, 2, 3, 4}
    assert {c["order"] for c in cases} == {0, 1}
    assert {c["flip"] for c in cases} == {True, False}
    assert {n for c in cases for n, _, _ in c["ops"]} == {"brightness", "contrast", "saturation", "hue"}
    assert any(degenerate(c) for c in cases), "no crop left a degenerate box"
    assert any(c["kind"] == "array" and c["boxes_is_list"] for c in cases)
    with open(os.path.join(HERE, "train_transform_golden.json"), "w") as f:
        json.dump(dict(mean=list(MEAN), cases=cases), f)
    print("wrote %d cases; degenerate crops in seeds %s" % (len(cases), [c["seed"] for c in cases if degenerate(c)]))


if __name__ == "__main__":
    main(sys.argv[1])
