"""-m "not gpu": the training transform on the host — `draw` against draws and boxes recorded from the reference's own
code (tests/golden/train_transform_golden.json, written by tests/golden/make_train_transform_golden.py), the CPU checker
(tests/train_transform_ref.py) against the recorded colour step and against independent resize definitions, the shared
Lanczos-4 weights against float64, and vy_train_transform's descriptor validation.  Nothing here launches a kernel."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

import train_transform_ref as R
from videoyolo_amd import _lib
from videoyolo_amd.transforms import YOLO3VideoTrainTransform

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = float(np.finfo(np.float32).eps)  # 2^-23: one ulp of a float32 in [1, 2)
CODES = {"brightness": 1, "contrast": 2, "saturation": 3, "hue": 4}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "train_transform_golden.json")) as f:
        return json.load(f)["cases"]


def _label(c):
    if c["kind"] in ("list", "empty_list"):
        return [np.asarray(b, c["dtype"]).reshape(-1, 5) for b in c["label"]]
    return np.asarray(c["label"], c["dtype"]).reshape(-1, 5)


def _same_boxes(got, want, dtype):
    w = np.asarray(want, dtype).reshape(-1, 5)
    return got.dtype == w.dtype and got.shape == w.shape and np.array_equal(got, w)


def _check_draw(c, aug, boxes):
    assert aug["order"] == c["order"]
    assert [(code, float(a), float(b)) for code, a, b in aug["ops"]] == [(CODES[n], a, b) for n, a, b in c["ops"]]
    if c["hue"] is None:
        assert aug["hue"] is None
    else:
        assert aug["hue"].dtype == np.float32 and np.array_equal(aug["hue"].reshape(-1), np.asarray(c["hue"], np.float32))
    assert aug["expand"] == (None if c["expand"] is None else tuple(c["expand"]))
    assert aug["crop"] == tuple(c["crop"]) and aug["interp"] == c["interp"] and aug["flip"] == c["flip"]
    assert aug["src"] == tuple(c["src"])
    assert isinstance(boxes, list) == c["boxes_is_list"] and boxes is aug["steps"]["flip"]
    for step in ("expand", "crop", "resize", "flip"):
        got, want = aug["steps"][step], c["steps"][step]
        if isinstance(got, list):  # per frame (or the one-element list the crop makes of an array label)
            assert len(got) == len(want) and all(_same_boxes(g, w, c["dtype"]) for g, w in zip(got, want)), (c["seed"], step)
        else:
            assert _same_boxes(got, want, c["dtype"]), (c["seed"], step)


def test_golden_covers_what_the_tests_need(golden):
    assert len(golden) >= 40
    assert {c["kind"] for c in golden} == {"array", "list", "empty_array", "empty_list"}
    assert {c["interp"] for c in golden} == {0, 1, 2, 3, 4} and {c["order"] for c in golden} == {0, 1}
    assert {c["expand"] is None for c in golden} == {True, False}
    degenerate = [c["seed"] for c in golden for r in (c["steps"]["crop"] if c["boxes_is_list"] else [c["steps"]["crop"]])
                  for b in r if b[2] < b[0] or b[3] < b[1]]
    assert degenerate, "no crop with a degenerate box"
    # an array label comes back as a one-element list unless every label is empty
    assert all(c["boxes_is_list"] for c in golden if c["kind"] == "array")
    assert not any(c["boxes_is_list"] for c in golden if c["kind"] == "empty_array")


def test_draw_reproduces_the_reference_under_the_global_seeds(golden):
    for c in golden:
        t = YOLO3VideoTrainTransform(1, c["out"][0], c["out"][1])
        label = _label(c)
        keep = [b.copy() for b in label] if isinstance(label, list) else label.copy()
        random.seed(c["seed"])
        np.random.seed(c["seed"])
        aug, boxes = t.draw(c["src"][0], c["src"][1], label)
        _check_draw(c, aug, boxes)
        # the caller's label is not written to
        assert all(np.array_equal(a, b) for a, b in zip(label, keep)) if isinstance(label, list) else np.array_equal(label, keep)


def test_private_generators_give_the_same_draws_and_leave_the_global_ones_alone(golden):
    random.seed(99)
    np.random.seed(99)
    want = (random.random(), np.random.uniform())
    random.seed(99)
    np.random.seed(99)
    for c in golden[:12]:
        t = YOLO3VideoTrainTransform(1, c["out"][0], c["out"][1],
                                     rng=(random.Random(c["seed"]), np.random.RandomState(c["seed"])))
        aug, boxes = t.draw(c["src"][0], c["src"][1], _label(c))
        _check_draw(c, aug, boxes)
    assert (random.random(), np.random.uniform()) == want


def test_multi_class_labels_are_refused():
    t = YOLO3VideoTrainTransform(1, 64, 64)
    with pytest.raises(NotImplementedError, match="multi-class"):
        t.draw(48, 48, np.zeros((2, 24), np.float32))
    with pytest.raises(NotImplementedError):
        t.draw(48, 48, [np.zeros((1, 5), np.float32), np.zeros((1, 9), np.float32)])


def test_checker_colour_step_equals_the_recorded_arrays(golden):
    for c in golden:
        ops = [(CODES[n], a, b) for n, a, b in c["ops"]]
        hue = None if c["hue"] is None else np.asarray(c["hue"], np.float32).reshape(3, 3)
        got = R.colour(np.asarray(c["frame"], np.uint8), ops, hue)
        want = np.asarray(c["colour"], np.float32).reshape(1, 4, 5, 3)
        assert got.dtype == np.float32 and np.array_equal(got, want), c["seed"]
    assert any(len(c["ops"]) == 4 for c in golden) or any(len(c["ops"]) == 3 for c in golden)


def test_descriptor_of_a_draw(golden):
    c = next(c for c in golden if c["expand"] is not None and c["hue"] is not None)
    random.seed(c["seed"])
    np.random.seed(c["seed"])
    aug, _ = YOLO3VideoTrainTransform(1, c["out"][0], c["out"][1]).draw(c["src"][0], c["src"][1], _label(c))
    d = YOLO3VideoTrainTransform.descriptor(aug, 77)
    assert ctypes.sizeof(d) == 144 and d.src_offset == 77
    assert (d.paste_x, d.paste_y, d.canvas_w, d.canvas_h) == tuple(c["expand"])
    assert (d.crop_x, d.crop_y, d.crop_w, d.crop_h) == tuple(c["crop"]) and (d.src_h, d.src_w) == tuple(c["src"])
    assert d.num_ops == len(c["ops"]) and [d.op[i] for i in range(d.num_ops)] == [CODES[n] for n, _, _ in c["ops"]]
    assert [d.hue[j][k] for j in range(3) for k in range(3)] == c["hue"]


# ---------------------------------------------------------------------------------------------------------------------
# the checker's resize against independent definitions.  The images hold the values a distorted frame can take
# (beyond [0, 255], negative too).  Tolerances are in ulps of the image's largest magnitude: every output is a sum of
# products weight * pixel with the weights summing to 1 in magnitude <= 1.7 (cubic), so the two sides' rounding
# differences scale with that magnitude, not with the (possibly cancelling) result.

def _image(h, w, seed):
    return (np.random.default_rng(seed).uniform(-120, 420, (h, w, 3))).astype(np.float32)


def _torch_resize(img, nh, nw, mode):
    import torch
    x = torch.as_tensor(img.transpose(2, 0, 1)[None].copy())
    kw = {} if mode == "nearest" else {"align_corners": False}
    y = torch.nn.functional.interpolate(x, size=(nh, nw), mode=mode, **kw)
    return y[0].numpy().transpose(1, 2, 0)


# dyadic scales (x2, x0.5, x1.5, x0.75, x0.25): the source coordinate (d + 0.5) * scale - 0.5 is then exact in float32 on
# both sides (torch forms it from a float32 scale, the checker from a double one), so what is compared is the
# interpolation arithmetic and not a coordinate that may round differently
SHAPES = [((24, 40), (48, 80)), ((48, 80), (24, 40)), ((48, 72), (32, 48)), ((24, 36), (32, 48)), ((24, 80), (48, 40)),
          ((64, 32), (16, 8))]


@pytest.mark.parametrize("src,dst", SHAPES)
def test_checker_nearest_is_torch_nearest(src, dst):
    img = _image(src[0], src[1], 1)
    assert np.array_equal(R.imresize(img, dst[1], dst[0], 0), _torch_resize(img, dst[0], dst[1], "nearest"))


@pytest.mark.parametrize("src,dst", SHAPES)
def test_checker_linear_is_torch_bilinear(src, dst):
    """Same taps and weights (1 - f, f) with f exact; the sides differ in the order of the four products' sum: at most
    3 roundings each of half an ulp of the magnitude -> 4 ulp bounds the difference."""
    img = _image(src[0], src[1], 2)
    got, want = R.imresize(img, dst[1], dst[0], 1), _torch_resize(img, dst[0], dst[1], "bilinear")
    assert np.abs(got - want).max() <= 4 * EPS * np.abs(img).max()


@pytest.mark.parametrize("src,dst", SHAPES)
def test_checker_cubic_is_torch_bicubic(src, dst):
    """Keys A = -0.75 on both sides, tap indices clamped on both, source coordinates exact.  The weights are the same cubic
    polynomials evaluated in a different operation order (OpenCV takes the fourth as 1 - the others): a fraction of an
    ulp of 1 each.  With sum of |weights| <= 1.7 over the 16 taps, the weight differences and the differently ordered
    float32 sums stay within a few ulp of the image's magnitude: 4."""
    img = _image(src[0], src[1], 3)
    got, want = R.imresize(img, dst[1], dst[0], 2), _torch_resize(img, dst[0], dst[1], "bicubic")
    assert np.abs(got - want).max() <= 4 * EPS * np.abs(img).max()


@pytest.mark.parametrize("src,dst", [((48, 80), (24, 40)), ((63, 60), (21, 12)), ((64, 32), (16, 8))])
def test_checker_integer_area_is_the_block_mean(src, dst):
    """Integer-valued pixels: the running float32 sum of a block is exact (< 2^24), so the result is the exact sum
    times the rounded 1.f / area, rounded: within 1 ulp of the exact mean (2 roundings of half an ulp)."""
    img = np.random.default_rng(4).integers(-300, 600, (src[0], src[1], 3)).astype(np.float32)
    iy, ix = src[0] // dst[0], src[1] // dst[1]
    want = img.astype(np.float64).reshape(dst[0], iy, dst[1], ix, 3).mean(axis=(1, 3))
    got = R.imresize(img, dst[1], dst[0], 3)
    assert np.all(np.abs(got - want) <= EPS * np.abs(want))


def test_checker_fractional_area_is_the_overlap_weighted_mean():
    """120 x 160 -> 64 x 96 (x1.875, x1.667): each output is the mean of the source over its cell, pixels weighted by
    their overlap — stated here in float64 from the definition.  float32 weights (half an ulp each) and a running sum
    of up to 3 x 3 products: 8 ulp of the magnitude bounds the difference."""
    img = _image(120, 160, 5)
    h, w, nh, nw = 120, 160, 64, 96

    def overlap(ssize, dsize):
        m = np.zeros((dsize, ssize))
        sc = ssize / dsize
        for d in range(dsize):
            for s in range(ssize):
                m[d, s] = max(0.0, min(s + 1, (d + 1) * sc) - max(s, d * sc)) / sc
        return m
    want = np.einsum("ys,swc,xw->yxc", overlap(h, nh), img.astype(np.float64), overlap(w, nw))
    got = R.imresize(img, nw, nh, 3)
    assert np.abs(got - want).max() <= 8 * EPS * np.abs(img).max()


def test_checker_area_enlarging_is_linear_with_area_coordinates():
    """37 x 53 -> 64 x 96 with INTER_AREA: taps s = floor(d * scale), s + 1 and weight f = frac((d + 1) - (s + 1) / scale)
    where that is positive — checked against the same definition in float64."""
    img = _image(37, 53, 6)
    got = R.imresize(img, 96, 64, 3)

    def mat(ssize, dsize):
        m = np.zeros((dsize, ssize))
        sc, inv = ssize / dsize, dsize / ssize
        for d in range(dsize):
            s = int(np.floor(d * sc))
            f = (d + 1) - (s + 1) * inv
            f = 0.0 if f <= 0 else f - np.floor(f)
            if s >= ssize - 1:
                s, f = ssize - 1, 0.0
            m[d, s] += 1 - f
            m[d, min(s + 1, ssize - 1)] += f
        return m
    want = np.einsum("ys,swc,xw->yxc", mat(37, 64), img.astype(np.float64), mat(53, 96))
    # f and 1 - f are float32 roundings (<= 2^-25 each) of a value in [0, 1) that double arithmetic gives to ~1e-14; a
    # weight error e moves an output by at most e |P1 - P0| <= 2 e max|img|: 2 * 2^-24 max|img| = 1 ulp per axis.  The
    # float32 sums (two products and an addition per axis) add at most 3 half-ulps each: 8 ulp bounds the total.
    assert np.abs(got - want).max() <= 8 * EPS * np.abs(img).max()


def test_same_size_is_a_copy():
    img = _image(9, 11, 7)
    for interp in range(5):
        assert np.array_equal(R.imresize(img, 11, 9, interp), img)


def test_lanczos_weights_against_float64_sinc():
    """vy_lanczos4_weights (include/vy_math.h) through its host export against sinc(d) sinc(d / 4), d = x + 3 - i,
    normalised, in float64.  No numerator is a difference, so each weight carries only its own roundings: a polynomial
    (<= 2 ulp), d (1/2), d * d (1/2), the divide (1/2), the sum's reciprocal (the weights alternate in sign with sum of
    |w| <= 1.7 |sum|) and the final product (1/2).  Those are independent roundings of about half an ulp each, not worst
    cases stacked: a few ulp relative, asserted as 6.  x = 1.0 (a coordinate a hair below an integer rounds there in
    float) is the next tap's sample: a unit weight at tap 4, as float64 gives."""
    xs = np.concatenate([np.linspace(0, 1, 257)[:-1], [1.2e-7, 1e-6, 1e-4, 1e-3, 0.999, 1 - 2.0 ** -24,
                                                       np.nextafter(np.float32(1), np.float32(0)), 1.0]]).astype(np.float32)
    worst = 0.0
    for x in xs:
        got = R.lanczos4_weights(x).astype(np.float64)
        d = float(x) + 3 - np.arange(8)
        want = np.sinc(d) * np.sinc(d / 4)
        want = want / want.sum()
        assert np.isfinite(got).all(), x
        if x >= 1:
            assert np.array_equal(got, np.eye(8)[4]) and np.abs(got - want).max() <= EPS
            continue
        if x < np.float32(1.1920928955e-7):  # OpenCV's unit weight below FLT_EPSILON: off by the neighbours' O(x) weights
            assert np.array_equal(got, np.eye(8)[3])
            assert np.abs(got - want).max() <= EPS
            continue
        assert abs(got.sum() - 1) <= 4 * EPS
        rel = np.abs(got - want) / np.abs(want)
        worst = max(worst, rel.max())
        assert rel.max() <= 6 * EPS, (x, got, want)
    print("worst relative error %.2f ulp" % (worst / EPS))


# ---------------------------------------------------------------------------------------------------------------------

def _valid():
    d = _lib.TrainAug()
    d.src_offset, d.src_h, d.src_w = 0, 30, 40
    d.paste_x, d.paste_y, d.canvas_w, d.canvas_h = 5, 7, 80, 60
    d.crop_x, d.crop_y, d.crop_w, d.crop_h = 3, 1, 50, 40
    d.interp, d.flip, d.num_ops = 2, 1, 2
    d.op[0], d.op[1] = 1, 4
    return d


BAD = {
    "crop leaves the canvas (x)": lambda d: setattr(d, "crop_w", 78),
    "crop leaves the canvas (y)": lambda d: setattr(d, "crop_y", 21),
    "negative crop offset": lambda d: setattr(d, "crop_x", -1),
    "paste leaves the canvas": lambda d: setattr(d, "paste_x", 41),
    "negative paste offset": lambda d: setattr(d, "paste_y", -1),
    "canvas smaller than the source": lambda d: setattr(d, "canvas_h", 36),
    "zero crop": lambda d: setattr(d, "crop_h", 0),
    "zero source": lambda d: setattr(d, "src_w", 0),
    "zero canvas": lambda d: setattr(d, "canvas_w", 0),
    "interp 5": lambda d: setattr(d, "interp", 5),
    "interp -1": lambda d: setattr(d, "interp", -1),
    "interp 9": lambda d: setattr(d, "interp", 9),
    "unknown op": lambda d: d.op.__setitem__(1, 5),
    "op 0": lambda d: d.op.__setitem__(0, 0),
    "too many ops": lambda d: setattr(d, "num_ops", 5),
    "negative op count": lambda d: setattr(d, "num_ops", -1),
    "negative offset": lambda d: setattr(d, "src_offset", -3),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_bad_descriptors_are_refused_before_anything_is_launched(what):
    """VY_ERR_INVALID with bogus non-null device pointers that are never dereferenced; the bad descriptor is the LAST of
    a batch longer than one chunk, so a launch-as-you-go implementation would have launched by then."""
    lib = _lib.load()
    n = _lib.VY_AUG_CHUNK + 2
    descs = (_lib.TrainAug * n)(*[_valid() for _ in range(n)])
    BAD[what](descs[n - 1])
    p = ctypes.c_void_p(0x1000)
    three = (ctypes.c_float * 3)(1, 1, 1)
    rc = lib.vy_train_transform(p, descs, n, 3, p, 64, 96, three, three, three, None)
    assert rc == -1, (what, rc)
    assert "descriptor %d" % (n - 1) in lib.vy_last_error().decode()


def test_bad_arguments_are_refused():
    lib = _lib.load()
    descs = (_lib.TrainAug * 1)(_valid())
    p = ctypes.c_void_p(0x1000)
    three = (ctypes.c_float * 3)(1, 1, 1)
    for args in ((None, descs, 1, 1, p, 64, 64, three, three, three), (p, None, 1, 1, p, 64, 64, three, three, three),
                 (p, descs, 0, 1, p, 64, 64, three, three, three), (p, descs, 1, 0, p, 64, 64, three, three, three),
                 (p, descs, 1, 1, None, 64, 64, three, three, three), (p, descs, 1, 1, p, 0, 64, three, three, three),
                 (p, descs, 1, 1, p, 64, 64, None, three, three)):
        assert lib.vy_train_transform(*args, None) == -1


def test_chunk_constant_matches_the_header():
    src = open(os.path.join(os.path.dirname(HERE), "include", "vyolo.h")).read()
    assert "#define VY_AUG_CHUNK %d\n" % _lib.VY_AUG_CHUNK in src
    assert ctypes.sizeof(_lib.TrainAug) * _lib.VY_AUG_CHUNK + 128 <= 4096
