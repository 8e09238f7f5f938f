"""-m "not gpu": mixup on the host — MixupDetection's draws, labels and clips against a short numpy restatement of
gluoncv.data.MixupDetection.__getitem__ [UPSTREAM-RECALLED: gluoncv is not available; restated from memory], the
arithmetic of MixedClip.numpy(), and vy_train_transform_mix's descriptor validation.  Nothing here launches a kernel."""
import ctypes
import os
import re

import numpy as np
import pytest

from videoyolo_amd import _lib
from videoyolo_amd.transforms import MixedClip, MixupDetection

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# the restatement: gluoncv's __getitem__ with the two departures of this library (labels cut to five columns before the
# ratio is appended, nothing blended: the sources and lambd are returned) and the blend as a function of its own

def ref_mix(img1, img2, lambd):
    """canvas = zeros(max h, max w) float32; canvas[:h1, :w1] = img1 * l1; canvas[:h2, :w2] += img2 * l2; astype(uint8),
    frame by frame.  l1 = float32(lambd), l2 = float32(1.0 - lambd) subtracted in double."""
    l1, l2 = F(lambd), F(1.0 - float(lambd))
    img1, img2 = [i if i.ndim == 4 else i[None] for i in (img1, img2)]
    h, w = max(img1.shape[1], img2.shape[1]), max(img1.shape[2], img2.shape[2])
    out, pre = [], []
    for f1, f2 in zip(img1, img2):
        canvas = np.zeros((h, w, 3), F)
        canvas[:f1.shape[0], :f1.shape[1], :] = f1.astype(F) * l1
        canvas[:f2.shape[0], :f2.shape[1], :] += f2.astype(F) * l2
        assert canvas.dtype == F
        pre.append(canvas)
        out.append(canvas.astype(np.uint8))
    return np.stack(out), np.stack(pre)


def ref_getitem(dataset, idx, mixup, args):
    img1, label1 = dataset[idx]
    lambd = 1
    if mixup is not None:
        lambd = max(0, min(1, mixup(*args)))
    if lambd >= 1:
        return None, lambd, np.hstack((label1[:, :5], np.ones((label1.shape[0], 1))))
    idx2 = np.random.choice(np.delete(np.arange(len(dataset)), idx))
    _, label2 = dataset[idx2]
    y1 = np.hstack((label1[:, :5], np.full((label1.shape[0], 1), lambd)))
    y2 = np.hstack((label2[:, :5], np.full((label2.shape[0], 1), 1. - lambd)))
    return idx2, lambd, np.vstack((y1, y2))


def _image(h, w, seed, k=None):
    shape = (h, w, 3) if k is None else (k, h, w, 3)
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _dataset(n=5, k=None):
    sizes = [(23, 31), (40, 17), (30, 30), (16, 48), (37, 29)]
    out = []
    for i in range(n):
        h, w = sizes[i % len(sizes)]
        cols = 5 + i % 2                                    # (N, 5) and (N, 6) labels alternate
        label = np.random.default_rng(100 + i).uniform(0, 16, (1 + i % 3, cols)).astype(F)
        out.append((_image(h, w, i, k), label))
    return out


class Counting(object):
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *args):
        self.calls += 1
        return self.fn(*args)


def test_draws_in_gluoncv_order_under_the_global_seed():
    ds = _dataset()
    mixed = 0
    for seed in range(12):
        idx = seed % len(ds)
        np.random.seed(seed)
        want_idx2, want_lambd, want_label = ref_getitem(ds, idx, np.random.beta, (1.5, 1.5))
        want_state = np.random.get_state()[1].copy(), np.random.get_state()[2]
        beta = Counting(np.random.beta)
        m = MixupDetection(ds, beta, 1.5, 1.5)
        assert len(m) == len(ds)
        np.random.seed(seed)
        clip, label = m[idx]
        state = np.random.get_state()
        assert beta.calls == 1
        assert np.array_equal(state[1], want_state[0]) and state[2] == want_state[1]   # the generator ends where gluoncv's does
        assert isinstance(clip, MixedClip) and clip.lambd == want_lambd
        assert clip.first[0] is not None and np.array_equal(clip.first[0], ds[idx][0])
        assert np.array_equal(clip.second[0], ds[want_idx2][0]) and want_idx2 != idx
        assert label.dtype == want_label.dtype and np.array_equal(label, want_label)
        mixed += 1
    assert mixed == 12  # beta(1.5, 1.5) < 1 always


def test_private_generator_leaves_the_global_one_alone():
    import random
    ds = _dataset()
    np.random.seed(5)
    want = ref_getitem(ds, 2, np.random.beta, (1.5, 1.5))
    np.random.seed(77)
    before = np.random.get_state()[1].copy()
    N = np.random.RandomState(5)
    clip, label = MixupDetection(ds, N.beta, 1.5, 1.5, rng=(random.Random(5), N))[2]
    assert np.array_equal(np.random.get_state()[1], before)
    assert clip.lambd == want[1] and np.array_equal(clip.second[0], ds[want[0]][0]) and np.array_equal(label, want[2])


def test_lambd_above_one_is_clamped_and_nothing_more_is_drawn():
    ds = _dataset()
    m = MixupDetection(ds, lambda: 1.3)
    np.random.seed(3)
    before = np.random.get_state()[1].copy()
    img, label = m[1]
    assert img is ds[1][0]                                       # the first source itself, as gluoncv returns it
    assert np.array_equal(np.random.get_state()[1], before)     # no second draw
    assert label.shape == (len(ds[1][1]), 6) and np.array_equal(label[:, 5], np.ones(len(label)))
    assert np.array_equal(label[:, :5], ds[1][1][:, :5])


def test_lambd_below_zero_is_clamped_and_the_sample_is_mixed():
    ds = _dataset()
    m = MixupDetection(ds, lambda: -0.2)
    np.random.seed(3)
    want_idx2, want_lambd, want_label = ref_getitem(ds, 0, lambda: -0.2, ())
    np.random.seed(3)
    clip, label = m[0]
    assert isinstance(clip, MixedClip) and clip.lambd == 0 and want_lambd == 0
    assert clip.l1 == F(0) and clip.l2 == F(1)
    n1 = len(ds[0][1])
    assert np.array_equal(label, want_label)
    assert np.array_equal(label[:n1, 5], np.zeros(n1)) and np.array_equal(label[n1:, 5], np.ones(len(label) - n1))
    assert np.array_equal(clip.numpy(), ref_mix(ds[0][0], ds[want_idx2][0], 0)[0])


def test_set_mixup_none_gives_ones_and_set_mixup_switches_back():
    ds = _dataset()
    m = MixupDetection(ds, np.random.beta, 1.5, 1.5)
    m.set_mixup(None)
    np.random.seed(0)
    before = np.random.get_state()[1].copy()
    for i in range(len(ds)):
        img, label = m[i]
        assert img is ds[i][0] and label.shape == (len(ds[i][1]), 6) and np.all(label[:, 5] == 1)
    assert np.array_equal(np.random.get_state()[1], before)
    m.set_mixup(np.random.beta, 1.5, 1.5)                        # train_yolov3.py:575
    assert isinstance(m[0][0], MixedClip)
    assert isinstance(MixupDetection(ds)[0][0], np.ndarray)     # no callable at construction: unmixed


def test_labels_of_five_and_six_columns_and_an_empty_second():
    a = (_image(20, 20, 1), np.array([[1, 2, 9, 8, 3], [4, 4, 12, 15, 0]], F))
    b = (_image(18, 25, 2), np.array([[2, 3, 17, 16, 7, 1]], F))      # with the reference's `difficult` column
    e = (_image(12, 12, 3), np.zeros((0, 5), F))
    for first, second, n in ((a, b, 3), (b, a, 3), (a, e, 2), (e, a, 2)):
        m = MixupDetection([first, second], lambda: 0.25)
        clip, label = m[0]
        assert label.shape == (n, 6)
        n1 = len(first[1])
        assert np.array_equal(label[:n1, :5], first[1][:, :5]) and np.array_equal(label[n1:, :5], second[1][:, :5])  # boxes unmoved
        assert np.all(label[:n1, 5] == 0.25) and np.all(label[n1:, 5] == 0.75)
    with pytest.raises(ValueError):
        MixupDetection([(a[0], np.zeros((2, 7), F)), b], lambda: 0.5)[0]


def test_clips():
    c3 = (_image(20, 24, 1, k=3), np.zeros((1, 5), F))
    c2 = (_image(20, 24, 2, k=2), np.zeros((1, 5), F))
    with pytest.raises(ValueError, match="frame t"):
        MixupDetection([c3, c2], lambda: 0.5)[0]
    other = (_image(31, 18, 3, k=3), np.zeros((2, 5), F))
    clip, _ = MixupDetection([c3, other], lambda: 0.5)[0]
    assert clip.shape == (3, 31, 24, 3)
    assert np.array_equal(clip.numpy(), ref_mix(c3[0], other[0], 0.5)[0])    # frame t with frame t
    flat = MixupDetection([(_image(23, 31, 4), c3[1]), (_image(40, 17, 5), c3[1])], lambda: 0.5)[1][0]
    assert flat.shape == (1, 40, 31, 3) and flat.first.shape == (1, 40, 17, 3) and flat.second.shape == (1, 23, 31, 3)
    with pytest.raises(TypeError):
        MixedClip(c3[0].astype(F), c3[0], 0.5)


def test_a_dataset_of_one_raises_what_choice_raises():
    ds = _dataset(1)
    with pytest.raises(ValueError) as want:
        np.random.choice(np.delete(np.arange(1), 0))
    with pytest.raises(ValueError) as got:
        MixupDetection(ds, lambda: 0.5)[0]
    assert str(got.value) == str(want.value)
    assert MixupDetection(ds, lambda: 1.0)[0][0] is ds[0][0]      # lambd >= 1 needs no second sample


@pytest.mark.parametrize("lambd", [0.0, 0.5, 0.37, 0.999])
def test_numpy_is_the_stated_arithmetic(lambd):
    """(23, 31) against (40, 17): each source is larger on one axis, so the (40, 31) canvas has all four regions."""
    a, b = _image(23, 31, 1), _image(40, 17, 2)
    a[0, 0], b[0, 0] = 255, 254                                  # 255 and 254 at 0.5 give 254.5 -> 254, not 255
    clip = MixedClip(a, b, lambd)
    assert clip.shape == (1, 40, 31, 3) and clip.l1 == F(lambd) and clip.l2 == F(1.0 - lambd)
    got = clip.numpy()
    want, pre = ref_mix(a, b, lambd)
    assert got.dtype == np.uint8 and got.shape == (1, 40, 31, 3) and np.array_equal(got, want)
    both, first, second, neither = got[0, :23, :17], got[0, :23, 17:], got[0, 23:, :17], got[0, 23:, 17:]
    assert np.array_equal(first, (a[:, 17:].astype(F) * F(lambd)).astype(np.uint8))
    assert np.array_equal(second, (b[23:].astype(F) * F(1.0 - lambd)).astype(np.uint8))
    assert not neither.any() and both.any()
    assert 0 <= pre.min() and pre.max() < 256
    if lambd not in (0.0,):
        # truncation, not rounding: somewhere the blend's fraction is above 0.5 and the result is the floor
        # (at 0.5 every fraction is 0 or exactly 0.5: there the comparison is with rounding half up)
        frac = pre - np.floor(pre)
        up = frac >= 0.5 if lambd == 0.5 else frac > 0.5
        rounded = np.floor(pre.astype(np.float64) + 0.5)
        assert up.any() and np.all(got[up] != rounded[up]) and np.array_equal(got[up], np.floor(pre[up]))
    if lambd == 0.5:
        assert pre[0, 0, 0, 0] == 254.5 and got[0, 0, 0, 0] == 254
    if lambd == 0.0:
        assert np.array_equal(got[0, :40, :17], b) and not got[0, :, 17:].any()   # the second source on the shared canvas


# ---------------------------------------------------------------------------------------------------------------------
# vy_train_transform_mix's validation: before the device is touched, with bogus non-null device pointers

def _valid_aug(src_h=40, src_w=31):
    d = _lib.TrainAug()
    d.src_offset, d.src_h, d.src_w = 0, src_h, src_w
    d.paste_x, d.paste_y, d.canvas_w, d.canvas_h = 5, 7, 80, 60
    d.crop_x, d.crop_y, d.crop_w, d.crop_h = 3, 1, 50, 40
    d.interp, d.flip, d.num_ops = 2, 1, 2
    d.op[0], d.op[1] = 1, 4
    return d


def _valid_mix(second=True):
    m = _lib.TrainMix()
    m.h1, m.w1, m.h2, m.w2 = (23, 31, 40, 17) if second else (40, 31, 12, 12)
    m.src2_offset = 23 * 31 * 3 * 3 if second else -1
    m.l1, m.l2 = 0.37, 0.63
    return m


def _call(descs, mixes, n, k=3):
    p = ctypes.c_void_p(0x1000)
    three = (ctypes.c_float * 3)(1, 1, 1)
    return _lib.load().vy_train_transform_mix(p, descs, mixes, n, k, p, 64, 96, three, three, three, None)


BAD_MIX = {
    "first height 0": lambda d, m: setattr(m, "h1", 0),
    "first width 0": lambda d, m: setattr(m, "w1", 0),
    "second height 0": lambda d, m: setattr(m, "h2", 0),
    "second width -1": lambda d, m: setattr(m, "w2", -1),
    "canvas height is not the larger": lambda d, m: setattr(m, "h2", 39),
    "canvas width is not the larger": lambda d, m: setattr(m, "w1", 32),
    "canvas smaller than a source": lambda d, m: setattr(d, "src_h", 23),
    "second offset -2": lambda d, m: setattr(m, "src2_offset", -2),
    "first offset negative": lambda d, m: setattr(d, "src_offset", -1),
    "l1 above 1": lambda d, m: setattr(m, "l1", 1.0001),
    "l1 negative": lambda d, m: setattr(m, "l1", -0.1),
    "l2 above 1": lambda d, m: setattr(m, "l2", 2.0),
    "l2 negative": lambda d, m: setattr(m, "l2", -1e-6),
    "l1 nan": lambda d, m: setattr(m, "l1", float("nan")),
    # what vy_train_transform refuses is refused here too
    "crop leaves the canvas": lambda d, m: setattr(d, "crop_w", 78),
    "interp 5": lambda d, m: setattr(d, "interp", 5),
    "unknown op": lambda d, m: d.op.__setitem__(1, 5),
}


def test_valid_descriptors_differ_from_each_bad_one_only_in_the_named_field():
    """The valid pair passes validation: with k = 2049 (checked after the descriptors) the error names k, not a
    descriptor — so each BAD_MIX case below is refused for its own field."""
    lib = _lib.load()
    descs = (_lib.TrainAug * 2)(_valid_aug(), _valid_aug())
    mixes = (_lib.TrainMix * 2)(_valid_mix(True), _valid_mix(False))
    assert _call(descs, mixes, 2, k=2049) == -1 and "k above 2048" in lib.vy_last_error().decode()


@pytest.mark.parametrize("what", sorted(BAD_MIX))
def test_bad_mix_descriptors_are_refused_before_anything_is_launched(what):
    """The bad descriptor is the LAST of a batch longer than one chunk (see tests/test_train_transform_host.py)."""
    lib = _lib.load()
    n = _lib.VY_MIX_CHUNK + 2
    descs = (_lib.TrainAug * n)(*[_valid_aug() for _ in range(n)])
    mixes = (_lib.TrainMix * n)(*[_valid_mix(i % 2 == 0) for i in range(n)])
    mixes[n - 1] = _valid_mix(True)
    BAD_MIX[what](descs[n - 1], mixes[n - 1])
    assert _call(descs, mixes, n) == -1, what
    assert "vy_train_transform_mix: descriptor %d" % (n - 1) in lib.vy_last_error().decode()


def test_an_unmixed_descriptor_must_have_the_first_source_as_its_canvas():
    lib = _lib.load()
    for field, value in (("h1", 39), ("w1", 30)):
        descs = (_lib.TrainAug * 1)(_valid_aug())
        mixes = (_lib.TrainMix * 1)(_valid_mix(False))
        setattr(mixes[0], field, value)
        assert _call(descs, mixes, 1) == -1 and "descriptor 0" in lib.vy_last_error().decode()


def test_bad_arguments_are_refused():
    lib = _lib.load()
    descs, mixes = (_lib.TrainAug * 1)(_valid_aug()), (_lib.TrainMix * 1)(_valid_mix())
    p = ctypes.c_void_p(0x1000)
    three = (ctypes.c_float * 3)(1, 1, 1)
    good = [p, descs, mixes, 1, 1, p, 64, 64, three, three, three]
    for i, bad in ((0, None), (1, None), (2, None), (3, 0), (4, 0), (4, 2049), (5, None), (6, 0), (7, 0), (8, None), (9, None),
                   (10, None)):
        args = list(good)
        args[i] = bad
        assert lib.vy_train_transform_mix(*args, None) == -1, i


def test_descriptor_sizes_and_chunk_match_the_header():
    src = open(os.path.join(os.path.dirname(HERE), "include", "vyolo.h")).read()
    assert "#define VY_MIX_CHUNK %d\n" % _lib.VY_MIX_CHUNK in src

    def header_size(name):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
        body = re.sub(r"\[VY_AUG_MAX_OPS\]", "[%d]" % _lib.VY_AUG_MAX_OPS, body)
        total = 0
        for ctype, names in re.findall(r"(int64_t|int32_t|float)\s+([^;]+);", body):
            for n in names.split(","):
                count = int(np.prod([int(v) for v in re.findall(r"\[(\d+)\]", n)] or [1]))
                total += count * (8 if ctype == "int64_t" else 4)
        return total                                            # the int64 comes first and every total is a multiple of 8
    assert ctypes.sizeof(_lib.TrainAug) == header_size("vy_train_aug") == 144
    assert ctypes.sizeof(_lib.TrainMix) == header_size("vy_train_mix") == 32
    assert [f for f, _ in _lib.TrainMix._fields_] == ["src2_offset", "h1", "w1", "h2", "w2", "l1", "l2"]
    # both descriptors of a chunk and the launch's other arguments fit the 4 KB argument segment
    assert (ctypes.sizeof(_lib.TrainAug) + ctypes.sizeof(_lib.TrainMix)) * _lib.VY_MIX_CHUNK + 128 <= 4096
