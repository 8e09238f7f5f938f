"""-m gpu: mixup inside the training transform's launch (csrc/augment.hip through vy_train_transform_mix) against the CPU
checker (tests/train_transform_ref.py) run on the MATERIALISED uint8 mix — materialised here by this file's own numpy
restatement of gluoncv's blend, not by the library's MixedClip.numpy().  Both sides are the stated sequence of fp32
operations, so every comparison is np.array_equal."""
import random

import numpy as np
import pytest

import train_transform_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
H, W = 32, 48
S1, S2 = (23, 31), (40, 17)          # each source is larger on one axis: the (40, 31) canvas has all four regions
B, CT, S, HUE = R.BRIGHTNESS, R.CONTRAST, R.SATURATION, R.HUE


def _frames(k, h, w, seed):
    """Full-range uint8 with structure (edges for the taps to disagree on) and noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 127 + 120 * np.sin(x / 3.0)[..., None] * np.cos(y / 2.0)[..., None] * np.array([1, 0.5, -1])
    return np.clip(base[None] + rng.normal(0, 40, (k, h, w, 3)), 0, 255).astype(np.uint8)


def mix(a, b, lambd):
    """gluoncv's blend, frame t with frame t: float32 zeros of the larger height and width, canvas[:h1, :w1] = a * l1,
    canvas[:h2, :w2] += b * l2 (each product rounded to float32, then added), astype(uint8) (truncation)."""
    l1, l2 = F(lambd), F(1.0 - float(lambd))
    k, h, w = a.shape[0], max(a.shape[1], b.shape[1]), max(a.shape[2], b.shape[2])
    canvas = np.zeros((k, h, w, 3), F)
    canvas[:, :a.shape[1], :a.shape[2]] = a.astype(F) * l1
    canvas[:, :b.shape[1], :b.shape[2]] += b.astype(F) * l2
    assert canvas.dtype == F and canvas.min() >= 0 and canvas.max() < 256
    return canvas.astype(np.uint8)


def _aug(src, crop, interp, flip=False, expand=None, ops=(), hue=None):
    return dict(src=tuple(src), crop=tuple(crop), interp=interp, flip=flip, expand=expand, ops=list(ops), hue=hue)


def _clip(a, b, lambd):
    from videoyolo_amd.transforms import MixedClip
    return MixedClip(a, b, lambd)


def _run(srcs, augs, k, width=W, height=H):
    from videoyolo_amd.transforms import YOLO3VideoTrainTransform
    got = YOLO3VideoTrainTransform(k, width, height).transform_frames(srcs, augs).cpu().numpy()
    assert got.shape == (len(srcs), k, 3, height, width) and got.dtype == np.float32
    return got


def _compare(pairs, lambds, augs, k, width=W, height=H, names=None):
    """pairs[i] = (first, second) mixed with lambds[i], or (clip, None) for an unmixed sample."""
    srcs = [a if b is None else _clip(a, b, l) for (a, b), l in zip(pairs, lambds)]
    got = _run(srcs, augs, k, width, height)
    for i, ((a, b), l, aug) in enumerate(zip(pairs, lambds, augs)):
        want = R.transform(a if b is None else mix(a, b, l), aug, width, height)
        bad = got[i] != want
        assert not bad.any(), "sample %s: %d of %d values differ, max |diff| %g" % (
            names[i] if names else i, int(bad.sum()), bad.size, float(np.abs(got[i] - want)[bad].max()))
    return got


# (crop (x0, y0, w, h) of the (40, 31) canvas, output (height, width), the area mode it reaches)
GEOMETRY = {
    "whole canvas": ((0, 0, 31, 40), (32, 48)),          # the width grows, the height shrinks: kAreaLinear
    "enlarging crop": ((3, 5, 26, 29), (32, 48)),        # both grow, the crop cuts through all four regions: kAreaLinear
    "shrinking whole canvas": ((0, 0, 31, 40), (24, 20)),  # x1.55, x1.67: kAreaFrac
    "integer factors": ((0, 0, 31, 40), (10, 31)),       # x1, x4: kAreaInt
}


@pytest.mark.parametrize("geometry", sorted(GEOMETRY))
def test_every_interp_and_flip_over_the_four_regions(geometry):
    """All five interpolations x flip on / off in one call.  The crop covers (or cuts through) the whole canvas, so both,
    first-only, second-only and neither, and the edges between them, fall under tap footprints."""
    crop, (oh, ow) = GEOMETRY[geometry]
    pairs, augs, names = [], [], []
    for interp in range(5):
        for flip in (False, True):
            pairs.append((_frames(1, *S1, seed=10 * interp + flip), _frames(1, *S2, seed=100 + 10 * interp + flip)))
            augs.append(_aug((40, 31), crop, interp, flip))
            names.append("interp %d flip %d" % (interp, flip))
    got = _compare(pairs, [0.37] * len(pairs), augs, 1, width=ow, height=oh, names=names)
    assert np.isfinite(got).all()


def test_the_mix_canvas_expanded():
    """The mixed canvas pasted at the odd offset (7, 5) into a 61 x 50 canvas: the fill, the zero region of the mix and the
    blended pixels all lie under linear and Lanczos taps (and the three other interpolations').  The zero region is part
    of the IMAGE: it comes out as colour-distorted zero, not as fill — checked on a same-size crop, which is a copy."""
    ex = (7, 5, 61, 50)
    ops = [(B, F(10.5), F(0))]
    pairs, augs, names = [], [], []
    for interp in range(5):
        pairs.append((_frames(1, *S1, seed=interp), _frames(1, *S2, seed=50 + interp)))
        augs.append(_aug((40, 31), (1, 1, 59, 48), interp, interp % 2 == 1, ex, ops))
        names.append("interp %d" % interp)
    pairs.append(pairs[0])
    augs.append(_aug((40, 31), (5, 7, W, H), 1, False, ex, ops))     # canvas (5..52, 7..38): a copy
    names.append("copy")
    got = _compare(pairs, [0.6] * len(pairs), augs, 1, names=names)
    zero = (F(0) + F(10.5)) / F(255) - R.MEAN
    zero = zero / R.STD
    fill = (R.FILL / F(255) - R.MEAN) / R.STD
    # output (y, x) = canvas (7 + y, 5 + x) = mix canvas (2 + y, x - 2): (25, 25) is mix (27, 23), neither source's
    assert np.array_equal(got[-1, 0, :, 25, 25], zero) and not np.array_equal(zero, fill)
    # (30, 0) is canvas (37, 5): left of the paste, the fill
    assert np.array_equal(got[-1, 0, :, 30, 0], fill)


def test_colour_ops_in_both_orders_on_a_mixed_sample():
    """All four ops in both orders, with arguments that drive values out of [0, 255] (nothing is clamped after the mix)."""
    from videoyolo_amd.transforms import hue_matrix
    hue = hue_matrix(17.3)
    cases = {
        "order 1": [(B, F(30.5), F(0)), (CT, F(1.5), F(0)), (S, F(1.45), F(1.0 - 1.45)), (HUE, F(0), F(0))],
        "order 0": [(B, F(-30.5), F(0)), (S, F(0.55), F(1.0 - 0.55)), (HUE, F(0), F(0)), (CT, F(0.51), F(0))],
    }
    pairs = [(_frames(1, *S1, seed=i), _frames(1, *S2, seed=9 + i)) for i in range(len(cases))]
    augs = [_aug((40, 31), (0, 0, 31, 40), 1 + i, i == 1, None, ops, hue) for i, ops in enumerate(cases.values())]
    _compare(pairs, [0.45] * 2, augs, 1, names=list(cases))
    for (a, b), ops in zip(pairs, cases.values()):
        v = R.colour(mix(a, b, 0.45), ops, hue)
        assert v.min() < 0 or v.max() > 255


def test_clips_across_a_chunk_boundary_mixed_and_unmixed_alternating():
    """k = 2, one sample more than the mix launch's chunk, every sample's two sources of their own sizes; the odd samples
    have no second source and are bit-equal to vy_train_transform on the same clip and draw."""
    from videoyolo_amd import _lib
    n = _lib.VY_MIX_CHUNK + 1
    pairs, lambds, augs = [], [], []
    for i in range(n):
        h1, w1, h2, w2 = 12 + i % 5, 20 - i % 7, 18 - i % 4, 11 + i % 6
        a = _frames(2, h1, w1, seed=i)
        if i % 2:
            pairs.append((a, None))
            ch, cw = h1, w1
        else:
            pairs.append((a, _frames(2, h2, w2, seed=200 + i)))
            ch, cw = max(h1, h2), max(w1, w2)
        lambds.append(0.1 + 0.8 * i / n)
        augs.append(_aug((ch, cw), (i % 3, i % 2, cw - i % 3, ch - i % 2), i % 5, i % 4 < 2, ops=[(B, F(i), F(0))]))
    got = _compare(pairs, lambds, augs, 2, width=24, height=16)
    assert not np.array_equal(got[n - 1], got[n - 3])          # the last sample lies in the second launch
    odd = list(range(1, n, 2))
    plain = _run([pairs[i][0] for i in odd], [augs[i] for i in odd], 2, width=24, height=16)
    assert np.array_equal(got[odd], plain)


def test_lambd_at_its_ends_and_the_truncation():
    """Same-size crops (copies), so an output pixel is one mixed pixel.  lambd = 0: the second source on the shared
    canvas, zeros elsewhere.  lambd = 0.999.  255 and 254 at 0.5 are 254.5: 254, not 255."""
    a, b = _frames(1, *S1, seed=1), _frames(1, *S2, seed=2)
    a[0, 0, 0], b[0, 0, 0] = 255, 254
    whole = _aug((40, 31), (0, 0, 31, 40), 0)
    got = _compare([(a, b)] * 3, [0.0, 0.999, 0.5], [whole] * 3, 1, width=31, height=40)
    second = np.zeros((1, 40, 31, 3), np.uint8)
    second[:, :, :17] = b
    assert np.array_equal(got[0], R.transform(second, whole, 31, 40))
    value = lambda v: (F(v) / F(255) - R.MEAN) / R.STD  # noqa: E731
    assert np.array_equal(got[2, 0, :, 0, 0], value(254)) and not np.array_equal(value(254), value(255))
    assert mix(a, b, 0.999)[0, 0, 0, 0] == 254                 # 255 * 0.999 + 254 * 0.001 = 254.999 -> 254 as well
    assert np.array_equal(got[1, 0, :, 0, 0], value(254))


# ---------------------------------------------------------------------------------------------------------------------
# batch() end to end

class _Dataset(list):
    pass


def _dataset():
    sizes = [(50, 70), (64, 48), (40, 90), (72, 60)]
    out = _Dataset()
    for i, (h, w) in enumerate(sizes):
        label = np.array([[w * 0.1, h * 0.1, w * 0.6, h * 0.7, i], [w * 0.5, h * 0.4, w * 0.95, h * 0.9, 10 + i]], F)
        out.append((_frames(1, h, w, seed=40 + i)[0], label))
    return out


LAMBDS = [0.37, 1.0, 0.6]


def _batches(net, seed=4):
    """The same three samples twice under the same seeds: as MixupDetection returns them, and materialised on the host.
    (Under this seed every drawn crop keeps boxes of both sources; a crop may also leave a source's boxes degenerate.)"""
    from videoyolo_amd.transforms import MixedClip, MixupDetection, YOLO3VideoTrainTransform
    out = []
    for materialise in (False, True):
        N = np.random.RandomState(seed)
        rng = (random.Random(seed), N)
        lambds = iter(LAMBDS)
        wrapped = MixupDetection(_dataset(), lambda: next(lambds), rng=rng)
        samples = [wrapped[i] for i in range(3)]
        assert [isinstance(s, MixedClip) for s, _ in samples] == [True, False, True]
        srcs = [s.numpy()[0] if materialise and isinstance(s, MixedClip) else s for s, _ in samples]
        t = YOLO3VideoTrainTransform(1, 64, 64, net=net, mixup=True, rng=rng)
        out.append((t.batch(srcs, [lab for _, lab in samples]), samples))
    return out


@pytest.fixture(scope="module")
def net(voc_classes, synth20):
    import videoyolo_amd as vy
    net = vy.yolo3_darknet53(voc_classes, pretrained_base=False)
    net.set_parameters(synth20)
    net.collect_params().reset_ctx("cuda:0")
    return net


def test_batch_equals_batch_on_the_materialised_clips_and_trains(net):
    """B = 3 at 64 x 64 (mixed, unmixed, mixed): x is bit-equal to batch() on the .numpy()-materialised clips under the
    same seeds, gt_boxes and the five targets are identical, the objectness targets of the mixed samples carry both
    ratios, and one recorded training step on the batch gives finite losses."""
    import torch
    from videoyolo_amd import autograd
    (device, samples), (host, _) = _batches(net)
    assert len(device) == 7 and tuple(device[0].shape) == (3, 3, 64, 64)
    for i, (d, h) in enumerate(zip(device, host)):
        assert np.array_equal(d.cpu().numpy(), h.cpu().numpy()), i
    x = device[0].cpu().numpy()
    assert np.isfinite(x).all() and not np.array_equal(x[0], x[2])
    obj = device[2].cpu().numpy()
    for i, lambd in enumerate(LAMBDS):
        ratios = set(np.unique(obj[i][obj[i] > 0]).tolist())
        want = {1.0} if lambd >= 1 else {float(F(lambd)), float(F(1.0 - lambd))}
        assert ratios == want, (i, ratios, want)
    with autograd.record():
        losses = net(device[0], *device[1:])
    torch.cuda.synchronize()
    for l in losses:
        v = l.asnumpy() if hasattr(l, "asnumpy") else l.detach().cpu().numpy()
        assert np.isfinite(v).all()


def test_call_takes_a_mixed_clip():
    """__call__ on a MixedClip, net=None: the image of the materialised clip under the same seeds."""
    from videoyolo_amd.transforms import YOLO3VideoTrainTransform
    a, b = _frames(2, *S1, seed=3), _frames(2, *S2, seed=4)
    label = np.array([[2, 3, 20, 20, 1, 0.3], [1, 5, 12, 30, 2, 0.7]], F)
    t = YOLO3VideoTrainTransform(2, W, H, rng=(random.Random(3), np.random.RandomState(3)))
    twin = YOLO3VideoTrainTransform(2, W, H, rng=(random.Random(3), np.random.RandomState(3)))
    img = t(_clip(a, b, 0.3), label)
    aug, _ = twin.draw(40, 31, label)
    assert aug["src"] == (40, 31)
    assert np.array_equal(img.cpu().numpy(), R.transform(mix(a, b, 0.3), aug, W, H))
