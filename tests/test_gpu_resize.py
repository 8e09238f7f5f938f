"""-m gpu: the fused resize + to_tensor + normalize kernel (csrc/preproc.hip through vy_preprocess_resize_frames)
against the restated reference transform (oracle/resize_oracle.py: YOLO3VideoInferenceTransform.__call__,
models/definitions/yolo/transforms.py:316-350 with imresize(interp=9) -> OpenCV area / cubic / linear on uint8).
Integer arithmetic and the rounding to uint8 must be bit-exact; the final float values too (same fp32 operation
sequence, no contraction).

The constructed cases of tests/entry_cases.py (area cells of up to 11 table entries, one integer and one fractional axis,
integer factors above the table's size, sources of one pixel or two rows, same-size frames of any area, the acceptance
bound) run through the same two assertions, on the smooth frames and on full-range noise;
tests/test_entry_cases_sensitivity.py shows on the CPU which bug each catches."""
import ctypes

import numpy as np
import pytest

import entry_cases as E
from entry_cases import smooth_frames as _frames

pytestmark = pytest.mark.gpu


CASES = [
    ("cubic enlarge", (2, 120, 160), (416, 416)),
    ("cubic enlarge odd", (1, 37, 53), (64, 96)),
    ("area fractional (720p -> 608)", (2, 720, 1280), (608, 608)),
    ("area fractional (480p -> 416)", (1, 480, 640), (416, 416)),
    ("area 2x2", (2, 192, 256), (96, 128)),
    ("area 3x3", (1, 288, 384), (96, 128)),
    ("area 4x2", (1, 256, 512), (128, 128)),
    ("linear mixed", (2, 50, 200), (96, 96)),
    ("linear one side equal", (1, 96, 300), (96, 128)),
    ("same size", (2, 96, 96), (96, 96)),
]


# the cases above on the smooth frames, as before; the constructed ones on both kinds of frames
ALL_CASES = [c + ("smooth",) for c in CASES] + [c[:3] + (kind,) for c in E.RESIZE_CASES + [E.INTEGER_11] for kind in E.FRAME_KINDS]


@pytest.mark.parametrize("name,src,dst,kind", ALL_CASES,
                         ids=[c[0] for c in CASES] + ["%s, %s" % (c[0], c[3]) for c in ALL_CASES[len(CASES):]])
def test_resize_normalize_matches_the_restated_transform(name, src, dst, kind):
    from videoyolo_amd import transforms
    from oracle import resize_oracle as R
    frames = E.FRAME_KINDS[kind](*src, seed=len(name))
    t = transforms.YOLO3VideoInferenceTransform(dst[1], dst[0])       # (width, height) like the reference
    got = t(frames).cpu().numpy()
    want, resized = R.inference_transform(frames, dst[1], dst[0])
    assert got.shape == want.shape == (src[0], 3) + dst
    # recover the uint8 value the kernel rounded to and compare the integers first (clearer failure)
    mean, std = np.asarray(transforms.MEAN, np.float32), np.asarray(transforms.STD, np.float32)
    back = np.rint((got.transpose(0, 2, 3, 1) * std + mean) * 255.0).astype(np.int64)
    diff = np.abs(back - resized.astype(np.int64))
    assert diff.max() == 0, "%s: %d pixels differ, max %d levels" % (name, int((diff > 0).sum()), int(diff.max()))
    assert np.array_equal(got, want)


def test_resized_frames_feed_the_network(voc_classes, synth20):
    """The transform's output is the network input: 720p frames -> 416 x 416 -> detections, identical to feeding the
    oracle-resized frames."""
    import videoyolo_amd as vy
    from videoyolo_amd import transforms
    from oracle import resize_oracle as R
    frames = _frames(2, 360, 640, seed=3)
    net = vy.yolo3_darknet53(voc_classes, pretrained_base=False)
    net.set_parameters(synth20)
    net.collect_params().reset_ctx("cuda:0")
    x = transforms.YOLO3VideoInferenceTransform(224, 224)(frames)
    want, _ = R.inference_transform(frames, 224, 224)
    a = [t.cpu().numpy() for t in net(x, return_index=True)]
    b = [t.cpu().numpy() for t in net(want, return_index=True)]
    assert all(np.array_equal(p, q) for p, q in zip(a, b))


def test_extreme_shrink_is_refused():
    from videoyolo_amd import _lib, transforms
    with pytest.raises(_lib.VyError):
        transforms.YOLO3VideoInferenceTransform(32, 32)(np.zeros((1, 500, 700, 3), np.uint8))


def test_the_acceptance_bound_of_the_area_table():
    """A fractional factor above kAreaMax - 2 = 10 on an axis is refused (x10.075), exactly 10 is accepted (the case
    above), and integer factors on both axes are block means of any size (x11 by x11)."""
    from videoyolo_amd import _lib, transforms
    _, src, dst = E.REFUSED
    with pytest.raises(_lib.VyError) as e:
        transforms.YOLO3VideoInferenceTransform(dst[1], dst[0])(np.zeros(src + (3,), np.uint8))
    assert e.value.code == -4    # VY_ERR_UNSUPPORTED
    for case in (E.ACCEPTED_AT_THE_BOUND, E.INTEGER_11):
        test_resize_normalize_matches_the_restated_transform(case[0], case[1], case[2], "noise")


def test_same_size_from_an_unaligned_pointer():
    """Through the raw C ABI: frames that start one byte into a buffer, at a size whose area is a multiple of 4.  The
    4-pixel kernel's 32-bit loads need an aligned source, so the entry point routes this call to the per-pixel kernel
    (byte loads): the same values as from the aligned copy, bit for bit."""
    import torch
    from videoyolo_amd import _lib, transforms
    from oracle import resize_oracle as R
    lib = _lib.load()
    b, h, w = 2, 6, 10
    frames = E.noise_frames(b, h, w, seed=1)
    flat = torch.zeros(frames.size + 8, dtype=torch.uint8, device="cuda:0")
    assert flat.data_ptr() % 4 == 0
    flat[1:1 + frames.size] = torch.as_tensor(frames).reshape(-1).cuda()
    view = flat[1:1 + frames.size]
    assert view.data_ptr() % 4 == 1
    out = torch.empty((b, 3, h, w), dtype=torch.float32, device="cuda:0")
    mean, std = np.asarray(transforms.MEAN, np.float32), np.asarray(transforms.STD, np.float32)
    args = (b, h, w, mean.ctypes.data_as(ctypes.c_void_p), std.ctypes.data_as(ctypes.c_void_p),
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(lib.vy_preprocess_frames(ctypes.c_void_p(view.data_ptr()), ctypes.c_void_p(out.data_ptr()), *args))
    want, _ = R.inference_transform(frames, w, h)
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(transforms.YOLO3VideoInferenceTransform(w, h)(frames).cpu().numpy(), want)   # the aligned copy


STREAM_CLASSES = 1   # the smallest class count: the CPU oracle keeps 100 rows a frame on these clips with one class


def test_same_size_stream_at_an_odd_area():
    """75 x 93 frames at a 75 x 93 network input through stream.HostFedDetector (the copy, on the copy stream) equal the
    synchronous path, bit for bit."""
    import videoyolo_amd as vy
    from videoyolo_amd import stream, transforms
    hw, batch, ncls = (75, 93), 2, STREAM_CLASSES
    rng = np.random.default_rng(3)
    clips = [rng.integers(0, 256, (batch,) + hw + (3,), dtype=np.uint8) for _ in range(2)]
    net = vy.yolo3_darknet53(["c%d" % i for i in range(ncls)], pretrained_base=False)
    net.initialize(init="synthetic", seed=233, obj_bias=-2.0)
    net.collect_params().reset_ctx("cuda:0")
    net.set_nms(0.45, 400, 100)
    t = transforms.YOLO3VideoInferenceTransform(hw[1], hw[0])
    want = [[a.cpu().numpy() for a in net(t(c))] for c in clips]
    det = stream.HostFedDetector(net, batch, hw, hw, depth=2)
    got = [[np.array(a) for a in out] for out in det.run(iter(clips))]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            assert a.shape == b.shape and np.array_equal(a, b)
    assert any((w[0] >= 0).any() for w in want), "the fixture keeps no detection: the comparison would be vacuous"
    assert not np.array_equal(want[0][1], want[1][1])
