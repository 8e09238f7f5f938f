"""-m gpu: the per-frame mAP on the device (vy_voc_frame_ap, csrc/voc_metric.hip), called directly on vy_voc_match's flags
and through FrameMApMetric.update on device tensors: equal to the reference's recorded per-frame scores, to hand-derived
answers exactly, and to frame_map_host within the derived bound 2 (rows + n_gt + 2) 2^-53."""
import ctypes
import math
import warnings

import numpy as np
import pytest
import torch

from videoyolo_amd import _lib
from videoyolo_amd.metrics import FrameMApMetric, VOCMApMetric, frame_map_host

import frame_map_cases as F
import voc_metric_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPE_IDS = [C.shape_id(s) for s in C.SHAPES]


def _dev(arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _ptr(t, spare):
    return None if t is None else ctypes.c_void_p((t if t.numel() else spare).data_ptr())


def _frame_ap(arrays, mapped, use_07, iou_thresh=0.5):
    """vy_voc_match, then vy_voc_frame_ap on its flags, both called directly: (frame_ap (B,) float64, frame_classes (B,)
    int32, flags (B, R) int8) as numpy.  arrays: float32 (pb, pl, ps, gb, gl, gd or None); mapped (B, M) int32."""
    pb, pl, ps, gb, gl, gd = arrays
    batch, rows, n_gt = pb.shape[0], pb.shape[1], gb.shape[1]
    t = _dev([pb, pl.reshape(batch, rows), ps.reshape(batch, rows), gb, mapped.reshape(batch, n_gt).astype(np.int32),
              None if gd is None else (gd.reshape(batch, n_gt) != 0).astype(np.uint8)])
    best = torch.full((batch, rows), -7, dtype=torch.int32, device=DEV)
    flags = torch.full((batch, rows), -7, dtype=torch.int8, device=DEV)
    ap = torch.full((batch,), -7.0, dtype=torch.float64, device=DEV)
    classes = torch.full((batch,), -7, dtype=torch.int32, device=DEV)
    spare = torch.zeros(16, device=DEV)
    p = lambda x: _ptr(x, spare)                               # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib = _lib.load()
    _lib.check(lib.vy_voc_match(batch, rows, n_gt, p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(t[4]), p(t[5]), iou_thresh, p(best),
                                p(flags), stream))
    _lib.check(lib.vy_voc_frame_ap(batch, rows, n_gt, p(t[1]), p(t[2]), p(flags), p(t[4]), p(t[5]), int(use_07), p(ap),
                                   p(classes), stream))
    return ap.cpu().numpy(), classes.cpu().numpy(), flags.cpu().numpy()


@pytest.mark.parametrize("shape", C.SHAPES, ids=SHAPE_IDS)
def test_kernel_on_seeded_batches(shape):
    arrays, mapped, want_flags, host, model = F.reference(shape)
    batch, rows, n_gt = shape[:3]
    got = {}
    for mode in (False, True):
        ap, classes, flags = _frame_ap(arrays, mapped, mode)
        got[mode] = ap
        assert np.array_equal(flags, want_flags)
        want = host[mode]
        assert np.array_equal(np.isnan(ap), np.isnan(want)), (ap, want)        # NaN frame for frame
        assert np.array_equal(classes, model[mode][1]), (classes, model[mode][1])
        assert np.array_equal(classes == 0, np.isnan(ap))
        ok = ~np.isnan(want)
        worst = float(np.abs(ap[ok] - want[ok]).max()) if ok.any() else 0.0
        print("%s use_07=%s: worst |device - host| = %.3g = %.4f of the bound %.3g" % (
            C.shape_id(shape), mode, worst, worst / F.bound(rows, n_gt), F.bound(rows, n_gt)))
        assert worst <= F.bound(rows, n_gt)
    # neither a constant nor the wrong mode can pass
    if n_gt >= 70:
        assert not np.isnan(got[False]).any() and not np.isnan(got[True]).any()
        if rows > 1:
            assert len(np.unique(got[False])) == batch and (got[False] != got[True]).all()
        else:                                                  # one row per frame: most frames score 0 in both modes
            assert len(np.unique(got[False])) > 1 and (got[False] != got[True]).any()
    if C.shape_id(shape) == "B67_R257_M1_C80":
        assert int(np.isnan(got[False]).sum()) == 14 and int(np.isnan(got[True]).sum()) == 14


def test_constructed_known_answers_on_the_device():
    for name, arrays, want_flags, area, eleven, want_classes, _ in F.constructed():
        mapped = arrays[4].reshape(1, -1).astype(np.int32)
        for mode, want in ((False, area), (True, eleven)):
            ap, classes, flags = _frame_ap(arrays, mapped, mode)
            assert np.array_equal(flags[0], want_flags), (name, flags)
            assert int(classes[0]) == want_classes, (name, classes)
            got = float(ap[0])
            if want is None:                                   # (e), area: m terms of about 1 / 10 in the kernel's order
                assert abs(got - int(name.split("_")[1]) / 10.0) <= F.bound(len(want_flags), 10), (name, got)
            elif name.startswith("a_"):                        # thirds
                assert F.ulps(got, want) <= 1, (name, mode, got, want)
            else:
                assert F.same(got, want), (name, mode, got, want)


@pytest.mark.parametrize("idx", range(12))
def test_device_fed_metric_equals_the_reference_golden(idx):
    case = F.golden_cases()[idx]
    arrays, class_map, want = F.golden_inputs(case)
    m = FrameMApMetric(iou_thresh=case["iou_thresh"], class_names=case["class_names"], class_map=class_map)
    m.update(*_dev(arrays))
    assert m.device_updates == 1
    keys, got = m.get()
    assert keys == list(range(len(want))) and got.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = ~np.isnan(want)
    assert np.abs(got[ok] - want[ok]).max() <= 1e-12, (got, want)
    assert m.unscored == [i for i in range(len(want)) if math.isnan(want[i])]


def test_update_does_not_synchronise():
    """After the first update (which uploads the class map) an update on device tensors makes no synchronising torch
    call: torch's sync debug mode raises on one."""
    shape = C.SHAPES[7]
    arrays, _, _, host, _ = F.reference(shape)
    t = _dev(arrays)
    m = FrameMApMetric(class_map=shape[5])
    m.update(*[a[:2] for a in t])
    torch.cuda.synchronize()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.cuda.set_sync_debug_mode("error")
    try:
        m.update(*[a[2:] for a in t])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert m.device_updates == 2 and all(isinstance(c, torch.Tensor) and c.is_cuda for c in m._chunks)
    got = m.get()[1]
    assert np.abs(got - host[False]).max() <= F.bound(shape[1], shape[2])


def test_two_updates_and_the_host_path_feed_one_metric_in_arrival_order():
    shape = C.SHAPES[7]                                        # 67 frames with a class map
    arrays, _, _, host, _ = F.reference(shape)
    part = lambda lo, hi: [a[lo:hi] for a in arrays]           # noqa: E731
    key = lambda i: ("video%d" % (i // 10), i)                 # noqa: E731
    for mode in (False, True):
        m = FrameMApMetric(class_map=shape[5], use_07_metric=mode)
        m.update(*_dev(part(0, 20)), keys=[key(i) for i in range(0, 20)])
        m.update(*part(20, 30), keys=[key(i) for i in range(20, 30)])          # numpy: the host path
        m.update(*[[t[:17], t[17:]] for t in _dev(part(30, 67))], keys=[key(i) for i in range(30, 67)])   # per-device lists
        assert m.device_updates == 2
        keys, got = m.get()
        assert keys == [key(i) for i in range(67)]
        assert np.array_equal(got[20:30], host[mode][20:30])
        assert np.abs(got - host[mode]).max() <= F.bound(shape[1], shape[2])
        assert [v for v, _, _ in m.by_video()] == [v for v, _, _ in sorted(
            (("video%d" % v, sum(got[10 * v:10 * v + 10].tolist()) / len(got[10 * v:10 * v + 10]), len(got[10 * v:10 * v + 10]))
             for v in range(7)), key=lambda r: (r[1], -r[2]))]
        assert m.worst(1)[0] == (key(int(np.argmin(got))), float(got.min()))
        m.reset()
        assert m.get()[0] == [] and m._chunks == []


def test_a_frame_scores_the_same_bits_alone_in_a_batch_and_on_every_run():
    shape = C.SHAPES[7]
    arrays, mapped, _, _, _ = F.reference(shape)
    for mode in (False, True):
        whole, classes, _ = _frame_ap(arrays, mapped, mode)
        again, _, _ = _frame_ap(arrays, mapped, mode)
        assert np.array_equal(whole.view(np.int64), again.view(np.int64))
        for i in (0, 33, 66):
            alone, n, _ = _frame_ap([a[i:i + 1] for a in arrays], mapped[i:i + 1], mode)
            assert alone.view(np.int64)[0] == whole.view(np.int64)[i] and n[0] == classes[i]


def test_no_rows_and_empty_batches_through_the_metric():
    gb = torch.tensor([[F.at(C.TALL, 0), F.at(C.TALL, 1)], [F.at(C.TALL, 0), F.at(C.TALL, 1)]], dtype=torch.float32, device=DEV)
    gl = torch.tensor([[0.0, 3.0], [-1.0, -1.0]], device=DEV)
    none = torch.zeros((2, 0, 4), device=DEV)
    m = FrameMApMetric()
    m.update(none, none[:, :, 0], none[:, :, 0], gb, gl)       # no rows: still launched, 0.0 with ground truth, NaN without
    assert m.device_updates == 1
    m.update(none[:0], none[:0, :, 0], none[:0, :, 0], gb[:0], gl[:0])
    assert m.device_updates == 1
    keys, got = m.get()
    assert keys == [0, 1] and got[0] == 0.0 and math.isnan(got[1]) and m.unscored == [1]


def test_straight_from_a_net():
    """The rows a randomly initialised yolo3_darknet53 returns for 3 frames of 64 x 64 go straight into a FrameMApMetric
    and a VOCMApMetric, with ground truths copied from some of its own boxes."""
    import videoyolo_amd as vy
    classes = ["c%d" % i for i in range(20)]
    net = vy.yolo3_darknet53(classes, pretrained_base=False)
    net.initialize(init="synthetic", seed=233, obj_bias=-2.0)
    net.collect_params().reset_ctx(torch.device(DEV))
    net.set_nms(0.45, 400, 100)
    x = torch.from_numpy(np.random.default_rng(7).standard_normal((3, 3, 64, 64)).astype(np.float32)).to(DEV)
    ids, scores, bboxes = net(x)
    bboxes = bboxes.clamp(0, 64)
    kept = scores[ids >= 0]
    assert len(torch.unique(kept)) == len(kept)                # distinct scores: the host path's order is defined
    gt_boxes = bboxes[:, 0:12:2].clone() + torch.tensor([1.0, 0.0, 0.0, -1.0], device=DEV)
    gt_ids = ids[:, 0:12:2].clone()
    gt_diff = torch.zeros_like(gt_ids)
    gt_diff[:, 1] = 1
    args = (bboxes, ids, scores, gt_boxes, gt_ids, gt_diff)
    per_frame, whole = FrameMApMetric(class_names=classes), VOCMApMetric(class_names=classes)
    per_frame.update(*args, keys=["f0", "f1", "f2"])
    whole.update(*args)
    assert per_frame.device_updates == 1 and whole.device_updates == 1
    keys, got = per_frame.get()
    want = frame_map_host(*[t.cpu().numpy() for t in args])
    assert keys == ["f0", "f1", "f2"] and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.nanmax(np.abs(got - want)) <= F.bound(100, 6) and np.nanmax(got) > 0        # something matched
    assert whole.get()[1][-1] > 0


def test_bad_arguments_are_refused():
    lib = _lib.load()
    t = torch.zeros(64, device=DEV)
    p = ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ap, classes = torch.zeros(4, dtype=torch.float64, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    ok = [1, 4, 2, p, p, p, p, None, 0, ctypes.c_void_p(ap.data_ptr()), ctypes.c_void_p(classes.data_ptr()), stream]
    assert lib.vy_voc_frame_ap(*ok) == 0
    for at, bad, word in ((3, None, "null"), (4, None, "null"), (5, None, "null"), (6, None, "null"), (9, None, "null"),
                          (10, None, "null"), (0, -1, "negative"), (1, -1, "negative"), (2, -1, "negative"),
                          (1, _lib.VY_VOC_ROWS_MAX + 1, "VY_VOC_ROWS_MAX")):
        args = list(ok)
        args[at] = bad
        assert lib.vy_voc_frame_ap(*args) == -1, (at, bad)     # VY_ERR_INVALID
        assert word in lib.vy_last_error().decode()
    torch.cuda.synchronize()
