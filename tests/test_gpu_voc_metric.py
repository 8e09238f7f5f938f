"""-m gpu: the VOC metric's matching on the device (vy_voc_match, csrc/voc_metric.hip), called directly and through
VOCMApMetric.update on device tensors: equal to the reference's recorded values, and to voc_match_host and the host path
value for value."""
import ctypes
import json
import math
import warnings

import numpy as np
import pytest
import torch

from videoyolo_amd import _lib
from videoyolo_amd.metrics import VOC07MApMetric, VOCMApMetric, voc_match_host

import voc_metric_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_refs = {}


def _dev(arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _match(arrays, iou_thresh, class_map=None):
    """vy_voc_match itself on a batch of float32 arrays: (flags, best) as numpy (B, R)."""
    pb, pl, ps, gb, gl, gd = arrays
    batch, rows, n_gt = pb.shape[0], pb.shape[1], gb.shape[1]
    mapped = np.stack([C.mapped_labels(gl[i], class_map) for i in range(batch)]).reshape(batch, n_gt)
    mapped = np.where(mapped >= 0, mapped, -1).astype(np.int32)
    t = _dev([pb, pl.reshape(batch, rows), ps.reshape(batch, rows), gb, mapped,
              None if gd is None else (gd.reshape(batch, n_gt) != 0).astype(np.uint8)])
    best = torch.full((batch, rows), -7, dtype=torch.int32, device=DEV)
    flags = torch.full((batch, rows), -7, dtype=torch.int8, device=DEV)
    spare = torch.zeros(16, device=DEV)
    p = lambda x: None if x is None else ctypes.c_void_p((x if x.numel() else spare).data_ptr())    # noqa: E731
    _lib.check(_lib.load().vy_voc_match(batch, rows, n_gt, p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(t[4]), p(t[5]), iou_thresh,
                                        p(best), p(flags), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return flags.cpu().numpy(), best.cpu().numpy()


def _reference(shape):
    """The seeded batch of a shape, its per-row flags and best by voc_match_host and the host-fed metric's get(), once."""
    key = C.shape_id(shape)
    if key not in _refs:
        batch, rows, n_gt, n_cls, difficult, class_map = shape
        arrays = C.random_batch(1000 + 7 * batch + rows + n_gt, batch, rows, n_gt, n_cls, difficult, class_map)
        pb, pl, ps, gb, gl, gd = arrays
        flags, best = np.zeros((batch, rows), np.int8), np.zeros((batch, rows), np.int64)
        for i in range(batch):
            flags[i], best[i] = voc_match_host(pb[i], pl[i], ps[i], gb[i], C.mapped_labels(gl[i], class_map),
                                               None if gd is None else gd[i], 0.5, return_best=True)
        host = VOCMApMetric(iou_thresh=0.5, class_map=class_map)
        host.update(*arrays)
        _refs[key] = (arrays, flags, best, host.get(), dict(host._n_pos))
    return _refs[key]


def _same_value(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def _close(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == pytest.approx(b, abs=1e-12)


@pytest.mark.parametrize("idx", range(20))
def test_device_metrics_equal_the_reference_golden(idx):
    case = C.golden_cases()[idx]
    for cls in (VOCMApMetric, VOC07MApMetric):
        m = cls(iou_thresh=case["iou_thresh"], class_names=case["class_names"])
        for u in C.golden_updates(case):
            m.update(*_dev(u))
        assert m.device_updates == len(case["updates"]) > 0
        name, value = m.get()
        exp = case["expected"][cls.__name__]
        assert name == exp["name"]
        if isinstance(exp["value"], list):
            assert len(value) == len(exp["value"])
            assert all(_close(float(a), float(b)) for a, b in zip(value, exp["value"])), (value, exp["value"])
        else:
            assert _close(float(value), float(exp["value"]))


def test_constructed_known_answers_on_the_device():
    arrays, want_flags, want_best = C.constructed_batch()
    flags, best = _match(arrays, 0.5)
    assert np.array_equal(flags, want_flags), (flags, want_flags)
    assert np.array_equal(best, want_best), (best, want_best)


@pytest.mark.parametrize("shape", C.SHAPES, ids=[C.shape_id(s) for s in C.SHAPES])
def test_kernel_equals_voc_match_host_per_row(shape):
    arrays, want_flags, want_best, _, _ = _reference(shape)
    flags, best = _match(arrays, 0.5, shape[5])
    assert np.array_equal(best, want_best), np.argwhere(best != want_best)[:5]
    assert np.array_equal(flags, want_flags), np.argwhere(flags != want_flags)[:5]
    if shape[1] > 1 and shape[2] > 1:                          # the batch reaches every kind of row
        assert all((flags == v).any() for v in ((-2, 0, 1, -1) if shape[4] else (-2, 0, 1)))
        taken = (want_best >= 0) & (flags == 0)
        assert taken.any()                                     # a second claimant of a ground truth


@pytest.mark.parametrize("shape", C.SHAPES, ids=[C.shape_id(s) for s in C.SHAPES])
def test_device_fed_metric_equals_host_fed_metric(shape):
    arrays, _, _, want, want_n_pos = _reference(shape)
    inputs = _dev(arrays)
    before = [None if t is None else t.clone() for t in inputs]
    m = VOCMApMetric(iou_thresh=0.5, class_map=shape[5])
    m.update(*inputs)
    assert m.device_updates == 1
    for t, b in zip(inputs, before):
        assert t is None or torch.equal(t, b)                  # the inputs are left alone
    got = m.get()
    assert got[0] == want[0] and _same_value(got[1], want[1]), (got, want)
    assert m._n_pos == want_n_pos
    assert m._chunks == []


def test_two_updates_lists_and_both_paths_feed_one_metric():
    shape = C.SHAPES[7]                                        # 67 images with a class map
    arrays, _, _, _, _ = _reference(shape)
    names = ["c%d" % i for i in range(25)]
    host = VOC07MApMetric(iou_thresh=0.5, class_names=names, class_map=shape[5])
    host.update(*arrays)
    m = VOC07MApMetric(iou_thresh=0.5, class_names=names, class_map=shape[5])
    part = lambda lo, hi: [a[lo:hi] for a in arrays]           # noqa: E731
    m.update(*_dev(part(0, 20)))
    m.update(*part(20, 30))                                    # numpy: the host path
    m.update(*[[t[:17], t[17:]] for t in _dev(part(30, 67))])  # lists of per-device tensors, joined along the batch
    assert m.device_updates == 2
    got, want = m.get(), host.get()
    assert got[0] == want[0] and all(_same_value(a, b) for a, b in zip(got[1], want[1])), (got, want)
    assert m._n_pos == host._n_pos
    m.reset()
    assert m._chunks == [] and m._n_pos == {} and m._scores == {}
    m.update(*_dev(part(0, 20)))
    m.reset()
    assert m._chunks == []
    assert math.isnan(VOCMApMetric().get()[1])


def test_fallbacks_take_the_host_path():
    """More rows than the cap, float64 ground truths and a dict class_map: no launch, the host path's results."""
    arrays = C.random_batch(5, 2, _lib.VY_VOC_ROWS_MAX + 1, 8, 5)
    host = VOCMApMetric(iou_thresh=0.5)
    host.update(*arrays)
    m = VOCMApMetric(iou_thresh=0.5)
    m.update(*_dev(arrays))
    assert m.device_updates == 0 and m._chunks == [] and m.get() == host.get()

    arrays = C.random_batch(6, 3, 50, 8, 5)
    host = VOCMApMetric(iou_thresh=0.5)
    host.update(*arrays)
    m = VOCMApMetric(iou_thresh=0.5)
    t = _dev(arrays)
    t[3] = t[3].double()
    m.update(*t)
    assert m.device_updates == 0 and m._chunks == [] and m.get() == host.get()
    m.update(*_dev(arrays)[:5], torch.from_numpy(arrays[5]).to(DEV).to(torch.int64))    # difficults of another dtype
    assert m.device_updates == 1

    as_dict = {i: v for i, v in enumerate(C.DROPPING_MAP)}
    as_dict[-1] = C.DROPPING_MAP[-1]
    arrays = C.random_batch(7, 3, 50, 8, 20, True, C.DROPPING_MAP)
    host = VOCMApMetric(iou_thresh=0.5, class_map=as_dict)
    host.update(*arrays)
    m = VOCMApMetric(iou_thresh=0.5, class_map=as_dict)
    m.update(*_dev(arrays))
    assert m.device_updates == 0 and m._chunks == [] and m.get() == host.get()
    seq = VOCMApMetric(iou_thresh=0.5, class_map=C.DROPPING_MAP)
    seq.update(*_dev(arrays))
    assert seq.device_updates == 1 and seq.get() == host.get()


def test_update_does_not_synchronise():
    """After the first update (which uploads the class map) an update on device tensors makes no synchronising torch
    call: torch's sync debug mode raises on one.  (The library call itself owns no device memory and copies nothing.)"""
    shape = C.SHAPES[7]
    arrays, _, _, want, _ = _reference(shape)
    t = _dev(arrays)
    m = VOCMApMetric(iou_thresh=0.5, class_map=shape[5])
    m.update(*[a[:2] for a in t])
    torch.cuda.synchronize()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.cuda.set_sync_debug_mode("error")
    try:
        m.update(*[a[2:] for a in t])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert m.device_updates == 2
    got = m.get()
    assert got[0] == want[0] and _same_value(got[1], want[1])


def test_equal_scores_take_the_lower_row_first_on_the_device():
    b = np.array([[C.A, C.A, C.A]], np.float32)
    arrays = (b, np.zeros((1, 3), np.float32), np.array([[0.5, 0.5, 0.7]], np.float32), np.array([[C.TALL]], np.float32),
              np.zeros((1, 1), np.float32), None)
    assert _match(arrays, 0.5)[0].tolist() == [[0, 0, 1]]
    arrays = arrays[:2] + (np.array([[0.5, 0.5, 0.2]], np.float32),) + arrays[3:]
    assert _match(arrays, 0.5)[0].tolist() == [[1, 0, 0]]


def test_straight_from_a_net():
    """The rows a randomly initialised yolo3_darknet53 returns for 3 frames of 64 x 64 go straight into update, with ground
    truths copied from some of its own boxes; the result equals the host path's."""
    import videoyolo_amd as vy
    classes = ["c%d" % i for i in range(20)]
    net = vy.yolo3_darknet53(classes, pretrained_base=False)
    net.initialize(init="synthetic", seed=233, obj_bias=-2.0)
    net.collect_params().reset_ctx(torch.device(DEV))
    net.set_nms(0.45, 400, 100)
    x = torch.from_numpy(np.random.default_rng(7).standard_normal((3, 3, 64, 64)).astype(np.float32)).to(DEV)
    ids, scores, bboxes = net(x)
    bboxes = bboxes.clamp(0, 64)
    assert ids.is_cuda and ids.shape == (3, 100, 1) and int((ids >= 0).sum()) > 6
    kept = scores[ids >= 0]
    assert len(torch.unique(kept)) == len(kept)                # distinct scores: the host path's order is defined
    gt_boxes = bboxes[:, 0:12:2].clone() + torch.tensor([1.0, 0.0, 0.0, -1.0], device=DEV)
    gt_ids = ids[:, 0:12:2].clone()
    gt_diff = torch.zeros_like(gt_ids)
    gt_diff[:, 1] = 1
    m, host = VOCMApMetric(class_names=classes), VOCMApMetric(class_names=classes)
    m.update(bboxes, ids, scores, gt_boxes, gt_ids, gt_diff)
    host.update(*[t.cpu().numpy() for t in (bboxes, ids, scores, gt_boxes, gt_ids, gt_diff)])
    assert m.device_updates == 1 and host.device_updates == 0
    got, want = m.get(), host.get()
    assert got[0] == want[0] and all(_same_value(a, b) for a, b in zip(got[1], want[1])), json.dumps([got[1], want[1]])
    assert any(v == v and v > 0 for v in got[1])               # something matched
