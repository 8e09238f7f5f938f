"""-m gpu: the COCO metric's matching on the device (vy_coco_match, csrc/coco_metric.hip), called directly and through
COCODetectionMetric.update on device tensors: rank and flags equal coco_match_host row for row, and a device-fed metric
equals a host-fed one — precision, recall, stats and strings — ties included."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from videoyolo_amd import _lib
from videoyolo_amd.metrics import COCODetectionMetric

import coco_metric_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (images, rows, ground truths per image, categories, contiguous_id_to_json, data_shape): every B, R, G and K of the
# kernel's branches — one row, more than 256 rows (the block-stride loop), the row cap, more than 100 rows of a category,
# no / one / many ground truths, one category (every chain group but one idle) and more categories than groups, more
# images than one launch's table (VY_COCO_CHUNK 128 is not reached by 67; test_more_images_than_one_launch does)
SHAPES = [(1, 1, 0, 1, True, None), (5, 100, 1, 20, False, (416, 416)), (67, 100, 70, 80, True, None),
          (5, 257, 300, 1, True, (320, 416)), (2, 1024, 70, 20, True, None)]
_refs = {}


def _reference(shape):
    """The seeded set of a shape and the host-fed metric (its chunk holds coco_match_host's rank and flags), once."""
    if shape not in _refs:
        b, r, g, k, use_map, data_shape = shape
        ds, arrays = C.seeded_set(500 + 3 * b + r + g + k, b, r, g, k, use_map, data_shape)
        host = COCODetectionMetric(ds, data_shape=data_shape)
        host.update(*arrays)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            strings = host.get()
        _refs[shape] = (ds, arrays, host, strings)
    return _refs[shape]


def _dev(arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _same_results(m, host, strings=None):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = m.get()
        want = host.get() if strings is None else strings
    assert np.array_equal(m.precision, host.precision) and np.array_equal(m.recall, host.recall)
    assert np.array_equal(m.stats, host.stats)
    assert got == want


def _match(metric, xywh, cat, score, rows, max_det):
    """vy_coco_match itself on host-prepared float64 rows: (rank, flags) as numpy."""
    batch, n = cat.shape
    n_a, n_t = len(metric._ar), len(metric._thr)
    t = metric._tables_on(torch.device(DEV))
    d = _dev([xywh, cat.astype(np.int32), score])
    rank = torch.full((batch, n), -7, dtype=torch.int32, device=DEV)
    flags = torch.full((batch, n, n_a, n_t), 77, dtype=torch.uint8, device=DEV)
    taken_bytes = int((metric._gt_off[rows + 1] - metric._gt_off[rows]).sum()) * n_a * n_t
    taken = torch.full((max(taken_bytes, 1),), 1, dtype=torch.uint8, device=DEV)      # dirty: the kernel clears its own
    p = lambda x: ctypes.c_void_p(x.data_ptr())                  # noqa: E731
    h = lambda a: a.ctypes.data_as(ctypes.c_void_p)              # noqa: E731
    gt_image, ar = rows.astype(np.int32), np.ascontiguousarray(metric._ar)
    _lib.check(_lib.load().vy_coco_match(
        batch, n, p(d[0]), p(d[1]), p(d[2]), h(gt_image), len(metric._eval_ids), h(metric._gt_off), p(t['_gt_xywh']),
        p(t['_gt_cat']), p(t['_gt_area']), p(t['_gt_crowd']), p(t['_gt_id']), n_t, h(metric._thr), n_a, h(ar), max_det,
        p(taken), taken_bytes, p(rank), p(flags), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return rank.cpu().numpy(), flags.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-R%d-G%d-K%d" % s[:4])
def test_kernel_equals_coco_match_host_row_for_row(shape):
    ds, arrays, host, _ = _reference(shape)
    rows, cat, score, rank, flags, keep, file_cat, xywh = host._chunks[0]
    got_rank, got_flags = _match(host, xywh, cat, score, rows, 100)
    assert np.array_equal(got_rank, rank)
    assert np.array_equal(got_flags, flags)
    assert (rank >= 0).any() or shape[1] == 1
    if shape[1] > 120:
        assert (rank == 99).any() and ((cat >= 0) & (rank < 0)).any()         # a category's rows were cut at max_det


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-R%d-G%d-K%d" % s[:4])
def test_device_fed_metric_equals_host_fed(shape):
    ds, arrays, host, strings = _reference(shape)
    inputs = _dev(arrays)
    before = [t.clone() for t in inputs]
    m = COCODetectionMetric(ds, data_shape=shape[5])
    m.update(*inputs)
    assert m.device_updates == 1
    for t, b in zip(inputs, before):
        assert torch.equal(t, b)                               # the inputs are left alone
    for kind in range(1, 5):
        assert np.array_equal(m._chunks[0][kind].cpu().numpy(), host._chunks[0][kind])
    _same_results(m, host, strings)


def test_small_max_det_and_custom_thresholds():
    """max_det below a category's rows, 16 thresholds x 8 ranges (128 chains: two category groups)."""
    ds, arrays = C.seeded_set(77, 3, 100, 20, 5)
    kw = dict(iou_thrs=np.linspace(.2, .95, 16), area_ranges=[[0, 1e10]] + [[a * 1000, (a + 3) * 1000] for a in range(7)],
              max_dets=[1, 3, 7])
    host, m = COCODetectionMetric(ds, **kw), COCODetectionMetric(ds, **kw)
    host.update(*arrays)
    m.update(*_dev(arrays))
    assert m.device_updates == 1
    for kind in range(1, 5):
        assert np.array_equal(m._chunks[0][kind].cpu().numpy(), host._chunks[0][kind])
    assert host._chunks[0][3].max() == 6
    _same_results(m, host)


def test_more_images_than_one_launch():
    b = _lib.VY_COCO_CHUNK + 3
    ds, arrays = C.seeded_set(78, b, 10, 3, 4)
    host, m = COCODetectionMetric(ds), COCODetectionMetric(ds)
    host.update(*arrays)
    m.update(*_dev(arrays))
    for kind in range(1, 5):
        assert np.array_equal(m._chunks[0][kind].cpu().numpy(), host._chunks[0][kind])
    _same_results(m, host)


@pytest.mark.parametrize("name", sorted(C.known_cases()))
def test_known_answers_through_the_device_path(name):
    case = C.known_cases()[name]
    ds, _, arrays = C.build_case(case)
    m = COCODetectionMetric(ds)
    m.update(*_dev([a.astype(np.float32) for a in arrays]))
    assert m.device_updates == 1
    m.get()
    for i, want in case[4].items():
        print(name, i, m.stats[i], want)
        assert abs(m.stats[i] - want) <= 1e-12


def test_what_takes_the_host_path():
    ds, arrays = C.seeded_set(79, 2, _lib.VY_COCO_ROWS_MAX + 1, 5, 3)
    m = COCODetectionMetric(ds)
    m.update(*_dev(arrays))                                                   # 1025 rows
    assert m.device_updates == 0
    m.reset()
    m.update(*arrays)                                                         # numpy
    m.reset()
    m.update(*[t.double() for t in _dev(arrays)])                             # another dtype
    assert m.device_updates == 0
    m.reset()
    m.update(*_dev([a[:, :1024] for a in arrays]))
    assert m.device_updates == 1


def test_update_does_not_synchronise():
    """After the first update (which uploads the dataset's tables) an update on device tensors makes no synchronising
    torch call: torch's sync debug mode raises on one."""
    shape = SHAPES[1]
    ds, arrays, host, strings = _reference(shape)
    t = _dev(arrays)
    m = COCODetectionMetric(ds, data_shape=shape[5])
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
    _same_results(m, host, strings)


def test_lists_two_updates_and_both_paths_feed_one_metric():
    shape = SHAPES[2]
    ds, arrays, host, strings = _reference(shape)
    m = COCODetectionMetric(ds)
    part = lambda lo, hi: [a[lo:hi] for a in arrays]                         # noqa: E731
    m.update(*_dev(part(40, 67)), sid=range(40, 67))
    m.update(*part(0, 10), sid=range(10))                                     # host arrays: the host path
    m.update(*[[x, y] for x, y in zip(_dev(part(10, 25)), _dev(part(25, 40)))], sid=range(10, 40))      # lists
    assert m.device_updates == 2
    with pytest.raises(ValueError, match="given before"):
        m.update(*_dev(part(3, 4)), sid=3)
    with pytest.raises(ValueError, match="not an image"):
        m.update(*_dev(part(3, 4)), sid=1000)
    _same_results(m, host, strings)


def test_rows_of_a_detector():
    """The rows a randomly initialised yolo3_darknet53(classes=20) returns for 3 frames of 64 x 64, ground truths copied
    from its own boxes."""
    import videoyolo_amd as vy
    classes = ["c%d" % i for i in range(20)]
    net = vy.yolo3_darknet53(classes, pretrained_base=False)
    net.initialize(init="synthetic", seed=233, obj_bias=-2.0)
    net.collect_params().reset_ctx(torch.device(DEV))
    net.set_nms(0.45, 400, 100)
    rng = np.random.default_rng(7)
    frames = torch.from_numpy(rng.standard_normal((3, 3, 64, 64)).astype(np.float32)).to(DEV)
    ids, scores, bboxes = net(frames)
    assert ids.is_cuda and ids.shape[0] == 3
    hi, hb = ids.cpu().numpy().reshape(3, -1), bboxes.cpu().numpy().reshape(3, -1, 4).astype(np.float64)
    anns = []
    for i in range(3):
        for r in np.flatnonzero(hi[i] >= 0)[:4 * i]:                          # image 0 has no ground truth
            x1, y1, x2, y2 = hb[i, r]
            anns.append(C.ann(i, int(hi[i, r]), [x1, y1, x2 - (x1 - 1), y2 - (y1 - 1)], len(anns)))
    ds = C.Dataset([0, 1, 2], anns, list(range(20)))
    dev_metric, host_metric = COCODetectionMetric(ds, score_thresh=0.0), COCODetectionMetric(ds, score_thresh=0.0)
    dev_metric.update(bboxes, ids, scores)
    host_metric.update(bboxes.cpu().numpy(), ids.cpu().numpy(), scores.cpu().numpy())
    assert dev_metric.device_updates == 1 and int((ids >= 0).sum()) > 0
    _same_results(dev_metric, host_metric)
    assert len(anns) < 2 or dev_metric.stats[0] > 0
