"""-m "not gpu": the VOC metric's matching rule stated per row (videoyolo_amd.metrics.voc_match_host) against the
existing per-class rule (VOCMApMetric._update_image) on the reference's recorded cases and on constructed images with
known answers, and the argument checks of the C entry vy_voc_match, which need no device."""
import ctypes

import numpy as np
import pytest

from videoyolo_amd import _lib, metrics
from videoyolo_amd.metrics import VOCMApMetric, voc_match_host

import voc_metric_cases as C


def _multiset(m):
    return {c: sorted(zip([float(s) for s in m._scores[c]], [int(f) for f in m._flags[c]])) for c in m._scores}


def test_golden_cases_are_what_the_comparison_assumes():
    """float32 inputs, no score tie within a class of an image (the existing rule's order is defined) and no pair of
    zero-area boxes (no NaN IoU)."""
    cases = C.golden_cases()
    assert len(cases) == 20
    for case in cases:
        for pb, pl, ps, gb, gl, gd in C.golden_updates(case):
            assert pb.dtype == ps.dtype == gb.dtype == np.float32
            area = lambda b: (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])    # noqa: E731
            for i in range(len(pb)):
                keep = pl[i].reshape(-1) >= 0
                pairs = np.stack([pl[i].reshape(-1)[keep], ps[i].reshape(-1)[keep]], 1)
                assert len(np.unique(pairs, axis=0)) == len(pairs)
                assert not ((area(pb[i])[keep] == 0).any() and (area(gb[i])[gl[i].reshape(-1) >= 0] == 0).any())


@pytest.mark.parametrize("idx", range(20))
def test_voc_match_host_reproduces_the_existing_rule(idx):
    """On every update of the golden cases the per-row flags give, class by class, exactly the (score, flag) multiset
    _update_image builds."""
    case = C.golden_cases()[idx]
    for pb, pl, ps, gb, gl, gd in C.golden_updates(case):
        want = VOCMApMetric(iou_thresh=case["iou_thresh"])
        got = {}
        n_det = 0
        for i in range(len(pb)):
            d = None if gd is None else gd[i]
            want._update_image(pb[i], pl[i], ps[i], gb[i], gl[i], d)
            flags = voc_match_host(pb[i], pl[i], ps[i], gb[i], gl[i], d, case["iou_thresh"])
            labels, scores = pl[i].reshape(-1), ps[i].reshape(-1)
            assert flags.dtype == np.int8 and flags.shape == labels.shape
            assert np.array_equal(flags == -2, ~(labels >= 0))
            for r in np.flatnonzero(labels >= 0):
                got.setdefault(int(labels[r]), []).append((float(scores[r]), int(flags[r])))
                n_det += 1
        assert n_det > 0
        want = _multiset(want)
        assert {c: sorted(v) for c, v in got.items()} == {c: v for c, v in want.items() if v}


@pytest.mark.parametrize("case", C.constructed(), ids=[c[0] for c in C.constructed()])
def test_constructed_known_answers(case):
    name, arrays, want_flags, want_best = case
    flags, best = voc_match_host(*arrays, 0.5, return_best=True)
    assert flags.tolist() == want_flags.tolist() and best.tolist() == want_best.tolist()
    # and the existing rule says the same of the rows that are detections
    m = VOCMApMetric(iou_thresh=0.5)
    m._update_image(*arrays)
    labels, scores = arrays[1], arrays[2]
    got = {}
    for r in np.flatnonzero(labels >= 0):
        got.setdefault(int(labels[r]), []).append((float(scores[r]), int(flags[r])))
    assert {c: sorted(v) for c, v in got.items()} == {c: v for c, v in _multiset(m).items() if v}


def test_the_constructed_ious_are_what_the_names_say():
    iou = lambda a, b: metrics.pairwise_iou(np.array([a], np.float32), np.array([b], np.float32))[0, 0]   # noqa: E731
    assert iou(C.A, C.TALL) == np.float32(0.5) == iou(C.A, C.TALL_UP)
    assert iou(C.A, C.TALLER) == np.float32(0.5) - np.float32(2.0 ** -24)
    with np.errstate(invalid="ignore"):
        assert np.isnan(iou(C.POINT, C.POINT)) and iou(C.POINT, C.FAR) == 0


def test_the_threshold_is_rounded_to_the_arrays_dtype():
    """0.7 is not a float32, and float32(0.7) lies below it: a float32 IoU of 7 / 10 matches at iou_thresh 0.7 only if the
    threshold is rounded to float32 too, as numpy does in _update_image.  float64 arrays compare in float64."""
    b32 = np.array([[0, 0, 7, 1]], np.float32)
    g32 = np.array([[0, 0, 10, 1]], np.float32)
    assert metrics.pairwise_iou(b32, g32)[0, 0] == np.float32(0.7) and float(np.float32(0.7)) < 0.7
    for dt in (np.float32, np.float64):
        args = (b32.astype(dt), np.zeros(1, dt), np.ones(1, dt), g32.astype(dt), np.zeros(1, dt), None)
        m = VOCMApMetric(iou_thresh=0.7)
        m._update_image(*args)
        assert voc_match_host(*args, 0.7).tolist() == m._flags[0] == [1]


def test_equal_scores_take_the_lower_row_first():
    """The one stated difference from _update_image, whose unstable argsort leaves equal scores to the sort."""
    b = np.array([C.A, C.A, C.A], np.float32)
    flags = voc_match_host(b, np.zeros(3), np.array([0.5, 0.5, 0.7], np.float32), np.array([C.TALL], np.float32), [0], None, 0.5)
    assert flags.tolist() == [0, 0, 1]
    flags = voc_match_host(b, np.zeros(3), np.array([0.5, 0.5, 0.2], np.float32), np.array([C.TALL], np.float32), [0], None, 0.5)
    assert flags.tolist() == [1, 0, 0]


def test_host_inputs_leave_the_device_counter_alone():
    case = C.golden_cases()[0]
    m = VOCMApMetric(iou_thresh=0.5, class_names=case["class_names"])
    for u in C.golden_updates(case):
        m.update(*u)
    assert m.device_updates == 0 and m._chunks == []
    m.reset()
    assert m._chunks == [] and m._n_pos == {}


@pytest.mark.parametrize("rows", [(3, 0, 5), (2, 0, 5)])
def test_chunks_to_host_gives_every_tensor_back_after_one_copy(rows):
    """Three chunks, one without rows; 1-, 4- and 8-byte kinds in mixed order with 1-D, 2-D and 3-D shapes.  With 7 rows
    in all the 4- and 1-byte kinds have byte counts that are no multiple of 8: joined in the given order, the wider kinds
    after them would sit at unaligned offsets."""
    import torch
    g = torch.Generator().manual_seed(0)
    ints = lambda dt, *shape: torch.randint(-100 if dt.is_signed else 0, 100, shape, generator=g).to(dt)    # noqa: E731
    chunks = [(ints(torch.int32, n), torch.randn(n, generator=g, dtype=torch.float64), ints(torch.uint8, n, 3),
               torch.rand(n, generator=g) < 0.5, ints(torch.int64, n), torch.randn((n, 4), generator=g, dtype=torch.float64),
               ints(torch.int8, n), torch.randn((n, 2, 3), generator=g), ints(torch.uint8, n, 4, 10)) for n in rows]
    got = metrics._chunks_to_host(chunks)
    assert isinstance(got, list) and len(got) == 3
    for c, h in zip(chunks, got):
        assert isinstance(h, tuple) and len(h) == len(c)
        for t, a in zip(c, h):
            want = t.numpy()
            assert isinstance(a, np.ndarray) and a.dtype == want.dtype and a.shape == want.shape and np.array_equal(a, want)
            assert a.flags.aligned
    assert metrics._chunks_to_host([]) == []


# ---------------------------------------------------------------------------------------------------------------------
# the C entry's argument checks: nothing is launched, no device is needed
def _call(lib, **over):
    a = dict(batch=2, rows=100, n_gt=8, det_box=16, det_label=16, det_score=16, gt_box=16, gt_label=16, gt_difficult=16,
             iou_thresh=0.5, best=16, flags=16)
    a.update(over)
    p = lambda v: None if v is None else ctypes.c_void_p(v)    # noqa: E731
    return lib.vy_voc_match(a["batch"], a["rows"], a["n_gt"], p(a["det_box"]), p(a["det_label"]), p(a["det_score"]),
                            p(a["gt_box"]), p(a["gt_label"]), p(a["gt_difficult"]), a["iou_thresh"], p(a["best"]),
                            p(a["flags"]), None)


def test_c_entry_argument_errors_need_no_device():
    lib = _lib.load()
    assert _lib.VY_VOC_ROWS_MAX == 1024
    bad = [{name: None} for name in ("det_box", "det_label", "det_score", "gt_box", "gt_label", "best", "flags")]
    bad += [dict(batch=-1), dict(rows=-1), dict(n_gt=-1), dict(rows=_lib.VY_VOC_ROWS_MAX + 1)]
    bad += [dict(iou_thresh=float("nan")), dict(iou_thresh=float("inf")), dict(iou_thresh=float("-inf"))]
    for over in bad:
        assert _call(lib, batch=0, **over) == -1 if "batch" not in over else _call(lib, **over) == -1, over
        assert "vy_voc_match" in lib.vy_last_error().decode(), over
    assert _call(lib, rows=1025, batch=0) == -1 and "VY_VOC_ROWS_MAX" in lib.vy_last_error().decode()
    # the empty calls: VY_OK, nothing launched (the pointers here are not device memory); no difficults is no error
    assert _call(lib, batch=0) == 0 and _call(lib, rows=0) == 0
    assert _call(lib, batch=0, rows=_lib.VY_VOC_ROWS_MAX, gt_difficult=None) == 0
