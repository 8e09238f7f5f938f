"""-m "not gpu": the ImageNet-VID motion / area mAP on the host.  vid_match_host and VIDDetectionMetric against the values
the reference's own vid_eval_motion produced (tests/golden/vid_metric_golden.json), and the argument checks of the C
entry, which need no device."""
import ctypes

import numpy as np
import pytest

import videoyolo_amd as vy
from videoyolo_amd import _lib
from videoyolo_amd.metrics import VIDDetectionMetric, vid_match_host

import vid_metric_cases as C


def _metric(c, **extra):
    return VIDDetectionMetric(C.case_dataset(c), **dict(c["kwargs"], **extra))


def test_golden_holds_every_listed_case():
    names = C.case_names()
    for want in ("random", "crowd_70gt_100det", "edges", "class_map_drops_last", "class_map_drops_middle", "agnostic",
                 "offset_list_ids"):
        assert want in names
    crowd = C.case("crowd_70gt_100det")
    assert any(len(v) == 70 for v in crowd["dataset"]["labels"].values())
    assert any(sum(1 for l, s in zip(f["labels"], f["scores"]) if l >= 0 and s >= 0.05) == 100 for f in crowd["frames"])
    for c in C.golden_cases():
        s = np.asarray(c["expected"]["det_scores"])
        assert len(np.unique(s)) == len(s) > 0                                   # no ties: the reference's order is defined
        assert any(len(v) == 0 for v in c["dataset"]["labels"].values()) or c["name"].startswith("crowd")
    edges = C.case("edges")
    mo = sum(edges["dataset"]["motion_ious"].values(), [])
    assert 0.7 in mo and 0.9 in mo
    area = [(r[2] - r[0] + 1) * (r[3] - r[1] + 1) for v in edges["dataset"]["labels"].values() for r in v]
    assert 2500 in area and 22500 in area


@pytest.mark.parametrize("name", C.case_names())
def test_host_metric_equals_the_reference(name):
    c = C.case(name)
    m = _metric(c)
    for sid, b, l, s in C.case_frames(c):
        m.update(b[None], l[None], s[None], sid=sid)
    C.check_against_golden(m, c)


@pytest.mark.parametrize("name", ["edges", "class_map_drops_last"])
def test_vid_match_host_per_frame_equals_the_reference(name):
    """vid_match_host called directly, frame by frame, on the tables the metric built."""
    c = C.case(name)
    m = _metric(c)
    _, _, want_tp, want_fp = C.expected_matches(c)
    by_sid = {sid: (b, l, s) for sid, b, l, s in C.case_frames(c)}
    at = 0
    for sid in c["expected"]["order"]:
        b, l, s = by_sid[sid]
        keep = np.flatnonzero((l >= 0) & (s.astype(np.float64) >= m._conf_score_thresh))
        keep = keep[np.argsort(-s[keep].astype(np.float64), kind="stable")]
        r = m._row[sid]
        g0, g1 = m._gt_off[r], m._gt_off[r + 1]
        tp, fp = vid_match_host(b[keep], l[keep], m._gt_box[g0:g1], m._gt_label[g0:g1], m._gt_thr[g0:g1],
                                m._gt_motion[g0:g1], vy.metrics.VID_MOTION_RANGES, vy.metrics.VID_AREA_RANGES,
                                m._empty_weight, m._gt_nig[r])
        assert np.array_equal(tp, want_tp[at:at + len(keep)]) and np.array_equal(fp, want_fp[at:at + len(keep)])
        at += len(keep)
    assert at == len(want_tp)


def test_the_edge_frames_score_as_stated():
    """The hand-built frames of the 'edges' case, slice 0 (every motion, every area), read off the reference's values."""
    c = C.case("edges")
    _, _, tp, fp = C.expected_matches(c)
    start = np.concatenate([[0], np.cumsum([sum(1 for l, s in zip(f["labels"], f["scores"]) if l >= 0 and s >= 0.05)
                                            for f in c["frames"]])])
    assert tp[start[0], 0] == 1                              # ov == thr matches
    assert tp[start[1]:start[2], 0].tolist() == [1, 0] and fp[start[1] + 1, 0] == 1.0   # the second detection misses
    assert tp[start[2]:start[3], 0].tolist() == [1, 1]       # equal overlap: one ground truth each
    assert tp[start[3], 0] == 1                              # small object: ov 0.43 >= thr 0.25
    assert start[7] == start[8]                              # the last frame keeps no row


def test_two_updates_equal_one_and_batches_equal_frames():
    c = C.case("random")
    frames = C.case_frames(c)
    one = _metric(c)
    one.update(np.stack([f[1] for f in frames]), np.stack([f[2] for f in frames]), np.stack([f[3] for f in frames])[..., None],
               sid=[f[0] for f in frames])
    two = _metric(c)
    h = len(frames) // 2
    for part in (frames[h:], frames[:h]):                    # any order of arrival
        two.update(np.stack([f[1] for f in part]), np.stack([f[2] for f in part])[..., None], np.stack([f[3] for f in part]),
                   None, None, None, sid=np.asarray([f[0] for f in part]))
    C.check_against_golden(one, c)
    C.check_against_golden(two, c)
    assert np.array_equal(one.ap, two.ap)
    one.reset()
    assert one.ap is None and len(one.matches()[0]) == 0
    for sid, b, l, s in frames:
        one.update([b[None]], [l[None]], [s[None]], sid=sid)  # lists of arrays, scalar sid
    C.check_against_golden(one, c)


def test_sid_errors():
    c = C.case("random")
    m = _metric(c)
    sid, b, l, s = C.case_frames(c)[0]
    with pytest.raises(ValueError, match="needs sid"):
        m.update(b[None], l[None], s[None])
    with pytest.raises(ValueError, match="not one of"):
        m.update(b[None], l[None], s[None], sid=12345)
    with pytest.raises(ValueError, match="2 ids for a batch of 1"):
        m.update(b[None], l[None], s[None], sid=[sid, sid])
    m.update(b[None], l[None], s[None], sid=sid)
    with pytest.raises(ValueError, match="given before"):
        m.update(b[None], l[None], s[None], sid=sid)
    other = C.case_frames(c)[1][0]
    with pytest.raises(ValueError, match="given before"):
        m.update(np.stack([b, b]), np.stack([l, l]), np.stack([s, s]), sid=[other, other])
    assert len(m._seen) == 1                                  # a refused call leaves nothing behind
    m.reset()
    m.update(b[None], l[None], s[None], sid=sid)


def test_ties_keep_their_order():
    """Equal scores: stable sorts, so a permutation of equal-score rows changes which one claims a ground truth, and the
    host path says which (the project's choice; the reference leaves it to argsort's internals)."""
    ds = C.StandInDataset([0], {0: np.array([[0, 0, 99, 99, 0.0]])}, {"0": [0.5]}, ["n00"], ["class_n00"])
    m = VIDDetectionMetric(ds)
    b = np.array([[[0, 0, 99, 99], [1, 1, 100, 100]]], np.float32)
    m.update(b, np.zeros((1, 2)), np.full((1, 2), 0.5), sid=0)
    assert m.matches()[3][:, 0].tolist() == [1, 0]


def test_exported():
    assert vy.VIDDetectionMetric is VIDDetectionMetric and "VIDDetectionMetric" in vy.__all__


# ---------------------------------------------------------------------------------------------------------------------
# the C entry's argument checks: nothing is launched, no device is needed
def _call(lib, **over):
    f64, i32, i64 = np.float64, np.int32, np.int64
    a = dict(n_frames=2, det_off=np.array([0, 3, 5], i64), det_box=16, det_label=16, det_score=16, conf=0.05,
             gt_frame=np.array([1, 0], i32), n_gt_frames=2, gt_off=np.array([0, 2, 3], i64), gt_box=16, gt_label=16, gt_thr=16,
             gt_motion=16, gt_nig=16, n_motion=2, motion=np.array([0, 1, 0, 0.7], f64), n_area=1, area=np.array([0, 1e10], f64),
             ew=np.array([1.0, 0.5], f64), flags=16, flags_bytes=6, tp=16, fp=16)
    a.update(over)

    def p(v):
        if v is None:
            return None
        return ctypes.c_void_p(v) if isinstance(v, int) else v.ctypes.data_as(ctypes.c_void_p)
    return lib.vy_vid_match(a["n_frames"], p(a["det_off"]), p(a["det_box"]), p(a["det_label"]), p(a["det_score"]), a["conf"],
                            p(a["gt_frame"]), a["n_gt_frames"], p(a["gt_off"]), p(a["gt_box"]), p(a["gt_label"]), p(a["gt_thr"]),
                            p(a["gt_motion"]), p(a["gt_nig"]), a["n_motion"], p(a["motion"]), a["n_area"], p(a["area"]),
                            p(a["ew"]), p(a["flags"]), a["flags_bytes"], p(a["tp"]), p(a["fp"]), None)


def test_c_entry_argument_errors_need_no_device():
    lib = _lib.load()
    f64, i32, i64 = np.float64, np.int32, np.int64
    for name in ("det_off", "det_box", "det_label", "det_score", "gt_frame", "gt_off", "gt_box", "gt_label", "gt_thr",
                 "gt_motion", "gt_nig", "motion", "area", "ew", "flags", "tp", "fp"):
        assert _call(lib, **{name: None}) == -1, name
        assert "vy_vid_match" in lib.vy_last_error().decode()
    assert _call(lib, n_frames=-1) == -1 and _call(lib, n_gt_frames=-1) == -1 and _call(lib, flags_bytes=-1) == -1
    assert _call(lib, det_off=np.array([0, 3, 2], i64)) == -1 and "ascend" in lib.vy_last_error().decode()
    assert _call(lib, det_off=np.array([-1, 3, 5], i64)) == -1
    assert _call(lib, gt_off=np.array([0, 2, 1], i64)) == -1 and "ascend" in lib.vy_last_error().decode()
    assert _call(lib, gt_off=np.array([1, 0, 3], i64)) == -1
    assert _call(lib, gt_frame=np.array([1, 2], i32)) == -1 and _call(lib, gt_frame=np.array([-1, 0], i32)) == -1
    nine = np.tile(np.array([0.0, 1.0]), 9)
    assert _call(lib, n_motion=9, motion=nine, ew=np.ones(9)) == -1 and _call(lib, n_area=9, area=nine) == -1
    assert _call(lib, n_motion=0) == -1 and _call(lib, n_area=0) == -1
    assert _call(lib, motion=np.array([0, 1, 0.9, 0.7], f64)) == -1 and "lo > hi" in lib.vy_last_error().decode()
    assert _call(lib, area=np.array([2500.0, 0.0], f64)) == -1
    assert _call(lib, flags_bytes=5) == -1 and "flag bytes" in lib.vy_last_error().decode()
    # an empty batch, and a batch without rows: VY_OK, nothing launched (the pointers here are not device memory)
    assert _call(lib, n_frames=0) == 0
    assert _call(lib, det_off=np.array([4, 4, 4], i64)) == 0
