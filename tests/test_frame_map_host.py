"""-m "not gpu": the per-frame mAP on the host — frame_map_host against the reference's recorded per-frame scores, the numpy
model of the kernel (tests/frame_map_model.py) against frame_map_host and against hand-derived answers, the planted
bugs, and FrameMApMetric's bookkeeping (keys, worst, by_video, unscored, lines, reset, fallbacks)."""
import math

import numpy as np
import pytest

import videoyolo_amd as vy
from videoyolo_amd.metrics import (FrameMApMetric, VOC07MApMetric, VOCMApMetric, frame_map_host, frame_metric_lines,
                                   voc_match_host)

import frame_map_cases as F
import frame_map_model as M
import voc_metric_cases as C

SHAPE_IDS = [C.shape_id(s) for s in C.SHAPES]


@pytest.mark.parametrize("idx", range(12))
def test_frame_map_host_equals_the_reference_golden(idx):
    case = F.golden_cases()[idx]
    arrays, class_map, want = F.golden_inputs(case)
    for frame in arrays[2]:
        kept = frame[frame >= 0]
        assert len(np.unique(kept)) == len(kept)               # distinct scores: the reference's order is defined
    got = frame_map_host(*arrays, iou_thresh=case["iou_thresh"], class_map=class_map)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = ~np.isnan(want)
    assert np.abs(got[ok] - want[ok]).max() <= 1e-12, (got, want)


def test_golden_covers_what_it_should():
    cases = F.golden_cases()
    assert len(cases) == 12 and all(len(c["expected"]) == 4 for c in cases)
    assert any(c["spec"]["class_map"] for c in cases) and any(c["spec"]["difficult"] for c in cases)
    assert any(not c["spec"]["difficult"] for c in cases)
    values = [e for c in cases for e in c["expected"]]
    assert any(e is None for e in values) and len({e for e in values if e is not None}) > 20


@pytest.mark.parametrize("shape", C.SHAPES, ids=SHAPE_IDS)
def test_model_equals_frame_map_host(shape):
    _, mapped, _, host, model = F.reference(shape)
    for mode in (False, True):
        got, classes = model[mode]
        want = host[mode]
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(classes == 0, np.isnan(want))
        ok = ~np.isnan(want)
        if ok.any():
            worst = np.abs(got[ok] - want[ok]).max()
            print("%s use_07=%s: worst |model - host| %.3g, bound %.3g" % (C.shape_id(shape), mode, worst, F.bound(*shape[1:3])))
            assert worst <= F.bound(shape[1], shape[2])


def test_seeded_batches_cannot_be_passed_by_a_constant():
    """What tests/test_gpu_frame_map.py relies on, shown here on the host values.  (B5_R1_M300_C20 has one row per frame:
    three of its five frames score 0 in both modes, so distinctness is asked of the shapes with more than one row.)"""
    for shape in C.SHAPES:
        host = F.reference(shape)[3]
        if shape[2] >= 70:
            assert not np.isnan(host[False]).any() and not np.isnan(host[True]).any()
            if shape[1] > 1:
                assert len(np.unique(host[False])) == shape[0]
                assert (host[False] != host[True]).all()
            else:
                assert len(np.unique(host[False])) > 1 and (host[False] != host[True]).any()
    assert int(np.isnan(F.reference(C.SHAPES[8])[3][False]).sum()) == 14 and C.shape_id(C.SHAPES[8]) == "B67_R257_M1_C80"


def _model_on(case, use_07, bug=None):
    _, (pb, pl, ps, gb, gl, gd), flags, area, eleven, classes, _ = case
    return M.frame_score(pl[0], ps[0], flags, gl[0], gd[0], use_07, bug)


def _constructed_failures(bug=None):
    """The constructed cases the model misses, as test_constructed_known_answers holds it to them."""
    missed = []
    for case in F.constructed():
        name, area, eleven, classes = case[0], case[3], case[4], case[5]
        for use_07, want in ((False, area), (True, eleven)):
            got, n = _model_on(case, use_07, bug)
            if want is None:                                   # (e), area: m terms of about 1 / 10 in the kernel's order
                want, tol = int(name.split("_")[1]) / 10.0, F.bound(len(case[2]), 10)
            else:
                tol = np.spacing(want) if name.startswith("a_") else 0.0
            if n != classes or not (F.same(got, want) or abs(got - want) <= tol):
                missed.append((name, use_07, got, want))
    return missed


def test_constructed_known_answers():
    for name, arrays, flags, area, eleven, classes, on_host in F.constructed():
        pb, pl, ps, gb, gl, gd = arrays
        got_flags = voc_match_host(pb[0], pl[0], ps[0], gb[0], gl[0], gd[0], 0.5)
        assert np.array_equal(got_flags, flags), (name, got_flags)
        if on_host:
            for use_07, want in ((False, area), (True, eleven)):
                got = frame_map_host(*arrays, use_07_metric=use_07)[0]
                if want is None:
                    assert abs(got - int(name.split("_")[1]) / 10.0) <= F.bound(len(flags), 10), (name, got)
                else:
                    assert F.same(got, want) or F.ulps(got, want) <= 1, (name, use_07, got, want)
    assert _constructed_failures() == []
    # (e): the thresholds recall m / 10 just misses
    assert [0.0 + k * 0.1 for k in (3, 6, 7)] == [0.30000000000000004, 0.6000000000000001, 0.7000000000000001]
    assert 3 / 10 < 0.0 + 3 * 0.1 and 6 / 10 < 0.0 + 6 * 0.1 and 7 / 10 < 0.0 + 7 * 0.1
    # (g): the device rule's answer, and what the other order would give
    g = [c for c in F.constructed() if c[0] == "g_equal_scores"][0]
    assert _model_on(g, False)[0] == 1.0 and _model_on(g, False, "ties_higher_row_first")[0] == 0.5


def _seeded_failures(bug, shapes=(C.SHAPES[3], C.SHAPES[7])):
    """Frames of the seeded batches on which the model with a planted bug leaves the bound around frame_map_host."""
    bad = 0
    for shape in shapes:
        (pb, pl, ps, gb, gl, gd), mapped, flags, host, _ = F.reference(shape)
        batch, rows, n_gt = shape[:3]
        for mode in (False, True):
            got, _ = M.batch_scores(pl.reshape(batch, rows), ps.reshape(batch, rows), flags, mapped,
                                    None if gd is None else gd.reshape(batch, n_gt), mode, bug)
            want = host[mode]
            bad += int(((np.isnan(got) != np.isnan(want)) | (np.abs(got - want) > F.bound(rows, n_gt))).sum())
    return bad


def _host_terms(shape, frame):
    """The terms of one seeded frame's area APs as the host classes form them: (rec step) * (envelope) at every step."""
    (pb, pl, ps, gb, gl, gd), _, _, _, _ = F.reference(shape)
    m = VOCMApMetric(iou_thresh=0.5, class_map=shape[5])
    m.update(*[None if a is None else a[frame:frame + 1] for a in (pb, pl, ps, gb, gl, gd)])
    terms = []
    for rec, prec in zip(*m._curves()):
        if rec is None or prec is None:
            continue
        r = np.concatenate([[0.0], rec, [1.0]])
        p = np.concatenate([[0.0], np.nan_to_num(prec), [0.0]])
        p = np.maximum.accumulate(p[::-1])[::-1]
        step = np.flatnonzero(r[1:] != r[:-1])
        terms += [t for t in ((r[step + 1] - r[step]) * p[step + 1]).tolist() if t != 0.0]
    return sorted(terms)


def _term_failures(bug, shape=C.SHAPES[3]):
    """Seeded frames whose area terms, as a sorted list, differ IN BITS from the host's."""
    (pb, pl, ps, gb, gl, gd), mapped, flags, _, _ = F.reference(shape)
    bad = 0
    for i in range(shape[0]):
        terms, _ = M.frame_terms(pl[i], ps[i], flags[i], mapped[i], None if gd is None else gd[i], False, bug)
        bad += sorted(t for t in terms.tolist() if t != 0.0) != _host_terms(shape, i)
    return bad


def test_model_terms_equal_the_host_terms_in_bits():
    assert _term_failures(None) == 0


@pytest.mark.parametrize("bug", M.BUGS)
def test_planted_bugs_are_caught(bug):
    """Each planted bug fails a constructed case, a seeded frame's bound, or (1 / npos, which moves a term by an ulp) the
    bit comparison of a seeded frame's terms."""
    caught = len(_constructed_failures(bug)) + _seeded_failures(bug)
    if bug == "one_over_npos":
        caught += _term_failures(bug)
    assert caught > 0, bug
    if bug in ("ties_higher_row_first", "thresholds_k_over_10", "ignored_as_fp", "padding_ranked", "skip_detectionless",
               "gtless_as_zero", "difficult_in_npos"):
        assert _constructed_failures(bug), bug                 # these have a constructed case of their own


# ------------------------------------------------------------------------------------------------------ the metric class
def _fed():
    """A metric fed on the host with 3 videos: scores known from the constructed cases."""
    cases = {c[0]: c for c in F.constructed()}
    m = FrameMApMetric()
    feed = [(("v1", 0), "c_class_without_ground_truth"), (("v1", 1), "b_class_without_detection"), (("v2", 0), "d_only_difficult"),
            (("v2", 1), "b_class_without_detection"), (("v3", 0), "d_only_difficult"), (("v0", 0), "a_tp_fp_tp"),
            (("v4", 0), "b_class_without_detection"), (("v4", 1), "i_no_rows"), (("v4", 2), "c_class_without_ground_truth")]
    for key, name in feed:
        m.update(*cases[name][1], keys=[key])
    return m, feed


def test_metric_keys_worst_by_video_unscored_reset():
    assert vy.FrameMApMetric is FrameMApMetric and "FrameMApMetric" in vy.__all__
    m, feed = _fed()
    assert m.device_updates == 0
    keys, scores = m.get()
    assert keys == [k for k, _ in feed] and scores.dtype == np.float64 and len(scores) == len(feed)
    a = 0.5 * 1.0 + 0.5 * (2.0 / 3.0)
    want = [1.0, 0.5, math.nan, 0.5, math.nan, a, 0.5, 0.0, 1.0]
    assert all(F.same(float(g), w) for g, w in zip(scores, want)), scores
    assert m.unscored == [("v2", 0), ("v3", 0)]
    worst = m.worst()
    assert [k for k, _ in worst] == [("v4", 1), ("v1", 1), ("v2", 1), ("v4", 0), ("v0", 0), ("v1", 0), ("v4", 2)]
    assert [s for _, s in worst] == [0.0, 0.5, 0.5, 0.5, a, 1.0, 1.0] and m.worst(2) == worst[:2]
    # summary.txt's order: (mean, -frames); v2 has one scored frame (0.5), v4 three (mean 0.5): v4 first
    assert m.by_video()[:4] == [("v4", 0.5, 3), ("v2", 0.5, 1), ("v1", 0.75, 2), ("v0", a, 1)]
    last = m.by_video()[4]
    assert last[0] == "v3" and math.isnan(last[1]) and last[2] == 0 and len(m.by_video()) == 5
    assert [v for v, _, _ in m.by_video(video_of=lambda key: key[0][:1])] == ["v"]
    m.reset()
    assert m.get()[0] == [] and m.get()[1].shape == (0,) and m.worst() == [] and m.by_video() == [] and m.unscored == []
    # default keys: the running index; a wrong number of keys is an error
    case = F.constructed()[0][1]
    two = [np.concatenate([a_, a_]) for a_ in case]
    m.update(*two)
    m.update(*case)
    assert m.get()[0] == [0, 1, 2]
    with pytest.raises(ValueError):
        m.update(*two, keys=["only one"])
    assert m.get()[0] == [0, 1, 2]


def test_frame_metric_lines():
    rows = [(3.0, 0.75, 0.125, 0.25, 0.5, 0.625), (0, 0.5, 0.0, 0.0, 1.0, 1.0)]
    assert frame_metric_lines("vid/000001.JPEG", rows, 0.5) == ["vid/000001.JPEG,3,0.75,0.125,0.25,0.5,0.625,0.5\n",
                                                                "vid/000001.JPEG,0,0.5,0.0,0.0,1.0,1.0,0.5\n"]
    assert frame_metric_lines("p", [], 1.0) == []
    assert frame_metric_lines("p", rows[:1], float("nan"))[0].endswith(",nan\n")


def test_host_fallbacks_and_modes():
    """numpy, float64 and a dict class_map take frame_map_host; use_07_metric and iou_thresh reach it."""
    shape = C.SHAPES[7]
    arrays, _, _, host, _ = F.reference(shape)
    part = [None if a is None else a[:6] for a in arrays]
    as_dict = {i: v for i, v in enumerate(C.DROPPING_MAP)}
    as_dict[-1] = C.DROPPING_MAP[-1]
    for mode in (False, True):
        for cm, args in ((shape[5], part), (as_dict, part), (shape[5], [None if a is None else a.astype(np.float64) for a in part])):
            m = FrameMApMetric(class_map=cm, use_07_metric=mode)
            m.update(*args)
            assert m.device_updates == 0 and np.array_equal(m.get()[1], host[mode][:6])
    strict = FrameMApMetric(iou_thresh=0.75, class_map=shape[5])
    strict.update(*part)
    assert np.array_equal(strict.get()[1], frame_map_host(*part, iou_thresh=0.75, class_map=shape[5]))
    assert (strict.get()[1] != host[False][:6]).any()


def test_voc_metric_is_unchanged_on_its_golden():
    """The acceptance test moved out of VOCMApMetric._update_device: its results on the reference's recorded cases are what
    they were (tests/test_metrics_golden.py holds the same through its own path)."""
    for case in C.golden_cases()[::3]:
        for cls in (VOCMApMetric, VOC07MApMetric):
            m = cls(iou_thresh=case["iou_thresh"], class_names=case["class_names"])
            for u in C.golden_updates(case):
                m.update(*u)
            assert m.device_updates == 0
            name, value = m.get()
            exp = case["expected"][cls.__name__]
            assert name == exp["name"]
            got, want = (value, exp["value"]) if isinstance(value, list) else ([value], [exp["value"]])
            assert all((math.isnan(a) and math.isnan(b)) or abs(a - b) <= 1e-12 for a, b in zip(got, want))
