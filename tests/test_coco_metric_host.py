"""-m "not gpu": the COCO metric on the host — the issue's known answers, seeded sets against the loop-for-loop
transcription of COCOeval (tests/coco_eval_ref.py), the transcription's own sensitivity to six planted faults, and the
argument checks of the C entry vy_coco_match, which need no device."""
import ctypes
import json
import os
import warnings

import numpy as np
import pytest

from videoyolo_amd import _lib
from videoyolo_amd.metrics import COCODetectionMetric, coco_match_host

import coco_eval_ref as REF
import coco_metric_cases as C

KNOWN = C.known_cases()
# (seed, images, rows, ground truths per image, categories, contiguous_id_to_json, data_shape)
SEEDED = [(1, 6, 130, 10, 1, True, None), (2, 8, 60, 12, 20, False, (416, 416)), (3, 8, 100, 30, 80, True, (320, 416))]


def _get(metric):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return metric.get()


# ---------------------------------------------------------------------------------------------------------------------
# 1. known answers
@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers(name):
    case = KNOWN[name]
    ds, results, arrays = C.build_case(case, as_file=name in ("A", "F"))
    ref = REF.evaluate(ds.data, results)
    m = COCODetectionMetric(ds)
    m.update(*arrays)
    names, values = _get(m)
    assert m.device_updates == 0 and m.stats.shape == (12,)
    for i, want in case[4].items():
        print(name, i, m.stats[i], ref['stats'][i], want)
        assert abs(m.stats[i] - want) <= 1e-12
        assert abs(ref['stats'][i] - want) <= 1e-12
    assert np.array_equal(m.precision, ref['precision']) and np.array_equal(m.recall, ref['recall'])
    assert values[0] == ref['summary'].strip()
    if ds.json_path:
        os.remove(ds.json_path)


def test_case_j_precision_of_the_empty_category_is_zero():
    ds, _, arrays = C.build_case(KNOWN['J'])
    m = COCODetectionMetric(ds)
    m.update(*arrays)
    names, values = _get(m)
    assert (m.precision[:, :, 1, 0, :] == 0).all() and (m.recall[:, 1, 0, :] == 0).all()
    assert names == ['~~~~ Summary metrics ~~~~\n', 'c0', 'c1', '~~~~ MeanAP @ IoU=[0.50,0.95] ~~~~\n']
    assert values[1:] == ['50.5', '0.0', '25.2']
    assert values[0].splitlines()[0] == 'Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.252'
    assert values[0].splitlines()[6] == ' Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 0.250'
    assert values[0].splitlines()[1].startswith(' Average Precision  (AP) @[ IoU=0.50      | area=   all')


def test_defaults_are_numpys_values():
    m = COCODetectionMetric(C.build_case(KNOWN['A'])[0])
    assert m._thr[8] == 0.8999999999999999 and m._thr[5] == 0.75 and len(m._rec_thrs) == 101
    assert m._ar.tolist() == [[0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10]] and m._max_dets == [1, 10, 100]


def test_no_results_gives_zero_where_there_is_ground_truth():
    ds, _, arrays = C.build_case(KNOWN['J'])
    m = COCODetectionMetric(ds)
    names, values = _get(m)
    assert m.stats.tolist() == [0, 0, 0, -1, 0, -1, 0, 0, 0, -1, 0, -1]
    assert values[-1] == '0.0'
    m.update(arrays[0], np.full_like(arrays[1], -1), arrays[2])               # rows, all of them padding
    _get(m)
    assert m.stats.tolist() == [0, 0, 0, -1, 0, -1, 0, 0, 0, -1, 0, -1]


def test_file_keys_area_ignore_and_foreign_ids():
    """The file's area decides the range (not w * h), an 'ignore' key has no effect, annotations of unknown images or
    categories and results of unknown categories take no part."""
    ds, results, arrays = C.build_case(KNOWN['A'])
    ds.data['annotations'][0]['area'] = 5000.0                                # medium by the file, small by w * h
    ds.data['annotations'][0]['ignore'] = 1
    ds.data['annotations'].append(C.ann(99, 0, [10, 10, 20, 20], 7))
    ds.data['annotations'].append(C.ann(0, 99, [10, 10, 20, 20], 8))
    m = COCODetectionMetric(ds)
    boxes, labels, scores = arrays
    m.update(np.concatenate([boxes, boxes], 1), np.concatenate([labels, labels + 5], 1), np.concatenate([scores, scores], 1))
    _get(m)
    ref = REF.evaluate(ds.data, results + [dict(results[0], category_id=5)])
    assert np.array_equal(m.precision, ref['precision']) and np.array_equal(m.stats, ref['stats'])
    assert m.stats[3] == -1 and m.stats[4] > -1 and m.stats[0] == C.U


def test_results_file_and_constructor_checks(tmp_path):
    ds, results, arrays = C.build_case(KNOWN['F'])
    m = COCODetectionMetric(ds, save_prefix=str(tmp_path / "res"), use_time=False, cleanup=True)
    m.update(*arrays)
    _get(m)
    path = str(tmp_path / "res.json")
    written = json.load(open(path))
    key = lambda d: (d['image_id'], d['score'])                              # noqa: E731
    assert sorted(written, key=key) == sorted(results, key=key)
    del m
    assert not os.path.exists(path)                                           # cleanup
    none = COCODetectionMetric(ds)
    assert none._filename is None and list(tmp_path.iterdir()) == []
    with pytest.raises(ValueError):
        COCODetectionMetric(ds, data_shape=416)
    with pytest.raises(AssertionError):
        COCODetectionMetric(ds, data_shape=(416, 416, 3))
    with pytest.raises(ValueError):
        COCODetectionMetric(ds, iou_thrs=np.linspace(0, 1, 17))
    with pytest.raises(ValueError):
        COCODetectionMetric(ds, area_ranges=[[0, 1]] * 9)


def test_sid_names_the_images():
    ds, results, arrays = C.build_case(KNOWN['F'])
    a, b = COCODetectionMetric(ds), COCODetectionMetric(ds)
    a.update(*arrays)
    b.update(*[x[1:] for x in arrays], sid=[1])
    b.update(*[x[:1] for x in arrays], sid=0)
    assert _get(a) == _get(b) and np.array_equal(a.precision, b.precision)
    with pytest.raises(ValueError, match="given before"):
        b.update(*[x[:1] for x in arrays], sid=0)
    with pytest.raises(ValueError, match="not an image"):
        b.update(*[x[:1] for x in arrays], sid=17)
    with pytest.raises(ValueError):
        a.update(*[x[:1] for x in arrays])                                    # the counter is past the last image
    a.reset()
    a.update(*arrays)
    assert _get(a) == _get(b)


def test_coco_match_host_outputs_are_in_row_order():
    """Case D's rows shuffled, a padding row between them: rank and flags follow the rows."""
    thr, ar = np.linspace(.5, .95, 10), np.array([[0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10]])
    det = np.array([[400, 400, 40, 40], [0, 0, 0, 0], [200, 200, 40, 40], [10, 10, 20, 20], [30, 30, 20, 20.]])
    cat, score = np.array([0, -1, 0, 0, 0]), np.array([.6, .99, .7, .9, .8])
    gt = np.array([[0, 0, 100, 100], [200, 200, 40, 40.]])
    rank, flags = coco_match_host(det, cat, score, gt, [0, 0], [10000, 1600], [1, 0], [1, 2], thr, ar, 100)
    assert rank.tolist() == [3, -1, 2, 0, 1] and rank.dtype == np.int32 and flags.shape == (5, 4, 10) and flags.dtype == np.uint8
    assert (flags[3] == 3).all() and (flags[4] == 3).all()                    # in the crowd: matched and ignored, both
    assert (flags[2, 0] == 1).all() and (flags[2, 2] == 1).all() and (flags[2, 1] == 3).all()
    assert (flags[0, 0] == 0).all() and (flags[0, 1] == 2).all() and (flags[1] == 0).all()
    rank, flags = coco_match_host(det, cat, score, gt, [0, 0], [10000, 1600], [1, 0], [1, 2], thr, ar, 2)
    assert rank.tolist() == [-1, -1, -1, 0, 1] and not flags[[0, 1, 2]].any()


# ---------------------------------------------------------------------------------------------------------------------
# 2. seeded sets
@pytest.mark.parametrize("spec", SEEDED, ids=lambda s: "K%d" % s[4])
def test_seeded_sets_equal_the_transcription(spec):
    seed, n_images, rows, n_gt, n_cats, use_map, data_shape = spec
    ds, arrays = C.seeded_set(seed, n_images, rows, n_gt, n_cats, use_map, data_shape, as_file=n_cats == 20)
    cond = C.conditions(ds, arrays, data_shape)
    must = [k for k in cond if k != 'over_100'] + (['over_100'] if rows > 120 else [])
    assert all(cond[k] for k in must), cond
    assert use_map == hasattr(ds, 'contiguous_id_to_json')
    ref = REF.evaluate(ds.data, C.results_of(ds, arrays, data_shape=data_shape))
    m = COCODetectionMetric(ds, data_shape=data_shape)
    m.update(*arrays)
    names, values = _get(m)
    assert np.array_equal(m.precision, ref['precision'])
    assert np.array_equal(m.recall, ref['recall'])
    assert np.array_equal(m.stats, ref['stats']) and values[0] == ref['summary'].strip()
    assert m.precision.shape == (10, 101, n_cats, 4, 3) and m.recall.shape == (10, n_cats, 4, 3)
    ap_all = m.precision[:, :, :, 0, 2]
    assert values[-1] == '{:.1f}'.format(100 * np.mean(ap_all[ap_all > -1])) and len(values) == n_cats + 2
    # image by image in any order, torch CPU tensors and float64: the same
    import torch
    again = COCODetectionMetric(ds, data_shape=data_shape)
    for i in reversed(range(n_images)):
        part = [a[i:i + 1] for a in arrays]
        again.update(*([torch.from_numpy(a) for a in part] if i % 2 else [a.astype(np.float64) for a in part]), sid=[i])
    assert _get(again) == (names, values) and np.array_equal(again.precision, m.precision)
    if ds.json_path:
        os.remove(ds.json_path)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the transcription notices a planted fault
FAULTS = {
    'crowd_union': ("u = da if crowd else da + ga - i", "u = da + ga - i"),
    'break_rule': ("                        break\n", "                        pass\n"),
    'dtm_is_m': ("dtm[tind][dind] = gt[m]['id']", "dtm[tind][dind] = 1"),
    'exclusive_end': ("return area < rng[0] or area > rng[1]", "return area < rng[0] or area >= rng[1]"),
    'unstable_tie': ("return [int(i) for i in np.argsort(-np.asarray(scores, np.float64), kind='mergesort')]",
                     "return [len(scores) - 1 - int(i) for i in np.argsort(-np.asarray(scores, np.float64)[::-1], kind='mergesort')]"),
    'side_right': ("side='left'", "side='right'"),
}
# which known case shows each fault (the break rule needs an ignored ground truth that overlaps a matched one: case K)
SHOWN_BY = {'crowd_union': 'D', 'break_rule': 'K', 'dtm_is_m': 'E', 'exclusive_end': 'G', 'unstable_tie': 'H_miss_first',
            'side_right': 'A'}
CASE_K = (1, 1, [(0, 0, C.B40, 1, 0), (0, 0, C.B40, 2, 1)], [(0, 0, C.B40, .9)], {0: C.U, 6: 1})


def _faulted(name):
    src = open(REF.__file__).read()
    old, new = FAULTS[name]
    assert src.count(old) == 1, name
    mod = {}
    exec(compile(src.replace(old, new), "coco_eval_ref_" + name, "exec"), mod)
    return mod['evaluate']


@pytest.mark.parametrize("name", sorted(FAULTS))
def test_transcription_sensitivity(name):
    evaluate = _faulted(name)
    cases = dict(KNOWN, K=CASE_K)
    changed = []
    for cname, case in sorted(cases.items()):
        ds, results, _ = C.build_case(case)
        clean, bad = REF.evaluate(ds.data, results), evaluate(ds.data, results)
        for i, want in case[4].items():
            assert abs(clean['stats'][i] - want) <= 1e-12
        if not (np.array_equal(clean['precision'], bad['precision']) and np.array_equal(clean['recall'], bad['recall'])):
            changed.append(cname)
    print(name, changed)
    assert SHOWN_BY[name] in changed
    # and on a seeded set
    seed, n_images, rows, n_gt, n_cats, use_map, data_shape = SEEDED[0]
    ds, arrays = C.seeded_set(seed, n_images, rows, n_gt, n_cats, use_map, data_shape)
    results = C.results_of(ds, arrays)
    clean, bad = REF.evaluate(ds.data, results), evaluate(ds.data, results)
    assert not (np.array_equal(clean['precision'], bad['precision']) and np.array_equal(clean['recall'], bad['recall']))


# ---------------------------------------------------------------------------------------------------------------------
# 4. the C entry's argument checks: nothing is launched, no device is needed
def _call(lib, **over):
    a = dict(batch=2, rows=100, det_xywh=16, det_cat=16, det_score=16, gt_image=np.array([0, 1], np.int32), n_images=2,
             gt_off=np.array([0, 3, 5], np.int64), gt_xywh=16, gt_cat=16, gt_area=16, gt_crowd=16, gt_id=16, n_thr=10,
             iou_thrs=np.linspace(.5, .95, 10), n_area=4, area_ranges=np.array(REF.AREA_RANGES, np.float64), max_det=100,
             taken=16, taken_bytes=200, rank=16, flags=16)
    a.update(over)
    p = lambda v: None if v is None else ctypes.c_void_p(v) if isinstance(v, int) else v.ctypes.data_as(ctypes.c_void_p)    # noqa: E731
    return lib.vy_coco_match(a["batch"], a["rows"], p(a["det_xywh"]), p(a["det_cat"]), p(a["det_score"]), p(a["gt_image"]),
                             a["n_images"], p(a["gt_off"]), p(a["gt_xywh"]), p(a["gt_cat"]), p(a["gt_area"]), p(a["gt_crowd"]),
                             p(a["gt_id"]), a["n_thr"], p(a["iou_thrs"]), a["n_area"], p(a["area_ranges"]), a["max_det"],
                             p(a["taken"]), a["taken_bytes"], p(a["rank"]), p(a["flags"]), None)


def test_c_entry_argument_errors_need_no_device():
    lib = _lib.load()
    assert _lib.VY_COCO_ROWS_MAX == 1024 and _lib.VY_COCO_MAX_THRS == 16 and _lib.VY_COCO_MAX_RANGES == 8
    bad = [{name: None} for name in ("det_xywh", "det_cat", "det_score", "gt_image", "gt_off", "gt_xywh", "gt_cat", "gt_area",
                                     "gt_crowd", "gt_id", "iou_thrs", "area_ranges", "rank", "flags", "taken")]
    bad += [dict(batch=-1), dict(rows=-1), dict(n_images=-1), dict(max_det=-1), dict(taken_bytes=-1)]
    bad += [dict(rows=_lib.VY_COCO_ROWS_MAX + 1), dict(n_thr=0), dict(n_thr=17, iou_thrs=np.linspace(0, 1, 17)), dict(n_area=0),
            dict(n_area=9, area_ranges=np.zeros((9, 2)))]
    for v in (float("nan"), float("inf"), float("-inf")):
        thr = np.linspace(.5, .95, 10)
        thr[3] = v
        bad.append(dict(iou_thrs=thr))
    bad += [dict(area_ranges=np.array([[0, 1], [2, 1], [0, 1], [0, 1.]])), dict(gt_image=np.array([0, 2], np.int32)),
            dict(gt_image=np.array([-1, 0], np.int32)), dict(gt_off=np.array([0, 3, 2], np.int64)), dict(taken_bytes=199)]
    for over in bad:
        assert _call(lib, **over) == -1, over
        assert "vy_coco_match" in lib.vy_last_error().decode(), over
    assert _call(lib, rows=1025, batch=0) == -1 and "VY_COCO_ROWS_MAX" in lib.vy_last_error().decode()
    # the empty calls: VY_OK, nothing launched (the pointers here are not device memory)
    assert _call(lib, batch=0) == 0 and _call(lib, rows=0) == 0
    assert _call(lib, batch=0, rows=_lib.VY_COCO_ROWS_MAX, taken=None, taken_bytes=0) == 0
