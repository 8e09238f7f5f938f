"""The COCO metric against THE REAL pycocotools COCOeval: tests/golden/coco_metric_golden.json, written by
tests/golden/make_coco_metric_golden.py on a machine that has pycocotools (tests/golden/COCO_RUNBOOK.md).  The file DOES
NOT EXIST YET, so every test here skips and the rule stays [UPSTREAM-RECALLED]; the day it is captured these light up:
`-m "not gpu"` holds the transcription (tests/coco_eval_ref.py) and the metric's host path to COCOeval's own precision,
recall and stats, `-m gpu` the device path."""
import importlib.util
import json
import os
import warnings

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "coco_metric_golden.json")
_spec = importlib.util.spec_from_file_location("make_coco_metric_golden", os.path.join(HERE, "golden", "make_coco_metric_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
NAMES = sorted(G.cases())


def _case(name):
    if not os.path.exists(PATH):
        pytest.skip("tests/golden/coco_metric_golden.json has not been captured (needs pycocotools)")
    with open(PATH) as f:
        c = json.load(f)['cases'][name]
    return c, G.unpack(c['precision']), G.unpack(c['recall'])


def _feed(case, device=None):
    """The case's results as update() arrays: labels are the file's category ids, corners give the boxes back."""
    import coco_metric_cases as C
    from videoyolo_amd.metrics import COCODetectionMetric
    data, results = case['dataset'], case['results']
    images = sorted(im['id'] for im in data['images'])
    ds = C.Dataset(images, data['annotations'], [c['id'] for c in data['categories']])
    rows = max([sum(1 for r in results if r['image_id'] == i) for i in images] + [1])
    boxes, labels, scores = np.full((len(images), rows, 4), -1.0), np.full((len(images), rows), -1.0), np.full((len(images), rows), -1.0)
    for b, i in enumerate(images):
        for r, d in enumerate([d for d in results if d['image_id'] == i]):
            boxes[b, r], labels[b, r], scores[b, r] = C.corners(d['bbox']), d['category_id'], d['score']
    m = COCODetectionMetric(ds, score_thresh=-1e30)
    arrays = [boxes, labels, scores]
    if device is not None:
        import torch
        arrays = [torch.from_numpy(a.astype(np.float32)).to(device) for a in arrays]
    m.update(*arrays)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.get()
    return m


@pytest.mark.parametrize("name", NAMES)
def test_transcription_and_host_path_equal_cocoeval(name):
    import coco_eval_ref as REF
    case, precision, recall = _case(name)
    ref = REF.evaluate(case['dataset'], case['results'])
    assert np.array_equal(ref['precision'], precision) and np.array_equal(ref['recall'], recall)
    assert np.allclose(ref['stats'], case['stats'], rtol=0, atol=1e-12) and ref['summary'].strip() == case['summary']
    m = _feed(case)
    assert np.array_equal(m.precision, precision) and np.array_equal(m.recall, recall)
    assert np.allclose(m.stats, case['stats'], rtol=0, atol=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_device_path_equals_cocoeval(name):
    case, precision, recall = _case(name)
    m = _feed(case, "cuda:0")
    assert m.device_updates == 1
    assert np.array_equal(m.precision, precision) and np.array_equal(m.recall, recall)
