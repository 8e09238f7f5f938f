"""Generates tests/golden/coco_metric_golden.json by running THE REAL pycocotools COCOeval (iouType 'bbox') on the known
cases and small seeded sets of tests/coco_metric_cases.py.  Needs `import pycocotools`, which the build container does not
have: until somebody runs this on a machine that has it, the file is absent, tests/test_coco_metric_golden.py skips, and
the COCO metric's rule stays [UPSTREAM-RECALLED] (tests/golden/COCO_RUNBOOK.md).

Per case the file holds the inputs (the ground-truth dict and the results list) and COCOeval's own stats, precision and
recall (float64 bytes, zlib, base64).

    python tests/golden/make_coco_metric_golden.py
"""
import base64
import contextlib
import io
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def pack(a):
    a = np.ascontiguousarray(a, np.float64)
    return {'shape': list(a.shape), 'data': base64.b64encode(zlib.compress(a.tobytes(), 9)).decode()}


def unpack(d):
    return np.frombuffer(zlib.decompress(base64.b64decode(d['data'])), np.float64).reshape(d['shape'])


def cases():
    """name -> (ground-truth dict, results list)"""
    import coco_metric_cases as C
    out = {}
    for name, case in sorted(C.known_cases().items()):
        ds, results, _ = C.build_case(case)
        out['known_' + name] = (ds.data, results)
    for seed, n_images, rows, n_gt, n_cats, use_map, data_shape in [(1, 6, 130, 10, 1, True, None),
                                                                    (4, 6, 60, 12, 5, False, (416, 416))]:
        ds, arrays = C.seeded_set(seed, n_images, rows, n_gt, n_cats, use_map, data_shape)
        out['seeded_K%d' % n_cats] = (ds.data, C.results_of(ds, arrays, data_shape=data_shape))
    return out


def main():
    import pycocotools
    from pycocotools.coco import COCO
    from pycocotools.cocoeval import COCOeval
    golden = {'pycocotools': getattr(pycocotools, '__version__', 'unknown'), 'numpy': np.__version__, 'cases': {}}
    for name, (data, results) in cases().items():
        with contextlib.redirect_stdout(io.StringIO()):
            gt = COCO()
            gt.dataset = json.loads(json.dumps(data))
            gt.createIndex()
            if not results:
                raise ValueError("COCOeval needs at least one result: %s" % name)
            ev = COCOeval(gt, gt.loadRes(json.loads(json.dumps(results))), 'bbox')
            ev.evaluate()
            ev.accumulate()
            summary = io.StringIO()
            with contextlib.redirect_stdout(summary):
                ev.summarize()
        golden['cases'][name] = {'dataset': data, 'results': results, 'stats': [float(v) for v in ev.stats],
                                 'summary': summary.getvalue().strip(), 'precision': pack(ev.eval['precision']),
                                 'recall': pack(ev.eval['recall'])}
    path = os.path.join(HERE, 'coco_metric_golden.json')
    with open(path, 'w') as f:
        json.dump(golden, f)
    print("%s: %d cases, %d bytes, pycocotools %s" % (path, len(golden['cases']), os.path.getsize(path), golden['pycocotools']))


if __name__ == "__main__":
    main()
