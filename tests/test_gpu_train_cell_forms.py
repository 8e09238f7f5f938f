"""-m gpu: the float64 cell walker of test_gpu_train_cells.py under every launch form of the exact conv kernel, and the
census that ties the forms the default plans choose to the forms the walker has met.

test_gpu_train_cells.py walks the default plan of its shapes, so which tile and which schedule its bars meet is whatever
the cost model picks there.  Here a net is built under each forced form of conv_forms.FORCED — every tile with plain
launches, stream-K on few blocks (data gradients and the training forward with its per-tile statistics included), the
parked-chain forward, stream-K pieces of parked chains, weight gradients on the main stream — and the same walker runs,
with the same bounds.  Each test also reads the step's launch labels (VY_TRAIN_LABELS: the launcher's own account of
tile, LDS stages and schedule per launch) and asserts that the form it names served the launches it is meant to cover.

Shapes are the small ones of test_gpu_train_cells.py; every form runs on two single-frame shapes (the 128-row tiles on
the 32-wide one), except stream-K on 24 blocks of 128x64, which only (4, 2, 128, 224) and the window net on 3 clips of
two 96x32 frames can meet: no launch of the other small shapes has more than 24 such tiles.  Two forms have no small
shape at all — the two-stage 64x64 tile with parked chains needs more than 512 tiles on a 3x3 cell over 512 channels,
i.e. more than 2048 pixels at stride 32 — and the default plans of 416x416 batch 16 and 608x608 batch 8 choose them
(with and without stream-K): the heads net meets both in about ten seconds each, the backbone being absent — the stream-K
pieces under the default plan of 416x416 batch 16 (the chip-wide schedule a real step runs), the plain form forced at
batch 13, the smallest batch of 416x416 frames with more than 2048 such pixels.

The census (last tests of the file) asserts that every form a default training plan chooses at 416x416 batch 16,
608x608 batch 8 and 320x320 batch 16 is among the walked ones, and that every form a default inference plan chooses at
five shapes is met by test_gpu_infer_cell_forms.py; it prints the table form -> where it is checked."""
import itertools
import os
import time

import numpy as np
import pytest

import conv_forms as F
import test_gpu_train_cells as TC

pytestmark = pytest.mark.gpu

A, B, C = (1, 1, 64, 64), (3, 3, 96, 32), (4, 2, 128, 224)
NET_CASES = [("plain128x128", A), ("plain128x128", B), ("plain128x64", B), ("plain128x64", C), ("plain128x32", B),
             ("plain128x32", C), ("plain64x64", A), ("plain64x64", C), ("sk5_128x128", B), ("sk5_128x128", C),
             ("sk13_64x64", A), ("sk13_64x64", B), ("sk24_128x64", C), ("sk13", A), ("sk13", C), ("parked", A),
             ("parked", B), ("parked_sk13", B), ("parked_sk13", C), ("main_stream_wgrad", A), ("main_stream_wgrad", C)]
WMAX, WMEAN = ("max", 3, 1, 64, 64), ("mean", 2, 3, 96, 32)
WINDOW_CASES = [("sk5_128x128", WMAX), ("sk13", WMAX), ("plain128x32", WMAX), ("sk24_128x64", WMEAN),
                ("sk13_64x64", WMEAN), ("plain128x128", WMEAN)]
# the last two: the two-stage 64x64 tile with parked chains, as stream-K pieces (the default plan's choice) and plain
HEADS_CASES = [("sk13_64x64", (3, 3, 96, 32), None), ("plain128x64", (3, 3, 96, 32), None),
               ("default", (20, 16, 416, 416), "64x64ck4sk"), ("plain64x64", (3, 13, 416, 416), "64x64ck4")]
DEFAULT_SMALL = [A, B, C]  # walked under the default plan by test_gpu_train_cells.py
BUILDERS = {"net": TC._step, "window": TC._step_window, "heads": TC._step_heads}
_serial = itertools.count()


def _ids(v):
    return v if isinstance(v, str) else "-".join(str(x) for x in v) if isinstance(v, tuple) else None


def _where(kind, envname, shape):
    return "%s %s %s" % (kind, "x".join(str(x) for x in shape), envname)


def _forced_step(monkeypatch, tmp_path, kind, envname, shape):
    """One recorded step of a net created under FORCED[envname] -> (the builder's dict, conv launches, weight gradients)"""
    for k in F.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in F.FORCED.get(envname, {}).items():
        monkeypatch.setenv(k, v)
    labels = str(tmp_path / ("labels_%d.txt" % next(_serial)))  # a fresh path: the library fills each path once
    monkeypatch.setenv("VY_TRAIN_LABELS", labels)
    st = BUILDERS[kind](*shape)
    convs, wgrads = F.read_labels(labels, st["cells"])
    os.remove(labels)
    return st, convs, wgrads


def _walk_form(monkeypatch, tmp_path, kind, envname, shape, must_have=None):
    t0 = time.time()
    st, convs, wgrads = _forced_step(monkeypatch, tmp_path, kind, envname, shape)
    F.check_served(envname, convs, wgrads)
    forms = F.forms_of(convs)
    if must_have:
        assert ("fwd", must_have) in forms, sorted(forms)
    res, pools = TC._walk(st)
    print("\nforms served: %s" % " ".join("%s:%s" % f for f in sorted(forms)))
    print("weight gradients: %s" % sorted({w[1:2] + w[3:] for w in wgrads}))
    TC._report("%s %s" % (_where(kind, envname, shape), F.FORCED.get(envname, {})), res, t0, pools)
    F.record(_where(kind, envname, shape), forms | {("wgrad", "%s+%s" % (w[1].replace("wgrad_kernel", ""), w[3])) for w in wgrads})
    return res, pools


@pytest.mark.parametrize("envname,shape", NET_CASES, ids=_ids)
def test_every_training_cell_under_a_forced_form(monkeypatch, tmp_path, envname, shape):
    _walk_form(monkeypatch, tmp_path, "net", envname, shape)


@pytest.mark.parametrize("envname,shape", WINDOW_CASES, ids=_ids)
def test_every_window_cell_under_a_forced_form(monkeypatch, tmp_path, envname, shape):
    _, pools = _walk_form(monkeypatch, tmp_path, "window", envname, shape)
    assert sorted(pools) == ["pool.0", "pool.1", "pool.2"], sorted(pools)
    if shape[0] == "max":
        for name, (wins, ties, _) in pools.items():
            assert len(wins) == shape[1] and min(wins) > 0, (name, wins, ties)


@pytest.mark.parametrize("envname,shape,must_have", HEADS_CASES, ids=_ids)
def test_every_heads_cell_under_a_forced_form(monkeypatch, tmp_path, envname, shape, must_have):
    res, _ = _walk_form(monkeypatch, tmp_path, "heads", envname, shape, must_have)
    assert len([r for r in res if r.kind == "route view"]) == 3 and len([r for r in res if r.kind == "caller's route"]) == 3


# ---------------------------------------------------------------- the census
# A form may stand here only if no default plan of the census shapes chooses it and no switch can force it; each entry
# gives the reason.  (Empty: every form the plans choose is walked.)
EXEMPT = {}

TRAIN_PLANS = [(20, 16, 416, 416), (20, 8, 608, 608), (20, 16, 320, 320)]
INFER_PLANS = [(64, 608), (64, 416), (16, 416), (1, 416), (1, 608)]


def _labels_only(monkeypatch, tmp_path, kind, envname, shape):
    import torch
    st, convs, wgrads = _forced_step(monkeypatch, tmp_path, kind, envname, shape)
    torch.cuda.synchronize()
    del st
    torch.cuda.empty_cache()
    return F.forms_of(convs) | {("wgrad", "%s+%s" % (w[1].replace("wgrad_kernel", ""), w[3])) for w in wgrads}


def _table(title, forms, walked):
    print("\n%s" % title)
    for f in sorted(forms):
        where = sorted(walked.get(f, ()))
        print("  %-8s %-16s %s" % (f[0], f[1], "; ".join(where[:4]) + (" (+%d more)" % (len(where) - 4) if len(where) > 4 else "")
                                   if where else ("EXEMPT: " + EXEMPT[f] if f in EXEMPT else "NOT CHECKED")))


def test_census_every_form_a_training_plan_chooses_is_walked(monkeypatch, tmp_path):
    walked = {f: set(w) for f, w in F.WALKED.items()}
    for kind, cases in (("net", NET_CASES), ("window", WINDOW_CASES), ("heads", [c[:2] for c in HEADS_CASES])):
        for envname, shape in cases:  # a case that has not run in this process: its forms from a step without the walk
            where = _where(kind, envname, shape)
            if not any(where in w for w in walked.values()):
                for f in _labels_only(monkeypatch, tmp_path, kind, envname, shape):
                    walked.setdefault(f, set()).add(where + " (labels only in this run)")
    for shape in DEFAULT_SMALL:
        for f in _labels_only(monkeypatch, tmp_path, "net", "default", shape):
            walked.setdefault(f, set()).add("test_gpu_train_cells %s default" % "x".join(str(x) for x in shape))
    chosen = {}
    for shape in TRAIN_PLANS:
        for f in _labels_only(monkeypatch, tmp_path, "net", "default", shape):
            chosen.setdefault(f, set()).add("%dx%d batch %d" % (shape[2], shape[3], shape[1]))
    _table("forms the default training plans choose -> where the float64 walker meets them", chosen, walked)
    for f, shapes in sorted(chosen.items()):
        print("  %-8s %-16s chosen at %s" % (f[0], f[1], ", ".join(sorted(shapes))))
    assert not set(EXEMPT) & set(chosen), "a form a plan chooses is never exempt: %s" % sorted(set(EXEMPT) & set(chosen))
    # ("wgrad" rows — kernel instance + slab reduce — are printed for the record: the reduce follows the split count, which
    # grows with the pixels, so wide<32> and <32,128> with wide<8> are met by test_gpu_train_cells.py's large shapes only)
    missing = sorted(f for f in set(chosen) - set(walked) if f[0] != "wgrad")
    assert not missing, "chosen by a default training plan, walked by no per-cell test: %s" % missing


def test_census_every_form_an_inference_plan_chooses_is_compared(monkeypatch):
    import test_gpu_infer_cell_forms as I
    for k in F.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    met = {f: set(w) for f, w in F.WALKED.items() if f[0] == "infer"}
    for case in I.CASES:
        where = I.where(case)
        if not any(where in w for w in met.values()):  # not run in this process: the forms of the same plans, profile only
            for f in I.case_forms(monkeypatch, case):
                met.setdefault(f, set()).add(where + " (profile only in this run)")
    for k in F.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    chosen = {}
    for batch, size in INFER_PLANS:
        net = I.make_net()
        for _, f in F.infer_forms(net, np.zeros((batch, 3, size, size), np.float32)):
            chosen.setdefault(f, set()).add("%dx%d batch %d" % (size, size, batch))
        del net
    _table("forms the default inference plans choose -> where every element is compared", chosen, met)
    for f, shapes in sorted(chosen.items()):
        print("  %-8s %-16s chosen at %s" % (f[0], f[1], ", ".join(sorted(shapes))))
    assert not set(EXEMPT) & set(chosen), "a form a plan chooses is never exempt: %s" % sorted(set(EXEMPT) & set(chosen))
    missing = sorted(set(chosen) - set(met))
    assert not missing, "chosen by a default inference plan, compared by no per-cell test: %s" % missing
