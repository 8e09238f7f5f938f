"""-m gpu: a batch plan against single frames — every conv cell and the three heads, every frame, every element.

A batch plan is otherwise tied to the single-frame path only through its top detections.  Batch plans use stream-K,
parked chains and 128-wide tiles, which no single-frame plan uses; an element of such a tile that moves no top row was
checked by nothing.  Here a net with keep_activations() runs a batch; every frame is then run alone on a second net with
the same parameters and every cell's activation is compared on the device with the batch's slice (no tolerance: the
pinned summation order makes a frame's bits independent of what it is batched with).  The single-frame heads of one
frame are compared with OracleYolo3.raw_heads bit for bit, which ties the batch to the oracle element by element.  A
failure names the first differing cell in network order, i.e. the launch.

Shapes: the smallest at which the default plans hold the forms the census (test_gpu_train_cell_forms.py) finds at
608x608 / 416x416 batch 64, 416x416 batch 16 and one frame: 416x416 batch 16 (stream-K on three tiles, parked chains as
stream-K pieces), 608x608 batch 8 (plain 128x128, plain parked chains) and 416x416 batch 64 for the one form only
batch 64 chooses (128x128 parked chains as stream-K pieces).  The single-frame side runs the one-frame forms (split-K).

Two forced forms at 2 x 96x96 and 3 x 100x136 (an odd size: batch seams fall inside tiles): stream-K on 13 blocks, and
parked chains on the 128x128 tile.  There every cell is also compared with the oracle's own per-cell taps."""
import time

import numpy as np
import pytest

import conv_forms as F

pytestmark = pytest.mark.gpu

FORCED = {"default": {}, "sk13": {"VY_CONV_SK": "1", "VY_CONV_SK_SLOTS": "13"},
          "parked128x128": {"VY_CONV_KSPLIT": "0", "VY_CONV_FORCE": "128x128"}}
# (form name, batch, height, width, compare every cell with the oracle's taps)
CASES = [("default", 16, 416, 416, False), ("default", 8, 608, 608, False), ("default", 64, 416, 416, False),
         ("sk13", 2, 96, 96, True), ("sk13", 3, 100, 136, True),
         ("parked128x128", 2, 96, 96, True), ("parked128x128", 3, 100, 136, True)]
# what each forced form must have put on the chip, per case: schedule suffixes of the profile's forms
MUST = {"sk13": ("sk", "ck4sk"), "parked128x128": ("ck4",)}
NCLS = 20

_params = {}
_oracle_heads = {}


def params():
    if not _params:
        from videoyolo_amd import init
        from oracle import yolo3_oracle as O
        _params.update(init.synthetic_params(O.param_shapes(NCLS), seed=233))
    return _params


def make_net():
    import videoyolo_amd as vy
    net = vy.yolo3_darknet53(["c%d" % i for i in range(NCLS)], pretrained_base=False)
    net.set_parameters(params())
    net.collect_params().reset_ctx("cuda:0")
    return net


def where(case):
    return "infer %dx%d batch %d %s" % (case[2], case[3], case[1], case[0])


def _setenv(monkeypatch, name):
    for k in F.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in FORCED[name].items():
        monkeypatch.setenv(k, v)


def case_forms(monkeypatch, case):
    """The forms of a case's two plans (batch, one frame), from the profile alone"""
    name, B, H, W, _ = case
    _setenv(monkeypatch, name)
    forms = set()
    for b in (B, 1):
        net = make_net()
        forms |= {f for _, f in F.infer_forms(net, np.zeros((b, 3, H, W), np.float32))}
        del net
    return forms


def _frames(B, H, W):
    """(the generator fills in order: frame 0 of a size is the same whatever the batch, so its oracle run is shared)"""
    return np.random.default_rng(H * 1000 + W).standard_normal((B, 3, H, W)).astype(np.float32)


def _oracle_taps(x):
    """OracleYolo3.raw_heads with every cell's output tapped under the net's cell names -> (heads, taps)"""
    from oracle import yolo3_oracle as O
    orc = O.OracleYolo3(NCLS, params())
    taps = {}
    cell0, block0 = orc.cell, orc.block

    def cell(xx, pre, k, s):
        y = cell0(xx, pre, k, s)
        taps[pre] = y
        return y

    def block(xx, pre):
        y = block0(xx, pre)
        taps[pre + ".body.1"] = y  # the HIP path fuses the residual add into body.1's epilogue
        return y
    orc.cell, orc.block = cell, block
    return orc.raw_heads(x), taps


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-%d-%d" % c[:4])
def test_batch_plan_equals_single_frames_in_every_cell(monkeypatch, case):
    import torch
    name, B, H, W, with_taps = case
    t0 = time.time()
    _setenv(monkeypatch, name)
    x = _frames(B, H, W)
    xd = torch.from_numpy(x).to("cuda:0")
    batch = make_net()
    batch.keep_activations()
    batch(xd)
    cells = [n for n, (_, _, _) in F.conv_info(batch).items() if not n.endswith(".prediction")]
    names = cells + ["head.%d" % i for i in range(3)]
    got = [batch.read_activation(n) for n in cells] + [batch.read_head(i) for i in range(3)]
    assert all(g.shape[0] == B for g in got)
    forms = F.infer_forms(batch, xd)
    single = make_net()
    single.keep_activations()
    differs = torch.zeros((B, len(names)), dtype=torch.bool, device="cuda:0")
    heads0 = None
    for f in range(B):
        single(xd[f:f + 1])
        alone = [single.read_activation(n) for n in cells] + [single.read_head(i) for i in range(3)]
        if f == 0:
            heads0 = [h.cpu().numpy() for h in alone[-3:]]
            # not vacuous: against the batch's NEXT frame every cell differs (distinct random frames)
            crossed = torch.stack([(a[0] != g[1]).any() for a, g in zip(alone, got)]).cpu().numpy()
        for i, (a, g) in enumerate(zip(alone, got)):
            assert a.shape[1:] == g.shape[1:], (names[i], a.shape, g.shape)
            differs[f, i] = (a[0] != g[f]).any()
    forms1 = F.infer_forms(single, xd[:1])
    differs = differs.cpu().numpy()
    by_cell = dict(forms)
    sched = {F.split_form(f[1])[1] for _, f in forms}
    print("\n%s: %d frames x %d cells compared in %.1f s; batch forms %s; one-frame forms %s"
          % (where(case), B, len(names), time.time() - t0, sorted({f[1] for _, f in forms}), sorted({f[1] for _, f in forms1})))
    for want in MUST.get(name, ()):
        assert want in sched, "%s: no launch ran as %s (%s)" % (name, want, sorted(sched))
    assert crossed.all(), "cells equal across different frames: %s" % [n for n, c in zip(names, crossed) if not c]
    if differs.any():
        i = int(np.argmax(differs.any(axis=0)))  # first in network order
        bad_frames = np.nonzero(differs[:, i])[0].tolist()
        pytest.fail("%s: first differing cell %s (launch form %s), frames %s; %d cells differ in all"
                    % (where(case), names[i], by_cell.get(names[i], ("", "prediction conv / stem"))[1], bad_frames,
                       int(differs.any(axis=0).sum())))
    # frame 0 alone against the oracle: heads bit for bit (one oracle run per size, shared); with_taps: one oracle run of
    # the whole batch, every cell of the batch against its taps
    taps = {}
    if with_taps:
        heads, taps = _oracle_taps(x)
        heads = [h[:1] for h in heads]
    else:
        if (H, W) not in _oracle_heads:
            from oracle import yolo3_oracle as O
            _oracle_heads[(H, W)] = O.OracleYolo3(NCLS, params()).raw_heads(x[:1])
        heads = _oracle_heads[(H, W)]
    for i in range(3):
        assert heads0[i].shape == heads[i].shape
        assert np.array_equal(heads0[i], heads[i]), "single-frame head %d differs from the oracle: max |diff| %g" % (
            i, np.abs(heads0[i] - heads[i]).max())
    if with_taps:
        assert sorted(taps) == sorted(cells), sorted(set(taps) ^ set(cells))
        for n, g in zip(cells, got):
            want = taps[n]
            if n.startswith("transitions"):  # stored x2-replicated, cropped to the route it is concatenated with
                want = want.repeat(2, axis=-1).repeat(2, axis=-2)[:, :, :g.shape[2], :g.shape[3]]
            g = g.cpu().numpy()
            assert g.shape == want.shape, (n, g.shape, want.shape)
            assert np.array_equal(g, want), "%s (launch form %s) differs from the oracle's tap: max |diff| %g" % (
                n, by_cell.get(n, ("", "stem"))[1], np.abs(g - want).max())
    print("  wall time %.1f s" % (time.time() - t0))
    F.record(where(case), {f for _, f in forms} | {f for _, f in forms1})
