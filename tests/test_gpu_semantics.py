"""-m gpu: the per-net semantics setting (net.set_semantics / vy_net_set_semantics) on the device.

NMS flags: the HIP detection tail (`net.detect_heads`) against the switchable plain-Python box_nms of
tests/test_mxnet_kit_sensitivity.py on the CPU decode of the same head tensors, for the default setting, every single flip
and three combined settings, on every constructed case and launch path of tests/semantics_cases.py (whose census,
tests/test_semantics_host.py, shows on the CPU that each case discriminates the switches it names).  Bars: ids, scores and
boxes bit-equal, keep_idx the reference's row numbers, -1 past the reference's last kept row.  With the default setting the
outputs also equal the C reference's box_nms.  One flipped setting goes through a full forward, eagerly and as a captured
graph.  Running variance: one recorded step with `running_var_unbiased=True` against the CPU training reference with
RUNNING_VAR_UNBIASED = True, at the bars of tests/test_gpu_train_parity.py."""
import numpy as np
import pytest

import semantics_cases as SC
from conftest import frames
from test_mxnet_kit_sensitivity import py_box_nms

pytestmark = pytest.mark.gpu

CASES = SC.all_cases()
_NETS = {}


def _tail_net(classes):
    """A heads-only net per class count, made once: `detect_heads` runs the tail alone, on any kind of net."""
    if classes not in _NETS:
        import videoyolo_amd as vy
        net = vy.yolo3_no_backbone(["c%d" % i for i in range(classes)])
        net.initialize(init="synthetic", seed=233)
        net.collect_params().reset_ctx("cuda:0")
        _NETS[classes] = net
    return _NETS[classes]


def _run(case, setting):
    net = _tail_net(case["classes"])
    net.set_nms(case["nms_thresh"], case["nms_topk"], case["post_nms"])
    net.set_semantics(**dict(SC.DEFAULTS, **setting))
    try:
        outs = net.detect_heads(case["heads"], case["size"], return_index=True)
    finally:
        net.set_semantics(**SC.DEFAULTS)
    ids, scores, boxes, keep = [t.cpu().numpy() for t in outs]
    return np.concatenate([ids, scores, boxes], -1), keep.reshape(keep.shape[0], -1)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(case, got, keep, want):
    assert got.shape == want[..., :6].shape and keep.shape == want.shape[:2], (got.shape, keep.shape, want.shape)
    n_ref = (want[..., 0] >= 0).sum(1)
    print("%s: kept rows per image min %d max %d of %d" % (case["name"], n_ref.min(), n_ref.max(), want.shape[1]))
    assert np.array_equal(_bits(got), _bits(want[..., :6])), (case["name"], np.argwhere(_bits(got) != _bits(want[..., :6]))[:5])
    assert np.array_equal(keep, want[..., 6].astype(np.int64)), (case["name"], np.argwhere(keep != want[..., 6])[:5])
    for b in (0, got.shape[0] - 1):
        assert (got[b, n_ref[b]:] == -1).all() and (keep[b, n_ref[b]:] == -1).all()


PAIRS = [(c, n, s) for c in CASES for n, s in SC.settings_for(c)]


@pytest.mark.parametrize("case,setting", [(c, s) for c, _, s in PAIRS], ids=["%s-%s" % (c["name"], n) for c, n, _ in PAIRS])
def test_tail_follows_the_setting(case, setting):
    got, keep = _run(case, setting)
    _check(case, got, keep, SC.reference(case, py_box_nms, setting))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_default_setting_is_the_c_reference(case):
    """What the existing suite pins, restated on the new inputs: with all switches at their defaults the tail equals the C
    reference's box_nms on its own decode."""
    from oracle import yolo3_oracle as O
    got, keep = _run(case, {})
    rows, where = SC.decoded_rows(case)
    out, idx = O.box_nms(np.ascontiguousarray(rows[..., :6]), case["nms_thresh"], float(SC.VALID), case["nms_topk"], False)
    r = SC.out_rows(case)
    want = np.full((out.shape[0], r, 6), -1.0, np.float32)
    n = min(r, out.shape[1])
    want[:, :n] = out[:, :n]
    want = want[where]
    assert np.array_equal(_bits(got), _bits(want)), case["name"]
    kept = want[..., 0] >= 0
    assert np.array_equal(keep >= 0, kept)
    ref6 = SC.reference(case, py_box_nms, {})
    assert np.array_equal(keep, ref6[..., 6].astype(np.int64))


# ---------------------------------------------------------------------------------------------- a full forward, a graph
def _full_net(classes=3):
    import videoyolo_amd as vy
    net = vy.yolo3_darknet53(["c%d" % i for i in range(classes)], pretrained_base=False)
    net.initialize(init="synthetic", seed=233)
    net.collect_params().reset_ctx("cuda:0")
    return net


def _forward_reference(net, setting, topk, post):
    """`py_box_nms` under `setting` on the CPU decode of the prediction planes the forward just left."""
    from oracle import yolo3_oracle as O
    heads = [net.read_head(i).cpu().numpy() for i in range(3)]
    rows = O.OracleYolo3(3, {}).detections_from_heads(heads).astype(np.float32)
    idx = np.broadcast_to(np.arange(rows.shape[1], dtype=np.float32)[None, :, None], rows.shape[:2] + (1,))
    rows = np.concatenate([rows, idx], -1)
    return py_box_nms(rows, net.nms_thresh, float(SC.VALID), topk, False, **dict(SC.DEFAULTS, **setting))[:, :post]


def _forward(net, x):
    ids, scores, boxes, keep = [t.cpu().numpy() for t in net(x, return_index=True)]
    return np.concatenate([ids, scores, boxes], -1), keep.reshape(keep.shape[0], -1)


@pytest.mark.parametrize("hybrid", [False, True], ids=["eager", "graph"])
def test_setting_reaches_a_full_forward(hybrid):
    """net(x) on a YOLOV3 at 64 x 64: default first, then flipped on the same net — as a captured graph the second call must
    not replay the first call's kernel arguments."""
    net = _full_net()
    topk, post = 20, 20      # some of the 20 best suppress each other at 0.3 on this input (17 - 19 rows kept)
    net.set_nms(0.3, topk, post)
    if hybrid:
        net.hybridize()
    x = frames(2, 64, seed=7)
    got0, keep0 = _forward(net, x)
    want0 = _forward_reference(net, {}, topk, post)
    assert np.array_equal(_bits(got0), _bits(want0[..., :6])) and np.array_equal(keep0, want0[..., 6].astype(np.int64))
    # a flip that shows on this input: the cut after suppression refills the 20 rows, descending ties or +1 move survivors
    flip = None
    for cand in (dict(topk_first=False), dict(plus_one=True, strict_iou=False), dict(tie_ascending=False)):
        if not np.array_equal(_forward_reference(net, cand, topk, post), want0):
            flip = cand
            break
    assert flip is not None, "no switch changes this input's detections: the test shows nothing"
    net.set_semantics(**flip)
    got1, keep1 = _forward(net, x)
    want1 = _forward_reference(net, flip, topk, post)
    assert not np.array_equal(want1, want0)
    assert np.array_equal(_bits(got1), _bits(want1[..., :6])), flip
    assert np.array_equal(keep1, want1[..., 6].astype(np.int64)), flip
    net.set_semantics(**SC.DEFAULTS)
    got2, keep2 = _forward(net, x)
    assert np.array_equal(_bits(got2), _bits(got0)) and np.array_equal(keep2, keep0)


# ---------------------------------------------------------------------------------------------------- running variance
def _train_setup(C, B, S):
    from videoyolo_amd import init
    from oracle import targets_oracle as T
    from oracle import yolo3_oracle as O
    params = init.synthetic_params(O.param_shapes(C), seed=11)
    x = frames(B, S, seed=5)
    gt_boxes, gt_ids = T.synthetic_gt(B, S, C, m=3, seed=2, pad_to=5)
    return params, x, gt_boxes, T.prefetch_targets(C, S, S, gt_boxes, gt_ids)


def _step(net, x, gt, tg):
    import torch
    from videoyolo_amd import autograd
    with autograd.record():
        losses = net(x, gt, *tg)
        autograd.backward([losses[0] + losses[1] + losses[2] + losses[3]])
    torch.cuda.synchronize()
    return losses


def _reference_step(C, params, x, gt, tg, unbiased):
    from oracle import yolo3_train_oracle as TO

    class Unbiased(TO.OracleYolo3Train):     # the class attribute stays as it is for everybody else
        RUNNING_VAR_UNBIASED = bool(unbiased)

    orc = Unbiased(C, dict(params))
    losses = orc.forward_train(x, gt, *tg)
    return orc, losses


def _check_ratio(name, init, on, off, n):
    """What the flag adds, per element: running_var = fl(fl(init * 0.9f) + fl(v * fl(1 - 0.9f))) with v the biased variance
    (off) or v * n / (n - 1) (on), so (on - fl(init * 0.9f)) / (off - fl(init * 0.9f)) is n / (n - 1) up to rounding: each
    stored value is off by at most half an ulp of itself from its sum (2^-24 relative, both runs), and the three products
    in v's path by 2^-24 each.  Bound, from the number format alone: 2 * 2^-24 * (|on| + |off|) / |off - base| + 4 * 2^-24
    — 1e-6 where the variance is of order one, against n / (n - 1) - 1 = 1.2e-4 for the largest count here (8192).
    Returns the fraction of elements whose bound is under half of n / (n - 1) - 1: those pin the count."""
    eps = 2.0 ** -24
    base = (np.asarray(init, np.float32) * np.float32(0.9)).astype(np.float64)
    d_on, d_off = on.astype(np.float64) - base, off.astype(np.float64) - base
    ok = np.abs(d_off) > 0
    assert ok.any(), name
    f = n / (n - 1.0)
    ratio = d_on[ok] / d_off[ok]
    tol = 2 * eps * (np.abs(on[ok]) + np.abs(off[ok])) / np.abs(d_off[ok]) + 4 * eps
    worst = np.abs(ratio - f) / tol
    assert (worst <= 1).all(), (name, n, f, ratio[np.argmax(worst)], tol[np.argmax(worst)])
    return float((tol < 0.5 * (f - 1)).mean())


def test_running_variance_unbiased_matches_the_reference():
    """One recorded step of a YOLOV3 at 64 x 64, batch 2: running_var and running_mean of all 72 cells, the losses and the
    gradients against the CPU training reference with RUNNING_VAR_UNBIASED = True (bars of test_gpu_train_parity.py: losses
    1e-4, gradients 2e-3 of each tensor's max, running statistics rtol 1e-4 / atol 1e-5); the same step with the flag off
    differs in every running_var."""
    import videoyolo_amd as vy
    C, B, S = 4, 2, 64
    params, x, gt, tg = _train_setup(C, B, S)
    orc, ref_losses = _reference_step(C, params, x, gt, tg, True)
    ref_grads = orc.backward()
    got_var = {}
    for flag in (True, False):
        net = vy.yolo3_darknet53(["c%d" % i for i in range(C)], pretrained_base=False)
        net.set_parameters(params)
        net.collect_params().reset_ctx("cuda:0")
        net.set_semantics(running_var_unbiased=flag)
        losses = _step(net, x, gt, tg)
        for got, want in zip(losses, ref_losses):   # normalisation does not change: the losses are the same either way
            np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-4, atol=1e-4)
        for name, want in ref_grads.items():
            err = np.abs(net.grad(name) - want).max() / (np.abs(want).max() + 1e-6)
            assert err < 2e-3, (flag, name, err)
        got_var[flag] = {n: net.collect_params()[n].data() for n in orc.new_running}
    names = [n for n in orc.new_running if n.endswith("running_var")]
    assert len(names) == 72 and len(orc.new_running) == 144
    for name, want in orc.new_running.items():
        np.testing.assert_allclose(got_var[True][name], want, rtol=1e-4, atol=1e-5, err_msg=name)
        if name.endswith("running_mean"):
            assert np.array_equal(got_var[True][name], got_var[False][name]), name
    biased = _reference_step(C, params, x, gt, tg, False)[0].new_running
    for name in names:
        assert not np.array_equal(got_var[True][name], got_var[False][name]), name
        np.testing.assert_allclose(got_var[False][name], biased[name], rtol=1e-4, atol=1e-5, err_msg=name)
    # the count itself, cell by cell: the ratio of what the two runs added is n / (n - 1), n = B * H * W of the cell's output
    counts = {t["pre"] + ".1.running_var": t["z"].shape[0] * t["z"].shape[2] * t["z"].shape[3] for t in orc.tape if t["kind"] == "cell"}
    assert max(counts.values()) == B * S * S and min(counts.values()) == B * 2 * 2
    pinned = {n: _check_ratio(n, params[n], got_var[True][n], got_var[False][n], counts[n]) for n in names}
    print("elements whose rounding bound pins the count: min over cells %.2f (%s)" % min((v, k) for k, v in pinned.items()))
    assert all(v > 0 for v in pinned.values()), {k: v for k, v in pinned.items() if v == 0}


def test_running_variance_count_of_a_window_net():
    """A window net (max, k = 3, one clip, 64 x 64): its stages normalise over B * k = 3 frames — the count is
    B * fm * H * W with fm = 3 —, its heads over the one clip.  Stage statistics against the CPU training reference on the
    three frames as a batch; every cell against its own flag-off run scaled by n / (n - 1), n = the pixels per channel of that
    cell, at the suite's bar and then as the ratio of what the two runs added, to rounding (_check_ratio)."""
    import videoyolo_amd as vy
    C, K, S = 4, 3, 64
    params, x3, gt3, tg3 = _train_setup(C, K, S)
    orc, _ = _reference_step(C, params, x3, gt3, tg3, True)
    _, _, gt1, tg1 = _train_setup(C, 1, S)
    clip = x3.reshape((1, K, 3, S, S))
    got, counts = {}, {}
    for flag in (True, False):
        win = vy.yolo3_darknet53(["c%d" % i for i in range(C)], pretrained_base=False, k=K, k_join_type="max", k_join_pos="early")
        win.set_parameters(params)
        win.collect_params().reset_ctx("cuda:0")
        win.set_semantics(running_var_unbiased=flag)
        assert win.semantics["running_var_unbiased"] is flag
        _step(win, clip, gt1, tg1)
        got[flag] = {n: win.collect_params()[win._key(n)].data() for n in orc.new_running}
    for t in orc.tape:   # pixels per channel of every cell: the reference's three frames in the stages, one clip in the heads
        if t["kind"] == "cell":
            z = t["z"]
            counts[t["pre"] + ".1.running_var"] = (z.shape[0] if t["pre"].startswith("stages.") else 1) * z.shape[2] * z.shape[3]
    names = [n for n in orc.new_running if n.endswith("running_var")]
    assert len(names) == 72
    stage = [n for n in names if n.startswith("stages.")]
    assert counts[stage[0]] == 3 * 64 * 64 and min(counts.values()) == 4      # the stem: 3 frames; stride-32 heads: 2 x 2
    for n in stage:   # the reference saw the same three frames as one batch: the same count
        np.testing.assert_allclose(got[True][n], orc.new_running[n], rtol=1e-4, atol=1e-5, err_msg=n)
    for n in names:
        assert not np.array_equal(got[True][n], got[False][n]), n
        init = params[n]
        want = init * np.float32(0.9) + (got[False][n] - init * np.float32(0.9)) * np.float32(counts[n] / (counts[n] - 1.0))
        np.testing.assert_allclose(got[True][n], want, rtol=1e-4, atol=1e-5, err_msg="%s n=%d" % (n, counts[n]))
        mean = n.replace("running_var", "running_mean")
        assert np.array_equal(got[True][mean], got[False][mean]), mean
    pinned = {n: _check_ratio(n, params[n], got[True][n], got[False][n], counts[n]) for n in names}
    print("elements whose rounding bound pins the count: min over cells %.2f (%s)" % min((v, k) for k, v in pinned.items()))
    assert all(v > 0 for v in pinned.values()), {k: v for k, v in pinned.items() if v == 0}
