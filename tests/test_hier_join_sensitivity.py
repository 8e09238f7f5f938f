"""-m "not gpu": the checks tests/test_gpu_hier_conv.py holds the learned join to are sharp.

A toy join in numpy: B = 2 clips, fm = 3 (so B * fm = 6 pooled frames made of 18), C = 8, 10x10.  The "device" side is a
frame-by-frame restatement of hier.hip's three join kernels and of the BatchNorm kernels around them (the fp32 helpers of
tests/test_train_cells64_sensitivity.py); it must pass every check of tests/hier_join_model.py, and each planted bug must
fail the check that is there for it."""
import numpy as np
import pytest

import hier_join_model as J
import test_train_cells64_sensitivity as S
from oracle import train_cells64 as R

F32 = np.float32

MUTATIONS = {
    "weights_in_reversed_frame_order": "join forward",
    "grouping_strided_instead_of_consecutive": "join forward",
    "first_product_fused_into_the_chain": "join forward",
    "statistics_counted_over_B_not_B_fm": "forward stats",
    "dw_summed_over_one_frame_only": "join weight gradient",
    "dw_in_reversed_frame_order": "join weight gradient",
    "gx_multiplied_by_w0_for_every_frame": "join data gradient",
    "gx_accumulated_onto_the_plane": "join data gradient",
    "nonzero_value_in_pooled_border": "borders",
    "leaky_mask_dropped_from_dz": "bn backward dz",
}


def _case():
    rng = np.random.default_rng(31)
    r = lambda *s: rng.standard_normal(s).astype(F32)  # noqa: E731
    B, fm, C, H = 2, 3, 8, 10
    return dict(B=B, fm=fm, C=C, H=H, pre=r(3 * B * fm, C, H, H), w=r(C, 3), gam=(1 + 0.2 * r(C)).astype(F32),
                bet=(0.3 * r(C)).astype(F32), g=r(B * fm, C, H, H), stale=r(3 * B * fm, C, H, H))


def _dev_z(pre, w, mut):
    n = pre.shape[0] // 3
    z = np.empty((n,) + pre.shape[1:], F32)
    for i in range(n):
        fr = [3 * i + t for t in range(3)]
        if mut == "grouping_strided_instead_of_consecutive":  # n, n + F, n + 2F
            fr = [i + t * n for t in range(3)]
        k = [w[:, t].reshape(-1, 1, 1) for t in range(3)]
        if mut == "weights_in_reversed_frame_order":
            k = k[::-1]
        x = [pre[f] for f in fr]
        if mut == "first_product_fused_into_the_chain":  # w0 x0 + w1 x1 rounded once: the first product never on its own
            acc = (k[0].astype(np.float64) * x[0] + k[1].astype(np.float64) * x[1]).astype(F32)
        else:
            acc = R.fmaf(k[1], x[1], (k[0] * x[0]).astype(F32))
        z[i] = R.fmaf(k[2], x[2], acc)
    return z


def _run(mut=None):
    c = _case()
    B, fm, C, H = c["B"], c["fm"], c["C"], c["H"]
    pre, w = c["pre"], c["w"]
    res = []
    z = _dev_z(pre, w, mut)
    res.append(J.check_forward("hjoin", pre, w, z))
    bn = S.dev_stats(z, c["gam"], c["bet"])
    if mut == "statistics_counted_over_B_not_B_fm":  # the sums run over every pooled frame, the count is B * H * W
        z64 = z.astype(np.float64)
        n = B * H * H
        mean = z64.sum(axis=(0, 2, 3)) / n
        var = np.maximum((z64 * z64).sum(axis=(0, 2, 3)) / n - mean * mean, 0)
        mf = mean.astype(F32)
        inv = (F32(1) / np.sqrt(var.astype(F32) + F32(1e-5))).astype(F32)
        sc = (c["gam"] * inv).astype(F32)
        bn = np.stack([mf, inv, sc, R.fmaf(-mf, sc, c["bet"])])
    res.append(R.check_stats("hjoin", z, bn[0], bn[1], c["gam"], c["bet"], bn[2], bn[3]))
    pooled = R.leaky(R.fmaf(z, bn[2].reshape(1, -1, 1, 1), bn[3].reshape(1, -1, 1, 1)))
    res.append(R.check_apply("hjoin", z, bn[2], bn[3], pooled))
    res.append(J.check_apply("hjoin", z, bn[2], bn[3], pooled))
    p_pad = S.pad(pooled)
    if mut == "nonzero_value_in_pooled_border":
        p_pad[4, 3, 0, 5] = F32(1e-3)
    res.append(R.border_zero("borders", "hjoin", p_pad))
    # backward: BatchNorm + leaky on the pooled plane's gradient, then the join
    rpc = J.bn_bwd_rows_per_chunk(B * fm, H, C)
    g = c["g"]
    bn_dev = bn
    if mut == "leaky_mask_dropped_from_dz":  # every element takes slope 1: a scale / shift under which all of y is positive
        bn_dev = bn.copy()
        bn_dev[2], bn_dev[3] = 0.0, 1.0
    dgam, dbet, dz = S.dev_bn_bwd(z, g, bn_dev, c["gam"], 1, rpc)
    res += R.check_bn_backward("hjoin", z, g, bn, c["gam"], 1, rpc, dgam, dbet, dz)
    gx = np.empty_like(pre)
    dw = np.zeros((C, 3))
    for i in range(z.shape[0]):
        for t in range(3):
            k = w[:, 0 if mut == "gx_multiplied_by_w0_for_every_frame" else t].reshape(-1, 1, 1)
            gx[3 * i + t] = (k * dz[i]).astype(F32)
            if mut == "dw_summed_over_one_frame_only" and i % 3:
                continue
            col = 2 - t if mut == "dw_in_reversed_frame_order" else t
            dw[:, col] += (pre[3 * i + t].astype(np.float64) * dz[i]).sum(axis=(1, 2))
    if mut == "gx_accumulated_onto_the_plane":
        gx = (c["stale"] + gx).astype(F32)
    res.append(J.check_data_grad("hjoin", dz, w, gx))
    res.append(J.check_weight_grad("hjoin", pre, dz, dw.astype(F32)))
    return res


def test_toy_join_passes_every_check():
    res = _run()
    bad = [r for r in res if not r.ok]
    assert not bad, bad
    assert {"join forward", "join apply", "join data gradient", "join weight gradient", "forward stats", "bn backward dz",
            "borders"} <= {r.kind for r in res}


def test_the_model_is_the_triple_filter():
    """z against the plain float64 sum: the pinned order is a rounding of it, nothing else"""
    c = _case()
    f = c["pre"].astype(np.float64).reshape((-1, 3) + c["pre"].shape[1:])
    want = sum(c["w"][:, t].astype(np.float64).reshape(1, -1, 1, 1) * f[:, t] for t in range(3))
    absum = sum(np.abs(c["w"][:, t].astype(np.float64).reshape(1, -1, 1, 1) * f[:, t]) for t in range(3))
    assert R._bounded("join", "model", J.join_z(c["pre"], c["w"]), want, absum, 3).ok
    dw, absum = J.join_dw64(c["pre"], c["g"])
    assert dw.shape == absum.shape == (c["C"], 3) and (np.abs(dw) <= absum).all()
    assert np.allclose(dw[:, 1], (f[:, 1] * c["g"].astype(np.float64)).sum(axis=(0, 2, 3)))
    sc, sh = J.fold(np.ones(4), np.zeros(4), np.zeros(4), np.full(4, F32(1) - F32(1e-5)))
    assert np.array_equal(sc, np.ones(4, F32)) and not sh.any()  # the identity pin of the GPU test exists in fp32


def test_rows_per_chunk_is_the_kernels():
    assert [J.bn_bwd_rows_per_chunk(6, 64, 32), J.bn_bwd_rows_per_chunk(48, 416, 32), J.bn_bwd_rows_per_chunk(16, 52, 512)] == \
        [1, 20, 2]


@pytest.mark.parametrize("mut", sorted(MUTATIONS))
def test_every_planted_bug_fails_its_check(mut):
    res = _run(mut)
    bad = [r for r in res if not r.ok]
    assert bad, "mutation %s passed every check" % mut
    assert MUTATIONS[mut] in {r.kind for r in bad}, (mut, bad)
    print("%s: fails %s" % (mut, sorted(set(r.kind for r in bad))))
