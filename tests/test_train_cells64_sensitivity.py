"""-m "not gpu": the per-cell training bars of oracle/train_cells64.py are sharp.

Small synthetic cells — stride 1 and 2, 1x1 and 3x3, a residual skip, a x2 transition, a plane with two consumers —
with a "device" side computed in fp32 in a blocked order different from the reference's (split-K slabs, row chunks,
fp32 convolutions).  It must pass every check.  Each of eight mutations of a kernel must fail one; the test also
records whether the end-to-end bar (max|got - want| < 2e-3 max|want| over the tensor) would have caught it.

A toy window step (k = 3) does the same for the window net's checks: a per-frame route cell with its batch statistics,
the pool, one head consumer of the pooled plane, a stride-2 consumer of the per-frame route whose data gradient
accumulates onto what the pool backward wrote, and a route with no other contributor (the stride-32 case).  Some
elements of the clips tie and some do not.  Eight more mutations must each fail a check.

Two more planted bugs are the ways a broken stream-K hand-off would show: a data gradient whose chain misses one
32-channel k-step of one tap on one 64x64 tile (check_dgrad), and one tile's rows missing from the per-tile statistics
sums (check_stats)."""
import numpy as np
import pytest
import torch

from oracle import train_cells64 as R

F32 = np.float32


# ---------------------------------------------------------------- fp32 "device" kernels
def dev_wgrad(dz, a, k, stride, kps, drop_split_pixel=False, dead_border=None):
    """split-K over the output pixels (b, y, x order): one fp32 slab per kps pixels, slabs added in order"""
    cols = torch.nn.functional.unfold(torch.from_numpy(a), k, padding=k // 2, stride=stride)  # (B, Cin k k, L)
    B, n, L = cols.shape
    colsm = cols.permute(1, 0, 2).reshape(n, B * L).numpy()
    dzm = np.ascontiguousarray(dz.transpose(1, 0, 2, 3).reshape(dz.shape[1], -1))
    P = dzm.shape[1]
    splits = -(-P // kps)
    acc = np.zeros((dzm.shape[0], n), F32)
    for i in range(splits):
        lo = i * kps + (1 if drop_split_pixel and i == 1 else 0)
        sl = slice(lo, min(P, (i + 1) * kps))
        acc = (acc + dzm[:, sl] @ colsm[:, sl].T).astype(F32)
    if dead_border is not None:  # dead table entries reading a NONZERO dz border pixel
        acc = (acc + (splits * kps - P) * np.outer(dead_border, colsm[:, P - 1])).astype(F32)
    return acc.reshape(dz.shape[1], a.shape[1], k, k), splits


def dev_dgrad(dz, w, stride, in_hw):
    k = w.shape[2]
    return torch.nn.grad.conv2d_input((dz.shape[0], w.shape[1]) + tuple(in_hw), torch.from_numpy(w),
                                      torch.from_numpy(dz), stride=stride, padding=k // 2).numpy()


def dev_stats(z, gam, bet, drop_last=False):
    zz = z[:-1] if drop_last else z
    z64 = zz.astype(np.float64)
    n = zz.shape[0] * zz.shape[2] * zz.shape[3]
    mean = z64.sum(axis=(0, 2, 3)) / n
    var = np.maximum((z64 * z64).sum(axis=(0, 2, 3)) / n - mean * mean, 0)
    mf, vf = mean.astype(F32), var.astype(F32)
    inv = (F32(1) / np.sqrt(vf + F32(1e-5))).astype(F32)
    sc = (gam * inv).astype(F32)
    sh = R.fmaf(-mf, sc, bet)
    return np.stack([mf, inv, sc, sh])


def dev_bn_bwd(z, g, bn, gam, ups, rpc, one_cell=False, no_slope_dgamma=False, no_dbeta_term=False):
    """the kernel's arithmetic in fp32: partial sums over chunks of rpc image rows, chunks added in float64"""
    mu, inv, sc, sh = [bn[i].reshape(1, -1, 1, 1) for i in range(4)]
    if ups == 2:
        g00, g01, g10, g11 = g[:, :, 0::2, 0::2], g[:, :, 0::2, 1::2], g[:, :, 1::2, 0::2], g[:, :, 1::2, 1::2]
        da = g00 * F32(4) if one_cell else (g00 + g01) + (g10 + g11)
    else:
        da = g
    da = da.astype(F32)
    pos = R.fmaf(z, sc, sh) > 0
    dy = np.where(pos, da, F32(0.1) * da).astype(F32)
    xh = ((z - mu) * inv).astype(F32)
    B, C, H, W = z.shape
    rows_dy = dy.transpose(0, 2, 1, 3).reshape(B * H, C, W)
    rows_p = ((da if no_slope_dgamma else dy) * xh).astype(F32).transpose(0, 2, 1, 3).reshape(B * H, C, W)
    s1 = np.zeros(C)
    s2 = np.zeros(C)
    for r0 in range(0, B * H, rpc):
        s1 += rows_dy[r0:r0 + rpc].sum(axis=(0, 2), dtype=F32)
        s2 += rows_p[r0:r0 + rpc].sum(axis=(0, 2), dtype=F32)
    n = B * H * W
    c1 = (gam * inv[0, :, 0, 0]).astype(F32).reshape(1, -1, 1, 1)
    c2 = np.zeros_like(c1) if no_dbeta_term else (s1 / n).astype(F32).reshape(1, -1, 1, 1)
    c3 = (s2 / n).astype(F32).reshape(1, -1, 1, 1)
    dz = (c1 * ((dy - c2) - xh * c3)).astype(F32)
    return s2.astype(F32), s1.astype(F32), dz


def pad(a, value=0.0):
    p = np.full(a.shape[:2] + (a.shape[2] + 2, a.shape[3] + 2), value, F32)
    p[:, :, 1:-1, 1:-1] = a
    return p


# ---------------------------------------------------------------- the synthetic cells
def _case():
    rng = np.random.default_rng(5)
    r = lambda *s: rng.standard_normal(s).astype(F32)  # noqa: E731
    B, C, S = 3, 16, 24
    c = dict(B=B, C=C, S=S)
    c["x"] = r(B, C, S, S)                              # producer output P (input of every cell below)
    c["w3"] = (r(C, C, 3, 3) * 0.2).astype(F32)          # 3x3 stride 1, consumer 1 of P, residual (output += P)
    c["w1"] = (r(C // 2, C, 1, 1) * 0.3).astype(F32)     # 1x1 transition, consumer 2 of P, x2 upsampled output
    c["ws"] = (r(2 * C, C, 3, 3) * 0.2).astype(F32)      # 3x3 stride 2
    c["gam"], c["bet"] = (1 + 0.2 * r(C)).astype(F32), (0.3 * r(C)).astype(F32)
    c["z"] = r(B, C, S, S)                               # raw conv output of the 3x3 cell
    c["g"] = r(B, C, S, S)                               # its output gradient
    c["zt"] = r(B, C // 2, S, S)                         # transition z, output gradient at 2x
    c["gt"] = r(B, C // 2, 2 * S, 2 * S)
    c["gamt"], c["bett"] = (1 + 0.2 * r(C // 2)).astype(F32), (0.3 * r(C // 2)).astype(F32)
    c["dz3"] = r(B, C, S, S)                             # dz of the consumers of P
    c["dz1"] = r(B, C // 2, S, S)
    c["dzs"] = r(B, 2 * C, S // 2, S // 2)
    c["skip"] = r(B, C, S, S)                            # gradient of the residual output (the skip addend)
    return c


MUTATIONS = ["wgrad_split_pixel_dropped", "dead_entries_read_nonzero_border", "stride2_parity_classes_swapped",
             "skip_addend_omitted", "transition_grad_from_one_cell", "leaky_slope_ignored_in_dgamma",
             "dbeta_term_dropped_from_dz", "last_image_left_out_of_stats"]


def _run(mut=None):
    c = _case()
    B, C, S = c["B"], c["C"], c["S"]
    res = []
    # forward statistics + apply (residual), 3x3 cell
    bn = dev_stats(c["z"], c["gam"], c["bet"], drop_last=mut == "last_image_left_out_of_stats")
    res.append(R.check_stats("cell3", c["z"], bn[0], bn[1], c["gam"], c["bet"], bn[2], bn[3]))
    out = (R.leaky(R.fmaf(c["z"], bn[2].reshape(1, -1, 1, 1), bn[3].reshape(1, -1, 1, 1))) + c["x"]).astype(F32)
    res.append(R.check_apply("cell3", c["z"], bn[2], bn[3], out, c["x"]))
    # BN + leaky backward, 3x3 cell (rows chunked by 5) and the x2 transition
    rpc = 5
    dg, db, dz = dev_bn_bwd(c["z"], c["g"], bn, c["gam"], 1, rpc, no_slope_dgamma=mut == "leaky_slope_ignored_in_dgamma",
                            no_dbeta_term=mut == "dbeta_term_dropped_from_dz")
    res += R.check_bn_backward("cell3", c["z"], c["g"], bn, c["gam"], 1, rpc, dg, db, dz)
    bnt = dev_stats(c["zt"], c["gamt"], c["bett"])
    outt = R.upsample2(R.leaky(R.fmaf(c["zt"], bnt[2].reshape(1, -1, 1, 1), bnt[3].reshape(1, -1, 1, 1))))
    res.append(R.check_apply("transition", c["zt"], bnt[2], bnt[3], outt, None, 2))
    dg, db, dzt = dev_bn_bwd(c["zt"], c["gt"], bnt, c["gamt"], 2, rpc, one_cell=mut == "transition_grad_from_one_cell")
    res += R.check_bn_backward("transition", c["zt"], c["gt"], bnt, c["gamt"], 2, rpc, dg, db, dzt)
    # weight gradients: 3x3 s1, 1x1, 3x3 s2 — split-K with a ragged last split (dead table entries)
    for name, dzw, k, s in (("cell3", c["dz3"], 3, 1), ("transition", c["dz1"], 1, 1), ("stride2", c["dzs"], 3, 2)):
        kps = 256 if s == 1 else 96
        border = None
        dz_pad = pad(dzw)
        if mut == "dead_entries_read_nonzero_border" and name == "cell3":
            border = np.full(dzw.shape[1], 0.5, F32)
            dz_pad[-1, :, -1, 0] = border  # the bottom-left border pixel of the last image
        got, splits = dev_wgrad(dzw, c["x"], k, s, kps, drop_split_pixel=mut == "wgrad_split_pixel_dropped",
                                dead_border=border)
        res.append(R.border_zero("borders", name + " dz", dz_pad))
        sel = [0, dzw.shape[1] - 1, 3, 5]
        res.append(R.check_wgrad(name, dzw, c["x"], k, s, sel, got[sel], splits, kps))
    # data gradient of P: two consumers (3x3 s1 + 1x1) and the residual skip addend ...
    dgp = (dev_dgrad(c["dz3"], c["w3"], 1, (S, S)) + dev_dgrad(c["dz1"], c["w1"], 1, (S, S))).astype(F32)
    if mut != "skip_addend_omitted":
        dgp = (dgp + c["skip"]).astype(F32)
    res.append(R.check_dgrad("P", dgp, [(c["dz3"], c["w3"], 1, 0), (c["dz1"], c["w1"], 1, 0)], [c["skip"]]))
    # ... and through a stride-2 consumer (four parity classes of input pixels)
    dgs = dev_dgrad(c["dzs"], c["ws"], 2, (S, S))
    if mut == "stride2_parity_classes_swapped":
        dgs = dgs.copy()
        dgs[:, :, 0::2, 1::2], dgs[:, :, 1::2, 0::2] = dgs[:, :, 1::2, 0::2].copy(), dgs[:, :, 0::2, 1::2].copy()
    res.append(R.check_dgrad("P (stride 2)", dgs, [(c["dzs"], c["ws"], 2, 0)]))
    return res


def test_blocked_fp32_device_passes_every_check():
    res = _run()
    bad = [r for r in res if not r.ok]
    assert not bad, bad
    for kind, v in R.summarize(res).items():
        print("%-20s worst err/bound %.3g, worst err/(u sqrt(n) S) %.3g" % (kind, v["worst_ratio"], v["worst_headroom"]))
    # the bounds are not vacuous: typical errors sit well inside them, but not by orders of magnitude beyond sqrt(n)
    assert all(r.headroom < 50 for r in res)


@pytest.mark.parametrize("mut", MUTATIONS)
def test_every_mutation_fails_the_per_cell_check(mut):
    res = _run(mut)
    bad = [r for r in res if not r.ok]
    assert bad, "mutation %s passed every check" % mut
    # the tensor the mutation lands in, judged by the end-to-end bar (border checks have no counterpart there)
    old = [r.old_bar_ok for r in bad if r.kind != "borders"]
    caught = old and not all(old)
    print("%s: fails %s; the 2e-3-of-max bar %s" % (mut, sorted(set(r.kind for r in bad)),
                                                    "catches it" if caught else "MISSES it"))


# ---------------------------------------------------------------- a broken stream-K hand-off
# A stream-K launch hands a tile's accumulators from the block that starts it to the block that finishes it.  If a
# hand-off is wrong, the finished tile lacks the k-steps of one piece: on a data gradient one 64x64 tile (64 pixels in
# (b, y, x) order x 64 input channels) misses 32 output channels of one tap; on the training forward the tile's rows
# are missing from the per-tile statistics sums.
HAND_OFF_MUTATIONS = ["dgrad_chain_misses_one_k_step_on_one_tile", "one_tile_rows_missing_from_statistics_sums"]
TILE = 64


def _run_hand_off(mut=None):
    rng = np.random.default_rng(17)
    r = lambda *s: rng.standard_normal(s).astype(F32)  # noqa: E731
    B, Cout, Cin, S = 2, 64, 96, 12        # data gradient: M = 288 pixels (4.5 tiles), N = 96 (1.5 tiles), K = 9 taps x 2 k-steps
    dz, w = r(B, Cout, S, S), (r(Cout, Cin, 3, 3) * 0.1).astype(F32)
    got = dev_dgrad(dz, w, 1, (S, S))
    if mut == "dgrad_chain_misses_one_k_step_on_one_tile":
        w_lost = w.copy()
        w_lost[32:64, :, 2, 0] = 0         # the second k-step (output channels 32 .. 63) of tap (2, 0)
        lost = dev_dgrad(dz, w_lost, 1, (S, S))
        flat, flat_lost = got.transpose(0, 2, 3, 1).reshape(B * S * S, Cin), lost.transpose(0, 2, 3, 1).reshape(B * S * S, Cin)
        flat = flat.copy()
        flat[TILE:2 * TILE, :TILE] = flat_lost[TILE:2 * TILE, :TILE]   # pixel tile 1, channel tile 0
        got = np.ascontiguousarray(flat.reshape(B, S, S, Cin).transpose(0, 3, 1, 2))
    res = [R.check_dgrad("P", got, [(dz, w, 1, 0)])]
    C, Sz = 16, 24                         # statistics: 1152 pixels = 18 tiles of 64 rows
    z, gam, bet = r(B, C, Sz, Sz), (1 + 0.2 * r(C)).astype(F32), (0.3 * r(C)).astype(F32)
    rows = z.transpose(0, 2, 3, 1).reshape(B * Sz * Sz, C).astype(np.float64)
    keep = np.ones(len(rows), bool)
    if mut == "one_tile_rows_missing_from_statistics_sums":
        keep[5 * TILE:6 * TILE] = False    # the sums lack tile 5; the count is still every pixel
    n = len(rows)
    mean = rows[keep].sum(axis=0) / n
    var = np.maximum((rows[keep] ** 2).sum(axis=0) / n - mean * mean, 0)
    mf = mean.astype(F32)
    inv = (F32(1) / np.sqrt(var.astype(F32) + F32(1e-5))).astype(F32)
    sc = (gam * inv).astype(F32)
    res.append(R.check_stats("cell", z, mf, inv, gam, bet, sc, R.fmaf(-mf, sc, bet)))
    return res


def test_hand_off_case_passes_unmutated():
    res = _run_hand_off()
    assert all(r.ok for r in res), res
    assert all(r.headroom < 50 for r in res)


@pytest.mark.parametrize("mut", HAND_OFF_MUTATIONS)
def test_a_broken_stream_k_hand_off_fails_its_check(mut):
    res = _run_hand_off(mut)
    bad = [r.kind for r in res if not r.ok]
    assert bad == ["data gradient" if mut.startswith("dgrad") else "forward stats"], (mut, res)
    old = [r.old_bar_ok for r in res if not r.ok]
    print("%s: fails %s; the 2e-3-of-max bar %s" % (mut, bad, "MISSES it" if all(old) else "catches it"))


# ---------------------------------------------------------------- the toy window step
def dev_pool(frames, B, k, join, frame_of=lambda b, t, B, k: b * k + t):
    """the pool kernel's loop over one clip's frames, clip by clip"""
    out = np.empty((B,) + frames.shape[1:], F32)
    for b in range(B):
        acc = frames[frame_of(b, 0, B, k)].copy()
        for t in range(1, k):
            v = frames[frame_of(b, t, B, k)]
            acc = np.where(v > acc, v, acc) if join == "max" else (acc + v).astype(F32)
        out[b] = acc if join == "max" else (acc / F32(k)).astype(F32)
    return out


def dev_pool_bwd(g, frames, pooled, B, k, join, mut=None):
    out = np.zeros_like(frames)
    for b in range(B):
        fr = frames[b * k:(b + 1) * k]
        if join == "mean":
            out[b * k:(b + 1) * k] = g[b] if mut == "mean_backward_without_the_division" else (g[b] / F32(k)).astype(F32)
            continue
        hold = fr == pooled[b]
        if mut == "max_backward_to_first_maximal_frame_only":
            hold &= np.cumsum(hold, axis=0) == 1
        gb = np.broadcast_to(g[b], fr.shape)
        if mut == "max_backward_split_among_ties":
            gb = (gb / hold.sum(axis=0).astype(F32)).astype(F32)
        out[b * k:(b + 1) * k] = np.where(hold, gb, F32(0))
    return out


WINDOW_MUTATIONS = ["max_backward_to_first_maximal_frame_only", "max_backward_split_among_ties",
                    "mean_backward_without_the_division", "frames_taken_as_t_times_B_plus_b",
                    "data_gradient_overwrites_pool_gradient", "pool_gradient_overwrites_data_gradient",
                    "backbone_statistics_counted_over_B", "nonzero_value_in_route_gradient_border"]


def _window_case():
    rng = np.random.default_rng(11)
    r = lambda *s: rng.standard_normal(s).astype(F32)  # noqa: E731
    B, k, C, S = 2, 3, 8, 12
    c = dict(B=B, k=k, C=C, S=S)
    for key in ("route", "route32"):  # per-frame route values: some elements tie (two frames, or all three), most do not
        f = r(B, k, C, S, S)
        tie2, tie3 = rng.random((B, C, S, S)) < 0.15, rng.random((B, C, S, S)) < 0.05
        f[:, 2] = np.where(tie2, f[:, 0], f[:, 2])
        f[:, 1] = np.where(tie3, f[:, 0], f[:, 1])
        f[:, 2] = np.where(tie3, f[:, 0], f[:, 2])
        c[key] = f.reshape(B * k, C, S, S)
    c["z"] = r(B * k, C, S, S)                            # raw conv output of the route cell, B*k frames
    c["gam"], c["bet"] = (1 + 0.2 * r(C)).astype(F32), (0.3 * r(C)).astype(F32)
    c["wh"] = (r(C, C, 1, 1) * 0.3).astype(F32)           # head consumer of the pooled plane, on B clips
    c["dzh"] = r(B, C, S, S)
    c["ws"] = (r(2 * C, C, 3, 3) * 0.2).astype(F32)       # the next stage's first conv: stride 2, on B*k frames
    c["dzs"] = r(B * k, 2 * C, S // 2, S // 2)
    c["g32"] = r(B, C, S // 2, S // 2)                    # pooled gradient of the route without another contributor
    c["route32"] = c["route32"][:, :, :S // 2, :S // 2].copy()
    return c


def _run_window(join, mut=None):
    c = _window_case()
    B, k, S = c["B"], c["k"], c["S"]
    res = []
    # backbone statistics over the B*k frames
    z = c["z"]
    bn = dev_stats(z, c["gam"], c["bet"])
    if mut == "backbone_statistics_counted_over_B":  # the sums run over every frame, the count is B * H * W
        z64 = z.astype(np.float64)
        n = B * S * S
        mean = z64.sum(axis=(0, 2, 3)) / n
        var = np.maximum((z64 * z64).sum(axis=(0, 2, 3)) / n - mean * mean, 0)
        mf = mean.astype(F32)
        inv = (F32(1) / np.sqrt(var.astype(F32) + F32(1e-5))).astype(F32)
        sc = (c["gam"] * inv).astype(F32)
        bn = np.stack([mf, inv, sc, R.fmaf(-mf, sc, c["bet"])])
    res.append(R.check_stats("route cell", z, bn[0], bn[1], c["gam"], c["bet"], bn[2], bn[3]))
    # the pool and its head consumer
    order = (lambda b, t, B_, k_: t * B_ + b) if mut == "frames_taken_as_t_times_B_plus_b" else (lambda b, t, B_, k_: b * k_ + t)
    frames = c["route"]
    pooled = dev_pool(frames, B, k, join, order)
    res.append(R.check_pool_forward("pool", frames, k, join, pooled))
    g_pool = dev_dgrad(c["dzh"], c["wh"], 1, (S, S))
    res.append(R.check_dgrad("pool", g_pool, [(c["dzh"], c["wh"], 1, 0)]))
    # the per-frame route gradient: the pool backward writes, the stride-2 consumer's data gradient accumulates
    gp = dev_pool_bwd(g_pool, frames, pooled, B, k, join, mut)
    gd = dev_dgrad(c["dzs"], c["ws"], 2, (S, S))
    g_route = (gp + gd).astype(F32)
    if mut == "data_gradient_overwrites_pool_gradient":
        g_route = gd
    if mut == "pool_gradient_overwrites_data_gradient":
        g_route = gp
    g_pad = pad(g_route)
    if mut == "nonzero_value_in_route_gradient_border":
        g_pad[1, 2, 0, 3] = F32(1e-3)
    res.append(R.border_zero("borders", "route grad", g_pad))
    res.append(R.check_dgrad("route", R.interior(g_pad), [(c["dzs"], c["ws"], 2, 0)],
                             [R.pool_backward(g_pool, frames, pooled, k, join)]))
    # a route whose gradient is the pool backward's alone: bit-equal
    f32_, g32 = c["route32"], c["g32"]
    p32 = dev_pool(f32_, B, k, join, order)
    res.append(R.check_pool_forward("pool32", f32_, k, join, p32))
    r, wins, ties = R.check_pool_backward("pool32", g32, f32_, p32, k, join, dev_pool_bwd(g32, f32_, p32, B, k, join, mut))
    res.append(r)
    return res, wins, ties


@pytest.mark.parametrize("join", ["max", "mean"])
def test_toy_window_step_passes_every_check(join):
    res, wins, ties = _run_window(join)
    bad = [r for r in res if not r.ok]
    assert not bad, bad
    # the clips hold both kinds of element: every frame wins some on its own, and some are tied
    assert min(wins) > 0 and ties > 0, (wins, ties)
    assert all(r.headroom < 50 for r in res)


def test_pool_reference_on_ties():
    """the numpy pool in temporal.hip's arithmetic: ties keep the earliest frame and every tied frame gets the full g"""
    f = np.array([[1, 3, -2, 0.0], [1, 2, -2, -0.0], [0, 3, -5, 0.0]], F32).reshape(3, 1, 1, 4)
    g = np.array([10, 20, 30, 40], F32).reshape(1, 1, 1, 4)
    m = R.pool_forward(f, 3, "max")
    assert np.array_equal(m.ravel(), [1, 3, -2, 0]) and not np.signbit(m.ravel()[3])
    assert np.array_equal(R.pool_backward(g, f, m, 3, "max").reshape(3, 4), [[10, 20, 30, 40], [10, 0, 30, 40], [0, 20, 0, 40]])
    mean = R.pool_forward(f, 3, "mean")
    want = ((f[0] + f[1]).astype(F32) + f[2]).astype(F32) / F32(3)
    assert np.array_equal(mean[0], want)
    assert np.array_equal(R.pool_backward(g, f, mean, 3, "mean"), np.repeat((g / F32(3)).astype(F32), 3, axis=0))
    assert R.pool_wins(f, 3) == ([0, 0, 0], 4)


@pytest.mark.parametrize("mut", WINDOW_MUTATIONS)
def test_every_window_mutation_fails_a_check(mut):
    join = "mean" if mut.startswith("mean") else "max"
    res, _, _ = _run_window(join, mut)
    bad = [r for r in res if not r.ok]
    assert bad, "mutation %s passed every check" % mut
    # the end-to-end bar is judged on the bounded checks that fail; a border value and a bit-equality of the pool have
    # no counterpart there, so a mutation that only fails those gets no verdict
    old = [r.old_bar_ok for r in bad if r.kind not in ("borders", "pool forward", "pool backward")]
    verdict = "is not applicable" if not old else ("MISSES it" if all(old) else "catches it")
    print("%s: fails %s; the 2e-3-of-max bar %s" % (mut, sorted(set(r.kind for r in bad)), verdict))


def test_fmaf_emulation_is_exact():
    """R.fmaf rounds a*b + c once, as the device's fmaf: against exact rational arithmetic on values built to hit
    fp32 midpoints"""
    from fractions import Fraction
    rng = np.random.default_rng(1)
    a = rng.standard_normal(4000).astype(F32)
    b = rng.standard_normal(4000).astype(F32)
    c = rng.standard_normal(4000).astype(F32)
    # c = -(a*b rounded) + a tiny residual: the exact sum sits near a rounding boundary of fp32
    c[::2] = (-(a[::2] * b[::2])).astype(F32)
    got = R.fmaf(a, b, c)
    for i in range(0, 4000, 7):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        want = np.float32(float(exact))  # float(Fraction) rounds once to double; exactness checked below
        assert got[i] == want or abs(Fraction(float(got[i])) - exact) <= abs(Fraction(float(want)) - exact), i
