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
sums (check_stats).

The SyncBatchNorm statistics exchange: a toy synchronised cell in the device's blocked order (per-tile double sums,
fp32 chunk partials, the 32-group ordered reduce in 32-column blocks, a "callback" that adds R.sync_peer's peer, the count
times the world size, the fp32 finalize with running statistics) passes check_sync_sums / check_stats / check_running /
check_bn_backward at world 3, 2 and 1; eight planted exchange bugs must each fail the check they belong to.

The two ends of the step get the same treatment: loss_kernel + loss_reduce_kernel, raw_preds_kernel and sgd_kernel are
restated in fp32 numpy (vy_math's exp / log, the 256-lane butterfly, the blocks summed in double; four momentum steps
with a multiplier change) and must pass check_losses / check_head_grad / check_raw_preds / SgdRef; nine loss faults, one
decode fault and four SGD faults must each fail one with ratio > 1.  The accuracies of vy_expf / vy_logf that the loss
terms' rounding counts rest on are held on dense grids, and the census conditions of every constructed case of
tests/test_gpu_loss_cells.py (tests/loss_cases.py) are settled here on the CPU oracle's train-mode heads forward."""
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


# ---------------------------------------------------------------- the SyncBatchNorm statistics exchange
# A synchronised cell in the device's blocked order: per-tile double sums (forward) or fp32 chunk partials (backward),
# the ordered reduce of the partial rows (32 row groups, 32-column blocks) into the local [2][C] sums, the exchange (the
# peer of R.sync_peer added by the "callback"), the count times the world size, the finalize in fp32.
def dev_reduce_partials(parts, drop_last_block=False):
    """reduce_partials_kernel: row group r adds rows r, r + 32, ... in order, then the 32 group sums in order"""
    p = np.asarray(parts, np.float64)
    groups = np.zeros((32, p.shape[1]))
    for t in range(p.shape[0]):
        groups[t % 32] += p[t]
    out = np.zeros(p.shape[1])
    for r in range(32):
        out += groups[r]
    if drop_last_block:  # the last block of 32 columns never launched: its sums keep what the buffer held
        out[(p.shape[1] - 1) // 32 * 32:] = 0.0
    return out


def dev_sync_stats(z, gam, bet, before, exchange, world, unbiased, mut=None):
    """-> (bn [4][C], running statistics after [2][C]).  exchange(local [2C] doubles) -> the global sums."""
    B, C, H, W = z.shape
    n = B * H * W
    rows = z.transpose(0, 2, 3, 1).reshape(n, C).astype(np.float64)
    parts = np.stack([np.concatenate([rows[i:i + 64].sum(0), (rows[i:i + 64] ** 2).sum(0)]) for i in range(0, n, 64)])
    local = dev_reduce_partials(parts, mut == "last_32_column_block_of_the_reduce_missing")
    glob = exchange(local)
    count = float(n if mut == "count_not_multiplied_by_world" else n * world)

    def stats(sums, cnt):
        mean = sums[:C] / cnt
        return mean.astype(F32), np.maximum(sums[C:] / cnt - mean * mean, 0).astype(F32)

    mf, vf = stats(glob, count)
    inv = (F32(1) / np.sqrt(vf + F32(1e-5))).astype(F32)
    sc = (gam * inv).astype(F32)
    rm, rv = stats(local, float(n)) if mut == "running_statistics_from_the_local_batch" else (mf, vf)
    if unbiased:
        cnt = float(n) if mut == "unbiased_factor_from_the_local_count" else count
        rv = (rv * F32(cnt / max(cnt - 1.0, 1.0))).astype(F32)
    mom = F32(0.9)
    om = F32(1) - mom
    after = np.stack([((before[0] * mom).astype(F32) + (rm * om).astype(F32)).astype(F32),
                      ((before[1] * mom).astype(F32) + (rv * om).astype(F32)).astype(F32)])
    return np.stack([mf, inv, sc, R.fmaf(-mf, sc, bet)]), after


def dev_sync_bn_bwd(z, g, bn, gam, rpc, exchange, world, mut=None):
    """-> (dgamma, dbeta, dz): fp32 partial rows over chunks of rpc image rows, the ordered reduce, the exchange, then
    dgamma / dbeta from the local sums and the coefficients of dz from the global sums over the global count"""
    mu, inv, sc, sh = [bn[i].reshape(1, -1, 1, 1) for i in range(4)]
    dy = np.where(R.fmaf(z, sc, sh) > 0, g, F32(0.1) * g).astype(F32)
    xh = ((z - mu) * inv).astype(F32)
    B, C, H, W = z.shape
    n = B * H * W
    rows_dy = dy.transpose(0, 2, 1, 3).reshape(B * H, C, W)
    rows_p = (dy * xh).astype(F32).transpose(0, 2, 1, 3).reshape(B * H, C, W)
    parts = np.stack([np.concatenate([rows_dy[r0:r0 + rpc].sum(axis=(0, 2), dtype=F32),
                                      rows_p[r0:r0 + rpc].sum(axis=(0, 2), dtype=F32)]) for r0 in range(0, B * H, rpc)])
    local = dev_reduce_partials(parts, mut == "last_32_column_block_of_the_reduce_missing")
    glob = exchange(local)
    count = float(n if mut == "count_not_multiplied_by_world" else n * world)
    own = glob if mut == "dgamma_dbeta_from_the_global_sums" else local
    coef, cnt = (local, float(n)) if mut == "backward_coefficients_from_the_local_sums" else (glob, count)
    c1 = (gam * inv[0, :, 0, 0]).astype(F32).reshape(1, -1, 1, 1)
    c2 = (coef[:C] / cnt).astype(F32).reshape(1, -1, 1, 1)
    c3 = (coef[C:] / cnt).astype(F32).reshape(1, -1, 1, 1)
    dz = (c1 * ((dy - c2) - xh * c3)).astype(F32)
    return own[C:].astype(F32), own[:C].astype(F32), dz


SYNC_MUTATIONS = ["count_not_multiplied_by_world", "backward_coefficients_from_the_local_sums",
                  "dgamma_dbeta_from_the_global_sums", "running_statistics_from_the_local_batch",
                  "unbiased_factor_from_the_local_count", "exchange_covers_the_first_C_doubles_only",
                  "last_32_column_block_of_the_reduce_missing", "forward_peer_added_twice"]


def _run_sync(mut=None, world=3, unbiased=True):
    rng = np.random.default_rng(23)
    r = lambda *s: rng.standard_normal(s).astype(F32)  # noqa: E731
    B, C, S, rpc = 3, 48, 24, 5            # 2C = 96 columns: three 32-column blocks; 1728 samples: 27 tiles, 15 chunks
    z, g = (0.5 + 1.5 * r(B, C, S, S)).astype(F32), r(B, C, S, S)
    gam, bet = (1 + 0.2 * r(C)).astype(F32), (0.3 * r(C)).astype(F32)
    before = np.stack([0.2 * r(C), (1 + 0.3 * np.abs(r(C))).astype(F32)])
    n = B * S * S
    calls = []

    def exchange(local):
        """the statistics callback: records what it is handed and the peer it adds"""
        i = len(calls)
        peer = R.sync_peer(i, local.reshape(2, C), n, world, forward=i == 0, seed=1)
        calls.append(dict(local=local.reshape(2, C).copy(), peer=peer))
        add = peer.reshape(-1).copy()
        if mut == "exchange_covers_the_first_C_doubles_only":
            add[C:] = 0.0
        glob = local + add
        if mut == "forward_peer_added_twice" and i == 0:  # the callback's result accumulated onto the local sums as well
            glob = glob + add
        return glob

    bn, after = dev_sync_stats(z, gam, bet, before, exchange, world, unbiased, mut)
    fwd = calls[0]
    kw = dict(peer=fwd["peer"], world=world)
    res = [R.check_sync_sums("sync cell", fwd["local"], z=z),
           R.check_stats("sync cell", z, bn[0], bn[1], gam, bet, bn[2], bn[3], **kw),
           R.check_running("sync cell", z, bn[0], before, after, unbiased=unbiased, **kw)]
    out = R.leaky(R.fmaf(z, bn[2].reshape(1, -1, 1, 1), bn[3].reshape(1, -1, 1, 1)))
    res.append(R.check_apply("sync cell", z, bn[2], bn[3], out))
    dg, db, dz = dev_sync_bn_bwd(z, g, bn, gam, rpc, exchange, world, mut)
    bwd = calls[1]
    res += R.check_bn_backward("sync cell", z, g, bn, gam, 1, rpc, dg, db, dz, peer=bwd["peer"], world=world,
                               local_got=bwd["local"])
    told_apart = (bool(R.local_mean_differs(z, **kw).all()), res[-1].extra.get("local_only_differs"))
    return res, told_apart


@pytest.mark.parametrize("world,unbiased", [(3, True), (2, False), (1, False)])
def test_blocked_sync_device_passes_every_check(world, unbiased):
    res, told_apart = _run_sync(None, world, unbiased)
    bad = [r for r in res if not r.ok]
    assert not bad, bad
    assert {r.kind for r in res} == {"sync sums forward", "forward stats", "running stats", "forward apply",
                                     "bn backward dbeta", "bn backward dgamma", "sync sums backward", "bn backward dz"}
    for r in res:
        print(r)
    # the inputs tell a kernel that missed the exchange from a right one — unless there is no peer (world 1)
    assert told_apart == (world > 1, world > 1), told_apart
    assert all(r.headroom < 50 for r in res)


def test_sync_references_without_a_peer_are_the_per_device_ones():
    """peer=None, world=1: check_stats / check_bn_backward give the per-device Results bit for bit (a zero peer too)"""
    c = _case()
    bn = dev_stats(c["z"], c["gam"], c["bet"])
    dg, db, dz = dev_bn_bwd(c["z"], c["g"], bn, c["gam"], 1, 5)
    zero = np.zeros((2, c["C"]))
    a = [R.check_stats("cell3", c["z"], bn[0], bn[1], c["gam"], c["bet"], bn[2], bn[3])]
    a += R.check_bn_backward("cell3", c["z"], c["g"], bn, c["gam"], 1, 5, dg, db, dz)
    b = [R.check_stats("cell3", c["z"], bn[0], bn[1], c["gam"], c["bet"], bn[2], bn[3], peer=zero, world=1)]
    b += R.check_bn_backward("cell3", c["z"], c["g"], bn, c["gam"], 1, 5, dg, db, dz, peer=zero, world=1)
    assert [(r.kind, r.ratio, r.headroom, r.err_max) for r in a][:3] == [(r.kind, r.ratio, r.headroom, r.err_max) for r in b][:3]
    assert a[3].err_max == b[3].err_max and abs(a[3].ratio / b[3].ratio - 1) < 1e-8   # (dz: the bar gains 2 u64 |c|)


@pytest.mark.parametrize("n,world", [(4, 3), (8, 2), (4096, 2)])
def test_constructed_peer_moves_every_channel(n, world):
    """R.sync_peer at the sample counts of tests/test_gpu_syncbn_cells.py's deepest cells (4 and 8 local samples) and a
    large one, for every call index of a step: the global variance stays positive, the fp32 global mean is more than
    1 ulp from the local one and the variance moves in every channel, the backward peer is nonzero in every entry and
    changes with the call index; world 1 gives a zero peer."""
    C = 1024
    for index in range(12):
        z = (0.3 + np.random.default_rng(100 + index).standard_normal((n, C, 1, 1))).astype(F32)
        z64 = z.astype(np.float64)
        local = np.stack([z64.sum(axis=(0, 2, 3)), (z64 * z64).sum(axis=(0, 2, 3))])
        fwd = R.sync_peer(index, local, n, world, forward=True, seed=3)
        mean, var, count = R.stats64(z, fwd, world)
        assert count == n * world and (var > 0).all() and R.local_mean_differs(z, fwd, world).all()
        lvar = R.stats64(z)[1]   # (the two shifts can nearly cancel in a channel: the bar is what check_stats resolves)
        assert (np.abs(var - lvar) > 4 * np.spacing(lvar.astype(F32)).astype(np.float64)).all()
        bwd = R.sync_peer(index, local, n, world, forward=False, seed=3)
        assert np.abs(bwd).min() > 0
        assert not np.array_equal(bwd, R.sync_peer(index + 1, local, n, world, forward=False, seed=3))
        assert not R.sync_peer(index, local, n, 1, forward=True, seed=3).any()


@pytest.mark.parametrize("mut", SYNC_MUTATIONS)
def test_every_sync_mutation_fails_a_check(mut):
    res, _ = _run_sync(mut)
    bad = [r for r in res if not r.ok]
    assert bad, "mutation %s passed every check" % mut
    want = {"count_not_multiplied_by_world": "forward stats", "backward_coefficients_from_the_local_sums": "bn backward dz",
            "dgamma_dbeta_from_the_global_sums": "bn backward dgamma", "running_statistics_from_the_local_batch": "running stats",
            "unbiased_factor_from_the_local_count": "running stats", "exchange_covers_the_first_C_doubles_only": "forward stats",
            "last_32_column_block_of_the_reduce_missing": "sync sums forward", "forward_peer_added_twice": "forward stats"}
    assert want[mut] in {r.kind for r in bad}, (mut, bad)
    if mut in ("backward_coefficients_from_the_local_sums", "dgamma_dbeta_from_the_global_sums",
               "running_statistics_from_the_local_batch", "unbiased_factor_from_the_local_count"):
        assert {r.kind for r in bad} <= {want[mut], "bn backward dbeta"}, (mut, bad)   # nothing else moves
    old = [r.old_bar_ok for r in bad if r.kind != "running stats"]
    verdict = "is not applicable" if not old else ("MISSES it" if all(old) else "catches it")
    print("%s: fails %s; the 2e-3-of-max bar %s" % (mut, sorted(set(r.kind for r in bad)), verdict))


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


# ---------------------------------------------------------------- the loss kernels and the SGD kernel
# The rounding counts of the loss terms (oracle/train_cells64.py) rest on two accuracies of include/vy_math.h on the
# arguments the loss gives them; both are held here on dense grids.
def test_vy_math_accuracies_the_loss_counts_rest_on():
    from oracle import yolo3_oracle as O
    x = -np.concatenate([np.linspace(0, 86, 400001), np.abs(np.random.default_rng(0).standard_normal(200000)) * 3]).astype(F32)
    e, true = O.exp(x).astype(np.float64), np.exp(x.astype(np.float64))
    assert (np.abs(e - true) / true).max() <= 4 * R.U                       # vy_expf: 2 ulp
    y = np.linspace(1, 2, 400001).astype(F32)[1:]
    lg, true = O.log(y).astype(np.float64), np.log(y.astype(np.float64))
    assert (np.abs(lg - true) / true).max() <= 5 * R.U                      # vy_logf on (1, 2]: five roundings
    assert O.log(np.ones(1, F32))[0] == 0 and O.exp(np.array([-86.5, 88.6], F32)).tolist() == [0.0, np.inf]


import loss_cases as L  # noqa: E402

TOY = dict(C=80, smooth=True, thresh=0.5, M=16, valid=12, B=2, H=128, W=128, seed=21)   # N = 1008: four blocks, tail 240
LOSS_MUTATIONS = ["anchor_term_dropped", "above_threshold_anchor_taken_as_negative", "ge_instead_of_gt_at_the_threshold",
                  "smoothing_constant_1_40_at_80_classes", "omask_not_scaled_by_fractional_obj_t",
                  "box_weights_not_scaled_by_fractional_obj_t", "zero_scale_difference_given_gradient_plus_w",
                  "tail_lanes_read_the_last_anchor_again", "loss_reduce_skips_the_last_block",
                  "slot_1_anchor_decoded_with_slot_2_size"]


def _toy_heads(case):
    """random head planes with loss_cases.SATURATE's values; one stride-8 anchor of the untouched slot has raw box
    predictions 0, so its box is exact: centre 8 x + 4, sides 33 x 23"""
    rng = np.random.default_rng(case["seed"])
    P = 5 + case["C"]
    preds = []
    for i, s in enumerate((32, 16, 8)):
        p = (rng.standard_normal((case["B"], 3 * P, case["H"] // s, case["W"] // s)) * 1.5).astype(F32)
        for (si, slot), chans in L.SATURATE.items():
            if si == i:
                for ch, v in chans.items():
                    p[:, slot * P + ch] += F32(v)
        preds.append(p)
    preds[2][0, 2 * P:2 * P + 4, 5, 7] = 0
    return preds


def _plane_rows(rows, preds, C):
    """(B, N, P) rows back into the head-plane layout"""
    out, n0 = [], 0
    for p in preds:
        B, _, H, W = p.shape
        n1 = n0 + 3 * H * W
        out.append(np.ascontiguousarray(rows[:, n0:n1].reshape(B, H * W, 3 * (5 + C)).transpose(0, 2, 1).reshape(p.shape)))
        n0 = n1
    return out


def dev_loss(case, preds, gt, tg, made, mut=None):
    """loss_kernel + loss_reduce_kernel in fp32 numpy (vy_math's exp / log through the oracle library): per-anchor terms
    in the kernel's operation order, the 256-lane butterfly per block, the blocks summed in double -> (losses (4, B),
    d(loss)/d(pred) planes)"""
    from oracle import yolo3_oracle as O
    from oracle.yolo3_train_oracle import OracleYolo3Train
    C, B, thresh = case["C"], case["B"], F32(case["thresh"])
    rows, _ = R.raw_layout(preds, C)
    N = rows.shape[1]
    obj_t, ctr_t, scl_t, wgt_t, cls_t = [np.asarray(t, F32) for t in tg]
    with np.errstate(over="ignore", invalid="ignore"):
        box = OracleYolo3Train(C, {}).split_preds(preds)["box"]
        best = np.fmax.reduce(O.batch_iou(box, gt), axis=-1, initial=F32(-1))
    pos = obj_t[..., 0] > 0
    ign = (best >= thresh) if mut == "ge_instead_of_gt_at_the_threshold" else (best > thresh)
    if mut == "above_threshold_anchor_taken_as_negative":
        b, n = next((b, n) for b, n, k, _ in made if k == "above")
        ign[b, n] = False
    objness = np.where(pos, obj_t[..., 0], np.where(ign, F32(-1), F32(0))).astype(F32)

    def bce(x, z):
        return ((np.maximum(x, F32(0)) - x * z).astype(F32) + O.log((F32(1) + O.exp(-np.abs(x))).astype(F32))).astype(F32)

    def sig(x):
        return O.sigmoid(np.ascontiguousarray(x, F32))

    hard = np.where(objness > 0, F32(1), objness)
    omask = np.where(objness > 0, F32(1) if mut == "omask_not_scaled_by_fractional_obj_t" else objness,
                     (objness >= 0).astype(F32)).astype(F32)
    ro = rows[..., 4]
    t = np.zeros((4, B, N), F32)
    d = np.zeros_like(rows)
    t[0] = bce(ro, hard) * omask
    d[..., 4] = (sig(ro) - hard) * omask
    scale = F32(1) if mut == "box_weights_not_scaled_by_fractional_obj_t" else objness
    w = np.where(pos[..., None], wgt_t * scale[..., None], F32(0)).astype(F32)
    l0, l1 = bce(rows[..., 0], ctr_t[..., 0]) * w[..., 0], bce(rows[..., 1], ctr_t[..., 1]) * w[..., 1]
    t[1] = (l0.astype(F32) + l1.astype(F32)).astype(F32)
    d[..., 0:2] = (sig(rows[..., 0:2]) - ctr_t) * w
    diff = (rows[..., 2:4] - scl_t).astype(F32)
    t[2] = ((np.abs(diff[..., 0]) * w[..., 0]).astype(F32) + (np.abs(diff[..., 1]) * w[..., 1]).astype(F32)).astype(F32)
    zero = w if mut == "zero_scale_difference_given_gradient_plus_w" else F32(0)
    d[..., 2:4] = np.where(diff > 0, w, np.where(diff < 0, -w, zero))
    sm = F32(1) / F32(40) if mut == "smoothing_constant_1_40_at_80_classes" else min(F32(1) / F32(C), F32(1) / F32(40))
    ct = cls_t
    if case["smooth"]:
        ct = np.where(ct > F32(0.5), (ct - sm).astype(F32), ct)
        ct = np.where((ct < F32(-0.5)) | (ct > F32(0.5)), ct, sm).astype(F32)
    cm = np.where(pos[..., None], (ct >= 0).astype(F32) * objness[..., None], F32(0)).astype(F32)
    lc = (bce(rows[..., 5:], ct) * cm).astype(F32)
    acc = np.zeros((B, N), F32)
    for c in range(C):
        acc = (acc + lc[..., c]).astype(F32)
    t[3] = acc
    d[..., 5:] = (sig(rows[..., 5:]) - ct) * cm
    if mut == "anchor_term_dropped":  # a plain negative of the untouched slot, in the third block
        n = next(n for n in range(512, 768) if objness[1, n] == 0 and (n - 240) % 3 == 2)
        t[:, 1, n] = 0
    # the block tree
    nb = -(-N // 256)
    lanes = np.zeros((4, B, nb * 256), F32)
    lanes[..., :N] = t
    if mut == "tail_lanes_read_the_last_anchor_again":
        lanes[..., N:] = t[..., N - 1:N]
    v = lanes.reshape(4, B, nb, 4, 64)
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., idx ^ off]).astype(F32)
    r = v[..., 0]
    part = ((r[..., 0] + r[..., 1]).astype(F32) + (r[..., 2] + r[..., 3]).astype(F32)).astype(F32)  # (4, B, nb)
    if mut == "loss_reduce_skips_the_last_block":
        part = part[..., :-1]
    return part.astype(np.float64).sum(-1).astype(F32), _plane_rows(d, preds, C)


def dev_raw_preds(preds, C, mut=None):
    """raw_preds_kernel in fp32 numpy"""
    from oracle import yolo3_oracle as O
    rows, geo = R.raw_layout(preds, C)
    gx, gy, stride, aw, ah = [geo[:, i].astype(F32)[None] for i in range(5)]
    if mut == "slot_1_anchor_decoded_with_slot_2_size":
        aw = aw.copy()
        aw[0, 1::3] = aw[0, 2::3]
    sg = lambda v: O.sigmoid(np.ascontiguousarray(v, F32))  # noqa: E731
    ex = lambda v: O.exp(np.ascontiguousarray(v, F32))  # noqa: E731
    with np.errstate(over="ignore"):
        cx, cy = ((sg(rows[..., 0]) + gx).astype(F32) * stride).astype(F32), ((sg(rows[..., 1]) + gy).astype(F32) * stride).astype(F32)
        hw, hh = ((ex(rows[..., 2]) * aw).astype(F32) / F32(2)).astype(F32), ((ex(rows[..., 3]) * ah).astype(F32) / F32(2)).astype(F32)
        box = np.stack([cx - hw, cy - hh, cx + hw, cy + hh], -1).astype(F32)
    return box, rows[..., 0:2], rows[..., 2:4], rows[..., 4:5], rows[..., 5:]


@pytest.fixture(scope="module")
def toy_loss_case():
    from oracle.yolo3_train_oracle import OracleYolo3Train
    case = TOY
    preds = _toy_heads(case)
    with np.errstate(over="ignore"):
        pr = OracleYolo3Train(case["C"], {}).split_preds(preds)
    gt, tg, made = L.construct(case, pr["box"], pr["wh"], pr["obj"])
    # a gt row whose IoU with the exact anchor is 0.5 = the threshold in every fp32 step: the left half of its box
    n = 3 * (4 * 4 + 8 * 8) + (5 * 16 + 7) * 3 + 2
    assert pr["box"][0, n].tolist() == [60 - 16.5, 44 - 11.5, 60 + 16.5, 44 + 11.5] and not tg[0][0, n, 0] > 0
    gt[0, case["valid"]] = [60 - 16.5, 44 - 11.5, 60, 44 + 11.5]
    terms = R.loss_terms64(case["C"], preds, gt, tg, case["thresh"], case["smooth"])
    assert terms["ious_max"][0, n] == F32(0.5) and terms["decision"][0, n] == 0 and not terms["exempt"][0, n]
    L.conditions(case, terms, made)
    want = R.head_grads(case["C"], preds, gt, tg, case["thresh"], case["smooth"])
    return case, preds, gt, tg, made, terms, want


def _run_loss(toy, mut=None):
    case, preds, gt, tg, made, terms, (want, exempt) = toy
    losses, dpred = dev_loss(case, preds, gt, tg, made, mut)
    res = R.check_losses("toy", losses, terms)
    res += [R.check_head_grad("head %d" % i, dpred[i], want[i], exempt[i]) for i in range(3)]
    res += R.check_raw_preds("toy", preds, *dev_raw_preds(preds, case["C"], mut))
    return res


def test_loss_restatement_passes_every_check(toy_loss_case):
    res = _run_loss(toy_loss_case)
    bad = [r for r in res if not r.ok]
    assert not bad, bad
    for r in res:
        print(r)
    assert len([r for r in res if r.kind == "loss value"]) == 4 and all(np.isfinite(r.ratio) for r in res)


@pytest.mark.parametrize("mut", LOSS_MUTATIONS)
def test_every_loss_mutation_fails_a_check(toy_loss_case, mut):
    res = _run_loss(toy_loss_case, mut)
    bad = [r for r in res if not r.ok]
    assert bad and all(r.ratio > 1 for r in bad), "mutation %s passed every check" % mut
    kinds = {"zero_scale_difference_given_gradient_plus_w": "loss gradient",
             "slot_1_anchor_decoded_with_slot_2_size": "decoded boxes"}
    assert kinds.get(mut, "loss value") in {r.kind for r in bad}, (mut, bad)
    print("%s: fails %s, worst err/bound %.3g" % (mut, sorted(set(r.name for r in bad)), max(r.ratio for r in bad)))


@pytest.mark.parametrize("case", L.CASES + [L.CAP_CASE], ids=L.case_id)
def test_census_conditions_of_the_constructed_cases_hold_on_the_oracle(case):
    """The device's raw head predictions are bit-equal to the oracle's train-mode forward on the same inputs, so the
    construction the GPU test makes from the device's boxes is this one: its conditions are settled here."""
    from oracle.yolo3_train_oracle import OracleYolo3Train
    C = case["C"]
    preds = L.oracle_heads_forward(C, L.heads_params(C), L.routes(case["B"], case["H"], case["W"], case["seed"]))
    with np.errstate(over="ignore"):
        pr = OracleYolo3Train(C, {}).split_preds(preds)
    gt, tg, made = L.construct(case, pr["box"], pr["wh"], pr["obj"])
    terms = R.loss_terms64(C, preds, gt, tg, case["thresh"], case["smooth"])
    print(L.case_id(case), L.conditions(case, terms, made))
    assert np.isinf(pr["box"]).any() and not np.isnan(pr["box"]).any() and np.isfinite(terms["terms"]).all()
    assert (gt[:, case["valid"]:case["M"] - 1] == -1).all()           # -1 padding behind the valid rows


# sgd_kernel in fp32 numpy: 4 steps on toy segments of 21 and 21 x 64 elements, multipliers changed before step 3
SGD_MUTATIONS = ["lr_mult_ignored", "wd_applied_with_wd_mult_0", "momentum_reset_at_the_multiplier_change",
                 "last_size_mod_4_elements_not_updated"]


def _run_sgd(mut=None):
    rng = np.random.default_rng(3)
    lr, mu, wd, resc = F32(1e-3), F32(0.9), F32(5e-4), F32(1.0 / 3)
    segs = {"bias": 21, "weight": 21 * 64, "gamma": 512, "frozen": 64}
    mult = {"bias": (10.0, 0.0), "weight": (0.1, 1.0), "gamma": (0.0, 1.0), "frozen": (1.0, 1.0)}
    enabled = {n: n != "frozen" for n in segs}
    w = {n: rng.standard_normal(s).astype(F32) for n, s in segs.items()}
    m = {n: np.zeros(s, F32) for n, s in segs.items()}
    refs = {n: R.SgdRef((s,)) for n, s in segs.items()}
    res = []
    for step in range(1, 5):
        if step == 3:
            mult.update(bias=(1.0, 1.0), weight=(10.0, 0.0), gamma=(1.0, 0.0))
            enabled.update(frozen=True, gamma=True)
            if mut == "momentum_reset_at_the_multiplier_change":
                m = {n: np.zeros_like(v) for n, v in m.items()}
        for n, s in segs.items():
            g = rng.standard_normal(s).astype(F32)
            before = w[n].copy()
            if enabled[n]:
                lm, wm = mult[n]
                lr_k = lr if mut == "lr_mult_ignored" else (lr * F32(lm)).astype(F32)
                wd_k = wd if mut == "wd_applied_with_wd_mult_0" else (wd * F32(wm)).astype(F32)
                gg = ((g * resc).astype(F32) + (wd_k * w[n]).astype(F32)).astype(F32)
                mm = ((mu * m[n]).astype(F32) - (lr_k * gg).astype(F32)).astype(F32)
                upd = slice(0, s - s % 4) if mut == "last_size_mod_4_elements_not_updated" else slice(None)
                m[n][upd] = mm[upd]
                w[n][upd] = (w[n] + mm).astype(F32)[upd]
            res.append(refs[n].step("%s step %d" % (n, step), before, g, w[n], lr, mu, wd, resc, mult[n][0], mult[n][1],
                                    enabled[n]))
    return res


def test_sgd_restatement_passes_every_check():
    res = _run_sgd()
    assert all(r.ok for r in res), [r for r in res if not r.ok]
    assert {r.kind for r in res} == {"sgd step", "sgd frozen", "sgd lr_mult 0"}
    assert max(r.ratio for r in res if r.kind == "sgd step") > 0.01   # the bound is within two orders of the error


@pytest.mark.parametrize("mut", SGD_MUTATIONS)
def test_every_sgd_mutation_fails_a_check(mut):
    bad = [r for r in _run_sgd(mut) if not r.ok]
    assert bad and all(r.ratio > 1 for r in bad), "mutation %s passed every check" % mut
    print("%s: fails %s" % (mut, sorted(set(r.name for r in bad))[:6]))
