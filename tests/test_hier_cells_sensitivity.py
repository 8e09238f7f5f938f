"""-m "not gpu": the checks tests/test_gpu_hier.py holds the hierarchical net to are sharp.

A toy [3,3,1,1,1] step in numpy, B = 2 clips of T = 9 frames: a residual block output on the B * 9 frames (batch
statistics, apply with the skip), the first pool into B * 3 frames, the stride-2 cell behind it (its statistics count
B * 3 * H * W, its data gradient lands on the pooled plane's gradient), the pool backward into the block output's
gradient plane, and the second pool into B frames with its own backward.  Some elements of the triples tie.  The "device"
side is the fp32 restatement of tests/test_train_cells64_sensitivity.py (frame-by-frame pool loops, a blocked data
gradient); it must pass every check, and each of the planted bugs must fail one."""
import numpy as np
import pytest

import test_train_cells64_sensitivity as S
from oracle import train_cells64 as R

F32 = np.float32

MUTATIONS = ["grouping_strided_instead_of_consecutive", "pooled_before_the_residual_add", "statistics_counted_over_B_not_B_fm",
             "backward_accumulates_instead_of_writing", "backward_to_the_first_tied_frame_only",
             "second_pool_grouping_strided", "nonzero_value_in_pooled_border"]


def _case():
    rng = np.random.default_rng(23)
    r = lambda *s: rng.standard_normal(s).astype(F32)  # noqa: E731
    B, T, C, H = 2, 9, 8, 12
    c = dict(B=B, T=T, C=C, H=H)
    # the block's raw conv output and its skip on the B * T frames; triples tie where the frames are copies of each other
    z, skip = r(B * T // 3, 3, C, H, H), r(B * T // 3, 3, C, H, H)
    tie2, tie3 = rng.random((B * T // 3, C, H, H)) < 0.15, rng.random((B * T // 3, C, H, H)) < 0.05
    for a in (z, skip):
        a[:, 1] = np.where(tie2 | tie3, a[:, 0], a[:, 1])
        a[:, 2] = np.where(tie3, a[:, 0], a[:, 2])
    c["z"], c["skip"] = z.reshape(B * T, C, H, H), skip.reshape(B * T, C, H, H)
    c["gam"], c["bet"] = (1 + 0.2 * r(C)).astype(F32), (0.3 * r(C)).astype(F32)
    # the stride-2 cell behind the first pool, on B * 3 frames
    c["w1"] = (r(2 * C, C, 3, 3) * 0.2).astype(F32)
    c["gam1"], c["bet1"] = (1 + 0.2 * r(2 * C)).astype(F32), (0.3 * r(2 * C)).astype(F32)
    c["dz1"] = r(B * 3, 2 * C, H // 2, H // 2)
    # its output gradient is the second pool's backward: the pooled gradient on B frames
    c["g2"] = r(B, 2 * C, H // 2, H // 2)
    c["stale"] = r(B * T, C, H, H)  # what the block output's gradient plane held before (an earlier step's values)
    return c


def _strided(frames_in):
    """frame of (pooled frame n of the flat axis, position t) when a clip's frames are grouped n, n + T/3, n + 2T/3"""
    def frame_of(n, t, n_out, k, per_clip=frames_in):
        clip, local = divmod(n, per_clip // 3)
        return clip * per_clip + local + t * (per_clip // 3)
    return frame_of


def _run(mut=None):
    from oracle import yolo3_oracle as O
    c = _case()
    B, T, C, H = c["B"], c["T"], c["C"], c["H"]
    res = []
    consecutive = lambda n, t, n_out, k: 3 * n + t  # noqa: E731
    # the block output on B * T frames: statistics over all of them, apply with the skip
    bn = S.dev_stats(c["z"], c["gam"], c["bet"])
    res.append(R.check_stats("block", c["z"], bn[0], bn[1], c["gam"], c["bet"], bn[2], bn[3]))
    act = R.leaky(R.fmaf(c["z"], bn[2].reshape(1, -1, 1, 1), bn[3].reshape(1, -1, 1, 1)))
    out = (act + c["skip"]).astype(F32)
    res.append(R.check_apply("block", c["z"], bn[2], bn[3], out, c["skip"]))
    # the first pool: B * T -> B * 3 frames, consecutive triples
    order = _strided(T) if mut == "grouping_strided_instead_of_consecutive" else consecutive
    if mut == "pooled_before_the_residual_add":
        pooled = (S.dev_pool(act, B * 3, 3, "max", order) + S.dev_pool(c["skip"], B * 3, 3, "max", order)).astype(F32)
    else:
        pooled = S.dev_pool(out, B * 3, 3, "max", order)
    res.append(R.check_pool_forward("hpool.0", out, 3, "max", pooled))
    p_pad = S.pad(pooled)
    if mut == "nonzero_value_in_pooled_border":
        p_pad[4, 3, 0, 5] = F32(1e-3)
    res.append(R.border_zero("borders", "hpool.0", p_pad))
    # the stride-2 cell on the B * 3 pooled frames: bit-equal conv, statistics over B * 3 * H * W
    z1 = O.conv2d(pooled, c["w1"], 2, 1)
    res.append(R.check_forward_conv("cell", pooled, c["w1"], 2, z1))
    bn1 = S.dev_stats(z1, c["gam1"], c["bet1"])
    if mut == "statistics_counted_over_B_not_B_fm":  # the sums run over every frame, the count is B * H * W
        z64 = z1.astype(np.float64)
        n = B * z1.shape[2] * z1.shape[3]
        mean = z64.sum(axis=(0, 2, 3)) / n
        var = np.maximum((z64 * z64).sum(axis=(0, 2, 3)) / n - mean * mean, 0)
        mf = mean.astype(F32)
        inv = (F32(1) / np.sqrt(var.astype(F32) + F32(1e-5))).astype(F32)
        sc = (c["gam1"] * inv).astype(F32)
        bn1 = np.stack([mf, inv, sc, R.fmaf(-mf, sc, c["bet1"])])
    res.append(R.check_stats("cell", z1, bn1[0], bn1[1], c["gam1"], c["bet1"], bn1[2], bn1[3]))
    out1 = R.leaky(R.fmaf(z1, bn1[2].reshape(1, -1, 1, 1), bn1[3].reshape(1, -1, 1, 1)))
    res.append(R.check_apply("cell", z1, bn1[2], bn1[3], out1))
    # the second pool: B * 3 -> B frames, and its backward into the cell's output gradient
    order2 = _strided(3 * B) if mut == "second_pool_grouping_strided" else consecutive
    pooled2 = S.dev_pool(out1, B, 3, "max", order2)
    res.append(R.check_pool_forward("hpool.1", out1, 3, "max", pooled2))
    g1 = S.dev_pool_bwd(c["g2"], out1, pooled2, B, 3, "max")
    r, wins2, ties2 = R.check_pool_backward("hpool.1", c["g2"], out1, pooled2, 3, "max", g1)
    res.append(r)
    # backward at the first pool: the cell's data gradient lands on the pooled plane's gradient ...
    g_pool = S.dev_dgrad(c["dz1"], c["w1"], 2, (H, H))
    res.append(R.check_dgrad("hpool.0", g_pool, [(c["dz1"], c["w1"], 2, 0)]))
    # ... and hier_pool_bwd WRITES the block output's gradient plane
    g_out = S.dev_pool_bwd(g_pool, out, pooled, B * 3, 3, "max",
                           "max_backward_to_first_maximal_frame_only" if mut == "backward_to_the_first_tied_frame_only" else None)
    if mut == "backward_accumulates_instead_of_writing":
        g_out = (c["stale"] + g_out).astype(F32)
    r, wins, ties = R.check_pool_backward("hpool.0", g_pool, out, pooled, 3, "max", g_out)
    res.append(r)
    return res, (wins, ties), (wins2, ties2)


def test_toy_hier_step_passes_every_check():
    res, (wins, ties), (wins2, ties2) = _run()
    bad = [r for r in res if not r.ok]
    assert not bad, bad
    # both kinds of element at the first pool: every frame position wins some on its own, and some are tied
    assert min(wins) > 0 and ties > 0, (wins, ties)
    assert min(wins2) > 0, (wins2, ties2)
    assert all(r.headroom < 50 for r in res)


def test_strided_grouping_differs_from_consecutive():
    """the planted grouping really is another one: clip 1's pooled frame 0 takes frames 9, 12, 15, not 9, 10, 11"""
    f = _strided(9)
    assert [f(0, t, 6, 3) for t in range(3)] == [0, 3, 6] and [f(3, t, 6, 3) for t in range(3)] == [9, 12, 15]
    assert [f(5, t, 6, 3) for t in range(3)] == [11, 14, 17]


@pytest.mark.parametrize("mut", MUTATIONS)
def test_every_planted_bug_fails_a_check(mut):
    res, _, _ = _run(mut)
    bad = [r for r in res if not r.ok]
    assert bad, "mutation %s passed every check" % mut
    want = {"grouping_strided_instead_of_consecutive": "pool forward", "pooled_before_the_residual_add": "pool forward",
            "statistics_counted_over_B_not_B_fm": "forward stats", "backward_accumulates_instead_of_writing": "pool backward",
            "backward_to_the_first_tied_frame_only": "pool backward", "second_pool_grouping_strided": "pool forward",
            "nonzero_value_in_pooled_border": "borders"}[mut]
    assert want in {r.kind for r in bad}, (mut, bad)
    print("%s: fails %s" % (mut, sorted(set(r.kind for r in bad))))
