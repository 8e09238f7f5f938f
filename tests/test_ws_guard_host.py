"""-m "not gpu": the guard switch of the planners (VY_PLAN_GUARD), the region table (vy_net_plan_region) and the checker
of tests/ws_guard.py, without a device.

Invariants, for every kind of net and conv mode of tests/test_plan_host.py plus the hierarchical net with one and four
pools, at three clip / training shapes and one video plan: the table is ascending, aligned, disjoint and ends at the
matching size query; with a guard every region sits at its guard-0 offset plus the gaps in front of it, uses the bytes
it used, and the total grows by regions x guard.  Sensitivity: the checker, on a numpy buffer laid out by a real table,
reports each planted fault against the region in front of it and nothing on an untouched buffer.
"""
import ctypes

import numpy as np
import pytest

import test_plan_host as P
import ws_guard as G
from videoyolo_amd import _lib

GUARD = 4096
KINDS = list(P.KINDS) + ["hier1", "hier4"]


def _create(lib, kind, classes=20):
    if not kind.startswith("hier"):
        return P._create(lib, kind, classes)
    h = ctypes.c_void_p()
    _lib.check(lib.vy_net_create_hier(classes, int(kind[4:]), ctypes.byref(h)))
    return h


def _plans(kind):
    """(plan, shape) of every table a net of this kind has at the test's shapes"""
    out = [(p, s) for s in P.SHAPES[:3] for p in ("clip", "train")]
    if kind.startswith("window"):
        out += [("video", P.VIDEO[0] + s[1:]) for s in P.SHAPES[:3]]
    return out


def _tables(lib, monkeypatch, kind, mode, st, guard):
    monkeypatch.delenv("VY_SPLIT_TRAIN", raising=False)
    if st is not None:
        monkeypatch.setenv("VY_SPLIT_TRAIN", str(st))
    monkeypatch.setenv("VY_PLAN_GUARD", str(guard))
    h = _create(lib, kind)
    out = {}
    try:
        _lib.check(lib.vy_net_set_conv_mode(h, mode))
        for keep in (0, 1):
            _lib.check(lib.vy_net_set_keep_activations(h, keep))
            for plan, shape in _plans(kind):
                if G.plan_bytes(lib, h, plan, shape) == 0:  # (a training shape that is no multiple of 32: refused)
                    r = _lib.PlanRegion()
                    assert lib.vy_net_plan_region(h, G.PLANS[plan], *shape, 0, 0, 0, ctypes.byref(r)) == -1  # VY_ERR_INVALID
                    continue
                out[(keep, plan, shape)] = (G.regions(lib, h, plan, shape), G.plan_bytes(lib, h, plan, shape))
    finally:
        lib.vy_net_destroy(h)
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_every_region_keeps_its_bytes_and_moves_by_the_gaps_in_front_of_it(kind, monkeypatch):
    lib = _lib.load()
    exact_only = kind.startswith(("window", "hier"))
    seen = set()
    for mode, st in P.MODES:
        if exact_only and mode != _lib.VY_CONV_EXACT_FP32:
            continue
        plain = _tables(lib, monkeypatch, kind, mode, st, 0)
        guarded = _tables(lib, monkeypatch, kind, mode, st, GUARD)
        assert plain and sorted(plain) == sorted(guarded)
        for key, (t0, total0) in plain.items():
            t1, total1 = guarded[key]
            assert [r[0] for r in t0] == [r[0] for r in t1], key
            for i, ((name, off0, used0, span0), (_, off1, used1, span1)) in enumerate(zip(t0, t1)):
                assert off1 == off0 + i * GUARD and used1 == used0 and span1 == span0 + GUARD, (key, name)
                assert span0 < used0 + 256, (key, name, "a guard-0 region is followed by its rounding slack alone")
            assert total1 == total0 + len(t0) * GUARD, key
            seen |= {r[0].split(":")[0] for r in t0}
    # the tables name what the plans carve: every kind of region this net can have has been met
    want = {"fold", "det.state", "det.hist", "det.entries", "det.list", "det.score", "sk.flags", "sk.slabs", "ck", "plane", "grad",
            "z", "wgrad_table", "train.save", "train.coef", "train.sums", "train.slices", "train.part", "train.slab",
            "train.loss_part", "train.loss", "train.zero", "train.sdesc", "train.seg", "train.chunk"}
    if kind.startswith("window"):
        want |= {"ring"}
    if not exact_only:
        want |= {"wsplit", "wino", "dgrad_image"}
    assert seen == want, (sorted(seen - want), sorted(want - seen))


def test_the_switch_takes_multiples_of_256_up_to_one_mebibyte(monkeypatch):
    lib = _lib.load()

    def total(value):
        if value is None:
            monkeypatch.delenv("VY_PLAN_GUARD", raising=False)
        else:
            monkeypatch.setenv("VY_PLAN_GUARD", value)
        h = _create(lib, "full")
        try:
            return lib.vy_net_workspace_bytes(h, 1, 64, 64), len(G.regions(lib, h, "clip", (1, 64, 64)))
        finally:
            lib.vy_net_destroy(h)

    base, n = total(None)
    for bad in ("0", "-256", "100", "4097", str((1 << 20) + 256), "x"):
        assert total(bad) == (base, n), bad
    for good in (256, 4096, 1 << 20):
        assert total(str(good)) == (base + n * good, n), good


def test_the_switch_is_per_net(monkeypatch):
    lib = _lib.load()
    monkeypatch.setenv("VY_PLAN_GUARD", "4096")
    a = _create(lib, "full")
    monkeypatch.delenv("VY_PLAN_GUARD")
    b = _create(lib, "full")
    try:
        assert lib.vy_net_workspace_bytes(a, 1, 64, 64) > lib.vy_net_workspace_bytes(b, 1, 64, 64)
    finally:
        lib.vy_net_destroy(a)
        lib.vy_net_destroy(b)


# ---------------------------------------------------------------- the checker's sensitivity
BAND = 1024


@pytest.fixture(scope="module")
def laid_out():
    """(table, buffer): a real training table under the guard and a host buffer laid out by it — bands and holes poison,
    the used bytes zero"""
    import os
    lib = _lib.load()
    old = os.environ.get("VY_PLAN_GUARD")
    os.environ["VY_PLAN_GUARD"] = str(GUARD)
    try:
        h = _create(lib, "full", 3)
    finally:
        if old is None:
            del os.environ["VY_PLAN_GUARD"]
        else:
            os.environ["VY_PLAN_GUARD"] = old
    try:
        table = G.regions(lib, h, "train", (1, 64, 64))
    finally:
        lib.vy_net_destroy(h)
    total = table[-1][1] + table[-1][3]
    buf = G.pattern(0, BAND + total + BAND).copy()
    for _, off, used, _ in table:
        buf[BAND + off:BAND + off + used] = 0
    return table, buf


def _region(table, name):
    return next(r for r in table if r[0] == name)


def test_an_untouched_buffer_reports_nothing(laid_out):
    table, buf = laid_out
    assert any(span - used > GUARD for _, _, used, span in table), "no region of the table has rounding slack"
    assert G.violations(buf, table, BAND) == []
    assert G.gap_bytes(table) >= len(table) * GUARD


def test_one_byte_behind_a_regions_used_end_in_the_slack(laid_out):
    table, buf = laid_out
    name, off, used, span = next(r for r in table if r[3] - r[2] > GUARD and r[0].startswith("train."))
    b = buf.copy()
    b[BAND + off + used] ^= 0xFF
    assert G.violations(b, table, BAND) == [(name, 0, 1)]


def test_one_byte_in_the_middle_of_a_gap(laid_out):
    table, buf = laid_out
    name, off, used, span = _region(table, "wgrad_table:yolo_blocks.0.body.2")
    b = buf.copy()
    at = off + span - GUARD // 2
    b[BAND + at] = 0
    assert G.violations(b, table, BAND) == [(name, at - off - used, 1)]


def test_a_word_at_either_band(laid_out):
    table, buf = laid_out
    total = table[-1][1] + table[-1][3]
    b = buf.copy()
    b[BAND - 4:BAND] = 0
    b[BAND + total:BAND + total + 4] = 0
    name, off, used, span = table[-1]
    assert G.violations(b, table, BAND) == [("<front band>", -4, 4), (name, span - used, 4)]


def test_another_nan_payload_is_not_poison(laid_out):
    table, buf = laid_out
    name, off, used, span = _region(table, "z:stages.1.0")
    at = off + span - 256
    b = buf.copy()
    b[BAND + at:BAND + at + 4] = np.frombuffer(np.uint32(0x7FC00000).tobytes(), np.uint8)
    got = G.violations(b, table, BAND)
    assert len(got) == 1 and got[0][0] == name and at - off - used <= got[0][1] < at - off - used + 4 and 1 <= got[0][2] <= 4


def test_a_table_with_two_overlapping_regions_is_refused(laid_out):
    table, buf = laid_out
    i = len(table) // 2
    name, off, used, span = table[i]
    bad = table[:i] + [(name, off - 256, used, span + 256)] + table[i + 1:]
    with pytest.raises(AssertionError, match="overlaps"):
        G.violations(buf, bad, BAND)
    with pytest.raises(AssertionError, match="overlaps"):
        G.check_table(bad, table[-1][1] + table[-1][3])
