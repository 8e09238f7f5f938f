"""-m "not gpu": a hierarchical net over a whole video on the host — the identity hier_detect_video rests on, in numpy
(tests/hier_video_model.py) on the chunks of video.hier_video_chunks; the chunks' counts and clamped frame indices; the
codes of the hier-video entries and of the entries around them; the region table of the hier-video plan.  Nothing here
launches a kernel."""
import ctypes

import numpy as np
import pytest

import hier_video_model as M
import ws_guard as G
from videoyolo_amd import _lib, video

C20 = ["c%d" % i for i in range(20)]


def _make(lib, n_pools, join=_lib.VY_HJOIN_MAX):
    h = ctypes.c_void_p()
    if n_pools:
        _lib.check(lib.vy_net_create_hier_join(20, n_pools, join, ctypes.byref(h)))
    else:
        _lib.check(lib.vy_net_create(20, ctypes.byref(h)))
    return h


# ------------------------------------------------------------------------------------------------ the identity
@pytest.mark.parametrize("join", ["max", "filter"])
@pytest.mark.parametrize("pools", [1, 2, 3, 4])
def test_chunks_of_dilated_joins_are_the_clips(pools, join):
    """Level n at position i, built from dilated triples over the clamped level-0 frames, is bit for bit what the clip
    window_indices(N, T, step)[i] gives — with the max and with a join that is sensitive to the order of its operands."""
    rng = np.random.default_rng(100 * pools + len(join))
    checked = 0
    for step in (1, 2, 3):
        for n in (1, 2, 5, 20, 23):
            frames = rng.standard_normal((n, 6)).astype(np.float32)
            frames[rng.integers(0, n)] = frames[0]  # ties between frames exist too
            want = M.clip_path(frames, pools, step, join)
            assert want.shape == (n, 6)
            for f in (1, 4, 16):
                got = M.chunk_path(frames, pools, step, f, join)
                assert got.dtype == want.dtype and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (step, n, f)
                checked += 1
            if n >= 5 and join == "filter":
                assert len(np.unique(want, axis=0)) > 1  # the frames differ: the equality is not vacuous
    assert checked == 45


def test_the_filter_join_is_order_sensitive_and_the_max_keeps_the_earliest():
    a, b, c = (np.float32(v) * np.ones(3, np.float32) for v in (1.0, 2.0, 3.0))
    assert not np.array_equal(M.join_filter(a, b, c), M.join_filter(c, b, a))
    assert not np.array_equal(M.join_filter(a, b, c), M.join_filter(b, a, c))
    pz, nz = np.zeros(1, np.float32), -np.zeros(1, np.float32)
    assert not np.signbit(M.join_max(pz, nz, nz))[0] and np.signbit(M.join_max(nz, pz, pz))[0]


# ------------------------------------------------------------------------------------------------ counts and indices
@pytest.mark.parametrize("pools,step,f", [(1, 1, 4), (2, 1, 4), (2, 2, 16), (3, 1, 16), (4, 1, 2), (3, 3, 1)])
def test_counts_and_clamped_frame_indices(pools, step, f):
    t = 3 ** pools
    reach = [step * (3 ** level - 1) // 2 for level in range(pools + 1)]
    assert [video.hier_reach(pools, step, level) for level in range(pools + 1)] == reach
    n = 2 * f + 3  # three chunks, the last one short
    chunks, counts = video.hier_video_chunks(n, pools, step, f)
    assert counts == [f + 2 * (reach[-1] - r) for r in reach]
    assert counts[0] == f + step * (t - 1) and counts[-1] == f
    assert [c for c, _ in chunks] == [list(range(a, min(a + f, n))) for a in range(0, n, f)]
    table = video.window_indices(n, t, step)
    for centres, index in chunks:
        a = centres[0]
        assert index.dtype == np.int64 and len(index) == counts[0]
        assert np.array_equal(index, np.clip(np.arange(a - reach[-1], a + f + reach[-1]), 0, n - 1))
        # the frames of centre i's clip are the level-0 positions i - h_n + t * step of the chunk
        for i in centres:
            assert np.array_equal(index[(i - a) + np.arange(t) * step], table[i])
    first, last = chunks[0][1], chunks[-1][1]
    assert (first[:reach[-1] + 1] == 0).all() and first[reach[-1] + 1] == min(1, n - 1)  # clamped at the start ...
    assert last[-1] == n - 1 and (last[-(reach[-1] + 1):] == n - 1).all()  # ... and at the end, padding included
    # the library's own count
    lib = _lib.load()
    h = _make(lib, pools)
    try:
        got = ctypes.c_int32(-1)
        _lib.check(lib.vy_net_hier_video_frames(h, f, step, ctypes.byref(got)))
        assert got.value == counts[0]
    finally:
        lib.vy_net_destroy(h)


def test_a_one_frame_video_is_one_chunk_of_that_frame():
    chunks, counts = video.hier_video_chunks(1, 3, 2, 4)
    assert len(chunks) == 1 and chunks[0][0] == [0] and not chunks[0][1].any() and len(chunks[0][1]) == counts[0] == 4 + 52


@pytest.mark.parametrize("args", [(0, 2, 1, 4), (5, 0, 1, 4), (5, 5, 1, 4), (5, 2, 0, 4), (5, 2, 1, 0), (5, 2, 65, 4),
                                  (5, 2, 1, 513)])
def test_chunks_check_their_arguments(args):
    with pytest.raises(ValueError, match="hier_video_chunks"):
        video.hier_video_chunks(*args)


# ------------------------------------------------------------------------------------------------ codes
def test_hier_video_entries_refuse_other_nets_before_touching_anything():
    """VY_ERR_STATE on a single-frame and on a window net, the bogus pointers never dereferenced; the sizing query 0"""
    lib = _lib.load()
    p = ctypes.c_void_p(0x1000)
    single = _make(lib, 0)
    win = ctypes.c_void_p()
    _lib.check(lib.vy_net_create_window(20, 3, _lib.VY_JOIN_MAX, ctypes.byref(win)))
    try:
        for h in (single, win):
            n = ctypes.c_int32(-7)
            assert lib.vy_net_hier_video_frames(h, 4, 1, ctypes.byref(n)) == -2 and n.value == -7
            assert "hierarchical" in lib.vy_last_error().decode()
            assert lib.vy_net_hier_video_workspace_bytes(h, 4, 1, 64, 64) == 0
            assert lib.vy_net_bind_hier_video(h, p, 1 << 30, 4, 1, 64, 64, None) == -2
            assert lib.vy_net_hier_video_detect(h, p, p, p, p, None, None) == -2
            assert "not bound" not in lib.vy_last_error().decode()
            r = _lib.PlanRegion()
            assert lib.vy_net_plan_region(h, _lib.VY_PLAN_HIER_VIDEO, 4, 64, 64, 1, 0, 0, ctypes.byref(r)) == -1
        assert lib.vy_net_hier_video_frames(None, 4, 1, None) == -1
    finally:
        lib.vy_net_destroy(single)
        lib.vy_net_destroy(win)


@pytest.mark.parametrize("join", [_lib.VY_HJOIN_MAX, _lib.VY_HJOIN_CONV])
def test_hierarchical_handles_keep_their_other_refusals_and_check_the_new_arguments(join):
    lib = _lib.load()
    h = _make(lib, 2, join)
    p = ctypes.c_void_p(0x1000)
    tab = (ctypes.c_int32 * 6)(0, 1, 2, 3, 4, 5)
    try:
        # the window net's video entries still refuse a hierarchical handle
        for fn, args in ((lib.vy_net_video_push, (p, tab, None)), (lib.vy_net_video_detect, (tab, p, p, p, None, None)),
                         (lib.vy_net_video_read_slot, (0, p, p, p, None)),
                         (lib.vy_net_bind_video, (p, 1 << 30, 4, 2, 8, 64, 64, None))):
            assert fn(h, *args) == -2, fn.__name__
        assert lib.vy_net_video_workspace_bytes(h, 4, 2, 8, 64, 64) == 0
        # the new ones get as far as the state of the net ...
        assert lib.vy_net_hier_video_detect(h, p, p, p, p, None, None) == -2
        assert "not bound" in lib.vy_last_error().decode()
        assert lib.vy_net_hier_video_detect(h, None, p, p, p, None, None) == -1
        # ... and refuse bad shapes: the sizing query with 0, the bind and the count with VY_ERR_INVALID
        n = ctypes.c_int32(0)
        for centres, step, hh, ww in ((0, 1, 64, 64), (513, 1, 64, 64), (4, 0, 64, 64), (4, 65, 64, 64), (4, 1, 16, 64),
                                      (4, 1, 64, 5000)):
            assert lib.vy_net_hier_video_workspace_bytes(h, centres, step, hh, ww) == 0, (centres, step, hh, ww)
            assert lib.vy_last_error().decode()
            assert lib.vy_net_bind_hier_video(h, p, 1 << 40, centres, step, hh, ww, None) == -1
        assert lib.vy_net_hier_video_frames(h, 0, 1, ctypes.byref(n)) == -1
        assert lib.vy_net_hier_video_frames(h, 4, 0, ctypes.byref(n)) == -1
        assert lib.vy_net_hier_video_frames(h, 4, 1, None) == -1
        assert lib.vy_net_bind_hier_video(h, None, 1 << 30, 4, 1, 64, 64, None) == -1
        assert lib.vy_net_hier_video_workspace_bytes(h, 4, 1, 64, 64) > 0
    finally:
        lib.vy_net_destroy(h)


def test_python_surface():
    import videoyolo_amd as vy
    net = vy.yolo3_darknet53(C20, pretrained_base=False, new_model=True, hierarchical=[3, 3, 1, 1, 1], h_join_type="max")
    conv = vy.YOLOV3HierConv(C20, hierarchical=[3, 1, 1, 1, 1])
    for m in (net, conv):
        assert not hasattr(m, "video") and not hasattr(m, "detect_video")  # the pinned surface of the class stands
        with pytest.raises(ValueError, match=r"\(n, 3, H, W\)"):
            vy.hier_detect_video(m, np.zeros((2, 9, 3, 64, 64), np.float32))
        with pytest.raises(ValueError, match=r"\(n, 3, H, W\)"):
            vy.hier_detect_video(m, np.zeros((0, 3, 64, 64), np.float32))
        with pytest.raises(ValueError, match="hier_video_chunks"):
            vy.hier_detect_video(m, np.zeros((2, 3, 64, 64), np.float32), step=0)
        with pytest.raises(RuntimeError, match="not on a device"):
            vy.hier_detect_video(m, np.zeros((2, 3, 64, 64), np.float32))
    assert vy.hier_detect_video is vy.video.hier_detect_video and "hier_detect_video" in vy.__all__
    for other in (vy.yolo3_darknet53(C20, pretrained_base=False),
                  vy.yolo3_darknet53(C20, pretrained_base=False, k=3, k_join_type="max", k_join_pos="early")):
        with pytest.raises(TypeError, match="hierarchical"):
            vy.hier_detect_video(other, np.zeros((2, 3, 64, 64), np.float32))


def test_more_than_one_rank_is_refused(monkeypatch):
    import videoyolo_amd as vy
    from videoyolo_amd import parallel
    monkeypatch.setattr(parallel, "world_size", lambda: 2)
    net = vy.YOLOV3Hier(C20, hierarchical=[3, 1, 1, 1, 1])
    with pytest.raises(NotImplementedError, match="one rank"):
        vy.hier_detect_video(net, np.zeros((2, 3, 64, 64), np.float32))


# ------------------------------------------------------------------------------------------------ the region table
def _regions(lib, h, centres, step, hh, ww):
    table, r = [], _lib.PlanRegion()
    while True:
        rc = lib.vy_net_plan_region(h, _lib.VY_PLAN_HIER_VIDEO, centres, hh, ww, step, 0, len(table), ctypes.byref(r))
        if rc == _lib.VY_ERR_RANGE:
            break
        _lib.check(rc)
        table.append((r.name.decode(), int(r.offset), int(r.bytes), int(r.span)))
    return table


@pytest.mark.parametrize("guard", [0, G.GUARD])
@pytest.mark.parametrize("pools", [1, 2, 3, 4])
def test_region_table_of_the_hier_video_plan(monkeypatch, pools, guard):
    """check_table on the plan's table at step 1 and 2 and two sizes; every plane holds the positions of its level: its bytes
    are the bytes of one frame of that plane (the clip plan at one clip holds fm of them) times centres + step (T - T / fm)"""
    monkeypatch.setenv("VY_PLAN_GUARD", str(guard))
    lib = _lib.load()
    t = 3 ** pools
    for join in (_lib.VY_HJOIN_MAX, _lib.VY_HJOIN_CONV):
        h = _make(lib, pools, join)
        try:
            for keep in (0, 1):
                _lib.check(lib.vy_net_set_keep_activations(h, keep))
                for step in (1, 2):
                    for centres, hh, ww in ((4, 64, 64), (3, 40, 72)):
                        table = _regions(lib, h, centres, step, hh, ww)
                        G.check_table(table, int(lib.vy_net_hier_video_workspace_bytes(h, centres, step, hh, ww)))
                        assert all(span - used >= guard for _, _, used, span in table)
                        clip = {name: used for name, _, used, _ in G.regions(lib, h, "clip", (1, hh, ww))}
                        planes = [(name, used) for name, _, used, _ in table if name.startswith("plane:")]
                        assert [n for n, _ in planes] == [n for n in clip if n.startswith("plane:")]
                        levels = set()
                        for name, used in planes:
                            fm = ctypes.c_int32(0)
                            _lib.check(lib.vy_net_tap_frames(h, name[len("plane:"):].encode(), ctypes.byref(fm)))
                            assert clip[name] % fm.value == 0
                            count = centres + step * (t - t // fm.value)
                            assert used == clip[name] // fm.value * count, (name, fm.value, used)
                            levels.add(fm.value)
                        assert levels == {3 ** k for k in range(pools + 1)}
                        # everything that is no plane is sized for `centres` clips, as the clip plan at that batch
                        at_b = {name: used for name, _, used, _ in G.regions(lib, h, "clip", (centres, hh, ww))}
                        for name, _, used, _ in table:
                            if not name.startswith("plane:") and name != "ck":
                                assert used == at_b[name], name
        finally:
            lib.vy_net_destroy(h)
