"""-m "not gpu": a window net over a whole video, on the host — the clip table of the reference's loop
(datasets/imgnetvid.py:486-506) against tables worked out by hand, the session's frame -> slot bookkeeping replayed on a
fake backend that records slot writes and reads, and the C-ABI's refusals and sizing.  Nothing here launches a kernel."""
import ctypes

import numpy as np
import pytest

from videoyolo_amd import _lib
from videoyolo_amd.video import RingSchedule, min_ring, window_indices

SLOT_BYTES_416 = 4 * (52 * 52 * 256 + 26 * 26 * 512 + 13 * 13 * 1024)  # the three routes of one 416x416 frame
assert SLOT_BYTES_416 == 4845568


# ---------------------------------------------------------------------------------------------- the clip table
@pytest.mark.parametrize("n,k,step,want", [
    (5, 3, 1, [[0, 0, 1], [0, 1, 2], [1, 2, 3], [2, 3, 4], [3, 4, 4]]),
    (6, 4, 2, [[0, 0, 0, 2], [0, 0, 1, 3], [0, 0, 2, 4], [0, 1, 3, 5], [0, 2, 4, 5], [1, 3, 5, 5]]),
    (4, 5, 1, [[0, 0, 0, 1, 2], [0, 0, 1, 2, 3], [0, 1, 2, 3, 3], [1, 2, 3, 3, 3]]),
    (3, 2, 1, [[0, 0], [0, 1], [1, 2]]),
])
def test_window_indices_by_hand(n, k, step, want):
    got = window_indices(n, k, step)
    assert got.shape == (n, k) and np.issubdtype(got.dtype, np.integer)
    assert got.tolist() == want


def test_window_indices_properties():
    import videoyolo_amd as vy
    assert vy.window_indices is window_indices
    for k in range(2, 8):
        for step in range(1, 4):
            for n in range(1, 21):
                t = window_indices(n, k, step)
                assert t.shape == (n, k)
                assert np.array_equal(t[:, k // 2], np.arange(n)), (n, k, step)
                assert (np.diff(t, axis=1) >= 0).all(), (n, k, step)
                assert t.min() >= 0 and t.max() <= n - 1, (n, k, step)
    for bad in ((0, 3, 1), (4, 0, 1), (4, 3, 0)):
        with pytest.raises(ValueError):
            window_indices(*bad)


# ---------------------------------------------------------------------------------------------- ring bookkeeping
class FakeRing:
    """Stands in for the library: remembers which frame every slot holds, checks every read against the clip table."""

    def __init__(self, sched):
        self.s = sched
        self.slot = {}
        self.emitted = []
        self.reads = []  # (frame, [frames its clip read])
        self.pushes = self.detects = 0

    def run(self, ops):
        s = self.s
        n_emitted = 0
        for op, ids, table in ops:
            if op == "push":
                self.pushes += 1
                assert 1 <= len(ids) <= s.F and len(table) == s.F
                assert all(-1 <= v < s.R for v in table)
                assert all(v == -1 for v in table[len(ids):]), "padding frames must not be stored"
                stored = table[:len(ids)]
                assert len(set(stored)) == len(stored) and min(stored) >= 0
                for f, v in zip(ids, stored):
                    self.slot[v] = f
            else:
                self.detects += 1
                assert op == "detect" and 1 <= len(ids) <= s.B
                assert len(table) == s.B and all(len(r) == s.k for r in table)
                assert all(0 <= v < s.R for r in table for v in r)
                for f, row in zip(ids, table):
                    self.reads.append((f, [self.slot.get(v) for v in row]))
                self.emitted += ids
                n_emitted += len(ids)
        return n_emitted


def _replay(k, step, F, T, pieces=None):
    s = RingSchedule(k, step, F)
    assert s.R == min_ring(k, step, F) == F + (k - 1) * step
    fake = FakeRing(s)
    lag = (k - 1 - k // 2) * step
    done = 0
    for n in pieces or [T]:
        got = fake.run(s.push(n))
        done += n
        assert len(fake.emitted) == max(0, done - lag), "a push returns every frame whose look-ahead is stored"
        assert got == len(fake.emitted) - max(0, done - n - lag)
    fake.run(s.flush())
    assert (s.pushed, s.emitted) == (0, 0), "flush resets the session"
    want = window_indices(T, k, step)
    assert fake.emitted == list(range(T)), "every frame once, in order"
    for f, read in fake.reads:
        assert read == want[f].tolist(), (k, step, F, T, f, read)
    return fake


@pytest.mark.parametrize("k", range(2, 8))
@pytest.mark.parametrize("step", [1, 2, 3])
@pytest.mark.parametrize("F", [1, 4, 16])
def test_ring_schedule_reads_the_frames_the_table_names(k, step, F):
    for T in sorted({1, k - 1, F, 3 * F + 5}):
        fake = _replay(k, step, F, T)
        assert fake.pushes == -(-T // F)
    _replay(k, step, F, 3 * F + 5, pieces=[1, F + 1, F, F + 3])  # uneven pieces: the same clips
    # a ring one slot smaller than the default is refused at construction
    with pytest.raises(ValueError, match="too small"):
        RingSchedule(k, step, F, ring=min_ring(k, step, F) - 1)
    assert RingSchedule(k, step, F, ring=min_ring(k, step, F) + 3).R == min_ring(k, step, F) + 3


def test_ring_wraps_and_the_default_is_tight():
    """With the default ring the slots are reused many times over a long video — and one slot fewer really loses a frame."""
    k, step, F, T = 3, 2, 4, 23
    s = RingSchedule(k, step, F)
    assert s.R == 8 and T > 2 * s.R
    _replay(k, step, F, T)
    small = RingSchedule(k, step, F, ring=s.R)
    small.R -= 1  # behind the constructor's back
    fake = FakeRing(small)
    fake.run(small.push(T))
    want = window_indices(T, k, step)
    assert any(read != want[f].tolist() for f, read in fake.reads if f + step < T)


def test_schedule_limits():
    with pytest.raises(ValueError):
        RingSchedule(1, 1, 4)
    with pytest.raises(ValueError):
        RingSchedule(3, 0, 4)
    with pytest.raises(ValueError):
        RingSchedule(3, 1, 0)
    with pytest.raises(ValueError):
        RingSchedule(3, 1, _lib.VY_VIDEO_TABLE_MAX + 1)
    # clips per detect shrink so that clips * k fits the table
    s = RingSchedule(64, 1, 16)
    assert s.B * 64 <= _lib.VY_VIDEO_TABLE_MAX and s.B == 8
    _replay(64, 1, 16, 40)


def test_python_surface():
    import videoyolo_amd as vy
    c20 = ["c%d" % i for i in range(20)]
    win = vy.yolo3_darknet53(c20, pretrained_base=False, k=3, k_join_type="max", k_join_pos="early")
    assert callable(win.video) and callable(win.detect_video)
    with pytest.raises(RuntimeError, match="not on a device"):
        win.video()
    single = vy.yolo3_darknet53(c20, pretrained_base=False)
    assert not hasattr(single, "video") and not hasattr(single, "detect_video")
    assert not hasattr(vy.yolo3_no_backbone(c20), "detect_video")


def test_video_is_one_rank_only(monkeypatch):
    import videoyolo_amd as vy
    from videoyolo_amd import parallel
    win = vy.yolo3_darknet53(["a", "b"], pretrained_base=False, k=2, k_join_type="mean", k_join_pos="early")
    monkeypatch.setattr(parallel, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError):
        win.detect_video(np.zeros((3, 3, 64, 64), np.float32))


# ---------------------------------------------------------------------------------------------- C-ABI without a device
def _video_entries(lib, h):
    p = ctypes.c_void_p(16)  # never dereferenced: the kind check comes first
    tbl = (ctypes.c_int32 * 64)()
    return {
        "workspace_bytes": lambda: lib.vy_net_video_workspace_bytes(h, 16, 16, 18, 416, 416),
        "bind": lambda: lib.vy_net_bind_video(h, p, 1 << 40, 16, 16, 18, 416, 416, None),
        "push": lambda: lib.vy_net_video_push(h, p, tbl, None),
        "detect": lambda: lib.vy_net_video_detect(h, tbl, p, p, p, p, None),
        "read_slot": lambda: lib.vy_net_video_read_slot(h, 0, p, p, p, None),
    }


@pytest.mark.parametrize("create", ["vy_net_create", "vy_net_create_heads"])
def test_video_entries_refuse_other_nets(create):
    lib = _lib.load()
    h = ctypes.c_void_p()
    _lib.check(getattr(lib, create)(20, ctypes.byref(h)))
    try:
        for name, call in _video_entries(lib, h).items():
            got = call()
            if name == "workspace_bytes":
                assert got == 0, name
            else:
                assert got == -2, (name, got)  # VY_ERR_STATE
            assert b"window net" in lib.vy_last_error(), name
    finally:
        lib.vy_net_destroy(h)


def test_video_entries_need_a_video_binding():
    lib = _lib.load()
    h = ctypes.c_void_p()
    _lib.check(lib.vy_net_create_window(20, 3, 0, ctypes.byref(h)))
    try:
        calls = _video_entries(lib, h)
        for name in ("push", "detect", "read_slot"):
            assert calls[name]() == -2, name  # nothing bound at all
        p = ctypes.c_void_p(16)
        tbl = (ctypes.c_int32 * 64)()
        assert lib.vy_net_video_push(h, None, tbl, None) == -1
        assert lib.vy_net_video_push(h, p, None, None) == -1
        assert lib.vy_net_video_detect(h, None, p, p, p, p, None) == -1
        assert lib.vy_net_video_detect(h, tbl, None, p, p, p, None) == -1
        assert lib.vy_net_video_read_slot(h, 0, p, None, p, None) == -1
        assert lib.vy_net_bind_video(h, None, 1 << 40, 16, 16, 18, 416, 416, None) == -1
        assert lib.vy_net_bind_video(h, p, 16, 0, 16, 18, 416, 416, None) == -1
    finally:
        lib.vy_net_destroy(h)


def test_video_workspace_sizing():
    lib = _lib.load()
    h = ctypes.c_void_p()
    k = 3
    _lib.check(lib.vy_net_create_window(20, k, 0, ctypes.byref(h)))
    try:
        size = lambda f, b, r, hh=416, ww=416: lib.vy_net_video_workspace_bytes(h, f, b, r, hh, ww)
        for bad in ((0, 16, 18), (16, 0, 18), (16, 16, 0), (-1, 16, 18), (16, 16, -3)):
            assert size(*bad) == 0, bad
            assert b">= 1" in lib.vy_last_error(), bad
        # the tables travel in the kernel arguments: frames and clips * k are bounded
        lim = _lib.VY_VIDEO_TABLE_MAX
        assert size(lim + 1, 16, 18) == 0 and b"table entries" in lib.vy_last_error()
        assert size(16, lim // k + 1, 18) == 0 and b"table entries" in lib.vy_last_error()
        assert size(16, 16, 18, 16, 416) == 0  # the ordinary shape limits
        r = min_ring(k, 1, 16)
        b0 = size(16, 16, r)
        assert b0 >= r * SLOT_BYTES_416
        per_slot = size(16, 16, r + 1) - b0
        assert per_slot >= SLOT_BYTES_416
        assert size(16, 16, r + 8) - b0 == 8 * per_slot
        # F and B are independent: the backbone planes follow the frames, the head planes the clips
        assert size(8, 16, r) < b0 and size(16, 8, r) < b0
        # the video plan at F = B*k frames holds the clip plan's planes plus the ring
        clip = lib.vy_net_workspace_bytes(h, 4, 416, 416)
        assert 0 <= size(4 * k, 4, r) - clip - r * per_slot < 256
        # split conv modes stay refused on a window net
        assert lib.vy_net_set_conv_mode(h, _lib.VY_CONV_SPLIT_BF16X3) == -4
    finally:
        lib.vy_net_destroy(h)
