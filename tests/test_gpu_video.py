"""-m gpu: a window net over a whole video (net.video / net.detect_video: Darknet-53 once per frame, routes in a ring,
clips pooled out of the ring) against the nets that are already bit-exact.  Every comparison is bit equality: ring slots
against the single-frame net's routes, detections against the clip net on the materialised clips, the gather-pool against
the numpy pool of test_gpu_window.py, and the clip and training plans of the same net before and after a session."""
import ctypes

import numpy as np
import pytest

from test_gpu_window import C, _full, _params, _same, _win, np_pool

pytestmark = pytest.mark.gpu
NAMES = ("ids", "scores", "bboxes", "keep_idx")


@pytest.fixture(scope="module")
def params():
    return _params()


def _video(t, h, w, seed=11):
    return np.random.default_rng(seed).standard_normal((t, 3, h, w)).astype(np.float32)


def _clip_net_outputs(net, frames, step, chunk=8):
    """net(frames[window_indices]) in chunks of clips."""
    import torch
    from videoyolo_amd import window_indices
    idx = window_indices(len(frames), net.k, step)
    outs = [net(frames[idx[i:i + chunk]], return_index=True) for i in range(0, len(idx), chunk)]
    return tuple(torch.cat(ts, 0) for ts in zip(*outs))


# ---------------------------------------------------------------------------------------------- 1. ring = features, 6. input
@pytest.mark.parametrize("h,w", [(416, 416), (200, 264)])
def test_ring_slots_hold_the_single_frame_routes(params, h, w):
    import torch
    frames = _video(6, h, w, seed=h)
    win = _win(params, 3, "max")
    session = win.video(frames_per_step=4)
    xt = torch.from_numpy(frames).cuda()
    out = session.push(xt)
    assert np.array_equal(xt.cpu().numpy(), frames), "the caller's input was written"
    assert out[0].shape[0] == 5  # k = 3, step 1: one frame of look-ahead
    full = _full(params)
    slots = set()
    for f in range(6):
        want = full.extract_features(frames[f:f + 1])
        got = session.read_slot(session.slot_of(f))
        slots.add(session.slot_of(f))
        for i in range(3):
            assert _same(got[i], want[i]), (f, i)
    assert len(slots) == 6
    assert session.flush()[0].shape[0] == 1


# ---------------------------------------------------------------------------------------------- 2. video = clip net
GRID = [(k, step, 416, 416) for k, step in ((2, 1), (3, 1), (3, 2), (5, 1))] + [(3, 2, 200, 264), (2, 1, 200, 264)]


@pytest.mark.parametrize("join", ["max", "mean"])
@pytest.mark.parametrize("k,step,h,w", GRID)
def test_video_equals_the_clip_net(params, join, k, step, h, w):
    from videoyolo_amd.video import min_ring
    t = 23
    frames = _video(t, h, w, seed=k * 10 + step)
    win = _win(params, k, join)
    assert t > 2 * min_ring(k, step, 4), "the ring wraps several times"
    assert t % 4 and (t - (k - 1 - k // 2) * step) % 4, "the last push and the last detect are padded"
    got = win.detect_video(frames, step=step, frames_per_step=4, return_index=True)
    want = _clip_net_outputs(win, frames, step)
    for name, g, r in zip(NAMES, got, want):
        assert g.shape[0] == t
        assert _same(g, r), name
    plain = win.detect_video(frames, step=step, frames_per_step=4)
    assert len(plain) == 3 and all(_same(a, b) for a, b in zip(plain, want))


@pytest.mark.parametrize("join", ["max", "mean"])
def test_video_shorter_than_the_window(params, join):
    frames = _video(2, 416, 416, seed=3)
    win = _win(params, 5, join)
    got = win.detect_video(frames, return_index=True)  # frames_per_step 16: one padded push, one padded detect
    want = _clip_net_outputs(win, frames, 1)
    for name, g, r in zip(NAMES, got, want):
        assert g.shape[0] == 2 and _same(g, r), name


# ---------------------------------------------------------------------------------------------- 3. pool localised
@pytest.mark.parametrize("join", ["max", "mean"])
def test_gather_pool_against_the_numpy_pool(params, join):
    import torch
    k, f, b = 3, 4, 4
    frames = _video(f, 416, 416, seed=8)
    win = _win(params, k, join, keep=True)
    session = win.video(frames_per_step=f, ring=9)
    assert (session.frames_per_step, session.clips_per_step, session.ring) == (f, b, 9)
    session._ensure_bound(416, 416)
    slots = [7, 2, 8, 0]  # anywhere in the ring: the library does not track frames
    session.raw_push(torch.from_numpy(frames).cuda(), slots)
    table = [[7, 2, 8], [0, 0, 0], [8, 8, 7], [2, 7, 2]]  # one slot k times; repeats in a row; out of frame order
    session.raw_detect(table)
    feats = [t.cpu().numpy() for t in _full(params).extract_features(frames)]
    frame_of = {s: i for i, s in enumerate(slots)}
    gather = np.array([[frame_of[s] for s in row] for row in table]).reshape(-1)
    for i in range(3):
        want = torch.from_numpy(np_pool(feats[i][gather], k, join)).cuda()
        assert _same(session.read_activation("pool.%d" % i), want), i
    assert tuple(session.read_activation("stages.0.0").shape)[0] == f
    # bad tables are refused before anything runs
    from videoyolo_amd import _lib
    for bad in ([[7, 2, 9]] + table[1:], [[-1, 2, 8]] + table[1:]):
        with pytest.raises(_lib.VyError) as e:
            session.raw_detect(bad)
        assert e.value.code == -1
    with pytest.raises(_lib.VyError) as e:
        session.raw_push(torch.from_numpy(frames).cuda(), [0, 1, -2, 3])
    assert e.value.code == -1
    session.raw_push(torch.from_numpy(frames).cuda(), [-1, -1, 5, -1])  # -1: not stored
    got = session.read_slot(5)
    assert _same(got[2], torch.from_numpy(feats[2][2:3]).cuda())
    assert not session.read_slot(4)[0].any().item(), "a slot nobody wrote stays the zeros of the bind"


# ---------------------------------------------------------------------------------------------- 4. incremental = whole
def test_incremental_pushes_equal_the_whole_video(params):
    import torch
    k, step, t = 3, 2, 23
    frames = _video(t, 416, 416, seed=4)
    win = _win(params, k, "max")
    whole = win.detect_video(frames, step=step, frames_per_step=4, return_index=True)
    session = win.video(frames_per_step=4, step=step)
    lag = (k - 1 - k // 2) * step
    blocks, done, at = [], 0, 0
    for n in (1, 7, 4, 11):
        out = session.push(frames[at:at + n], return_index=True)
        at += n
        ready = max(0, at - lag)
        assert out[0].shape[0] == ready - done, (n, out[0].shape)
        done = ready
        blocks.append(out)
    with pytest.raises(ValueError, match="frame size"):
        session.push(_video(1, 200, 264))
    tail = session.flush(return_index=True)
    assert tail[0].shape[0] == lag
    blocks.append(tail)
    for j, name in enumerate(NAMES):
        assert _same(torch.cat([b[j] for b in blocks], 0), whole[j]), name
    # the flushed session takes another video, of another size
    small = _video(3, 200, 264, seed=6)
    a = session.push(small, return_index=True)
    b = session.flush(return_index=True)
    want = _clip_net_outputs(win, small, step)
    for j, name in enumerate(NAMES):
        assert _same(torch.cat([a[j], b[j]], 0), want[j]), name


# ---------------------------------------------------------------------------------------------- 5. plans coexist
def test_clip_video_and_training_plans_on_one_net(params):
    import torch
    from videoyolo_amd import _lib
    from test_gpu_window import _clips, _step, _targets
    k, join = 3, "max"
    win = _win(params, k, join)
    clips = _clips(2, k, 416, 416, seed=1)
    before = win(clips, return_index=True)
    frames = _video(9, 416, 416, seed=2)
    session = win.video(frames_per_step=4)
    first = session.push(frames[:5], return_index=True)
    # the net is bound for video: the clip entry of the library refuses
    p = ctypes.c_void_p(clips.ctypes.data)
    assert win._lib.vy_net_forward_infer(win._h, p, p, p, p, None, None) == -2
    assert win._lib.vy_net_train_backward(win._h, p, None) == -2
    after = win(clips, return_index=True)  # binds the clip plan again
    for name, a, b in zip(NAMES, before, after):
        assert _same(a, b), name
    # the session lost its ring to that call: a clear error, then it starts over
    with pytest.raises(RuntimeError, match="ring is lost"):
        session.push(frames[5:])
    got = [session.push(frames, return_index=True), session.flush(return_index=True)]
    want = _clip_net_outputs(win, frames, 1)
    for j, name in enumerate(NAMES):
        assert _same(torch.cat([g[j] for g in got], 0), want[j]), name
    assert _same(got[0][0][:4], first[0][:4])
    # a video entry on the clip plan refuses too
    tbl = (ctypes.c_int32 * 16)()
    assert win._lib.vy_net_video_detect(win._h, tbl, p, p, p, None, None) == -2
    session.push(frames[:4])  # the session holds the binding (and frames) again
    # a training step on the same net equals a fresh window net's
    s = 128
    x = _clips(2, k, s, s, seed=5)
    gt, tg = _targets(2, s)
    l_used, _ = _step(win, x, gt, tg)
    l_fresh, _ = _step(_win(params, k, join), x, gt, tg)
    for i in range(4):
        assert _same(l_used[i], l_fresh[i]), i
    with pytest.raises(RuntimeError, match="ring is lost"):
        session.flush()
    assert isinstance(_lib.VY_VIDEO_TABLE_MAX, int)
