"""-m gpu: the inference plan is a value (NetPlan): computed by a const function, committed whole by a bind.

1. sizing is pure: the three sizing queries at another shape, between a bind and a launch sequence, change no bit of it —
   an inference forward, a training step, a video detect;
2. a refused bind (workspace too small) changes nothing;
3. a training plan dies with the inference plan it was carved behind: after vy_net_bind_workspace / vy_net_bind_video on
   the training workspace, at the same shape, the training forward is refused before anything is launched, and
   vy_net_bind_train makes the step a fresh net's again.

Shapes A = (2, 96, 64) and B = (1, 64, 128): not square and different in every plane size, so a swapped H / W or a field
that leaks from a query shows.  20 classes, synthetic parameters; every comparison is bit-equality."""
import ctypes

import numpy as np
import pytest

from test_gpu_window import CLASSES, _full, _params, _same, _win

pytestmark = pytest.mark.gpu
C = len(CLASSES)
A = (2, 96, 64)
B = (1, 64, 128)
VIDEO = (4, 2, 6)  # frames, clips, ring
NAMES = ("ids", "scores", "bboxes", "keep_idx")
VY_ERR_INVALID, VY_ERR_STATE = -1, -2


@pytest.fixture(scope="module")
def params():
    return _params()


def _x(shape, k=0, seed=3):
    b, h, w = shape
    lead = (b, k) if k else (b,)
    return np.random.default_rng(seed).standard_normal(lead + (3, h, w)).astype(np.float32)


def _targets(shape, seed=2):
    from oracle import targets_oracle as T
    b, h, w = shape
    gt_boxes, gt_ids = T.synthetic_gt(b, min(h, w), C, m=3, seed=seed, pad_to=5)
    return gt_boxes, T.prefetch_targets(C, h, w, gt_boxes, gt_ids)


def _query_all(net, shape=B):
    """The three sizing queries on `net` (the video one answers 0 on a net without a window: a query all the same)."""
    lib, h = net._lib, net._h
    got = [lib.vy_net_workspace_bytes(h, *shape), lib.vy_net_train_workspace_bytes(h, *shape),
           lib.vy_net_video_workspace_bytes(h, *VIDEO, *shape[1:])]
    assert got[0] > 0 and got[1] > got[0]
    return got


def _queries(net, third):
    """... on the bound net, and on a third net with keep_activations 0 and 1."""
    from videoyolo_amd import _lib
    _query_all(net)
    sizes = []
    for keep in (0, 1):
        _lib.check(third._lib.vy_net_set_keep_activations(third._h, keep))
        sizes.append(_query_all(third))
    assert sizes[0][0] < sizes[1][0]


def _bind_train(net, shape):
    import torch
    with torch.cuda.device(net._device):
        net._ensure_plan(*shape, train=True)


def _step(net, x, gt, tg):
    """One recorded forward and backward: (the four losses, the whole gradient buffer)."""
    import torch
    from videoyolo_amd import autograd
    with autograd.record():
        losses = net(x, gt, *tg)
        autograd.backward([losses[0] + losses[1] + losses[2] + losses[3]])
    torch.cuda.synchronize()
    return torch.stack([l.detach() for l in losses]), net._grads


def _assert_same_step(got, want):
    assert _same(got[0], want[0]), "losses"
    assert _same(got[1], want[1]), "gradients"
    assert bool(want[1].abs().sum() > 0)


# ---------------------------------------------------------------------------------------------- 1. sizing is pure
def test_queries_leave_a_bound_forward_alone(params):
    net, third = _full(params), _full(params)
    x = _x(A)
    first = net(x, return_index=True)
    _queries(net, third)
    for name, g, w in zip(NAMES, net(x, return_index=True), first):
        assert _same(g, w), name


def test_queries_leave_a_training_step_alone(params):
    x, (gt, tg) = _x(A), _targets(A)
    want = _step(_full(params), x, gt, tg)
    net, third = _full(params), _full(params)
    _bind_train(net, A)
    _queries(net, third)
    _assert_same_step(_step(net, x, gt, tg), want)


def test_queries_leave_a_video_plan_alone(params):
    import torch
    from videoyolo_amd.video import VideoSession
    f, b, r = VIDEO
    win, third = _win(params, 2, "max"), _win(params, 2, "max")
    session = VideoSession(win, frames_per_step=f, ring=r, clips_per_step=b)
    frames = torch.from_numpy(_x((f, 64, 64), seed=7)).cuda()
    table = [[0, 1], [2, 3]]
    with torch.cuda.device(win._device):
        session._ensure_bound(64, 64)
        session.raw_push(frames, list(range(f)))
        first = session.raw_detect(table, return_index=True)
        _queries(win, third)
        assert win._lib.vy_net_video_workspace_bytes(win._h, 16, 16, 18, 64, 128) > 0
        again = session.raw_detect(table, return_index=True)
    for name, g, w in zip(NAMES, again, first):
        assert _same(g, w), name


# ---------------------------------------------------------------------------------------------- 2. a refused bind
def test_a_refused_bind_changes_nothing(params):
    net = _full(params)
    x = _x(A)
    first = net(x, return_index=True)
    lib = net._lib
    need = lib.vy_net_workspace_bytes(net._h, *B)
    rc = lib.vy_net_bind_workspace(net._h, ctypes.c_void_p(net._ws.data_ptr()), need - 256, *B, net._stream())
    assert rc == VY_ERR_INVALID and b"too small" in lib.vy_last_error()
    for name, g, w in zip(NAMES, net(x, return_index=True), first):
        assert _same(g, w), name


# ---------------------------------------------------------------------------------------------- 3. a stale training plan
@pytest.mark.parametrize("kind", ["workspace", "video"])
def test_a_stale_training_plan_is_refused(params, kind):
    """The training workspace is the larger one, so every offset of either plan stays inside the buffer whatever runs."""
    import torch
    k = 2 if kind == "video" else 0
    make = (lambda: _win(params, 2, "max")) if k else (lambda: _full(params))
    x, (gt, tg) = _x(A, k), _targets(A)
    want = _step(make(), x, gt, tg)
    net = make()
    lib = net._lib
    _bind_train(net, A)
    ws, n = ctypes.c_void_p(net._ws.data_ptr()), net._ws.numel()
    if k:
        rc = lib.vy_net_bind_video(net._h, ws, n, *VIDEO, *A[1:], net._stream())
    else:
        rc = lib.vy_net_bind_workspace(net._h, ws, n, *A, net._stream())
    assert rc == 0, lib.vy_last_error()
    dev = [net._dev(t) for t in (x, gt) + tuple(tg)]
    losses = torch.full((4, A[0]), -7.0, dtype=torch.float32, device=net._device)
    p = [ctypes.c_void_p(t.data_ptr()) for t in dev]
    rc = lib.vy_net_train_forward(net._h, p[0], p[1], int(dev[1].shape[1]), *p[2:], ctypes.c_void_p(losses.data_ptr()),
                                  net._stream())
    assert rc == VY_ERR_STATE, (rc, lib.vy_last_error())
    if not k:
        assert b"training workspace not bound" in lib.vy_last_error()
    torch.cuda.synchronize()
    assert bool((losses == -7.0).all()), "the refused step wrote its output"
    net._plan = None  # the binding is the test's now: the next call binds for training again
    _assert_same_step(_step(net, x, gt, tg), want)
