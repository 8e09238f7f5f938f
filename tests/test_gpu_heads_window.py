"""-m gpu: the windowed heads-only net (yolo3_no_backbone with k > 1).  route_import_pool gathers, pools and transposes a
window of stored per-frame routes in one launch; the rest of the net is the heads-only net on the same plan, and the heads
of a window net see nothing but the pooled routes.  So every bar here is bit-equality: the pooled planes against
oracle.train_cells64.pool_forward, detections / losses / gradients / statistics / the SGD step against the heads-only net fed
the numpy-pooled routes, and against the full window net on the frames the routes came from."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.train_cells64 import pool_forward

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 20
CLASSES = ["c%d" % i for i in range(C)]
ROUTE_CELLS = ("stages.0.14.body.1", "stages.1.8.body.1", "stages.2.4.body.1")  # features[14], [23], [28]
# (tap cell, first channel of the route in the cell's input view, channels): stride 8, 16, 32
ROUTE_TAPS = (("yolo_blocks.2.body.0", 128, 256), ("yolo_blocks.1.body.0", 256, 512), ("yolo_blocks.0.body.0", 0, 1024))
# (join, k, B, H, W): the smallest shapes that reach each branch of the kernel
CASES = [
    ("max", 3, 2, 64, 64),      # full, quarter and sixteenth tiles, vector path
    ("mean", 2, 3, 96, 32),     # H*W = 48, 12 and 3: the last is the dword path with a 3-pixel tile
    ("max", 4, 2, 128, 224),    # tiles that span image rows
    ("mean", 3, 2, 416, 416),   # 2704 and 676 pixels, a partial last tile among many; 169 pixels on the dword path
]


@pytest.fixture(scope="module")
def params():
    from videoyolo_amd import init
    from oracle import yolo3_oracle as O
    return init.synthetic_params(O.param_shapes(C), seed=233)


def _on_device(net, params, heads_only):
    net.set_parameters({k: v for k, v in params.items() if not (heads_only and k.startswith("stages."))})
    net.collect_params().reset_ctx("cuda:0")
    return net


def _hw(params, k, join):
    import videoyolo_amd as vy
    net = vy.yolo3_no_backbone(CLASSES, k=k, k_join_type=join, k_join_pos="early")
    assert type(net) is vy.YOLOV3NoBackboneWindow
    return _on_device(net, params, True)


def _heads(params):
    import videoyolo_amd as vy
    return _on_device(vy.yolo3_no_backbone(CLASSES), params, True)


def _full(params):
    import videoyolo_amd as vy
    return _on_device(vy.yolo3_darknet53(CLASSES, pretrained_base=False), params, False)


def _win(params, k, join, freeze_base=False):
    import videoyolo_amd as vy
    return _on_device(vy.yolo3_darknet53(CLASSES, pretrained_base=False, freeze_base=freeze_base, k=k, k_join_type=join,
                                         k_join_pos="early"), params, False)


def _bits(t):
    import torch
    return t.detach().contiguous().view(torch.int32).cpu()


def _same(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _all_same(got, want, what):
    assert len(got) == len(want)
    for i, (g, r) in enumerate(zip(got, want)):
        assert _same(g, r), (what, i)


def _bank(t, h, w, seed):
    rng = np.random.default_rng(seed)
    h8, w8 = -(-h // 8), -(-w // 8)
    return [rng.standard_normal(s).astype(np.float32) for s in
            ((t, 256, h8, w8), (t, 512, -(-h8 // 2), -(-w8 // 2)), (t, 1024, -(-h8 // 4), -(-w8 // 4)))]


def _table(b, k, t, seed):
    """Permutes, skips (t > b * k) and repeats frames; one row repeats a frame inside the row."""
    rng = np.random.default_rng(seed)
    tab = rng.permutation(t)[:b * k].reshape(b, k)
    tab[0, 1] = tab[0, 0]
    tab[b - 1, 0] = tab[0, k - 1]
    return tab


def _pooled(bank, table, k, join):
    import torch
    return [torch.from_numpy(pool_forward(f[table.reshape(-1)], k, join)).cuda() for f in bank]


def _targets(b, h, w, seed=2):
    from oracle import targets_oracle as T
    gt_boxes, gt_ids = T.synthetic_gt(b, min(h, w), C, m=3, seed=seed, pad_to=5)
    return gt_boxes, T.prefetch_targets(C, h, w, gt_boxes, gt_ids)


def _record(net, inputs, gt, tg):
    from videoyolo_amd import autograd
    with autograd.record():
        losses = net.from_bank(*inputs, gt, *tg) if len(inputs) == 4 else net(*inputs, gt, *tg)
        autograd.backward([losses[0] + losses[1] + losses[2] + losses[3]])
    return losses


def _check_step_equal(wn, hn, what):
    for name, p in hn.collect_params().items():
        if p.trainable:
            assert np.array_equal(wn.grad(name), hn.grad(name)), (what, name)
        else:  # BatchNorm running statistics
            assert np.array_equal(wn.collect_params()[name].data(), p.data()), (what, name)


# ------------------------------------------------------------------------------------- 1-2. the planes, the heads net
@pytest.mark.parametrize("join,k,b,h,w", CASES)
def test_pooled_planes_and_every_output_equal_the_heads_net(params, join, k, b, h, w):
    import torch
    import videoyolo_amd as vy
    from videoyolo_amd import autograd
    t = b * k + 3
    bank = _bank(t, h, w, seed=k + b)
    table = _table(b, k, t, seed=h)
    assert len(set(table.reshape(-1))) < b * k < t  # frames repeat, frames are skipped
    dev = [torch.from_numpy(f).cuda() for f in bank]
    pooled = _pooled(bank, table, k, join)
    wn, hn = _hw(params, k, join), _heads(params)

    # detections
    _all_same(wn.from_bank(*dev, table, return_index=True), hn(*pooled, return_index=True), "detect")

    # train mode without recording: the five device tensors of the 8-tuple ...
    with autograd.train_mode():
        ow, oh = wn.from_bank(*dev, table), hn(*pooled)
    for i in (0, 4, 5, 6, 7):
        assert _same(ow[i], oh[i]), i
    # ... and (1) where the pooled routes landed: the route channels of the three planes, interior only
    for (cell, co, ch), want in zip(ROUTE_TAPS, pooled):
        tap = wn.read_train_tap(cell, "input")
        assert tuple(tap.shape) == (b, co + ch, want.shape[2] + 2, want.shape[3] + 2), cell
        assert _same(tap[:, co:, 1:-1, 1:-1], want), cell
        assert _same(tap, hn.read_train_tap(cell, "input")), cell  # the transition's channels too
        tap[:, :, 1:-1, 1:-1] = 0
        assert not tap.any().item(), cell  # borders stay zero
    for i, want in enumerate(pooled):  # the window net's tap names serve this net too
        assert _same(wn.read_activation("pool.%d" % i), want), i

    # a recorded step: the four losses, every gradient, every running statistic, then one Trainer.step
    gt, tg = _targets(b, h, w)
    _all_same(_record(wn, dev + [table], gt, tg), _record(hn, pooled, gt, tg), "losses")
    _check_step_equal(wn, hn, "step")
    opt = {'learning_rate': 1e-3, 'wd': 5e-4, 'momentum': 0.9}
    vy.Trainer(wn.collect_params(), 'sgd', dict(opt)).step(b)
    vy.Trainer(hn.collect_params(), 'sgd', dict(opt)).step(b)
    for name, p in hn.collect_params().items():
        assert np.array_equal(wn.collect_params()[name].data(), p.data()), name
    assert not np.array_equal(wn.collect_params()["transitions.1.0.weight"].data(), params["transitions.1.0.weight"])
    torch.cuda.synchronize()
    for d, f in zip(dev, bank):
        assert np.array_equal(d.cpu().numpy(), f), "the bank was written"


def test_size_change_on_the_same_net(params):
    import torch
    k, join, b = 2, "max", 2
    wn, hn = _hw(params, k, join), _heads(params)
    for s in (320, 416):
        bank = _bank(b * k + 3, s, s, seed=s)
        table = _table(b, k, b * k + 3, seed=s)
        dev = [torch.from_numpy(f).cuda() for f in bank]
        pooled = _pooled(bank, table, k, join)
        gt, tg = _targets(b, s, s, seed=s)
        _all_same(_record(wn, dev + [table], gt, tg), _record(hn, pooled, gt, tg), ("losses", s))
        _check_step_equal(wn, hn, s)
        assert wn._plan == (b, s, s, True)
        _all_same(wn.from_bank(*dev, table, return_index=True), hn(*pooled, return_index=True), ("detect", s))


# ------------------------------------------------------------------------------------- 3. the (B, k, C, h, w) form
@pytest.mark.parametrize("join,k,b,h,w", CASES[:2])
def test_five_d_routes_equal_the_identity_table(params, join, k, b, h, w):
    import torch
    from videoyolo_amd import autograd
    bank = [torch.from_numpy(f).cuda() for f in _bank(b * k, h, w, seed=11)]
    clips = [f.view((b, k) + tuple(f.shape[1:])) for f in bank]
    ident = np.arange(b * k).reshape(b, k)
    wn = _hw(params, k, join)
    _all_same(wn(*clips, return_index=True), wn.from_bank(*bank, ident, return_index=True), "detect")
    with autograd.train_mode():
        o5, o4 = wn(*clips), wn.from_bank(*bank, ident)
    for i in (0, 4, 5, 6, 7):
        assert _same(o5[i], o4[i]), i
    gt, tg = _targets(b, h, w)
    l5 = _record(wn, clips, gt, tg)
    g5 = wn.grad("yolo_blocks.0.body.0.0.weight")
    l4 = _record(wn, bank + [ident], gt, tg)
    _all_same(l5, l4, "losses")
    assert np.array_equal(g5, wn.grad("yolo_blocks.0.body.0.0.weight"))
    # host arrays are taken too
    _all_same(wn(*[c.cpu().numpy() for c in clips], return_index=True), wn(*clips, return_index=True), "host")


# ------------------------------------------------------------------------------------- 4. the full window net
def test_against_the_full_window_net(params):
    import torch
    from videoyolo_amd import autograd
    join, k, b, s = "max", 3, 2, 64
    x = np.random.default_rng(4).standard_normal((b, k, 3, s, s)).astype(np.float32)
    # detections: the routes a single-frame net extracts from the same frames
    f = _full(params).extract_features(x.reshape((b * k, 3, s, s)))
    wn = _hw(params, k, join)
    _all_same(wn(*[t.view((b, k) + tuple(t.shape[1:])) for t in f], return_index=True),
              _win(params, k, join)(x, return_index=True), "detect")
    # training: the per-frame routes of the frozen window net's own recorded forward (BatchNorm on batch statistics)
    frozen = _win(params, k, join, freeze_base=True)
    gt, tg = _targets(b, s, s)
    with autograd.record():
        lf = frozen(x, gt, *tg)
        routes = [frozen.read_activation(c) for c in ROUTE_CELLS]
        autograd.backward([lf[0] + lf[1] + lf[2] + lf[3]])
    assert routes[0].shape[0] == b * k
    lw = _record(wn, [r.view((b, k) + tuple(r.shape[1:])) for r in routes], gt, tg)
    _all_same(lw, lf, "losses")
    for name, p in wn.collect_params().items():
        if p.trainable:
            assert np.array_equal(wn.grad(name), frozen.grad(name)), name
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------- 5. a stored video
@pytest.mark.parametrize("t,step", [(7, 2), (1, 1)])
def test_detect_video_features_equals_detect_video(params, t, step):
    k, join, s = 3, "max", 64
    frames = np.random.default_rng(t).standard_normal((t, 3, s, s)).astype(np.float32)
    f = _full(params).extract_features(frames)
    wn = _hw(params, k, join)
    want = _win(params, k, join).detect_video(frames, step=step, return_index=True)
    got = wn.detect_video_features(*f, step=step, return_index=True)
    assert got[0].shape[0] == t
    _all_same(got, want, "video")
    _all_same(wn.detect_video_features(*f, step=step, clips_per_step=4), want[:3], "chunks of 4")


# ------------------------------------------------------------------------------------- 6. ties
@pytest.mark.parametrize("join,k", [("max", 3), ("mean", 2)])
def test_identical_frames_give_the_heads_nets_result(params, join, k):
    import torch
    b, s = 2, 64
    bank = [torch.from_numpy(f).cuda() for f in _bank(b, s, s, seed=8)]
    table = np.repeat(np.arange(b)[:, None], k, axis=1)
    _all_same(_hw(params, k, join).from_bank(*bank, table, return_index=True), _heads(params)(*bank, return_index=True), join)


def test_signed_zero_ties_keep_the_earliest_frame():
    import torch
    import videoyolo_amd as vy
    from videoyolo_amd import autograd
    k, b, s = 2, 1, 64
    bank = _bank(3, s, s, seed=1)
    for f in bank:  # frame 0: -0 then +0 along the flattened tensor, frame 1 the opposite sign, frame 2 all -0
        flat = f.reshape(3, -1)
        flat[0, 0::2], flat[0, 1::2] = -0.0, 0.0
        flat[1, 0::2], flat[1, 1::2] = 0.0, -0.0
        flat[2, :] = -0.0
    net = vy.yolo3_no_backbone(CLASSES, k=k, k_join_type="max", k_join_pos="early")
    net.initialize(init="synthetic", seed=5)
    net.collect_params().reset_ctx("cuda:0")
    dev = [torch.from_numpy(f).cuda() for f in bank]
    for table in ([[0, 1]], [[1, 0]], [[2, 1]], [[1, 2]]):
        with autograd.train_mode():
            net.from_bank(*dev, np.array(table))
        for (cell, co, ch), f in zip(ROUTE_TAPS, bank):
            got = net.read_train_tap(cell, "input")[:, co:, 1:-1, 1:-1].cpu().numpy().view(np.uint32)
            assert np.array_equal(got, f[table[0][0]][None].view(np.uint32)), (table, cell)  # the earliest frame's bits
            assert np.array_equal(got, pool_forward(f[table[0]], k, "max").view(np.uint32)), (table, cell)


# ------------------------------------------------------------------------------------- 7. the table limit
def test_a_full_table_runs_and_one_more_entry_is_refused(params):
    import torch
    from videoyolo_amd import _lib
    k, join, s = 4, "max", 64
    b = _lib.VY_VIDEO_TABLE_MAX // k
    bank = _bank(5, s, s, seed=3)
    table = np.random.default_rng(0).integers(0, 5, (b, k))
    dev = [torch.from_numpy(f).cuda() for f in bank]
    _all_same(_hw(params, k, join).from_bank(*dev, table, return_index=True),
              _heads(params)(*_pooled(bank, table, k, join), return_index=True), "512 entries")
    # 171 x 3 = 513: Python refuses it, and so does the library, before anything is launched
    wn = _hw(params, 3, join)
    with pytest.raises(ValueError, match="table entries"):
        wn.from_bank(*dev, np.zeros((171, 3), np.int64))
    with torch.cuda.device(wn._device):
        wn._ensure_plan(171, s, s)
        outs = wn._detect_outputs(171, wn._out_rows(), False)
        for o in outs[:3]:
            o.fill_(-7.0)
        tab = (ctypes.c_int32 * 513)()
        rc = wn._lib.vy_net_forward_infer_bank(wn._h, *[ctypes.c_void_p(d.data_ptr()) for d in dev], 5, tab,
                                               *[ctypes.c_void_p(o.data_ptr()) for o in outs[:3]], None, wn._stream())
        assert rc == -1 and "table entries" in wn._lib.vy_last_error().decode()
        # an entry out of range is refused the same way
        wn._ensure_plan(2, s, s)
        bad = (ctypes.c_int32 * 6)(0, 1, 2, 3, 4, 5)
        rc = wn._lib.vy_net_forward_infer_bank(wn._h, *[ctypes.c_void_p(d.data_ptr()) for d in dev], 5, bad,
                                               *[ctypes.c_void_p(o.data_ptr()) for o in outs[:3]], None, wn._stream())
        assert rc == -1 and "outside [0, 5)" in wn._lib.vy_last_error().decode()
    torch.cuda.synchronize()
    for o in outs[:3]:
        assert (o == -7.0).all().item(), "an output was written by a refused call"


# ------------------------------------------------------------------------------------- 8. the example
def test_train_heads_window_example_runs():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "examples/train_heads_window.py", "--size", "128", "--batch", "4", "--frames", "10",
                        "--k", "3", "--step", "2", "--steps", "3", "--chunk", "4"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, universal_newlines=True)
    assert p.returncode == 0, p.stdout[-3000:]
    assert "extracted" in p.stdout and "bit for bit" in p.stdout and "mAP" in p.stdout
