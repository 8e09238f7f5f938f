"""-m gpu: the k-frame clip net (yolo3_darknet53 with k > 1, early join) against nets that are already bit-exact.  The
window net's backbone runs the full net's launches on B*k frames and its heads the heads net's launches on B clips, so
the bars are bit-equality: pooled routes against a numpy pool of the full net's routes, detections and the training step's
head side against the heads net on those pooled routes, identical frames against the single-frame net, backbone BatchNorm
statistics against the full net's train-mode forward.  Backbone gradients are checked against a torch float64 twin."""
import numpy as np
import pytest

from conftest import frames
from oracle.train_cells64 import pool_forward as np_pool
from test_oracle_train_vs_torch import TorchYolo3Train

pytestmark = pytest.mark.gpu
C = 20
CLASSES = ["c%d" % i for i in range(C)]
ROUTE_CELLS = ("stages.0.14.body.1", "stages.1.8.body.1", "stages.2.4.body.1")


def _params(seed=233):
    from videoyolo_amd import init
    from oracle import yolo3_oracle as O
    return init.synthetic_params(O.param_shapes(C), seed=seed)


def _full(params, keep=False):
    import videoyolo_amd as vy
    net = vy.yolo3_darknet53(CLASSES, pretrained_base=False)
    net.set_parameters(params)
    net.collect_params().reset_ctx("cuda:0")
    if keep:
        net.keep_activations()
    return net


def _heads(params):
    import videoyolo_amd as vy
    net = vy.yolo3_no_backbone(CLASSES)
    net.set_parameters({k: v for k, v in params.items() if not k.startswith("stages.")})
    net.collect_params().reset_ctx("cuda:0")
    return net


def _win(params, k, join, keep=False):
    import videoyolo_amd as vy
    net = vy.yolo3_darknet53(CLASSES, pretrained_base=False, k=k, k_join_type=join, k_join_pos="early")
    assert isinstance(net, vy.YOLOV3Window)
    net.set_parameters(params)  # a single-frame parameter dict: stage keys without '.model.'
    net.collect_params().reset_ctx("cuda:0")
    if keep:
        net.keep_activations()
    return net


def _clips(b, k, h, w, seed=5):
    return np.random.default_rng(seed).standard_normal((b, k, 3, h, w)).astype(np.float32)


def _bits(t):
    import torch
    return t.detach().contiguous().view(torch.int32).cpu()


def _same(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def params():
    return _params()


def _pooled_routes(params, x, k, join):
    """numpy pool of the full net's extract_features on the (B*k, 3, H, W) reshape, as device tensors."""
    import torch
    full = _full(params)
    b = x.shape[0]
    f = full.extract_features(x.reshape((b * k,) + x.shape[2:]))
    return [torch.from_numpy(np_pool(t.cpu().numpy(), k, join)).cuda() for t in f]


# ---------------------------------------------------------------------------------------------- 1-2. routes, detections
@pytest.mark.parametrize("join", ["max", "mean"])
@pytest.mark.parametrize("k,b,h,w", [(2, 2, 416, 416), (3, 2, 416, 416), (3, 1, 200, 264)])
def test_pooled_routes_and_detections(params, join, k, b, h, w):
    import torch
    x = _clips(b, k, h, w, seed=k + b)
    pooled = _pooled_routes(params, x, k, join)
    win = _win(params, k, join, keep=True)
    xt = torch.from_numpy(x).cuda()
    got = win(xt, return_index=True)
    assert np.array_equal(xt.cpu().numpy(), x), "the caller's input was written"
    for i in range(3):
        assert _same(win.read_activation("pool.%d" % i), pooled[i]), i
    # the per-frame taps of a backbone cell are the B*k frames
    assert tuple(win.read_activation("stages.0.0").shape)[0] == b * k
    heads = _heads(params)
    want = heads(*pooled, return_index=True)
    for name, g, r in zip(("ids", "scores", "bboxes", "keep_idx"), got, want):
        assert _same(g, r), name
    # the recycled-plane plan (no keep_activations) computes the same
    plain = _win(params, k, join)
    for name, g, r in zip(("ids", "scores", "bboxes", "keep_idx"), plain(x, return_index=True), want):
        assert _same(g, r), ("plain", name)


# ---------------------------------------------------------------------------------------------- 3. identity
@pytest.mark.parametrize("join,k", [("max", 3), ("mean", 2)])
def test_identical_frames_detect_as_the_single_frame_net(params, join, k):
    rng = np.random.default_rng(9)
    x1 = rng.standard_normal((2, 3, 416, 416)).astype(np.float32)
    clips = np.repeat(x1[:, None], k, axis=1)
    want = _full(params)(x1, return_index=True)
    got = _win(params, k, join)(clips, return_index=True)
    for name, g, r in zip(("ids", "scores", "bboxes", "keep_idx"), got, want):
        assert _same(g, r), name


# ---------------------------------------------------------------------------------------------- 4-7. training
def _targets(b, s, seed=2):
    from oracle import targets_oracle as T
    gt_boxes, gt_ids = T.synthetic_gt(b, s, C, m=3, seed=seed, pad_to=5)
    return gt_boxes, T.prefetch_targets(C, s, s, gt_boxes, gt_ids)


def _conv_names(net):
    import ctypes
    from videoyolo_amd import _lib
    out = []
    for i in range(net._lib.vy_net_num_convs(net._h)):
        info = _lib.ConvInfo()
        _lib.check(net._lib.vy_net_conv_info(net._h, i, ctypes.byref(info)))
        out.append(info.name.decode())
    return out


def _branch(win, names):
    """Sign of every BatchNorm cell's pre-activation in the recorded fp32 forward (z * scale + shift), frames first."""
    out = {}
    for n in names:
        if "prediction" in n:
            continue
        z = win.read_train_tap(n, "z")[:, :, 1:-1, 1:-1].double()
        bn = win.read_train_tap(n, "bn").double()
        out[n] = ((z * bn[2][None, :, None, None] + bn[3][None, :, None, None]) > 0).cpu().numpy()
    return out


class _Pool:
    """TemporalPooling 'direct' in float64 with the library's backward rule: max hands g to every frame equal to the max."""

    @staticmethod
    def apply(x, k, join, sel=None):
        """sel (optional, max): one-hot (B, k, ...) of the frame the fp32 run under test kept — the pooling analogue of the
        twin's sign-branch trick (a near-tie within fp32-vs-fp64 drift must not move a whole gradient to another frame)."""
        import torch

        class Max(torch.autograd.Function):
            @staticmethod
            def forward(ctx, v):
                m = v.max(1)[0]
                ctx.save_for_backward(v, m)
                return m

            @staticmethod
            def backward(ctx, g):
                v, m = ctx.saved_tensors
                return g[:, None] * (v == m[:, None]).to(g.dtype)

        v = x.view((-1, k) + tuple(x.shape[1:]))
        if join == "max" and sel is not None:
            return (v * torch.from_numpy(sel).to(v.dtype)).sum(1)
        return Max.apply(v) if join == "max" else v.mean(1)


class TorchWindowTrain(TorchYolo3Train):
    """The float64 twin: the single-frame train-mode graph with each route pooled over k frames as its stage ends."""

    def __init__(self, ncls, p, k, join, branch, frame_routes):
        super().__init__(ncls, p, branch)
        self.k, self.join = k, join
        self.sel = []  # per route: one-hot of the first frame holding the fp32 max
        for f in frame_routes:
            v = f.reshape((-1, k) + f.shape[1:])
            self.sel.append((np.arange(k)[None, :, None, None, None] == v.argmax(1)[:, None]).astype(np.float64))

    def forward_heads(self, x):
        import torch
        import torch.nn.functional as F
        p = self.p
        layers = [1, 2, 8, 8, 4]
        feats = [("c", 3, 1)]
        for n in layers:
            feats += [("c", 3, 2)] + [("b",)] * n
        routes = []
        for si, (lo, hi) in enumerate([(0, 15), (15, 24), (24, 29)]):
            for j, f in enumerate(feats[lo:hi]):
                pre = "stages.%d.%d" % (si, j)
                if f[0] == "c":
                    x = self.cell(x, pre, f[1], f[2])
                else:
                    x = x + self.cell(self.cell(x, pre + ".body.0", 1, 1), pre + ".body.1", 3, 1)
            routes.append(_Pool.apply(x, self.k, self.join, self.sel[si]))
        outs = []
        x = routes[2]
        for i in range(3):
            for j in range(5):
                x = self.cell(x, "yolo_blocks.%d.body.%d" % (i, j), 1 if j % 2 == 0 else 3, 1)
            tip = self.cell(x, "yolo_blocks.%d.tip" % i, 3, 1)
            outs.append(F.conv2d(tip, p["yolo_outputs.%d.prediction.weight" % i], p["yolo_outputs.%d.prediction.bias" % i]))
            if i == 2:
                break
            x = self.cell(x, "transitions.%d" % i, 1, 1)
            x = F.interpolate(x, scale_factor=2, mode="nearest")
            r = routes[1 - i]
            x = torch.cat([x[:, :, :r.shape[2], :r.shape[3]], r], 1)
        return outs


def _step(net, x, gt, tg, between=None):
    import torch
    from videoyolo_amd import autograd
    with autograd.record():
        losses = net(x, gt, *tg)
        out = between() if between else None
        autograd.backward([losses[0] + losses[1] + losses[2] + losses[3]])
    torch.cuda.synchronize()
    return losses, out


@pytest.mark.parametrize("join", ["max", "mean"])
def test_training_step(params, join):
    from videoyolo_amd import autograd
    b, k, s = 2, 3, 128
    x = frames(b * k, s, seed=5).reshape((b, k, 3, s, s))  # image-like frames, as the single-frame end-to-end bars use
    x0 = x.copy()
    gt, tg = _targets(b, s)
    import torch
    win = _win(params, k, join)
    names = _conv_names(win)
    # train mode without recording: the backbone is the full net's train-mode forward on the B*k frames, the 8-tuple the
    # heads net's on the pooled routes
    full = _full(params)
    with autograd.train_mode():
        ow = win(x)
        full(x.reshape((b * k, 3, s, s)))
    for c in ROUTE_CELLS:
        assert _same(win.read_activation(c), full.read_activation(c)), c
    pooled = [torch.from_numpy(np_pool(win.read_activation(c).cpu().numpy(), k, join)).cuda() for c in ROUTE_CELLS]
    for i in range(3):
        assert _same(win.read_activation("pool.%d" % i), pooled[i]), i
    heads = _heads(params)
    with autograd.train_mode():
        oh = heads(*pooled)
    for j in (0, 4, 5, 6, 7):
        assert _same(ow[j], oh[j]), j
    for name in names:  # BatchNorm running statistics: the full net's on B*k frames, the heads net's on B clips
        if "prediction" in name:
            continue
        ref = full if name.startswith("stages.") else heads
        for leaf in ("running_mean", "running_var"):
            key = "%s.1.%s" % (name, leaf)
            assert np.array_equal(win.collect_params()[win._key(key)].data(), ref.collect_params()[key].data()), key

    # 4. one recorded step: losses, head gradients and head BatchNorm taps equal the heads net's on the pooled routes
    win = _win(params, k, join)
    heads = _heads(params)
    lw, branch = _step(win, x, gt, tg, between=lambda: (_branch(win, names),
                                                          [win.read_activation(c).cpu().numpy() for c in ROUTE_CELLS]))
    branch, frame_routes = branch
    assert np.array_equal(x, x0)
    pooled = [torch.from_numpy(np_pool(f, k, join)).cuda() for f in frame_routes]
    for i in range(3):
        assert _same(win.read_activation("pool.%d" % i), pooled[i]), i
    with autograd.record():
        lh = heads(*pooled, gt, *tg)
        autograd.backward([lh[0] + lh[1] + lh[2] + lh[3]])
    torch.cuda.synchronize()
    for i in range(4):
        assert _same(lw[i], lh[i]), i
    for name, p in heads.collect_params().items():
        if p.trainable:
            assert np.array_equal(win.grad(name), heads.grad(name)), name
        else:
            assert np.array_equal(win.collect_params()[name].data(), p.data()), name
    for name in names:
        if name.startswith("stages.") or "prediction" in name:
            continue
        assert _same(win.read_train_tap(name, "bn"), heads.read_train_tap(name, "bn")), name
    for i in range(3):  # the pooled routes' gradients are the heads' input gradients
        g = win.read_grad_activation("pool.%d" % i)
        assert tuple(g.shape)[0] == b and g.abs().sum().item() > 0

    # 5. backbone gradients against the float64 twin (2e-3 of each tensor's max)
    tm = TorchWindowTrain(C, params, k, join, branch, frame_routes)
    tl = tm.losses(x.reshape((b * k, 3, s, s)), gt, *tg)
    for a, r in zip(lw, tl):
        np.testing.assert_allclose(a.cpu().numpy(), r.detach().numpy(), rtol=2e-4, atol=1e-4)
    sum(t.sum() for t in tl).backward()
    worst = 0.0
    for key, p in win.collect_params().items():
        if not p.trainable or not p.backbone:
            continue
        ref = tm.p[key.replace(".model.", ".", 1)].grad.numpy()
        err = float(np.abs(win.grad(key) - ref).max() / (np.abs(ref).max() + 1e-6))
        worst = max(worst, err)
        assert err < 2e-3, (key, err)
    print("worst backbone gradient mismatch (%s): %.2e" % (join, worst))

    # plane borders stay zero (per-frame route planes and their gradient planes included)
    for name in ("stages.1.0", "stages.2.0", "yolo_blocks.0.body.0", "yolo_blocks.2.body.0"):
        t = win.read_train_tap(name, "input")
        t[:, :, 1:-1, 1:-1] = 0
        assert not t.any().item(), name
    for name in ROUTE_CELLS:
        g = win.read_train_tap(name, "grad")
        assert g[:, :, 1:-1, 1:-1].abs().sum().item() > 0, name
        g[:, :, 1:-1, 1:-1] = 0
        assert not g.any().item(), name


# ---------------------------------------------------------------------------------------------- 6. the tie rule
@pytest.mark.parametrize("join,k", [("max", 3), ("mean", 2)])
def test_tie_rule_on_identical_frames(params, join, k):
    """Stride 32: the per-frame route gradient is window_pool_bwd's alone (stride 8 and 16 also receive the next stage's
    data gradient), so each frame's equals the pooled gradient (max: ties all get it) or the pooled gradient / 2 exactly."""
    b, s = 2, 128
    x1 = np.random.default_rng(4).standard_normal((b, 3, s, s)).astype(np.float32)
    clips = np.repeat(x1[:, None], k, axis=1)
    gt, tg = _targets(b, s)
    win = _win(params, k, join)
    _step(win, clips, gt, tg)
    gp = win.read_grad_activation("pool.2")
    gf = win.read_grad_activation(ROUTE_CELLS[2])
    assert tuple(gf.shape)[0] == b * k and gp.abs().sum().item() > 0
    gf = gf.view((b, k) + tuple(gp.shape[1:]))
    want = gp if join == "max" else gp / float(k)
    for t in range(k):
        assert _same(gf[:, t].contiguous(), want.contiguous()), t
    for i in range(2):
        assert tuple(win.read_grad_activation("pool.%d" % i).shape)[0] == b


# ---------------------------------------------------------------------------------------------- 7. re-planning
def test_multiscale_replanning(params):
    import torch
    from videoyolo_amd import autograd
    k, join, b = 2, "max", 2
    win = _win(params, k, join)
    heads = _heads(params)
    for s in (320, 416):
        x = _clips(b, k, s, s, seed=s)
        x0 = x.copy()
        gt, tg = _targets(b, s, seed=s)
        lw, frame_routes = _step(win, x, gt, tg,
                                 between=lambda: [win.read_activation(c).cpu().numpy() for c in ROUTE_CELLS])
        assert np.array_equal(x, x0)
        pooled = [torch.from_numpy(np_pool(f, k, join)).cuda() for f in frame_routes]
        with autograd.record():
            lh = heads(*pooled, gt, *tg)
            autograd.backward([lh[0] + lh[1] + lh[2] + lh[3]])
        torch.cuda.synchronize()
        for i in range(4):
            assert _same(lw[i], lh[i]), (s, i)
        for name in ("yolo_blocks.0.body.0.0.weight", "transitions.0.0.weight", "yolo_outputs.1.prediction.bias"):
            assert np.array_equal(win.grad(name), heads.grad(name)), (s, name)
        assert win._plan == (b, s, s, True)
        for name in ("stages.1.0", "stages.2.0"):
            t = win.read_train_tap(name, "input")
            t[:, :, 1:-1, 1:-1] = 0
            assert not t.any().item(), (s, name)
        # inference at the new size after training (running statistics moved): the heads net on the pooled routes of a full
        # net, both holding the window net's current parameters
        cur = {n.replace(".model.", ".", 1): p.data() for n, p in win.collect_params().items()}
        xi = _clips(1, k, s, s, seed=s + 1)
        want = _heads(cur)(*_pooled_routes(cur, xi, k, join), return_index=True)
        for name, g, r in zip(("ids", "scores", "bboxes", "keep_idx"), win(xi, return_index=True), want):
            assert _same(g, r), (s, name)
