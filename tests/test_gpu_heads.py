"""-m gpu: the heads-only net (yolo3_no_backbone) and the features-only forward against the full net.  The full net is
bit-exact to the CPU checker, and the heads net runs the same launches on the same planes, so every bar here is
bit-equality with the full net: the extracted routes, the detections, the losses, every head gradient, the head BatchNorm
statistics and the SGD step.  The caller's route buffers are never written, and the plane borders stay zero."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import frames

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 20
CLASSES = ["c%d" % i for i in range(C)]
ROUTE_CELLS = ("stages.0.14.body.1", "stages.1.8.body.1", "stages.2.4.body.1")  # features[14], [23], [28]


def _params(seed=233):
    from videoyolo_amd import init
    from oracle import yolo3_oracle as O
    return init.synthetic_params(O.param_shapes(C), seed=seed)


def _full(params, keep=False, freeze_base=False):
    import videoyolo_amd as vy
    net = vy.yolo3_darknet53(CLASSES, pretrained_base=False, freeze_base=freeze_base)
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


def _x(b, h, w, seed=5):
    return np.random.default_rng(seed).standard_normal((b, 3, h, w)).astype(np.float32)


def _bits(t):
    import torch
    return t.detach().contiguous().view(torch.int32).cpu()


def _same(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def params():
    return _params()


# ---------------------------------------------------------------------------------------------- 1. extract_features
@pytest.mark.parametrize("b,h,w", [(4, 416, 416), (2, 608, 608), (1, 609, 611), (3, 96, 32)])
def test_extract_features_equals_the_keep_activations_taps(params, b, h, w):
    x = _x(b, h, w)
    plain = _full(params)
    f = plain.extract_features(x)
    assert plain._lib.vy_net_get_conv_mode(plain._h) == 0
    keep = _full(params, keep=True)
    keep(x)
    for i, (cell, ch, s) in enumerate(zip(ROUTE_CELLS, (256, 512, 1024), (8, 16, 32))):
        assert tuple(f[i].shape) == (b, ch, -(-h // s), -(-w // s))
        assert _same(f[i], keep.read_activation(cell)), cell
    # a detection forward after the features-only one is unaffected (same plan, every plane rewritten)
    ids, scores, _ = plain(x)
    rids, rscores, _ = keep(x)
    assert _same(ids, rids) and _same(scores, rscores)


# ---------------------------------------------------------------------------------------------- 2. inference
@pytest.mark.parametrize("b,h,w", [(16, 416, 416), (64, 608, 608), (1, 609, 611)])
def test_heads_detections_equal_the_full_net(params, b, h, w):
    x = _x(b, h, w, seed=b)
    full = _full(params)
    heads = _heads(params)
    f = full.extract_features(x)
    for nms in ((0.45, 400, 100), (0.0, 400, 100), (0.45, -1, 100)):  # default; NMS off (raw (B, N*C, 6)); nms_topk=-1
        full.set_nms(*nms)
        heads.set_nms(*nms)
        want = full(x, return_index=True)
        got = heads(*f, return_index=True)
        for name, g, r in zip(("ids", "scores", "bboxes", "keep_idx"), got, want):
            assert _same(g, r), (nms, name)
        if nms[0] == 0.0:
            n = 3 * sum(-(-h // s) * -(-w // s) for s in (8, 16, 32))
            assert tuple(got[0].shape) == (b, n * C, 1)
        for i in range(3):
            assert _same(heads.read_head(i), full.read_head(i)), (nms, i)


def test_heads_detections_against_the_cpu_checker(params):
    from oracle import yolo3_oracle as O
    x = frames(2, 96)
    full = _full(params)
    heads = _heads(params)
    ids, scores, bboxes, keep = [t.cpu().numpy() for t in heads(*full.extract_features(x), return_index=True)]
    orc = O.OracleYolo3(C, params)
    raw = orc.raw_heads(x)
    for i in range(3):
        assert np.array_equal(heads.read_head(i).cpu().numpy(), raw[i]), i
    r_ids, r_scores, r_bboxes, r_keep = orc(x)
    assert np.array_equal(keep, r_keep) and np.array_equal(ids, r_ids)
    assert np.allclose(scores, r_scores, rtol=0, atol=1e-4)
    fin = np.isfinite(r_bboxes)
    assert np.allclose(bboxes[fin], r_bboxes[fin], rtol=0, atol=1e-4)


# ---------------------------------------------------------------------------------------------- 3-5. training
def _targets(b, s, seed=2):
    from oracle import targets_oracle as T
    gt_boxes, gt_ids = T.synthetic_gt(b, s, C, m=3, seed=seed, pad_to=5)
    return gt_boxes, T.prefetch_targets(C, s, s, gt_boxes, gt_ids)


def _routes_after_forward(full):
    return tuple(full.read_activation(c) for c in ROUTE_CELLS)


def _head_names(net):
    return [n for n in net.collect_params()]


def _conv_names(net):
    import ctypes
    from videoyolo_amd import _lib
    out = []
    for i in range(net._lib.vy_net_num_convs(net._h)):
        info = _lib.ConvInfo()
        _lib.check(net._lib.vy_net_conv_info(net._h, i, ctypes.byref(info)))
        out.append(info.name.decode())
    return out


def _step_pair(full, heads, x, gt, tg, check_untouched=False):
    """One recorded forward + backward on each net; returns the two loss tuples and the routes the heads got."""
    import torch
    from videoyolo_amd import autograd
    with autograd.record():
        lf = full(x, gt, *tg)
        routes = _routes_after_forward(full)
        autograd.backward([lf[0] + lf[1] + lf[2] + lf[3]])
    before = [r.clone() for r in routes]
    with autograd.record():
        lh = heads(*routes, gt, *tg)
        autograd.backward([lh[0] + lh[1] + lh[2] + lh[3]])
    torch.cuda.synchronize()
    if check_untouched:
        for r, r0 in zip(routes, before):
            assert _same(r, r0), "a route buffer of the caller was written"
    return lf, lh, routes


@pytest.mark.parametrize("b,s", [(16, 416), (4, 320)])
def test_heads_training_step_equals_the_frozen_full_net(params, b, s):
    import videoyolo_amd as vy
    from videoyolo_amd import autograd
    x = _x(b, s, s, seed=3)
    gt, tg = _targets(b, s)
    full = _full(params, freeze_base=True)
    heads = _heads(params)

    # train mode without recording: the 8-tuple (BatchNorm on batch statistics, running stats updated on both nets)
    with autograd.train_mode():
        of = full(x)
        oh = heads(*_routes_after_forward(full))
    for k in (0, 4, 5, 6, 7):
        assert _same(oh[k], of[k]), k
    for k in (1, 2, 3):
        for a, r in zip(oh[k], of[k]):
            assert np.array_equal(a, r), k

    lf, lh, routes = _step_pair(full, heads, x, gt, tg, check_untouched=True)
    for i in range(4):
        assert _same(lh[i], lf[i]), i
    # the accumulation plan of every head conv is the full net's: that is what makes bit-equality the expectation
    for name in _conv_names(heads):
        assert heads.train_conv_plan(name) == full.train_conv_plan(name), name
    for name in _head_names(heads):
        p = heads.collect_params()[name]
        if p.trainable:
            assert np.array_equal(heads.grad(name), full.grad(name)), name
        else:
            assert np.array_equal(p.data(), full.collect_params()[name].data()), name
    for name in _conv_names(heads):
        if "prediction" in name:
            continue
        assert _same(heads.read_train_tap(name, "bn"), full.read_train_tap(name, "bn")), name

    # 4. every plane border of the heads net is still zero (the imported routes' planes and the gradient planes)
    for name in ("yolo_blocks.0.body.0", "yolo_blocks.1.body.0", "yolo_blocks.2.body.0", "yolo_blocks.1.body.1"):
        t = heads.read_train_tap(name, "input")
        inner = t[:, :, 1:-1, 1:-1].clone()
        t[:, :, 1:-1, 1:-1] = 0
        assert not t.any().item(), name
        assert inner.abs().sum().item() > 0, name
    for name in ("transitions.0", "transitions.1", "yolo_blocks.0.body.4"):
        g = heads.read_train_tap(name, "grad")
        g[:, :, 1:-1, 1:-1] = 0
        assert not g.any().item(), name

    # one Trainer.step: head weights and running statistics equal those of the freeze_base=True full net
    tf = vy.Trainer(full.collect_params(), 'sgd', {'learning_rate': 1e-3, 'wd': 5e-4, 'momentum': 0.9})
    th = vy.Trainer(heads.collect_params(), 'sgd', {'learning_rate': 1e-3, 'wd': 5e-4, 'momentum': 0.9})
    tf.step(b)
    th.step(b)
    for name in _head_names(heads):
        assert np.array_equal(heads.collect_params()[name].data(), full.collect_params()[name].data()), name
    assert not np.array_equal(heads.collect_params()["transitions.1.0.weight"].data(),
                              params["transitions.1.0.weight"])
    # the frozen backbone did not move
    assert np.array_equal(full.collect_params()["stages.1.3.body.1.0.weight"].data(), params["stages.1.3.body.1.0.weight"])


def test_multiscale_training_replans_and_stays_bit_equal(params):
    full = _full(params, freeze_base=True)
    heads = _heads(params)
    for s in (320, 608, 416):
        x = _x(2, s, s, seed=s)
        gt, tg = _targets(2, s, seed=s)
        lf, lh, _ = _step_pair(full, heads, x, gt, tg)
        for i in range(4):
            assert _same(lh[i], lf[i]), (s, i)
        for name in ("yolo_blocks.0.body.0.0.weight", "yolo_blocks.1.body.0.0.weight", "transitions.0.0.weight",
                     "yolo_blocks.2.tip.1.gamma", "yolo_outputs.1.prediction.bias"):
            assert np.array_equal(heads.grad(name), full.grad(name)), (s, name)
        assert heads._plan == (2, s, s, True)


# ---------------------------------------------------------------------------------------------- 6. the example
def test_train_heads_example_runs():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "examples/train_heads.py", "--size", "320", "--batch", "4", "--frames", "8",
                        "--steps", "3"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600,
                       universal_newlines=True)
    assert p.returncode == 0, p.stdout[-3000:]
    assert "extracted" in p.stdout and "mAP" in p.stdout
