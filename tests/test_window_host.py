"""-m "not gpu": the k-frame clip net (yolo3_darknet53 with k > 1, early join) on the host — the constructor contract,
the C-ABI's argument errors and refusals, the parameter table against the single-frame net's, the reference's
``stages.N.model.*`` keys and .params round trips in both key forms, input-shape checks, and the test-side pooling
reference against an independent torch float64 twin.  Nothing here launches a kernel."""
import ctypes

import numpy as np
import pytest

from videoyolo_amd import _lib
from test_gpu_window import np_pool, _Pool

C20 = ["c%d" % i for i in range(20)]


def _window(classes=C20, k=3, join="max"):
    import videoyolo_amd as vy
    return vy.yolo3_darknet53(classes, pretrained_base=False, k=k, k_join_type=join, k_join_pos="early")


def test_constructor_contract():
    import videoyolo_amd as vy
    for k, join in ((2, "max"), (3, "mean"), (8, "max")):
        net = _window(k=k, join=join)
        assert isinstance(net, vy.YOLOV3Window) and isinstance(net, vy.YOLOV3)
        assert (net.k, net.k_join_type) == (k, join)
        kk, jj = ctypes.c_int32(), ctypes.c_int32()
        _lib.check(net._lib.vy_net_window(net._h, ctypes.byref(kk), ctypes.byref(jj)))
        assert (kk.value, jj.value) == (k, {"max": _lib.VY_JOIN_MAX, "mean": _lib.VY_JOIN_MEAN}[join])
    single = vy.yolo3_darknet53(C20, pretrained_base=False, k=1)
    assert type(single) is vy.YOLOV3
    kk = ctypes.c_int32(7)
    _lib.check(single._lib.vy_net_window(single._h, ctypes.byref(kk), None))
    assert kk.value == 0
    for bad in (dict(k=3), dict(k=3, k_join_type="max"), dict(k=3, k_join_type="max", k_join_pos="late"),
                dict(k=3, k_join_type="cat", k_join_pos="early"), dict(k=3, k_join_type="max", k_join_pos="early",
                                                                       block_conv_type="3"),
                dict(k=3, k_join_type="max", k_join_pos="early", rnn_pos="early"),
                dict(k=3, k_join_type="max", k_join_pos="early", corr_pos="early"),
                dict(k=3, k_join_type="max", k_join_pos="early", motion_stream="flownet"),
                dict(k=1, k_join_type="max", k_join_pos="early"), dict(k_join_type="max")):
        with pytest.raises(NotImplementedError):
            vy.yolo3_darknet53(C20, pretrained_base=False, **bad)


def test_create_window_argument_errors():
    lib = _lib.load()
    h = ctypes.c_void_p()
    for num_class, k, join in ((20, 1, 0), (20, 0, 0), (20, -2, 1), (20, 3, 2), (20, 3, -1), (0, 3, 0)):
        assert lib.vy_net_create_window(num_class, k, join, ctypes.byref(h)) == -1, (num_class, k, join)
    assert lib.vy_net_create_window(20, 3, 0, None) == -1
    _lib.check(lib.vy_net_create_window(20, 2, 1, ctypes.byref(h)))
    try:
        assert lib.vy_net_set_conv_mode(h, _lib.VY_CONV_SPLIT_BF16X3) == -4
        assert lib.vy_net_set_conv_mode(h, _lib.VY_CONV_SPLIT_BF16X3_TRAIN) == -4
        _lib.check(lib.vy_net_set_conv_mode(h, _lib.VY_CONV_EXACT_FP32))
        # a window net sizes more workspace than the single-frame net at the same clip count (B*k frames in the stages),
        # and less than the single-frame net at B*k frames (its heads run on B clips)
        full = ctypes.c_void_p()
        _lib.check(lib.vy_net_create(20, ctypes.byref(full)))
        try:
            for fn in (lib.vy_net_workspace_bytes, lib.vy_net_train_workspace_bytes):
                w, f1, f2 = fn(h, 4, 320, 320), fn(full, 4, 320, 320), fn(full, 8, 320, 320)
                assert 0 < f1 < w < f2, (w, f1, f2)
        finally:
            lib.vy_net_destroy(full)
    finally:
        lib.vy_net_destroy(h)


def test_refused_entries_return_state():
    lib = _lib.load()
    h = ctypes.c_void_p()
    _lib.check(lib.vy_net_create_window(20, 3, 0, ctypes.byref(h)))
    try:
        p = ctypes.c_void_p(16)  # never dereferenced: the kind check comes first
        assert lib.vy_net_forward_features(h, p, p, p, p, None) == -2
        n = ctypes.c_int32(4)
        stats = (_lib.LaunchStat * 4)()
        assert lib.vy_net_profile_infer(h, p, p, p, p, stats, ctypes.byref(n), None) == -2
        assert lib.vy_net_forward_infer_routes(h, p, p, p, p, p, p, p, None) == -2
        assert lib.vy_net_train_forward_routes(h, p, p, p, p, 0, p, p, p, p, p, p, None) == -2
        assert lib.vy_net_train_mode_forward_routes(h, p, p, p, p, p, p, p, p, None) == -2
        assert lib.vy_net_train_backward_routes(h, p, p, p, None) == -2
    finally:
        lib.vy_net_destroy(h)


@pytest.mark.parametrize("num_class", [1, 20, 80])
def test_param_table_is_the_single_frame_table(num_class):
    lib = _lib.load()
    a, b = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(lib.vy_net_create(num_class, ctypes.byref(a)))
    _lib.check(lib.vy_net_create_window(num_class, 4, 1, ctypes.byref(b)))
    try:
        assert lib.vy_net_num_params(a) == lib.vy_net_num_params(b) == 366
        assert lib.vy_net_param_bytes(a) == lib.vy_net_param_bytes(b)
        for i in range(lib.vy_net_num_params(a)):
            pa, pb = _lib.ParamInfo(), _lib.ParamInfo()
            _lib.check(lib.vy_net_param_info(a, i, ctypes.byref(pa)))
            _lib.check(lib.vy_net_param_info(b, i, ctypes.byref(pb)))
            assert bytes(pa) == bytes(pb), i
    finally:
        lib.vy_net_destroy(a)
        lib.vy_net_destroy(b)


def test_keys_and_params_round_trips(tmp_path):
    import videoyolo_amd as vy
    net = _window(k=3, join="mean")
    single = vy.yolo3_darknet53(C20, pretrained_base=False)
    keys, skeys = list(net.collect_params()), list(single.collect_params())
    assert len(keys) == len(skeys) == 366
    for k, s in zip(keys, skeys):
        if s.startswith("stages."):
            n, rest = s[len("stages."):].split(".", 1)
            assert k == "stages.%s.model.%s" % (n, rest)
        else:
            assert k == s
    assert len(net.collect_params('.*beta|.*gamma|.*bias')) == 147
    assert "stages.0.model.0.1.gamma" in net.collect_params('.*gamma')
    # a single-frame file loads into the window net (and the window net's file carries the .model. keys)
    single.initialize(init="synthetic", seed=4)
    f1 = str(tmp_path / "single.params")
    single.save_parameters(f1)
    net.load_parameters(f1)
    for k, s in zip(keys, skeys):
        assert np.array_equal(net.collect_params()[k].data(), single.collect_params()[s].data()), k
    f2 = str(tmp_path / "window.params")
    net.save_parameters(f2)
    with np.load(f2) as z:
        names = set(z.files)
    assert "stages.1.model.3.body.1.0.weight" in names and "stages.1.3.body.1.0.weight" not in names
    other = _window(k=3, join="mean")
    other.load_parameters(f2)
    for k in keys:
        assert np.array_equal(other.collect_params()[k].data(), net.collect_params()[k].data()), k
    # mxnet container, both key forms
    f3 = str(tmp_path / "window_mx.params")
    net.save_parameters(f3, format="mxnet")
    other = _window(k=3, join="mean")
    other.load_parameters(f3)
    assert np.array_equal(other.collect_params()["stages.2.model.4.body.1.0.weight"].data(),
                          single.collect_params()["stages.2.4.body.1.0.weight"].data())
    # freeze_base and reset_class keep the window configuration
    fz = vy.yolo3_darknet53(C20, pretrained_base=False, k=2, k_join_type="max", k_join_pos="early", freeze_base=True)
    frozen = [p for p in fz.collect_params().values() if p.grad_req == "null" and p.trainable]
    assert frozen and all(p.name.startswith("stages.") and ".model." in p.name for p in frozen)
    net.reset_class(C20[:5])
    assert isinstance(net, vy.YOLOV3Window) and net.k == 3 and net.num_class == 5
    assert list(net.collect_params())[0] == "stages.0.model.0.0.weight"
    import copy
    tw = copy.deepcopy(net)
    assert tw.k == 3 and tw.k_join_type == "mean"


def test_input_shape_and_world_checks(monkeypatch):
    import videoyolo_amd as vy
    from videoyolo_amd import parallel
    net = _window(k=3, join="max")
    with pytest.raises(ValueError, match=r"\(B, k, 3, H, W\)"):
        net(np.zeros((2, 3, 64, 64), np.float32))
    with pytest.raises(ValueError, match=r"k = 3"):
        net(np.zeros((2, 2, 3, 64, 64), np.float32))
    for fn in (net.extract_features, net.profile, net.detect_two_streams):
        with pytest.raises(NotImplementedError):
            fn(np.zeros((1, 3, 3, 64, 64), np.float32))
    monkeypatch.setattr(parallel, "world_size", lambda: 2)
    with pytest.raises(NotImplementedError):
        net.forward_train(np.zeros((1, 3, 3, 64, 64), np.float32), *([None] * 6))
    with pytest.raises(NotImplementedError):
        net.forward_train_mode(np.zeros((1, 3, 3, 64, 64), np.float32))
    assert vy.YOLOV3Window._key("stages.1.2.body.0.0.weight") == "stages.1.model.2.body.0.0.weight"


@pytest.mark.parametrize("join", ["max", "mean"])
def test_pool_reference_against_torch_float64(join):
    """np_pool / _Pool (the test-side references of test_gpu_window.py) against a plain torch float64 formulation, k = 3:
    forward values, and the backward rule (mean: g / k everywhere; max: g to every frame that equals the max)."""
    import torch
    k = 3
    rng = np.random.default_rng(1)
    f = rng.standard_normal((2 * k, 8, 5, 7)).astype(np.float32)
    f[1] = f[0]                    # ties: clip 0's first two frames are identical
    f[5, :, 2] = f[3, :, 2]        # clip 1: frames 0 and 2 tie on one row
    got = np_pool(f, k, join)
    ref = torch.from_numpy(f).double().view(2, k, 8, 5, 7)
    want = ref.amax(1) if join == "max" else ref.sum(1) / k
    np.testing.assert_allclose(got, want.numpy(), rtol=1e-6, atol=1e-6)
    if join == "max":  # the earliest frame's bits on ties (all equal here anyway), exact
        assert np.array_equal(got, want.float().numpy())
    x = torch.from_numpy(f).double().requires_grad_(True)
    g = torch.from_numpy(rng.standard_normal((2, 8, 5, 7))).double()
    (_Pool.apply(x, k, join) * g).sum().backward()
    gx = x.grad.view(2, k, 8, 5, 7)
    if join == "mean":
        assert torch.allclose(gx, (g / k)[:, None].expand_as(gx))
    else:
        eq = (ref == ref.amax(1, keepdim=True)).double()
        assert torch.equal(gx, g[:, None] * eq)
        assert torch.equal(gx[0, 0], gx[0, 1])              # both tied frames get the full gradient
        assert torch.equal(eq[0, 0], eq[0, 1]) and (eq[0, 0] * eq[0, 1]).sum() > 0  # ties where frames 0 and 1 are the max
