"""-m "not gpu": the windowed heads-only net (yolo3_no_backbone with k > 1) on the host — which constructor arguments give
it, the C-ABI constructor's argument checks, its plan against the heads-only net's (number for number: no per-frame plane),
the validation of routes and tables before the device is touched, the entry points refusing the wrong kind of net, and
parameter files.  Nothing here launches a kernel."""
import ctypes

import numpy as np
import pytest

from videoyolo_amd import _lib

C20 = ["c%d" % i for i in range(20)]


def _window(lib, h):
    k, join = ctypes.c_int32(-1), ctypes.c_int32(-1)
    _lib.check(lib.vy_net_window(h, ctypes.byref(k), ctypes.byref(join)))
    return k.value, join.value


@pytest.mark.parametrize("k,join", [(2, "mean"), (3, "max"), (5, "max")])
def test_constructor_routes_to_the_windowed_heads_net(k, join):
    import videoyolo_amd as vy
    net = vy.yolo3_no_backbone(C20, k=k, k_join_type=join, k_join_pos="early")
    assert type(net) is vy.YOLOV3NoBackboneWindow and isinstance(net, vy.YOLOV3NoBackbone)
    assert (net.k, net.k_join_type) == (k, join) and net._ONE_RANK
    assert _window(net._lib, net._h) == (k, {"max": _lib.VY_JOIN_MAX, "mean": _lib.VY_JOIN_MEAN}[join])
    # parameter names are the heads net's
    plain = vy.yolo3_no_backbone(C20)
    assert [(p.name, p.shape, p.kind, p.trainable, p.offset) for p in net.collect_params().values()] == \
           [(p.name, p.shape, p.kind, p.trainable, p.offset) for p in plain.collect_params().values()]


def test_without_k_the_constructor_returns_what_it_did():
    import videoyolo_amd as vy
    for kw in ({}, {"k": 1}, {"k": None}):
        net = vy.yolo3_no_backbone(C20, **kw)
        assert type(net) is vy.YOLOV3NoBackbone
        assert _window(net._lib, net._h) == (0, 0)


@pytest.mark.parametrize("kw", [
    dict(k=3, k_join_type="max", k_join_pos="late"), dict(k=3, k_join_type="cat", k_join_pos="early"),
    dict(k=3, k_join_type="max"), dict(k=3), dict(k=1, k_join_type="max", k_join_pos="early"),
    dict(k_join_type="mean", k_join_pos="early"), dict(k=0, k_join_type="max", k_join_pos="early"),
])
def test_other_temporal_combinations_are_not_implemented(kw):
    import videoyolo_amd as vy
    with pytest.raises(NotImplementedError):
        vy.yolo3_no_backbone(C20, **kw)


def test_c_abi_constructor_checks_its_arguments():
    lib = _lib.load()
    h = ctypes.c_void_p()
    for args in ((20, 1, _lib.VY_JOIN_MAX), (20, 0, _lib.VY_JOIN_MAX), (20, -3, _lib.VY_JOIN_MEAN), (20, 3, 2), (20, 3, -1),
                 (0, 3, _lib.VY_JOIN_MAX)):
        assert lib.vy_net_create_heads_window(*args, ctypes.byref(h)) == -1, args
        assert not h.value
    assert lib.vy_net_create_heads_window(20, 3, _lib.VY_JOIN_MAX, None) == -1
    _lib.check(lib.vy_net_create_heads_window(20, 4, _lib.VY_JOIN_MEAN, ctypes.byref(h)))
    try:
        assert _window(lib, h) == (4, _lib.VY_JOIN_MEAN)
    finally:
        lib.vy_net_destroy(h)


@pytest.mark.parametrize("k,join", [(2, _lib.VY_JOIN_MEAN), (3, _lib.VY_JOIN_MAX), (7, _lib.VY_JOIN_MAX)])
def test_plan_is_the_heads_nets_number_for_number(k, join):
    """Parameter table, conv list and both workspace sizes equal vy_net_create_heads': no per-frame plane crept in."""
    lib = _lib.load()
    heads, win = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(lib.vy_net_create_heads(20, ctypes.byref(heads)))
    _lib.check(lib.vy_net_create_heads_window(20, k, join, ctypes.byref(win)))
    try:
        assert lib.vy_net_num_params(win) == lib.vy_net_num_params(heads) == 106
        for i in range(lib.vy_net_num_params(heads)):
            a, b = _lib.ParamInfo(), _lib.ParamInfo()
            _lib.check(lib.vy_net_param_info(heads, i, ctypes.byref(a)))
            _lib.check(lib.vy_net_param_info(win, i, ctypes.byref(b)))
            assert bytes(a) == bytes(b), a.name
        assert lib.vy_net_param_bytes(win) == lib.vy_net_param_bytes(heads)
        assert lib.vy_net_num_convs(win) == lib.vy_net_num_convs(heads) == 23
        for i in range(lib.vy_net_num_convs(heads)):
            a, b = _lib.ConvInfo(), _lib.ConvInfo()
            _lib.check(lib.vy_net_conv_info(heads, i, ctypes.byref(a)))
            _lib.check(lib.vy_net_conv_info(win, i, ctypes.byref(b)))
            assert bytes(a) == bytes(b), a.name
        for b, h, w in ((2, 64, 64), (16, 416, 416)):
            need = lib.vy_net_workspace_bytes(heads, b, h, w)
            assert need > 0 and lib.vy_net_workspace_bytes(win, b, h, w) == need
            need = lib.vy_net_train_workspace_bytes(heads, b, h, w)
            assert need > 0 and lib.vy_net_train_workspace_bytes(win, b, h, w) == need
        # the split conv modes are accepted, as on the heads net (a full window net refuses them)
        assert lib.vy_net_set_conv_mode(win, _lib.VY_CONV_SPLIT_BF16X3) == 0
        assert lib.vy_net_set_conv_mode(heads, _lib.VY_CONV_SPLIT_BF16X3) == 0
        assert lib.vy_net_workspace_bytes(win, 2, 64, 64) == lib.vy_net_workspace_bytes(heads, 2, 64, 64) > 0
    finally:
        lib.vy_net_destroy(heads)
        lib.vy_net_destroy(win)


def _bank(t, h=64, w=64):
    h8, w8 = -(-h // 8), -(-w // 8)
    return [np.zeros((t, 256, h8, w8), np.float32), np.zeros((t, 512, -(-h8 // 2), -(-w8 // 2)), np.float32),
            np.zeros((t, 1024, -(-h8 // 4), -(-w8 // 4)), np.float32)]


def _clips(b, k, h=64, w=64):
    return [f.reshape((b, k) + f.shape[1:]) for f in _bank(b * k, h, w)]


@pytest.mark.parametrize("bad", ["rank4", "k", "sizes", "batch", "channels"])
def test_five_d_routes_are_checked_before_the_device(bad):
    import videoyolo_amd as vy
    net = vy.yolo3_no_backbone(C20, k=3, k_join_type="max", k_join_pos="early")
    f = _clips(2, 3)
    if bad == "rank4":
        f = _bank(6)
    elif bad == "k":
        f = _clips(3, 2)
    elif bad == "sizes":
        f[1] = np.zeros((2, 3, 512, 4, 5), np.float32)
    elif bad == "batch":
        f[2] = f[2][:1]
    elif bad == "channels":
        f[0] = np.zeros((2, 3, 128, 8, 8), np.float32)
    with pytest.raises(ValueError, match="route"):
        net(*f)


@pytest.mark.parametrize("bad", ["rank5", "k", "sizes", "equal_T", "negative", "513", "float", "flat"])
def test_bank_and_table_are_checked_before_the_device(bad):
    import videoyolo_amd as vy
    k = 3
    net = vy.yolo3_no_backbone(C20, k=k, k_join_type="mean", k_join_pos="early")
    f, table = _bank(7), np.array([[0, 1, 2], [6, 6, 5]], np.int64)
    if bad == "rank5":
        f = _clips(2, 3)
    elif bad == "k":
        table = table[:, :2]
    elif bad == "sizes":
        f[2] = np.zeros((7, 1024, 3, 2), np.float32)
    elif bad == "equal_T":
        table[1, 2] = 7
    elif bad == "negative":
        table[0, 0] = -1
    elif bad == "513":
        table = np.zeros((171, 3), np.int32)  # 171 x 3 = 513 entries
    elif bad == "float":
        table = table.astype(np.float32)
    elif bad == "flat":
        table = table.reshape(-1)
    with pytest.raises(ValueError):
        net.from_bank(*f, table)


def test_a_full_table_passes_the_check_and_stops_at_the_device():
    """B * k = 512 entries (the limit), odd route sizes, repeated frames: valid, so the call stops at the device check."""
    import videoyolo_amd as vy
    net = vy.yolo3_no_backbone(C20, k=4, k_join_type="max", k_join_pos="early")
    table = np.arange(512).reshape(128, 4) % 5
    with pytest.raises(RuntimeError, match="not on a device"):
        net.from_bank(*_bank(5, 609, 611), table)
    with pytest.raises(RuntimeError, match="not on a device"):
        net(*_clips(128, 4))
    with pytest.raises(ValueError, match="table entries"):
        net(*_clips(129, 4))
    with pytest.raises(ValueError, match="clips_per_step"):
        net.detect_video_features(*_bank(5), clips_per_step=129)


def test_image_entry_points_refuse_it():
    import videoyolo_amd as vy
    net = vy.yolo3_no_backbone(C20, k=2, k_join_type="max", k_join_pos="early")
    for fn in (net.extract_features, net.profile, net.detect_two_streams, net.load_darknet53_backbone):
        with pytest.raises(NotImplementedError):
            fn(np.zeros((1, 3, 64, 64), np.float32))
    assert not hasattr(net, "video")


def test_entries_of_another_kind_fail_with_state_error():
    """Image, *_routes and video entries on a windowed heads net, and *_bank entries on every other kind, return VY_ERR_STATE
    before touching anything (the bogus device pointers are never dereferenced, no workspace is bound)."""
    lib = _lib.load()
    full, heads, clip, win = (ctypes.c_void_p() for _ in range(4))
    _lib.check(lib.vy_net_create(20, ctypes.byref(full)))
    _lib.check(lib.vy_net_create_heads(20, ctypes.byref(heads)))
    _lib.check(lib.vy_net_create_window(20, 3, _lib.VY_JOIN_MAX, ctypes.byref(clip)))
    _lib.check(lib.vy_net_create_heads_window(20, 3, _lib.VY_JOIN_MAX, ctypes.byref(win)))
    p = ctypes.c_void_p(0x1000)
    tab = (ctypes.c_int32 * 6)(0, 1, 2, 3, 4, 5)
    try:
        calls = [
            (lib.vy_net_forward_infer, (p, p, p, p, None, None)),
            (lib.vy_net_forward_features, (p, p, p, p, None)),
            (lib.vy_net_train_forward, (p, p, 1, p, p, p, p, p, p, None)),
            (lib.vy_net_train_mode_forward, (p, p, p, p, p, p, None)),
            (lib.vy_net_train_backward, (p, None)),
            (lib.vy_net_forward_infer_routes, (p, p, p, p, p, p, None, None)),
            (lib.vy_net_train_forward_routes, (p, p, p, p, 1, p, p, p, p, p, p, None)),
            (lib.vy_net_train_mode_forward_routes, (p, p, p, p, p, p, p, p, None)),
            (lib.vy_net_video_push, (p, tab, None)),
            (lib.vy_net_video_detect, (tab, p, p, p, None, None)),
            (lib.vy_net_video_read_slot, (0, p, p, p, None)),
            (lib.vy_net_bind_video, (p, 1 << 30, 4, 2, 8, 64, 64, None)),
        ]
        for fn, args in calls:
            assert fn(win, *args) == -2, fn.__name__
            assert lib.vy_last_error().decode()
        assert lib.vy_net_video_workspace_bytes(win, 4, 2, 8, 64, 64) == 0
        bank_calls = [
            (lib.vy_net_forward_infer_bank, (p, p, p, 6, tab, p, p, p, None, None)),
            (lib.vy_net_train_forward_bank, (p, p, p, 6, tab, p, 1, p, p, p, p, p, p, None)),
            (lib.vy_net_train_mode_forward_bank, (p, p, p, 6, tab, p, p, p, p, p, None)),
        ]
        for h in (full, heads, clip):
            for fn, args in bank_calls:
                assert fn(h, *args) == -2, fn.__name__
                assert "bank" in lib.vy_last_error().decode()
        # the right kind with nothing bound is a different error: the state of the net, not of the entry
        for fn, args in bank_calls:
            assert fn(win, *args) == -2
            assert "not bound" in lib.vy_last_error().decode()
        assert lib.vy_net_train_backward_routes(win, None, None, None, None) == -2
        assert "not bound" in lib.vy_last_error().decode()
        assert lib.vy_net_train_backward_routes(heads, None, None, None, None) == -1  # a heads net still needs its routes
    finally:
        for h in (full, heads, clip, win):
            lib.vy_net_destroy(h)


def test_files_of_every_kind_of_net_load(tmp_path):
    import copy
    import videoyolo_amd as vy
    src = {}
    src["window"] = vy.yolo3_darknet53(C20, pretrained_base=False, k=3, k_join_type="max", k_join_pos="early")
    src["single"] = vy.yolo3_darknet53(C20, pretrained_base=False)
    src["heads"] = vy.yolo3_no_backbone(C20)
    for i, (kind, net) in enumerate(src.items()):
        net.initialize(init="synthetic", seed=11 + i)
        f = str(tmp_path / (kind + ".params"))
        net.save_parameters(f)
        got = vy.yolo3_no_backbone(C20, k=3, k_join_type="max", k_join_pos="early")
        if kind != "heads":
            with pytest.raises(AssertionError, match="not present in the net"):
                got.load_parameters(f)
        got.load_parameters(f, ignore_extra=True)
        for name, p in got.collect_params().items():
            assert np.array_equal(p.data(), net.collect_params()[name].data()), (kind, name)
    # its own file round-trips, and copies keep the kind, k and join
    f = str(tmp_path / "own.params")
    got.save_parameters(f)
    back = vy.yolo3_no_backbone(C20, k=2, k_join_type="mean", k_join_pos="early")
    back.load_parameters(f)
    twin = copy.deepcopy(back)
    assert type(twin) is vy.YOLOV3NoBackboneWindow and (twin.k, twin.k_join_type) == (2, "mean")
    assert np.array_equal(twin.collect_params()["yolo_blocks.0.tip.0.weight"].data(),
                          got.collect_params()["yolo_blocks.0.tip.0.weight"].data())
    back.reset_class(["a", "b"])
    assert type(back) is vy.YOLOV3NoBackboneWindow and (back.k, back.num_class) == (2, 2)
