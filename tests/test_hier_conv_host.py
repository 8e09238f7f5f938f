"""-m "not gpu": the hierarchical net with the learned join (YOLOV3HierConv, vy_net_create_hier_join) on the host — the C-ABI
constructor and its codes, its tables against the single-frame net's and the max net's, the join parameters, the tap names
both ways, the workspace sizes, keys, weight shapes, files, initial values, copies, freeze_base, what it refuses, and the
factory, which still raises for 'conv'.  Nothing here launches a kernel."""
import copy
import ctypes

import numpy as np
import pytest

import hier_cells
import hier_join_model as J
import test_hier_host as HH
from videoyolo_amd import _lib

C20 = HH.C20
LISTS = HH.LISTS
MAX, CONV = _lib.VY_HJOIN_MAX, _lib.VY_HJOIN_CONV
CHANNELS = (32, 64, 128, 256)  # zip(windows, channels), h_darknet.py:97-101
LEAVES = ("0.weight", "1.gamma", "1.beta", "1.running_mean", "1.running_var")


def _make(lib, n_pools, join=CONV, num_class=20):
    h = ctypes.c_void_p()
    _lib.check(lib.vy_net_create_hier_join(num_class, n_pools, join, ctypes.byref(h)))
    return h


def _params(lib, h):
    out = []
    for i in range(lib.vy_net_num_params(h)):
        info = _lib.ParamInfo()
        _lib.check(lib.vy_net_param_info(h, i, ctypes.byref(info)))
        out.append(info)
    return out


def _conv(hier=(3, 3, 1, 1, 1), **kw):
    import videoyolo_amd as vy
    return vy.YOLOV3HierConv(C20, hierarchical=list(hier), **kw)


# ------------------------------------------------------------------------------------------------ the C-ABI constructor
def test_constructor_codes():
    lib = _lib.load()
    h = ctypes.c_void_p()
    for args in ((20, 0, CONV), (20, 5, CONV), (20, -1, MAX), (20, 2, 2), (20, 2, -1), (0, 2, CONV), (1001, 2, MAX)):
        assert lib.vy_net_create_hier_join(*args, ctypes.byref(h)) == -1, args
        assert lib.vy_last_error()
    assert lib.vy_net_create_hier_join(20, 2, CONV, None) == -1
    assert "VY_HJOIN" in _err(lib, 20, 2, 7)


def _err(lib, *args):
    h = ctypes.c_void_p()
    assert lib.vy_net_create_hier_join(*args, ctypes.byref(h)) == -1
    return lib.vy_last_error().decode()


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_join_max_is_the_max_net(n):
    lib = _lib.load()
    a, b = HH._make(lib, n), _make(lib, n, MAX)
    try:
        pa, pb = _params(lib, a), _params(lib, b)
        assert len(pa) == len(pb) and all(bytes(x) == bytes(y) for x, y in zip(pa, pb))
        assert lib.vy_net_param_bytes(a) == lib.vy_net_param_bytes(b)
        assert [bytes(x) for x in HH._conv_infos(lib, a)] == [bytes(x) for x in HH._conv_infos(lib, b)]
        assert HH._hier(lib, a) == HH._hier(lib, b) == (n, 3 ** n)
        for fn in (lib.vy_net_workspace_bytes, lib.vy_net_train_workspace_bytes):
            assert fn(a, 2, 64, 64) == fn(b, 2, 64, 64) > 0
        assert HH._tap_frames(lib, b, "hpool.0") == 3 ** (n - 1)
    finally:
        lib.vy_net_destroy(a)
        lib.vy_net_destroy(b)


# ------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("hier", LISTS)
def test_single_frame_table_is_a_prefix_and_the_joins_follow(hier):
    lib = _lib.load()
    n = hier.index(1)
    base, h, mx = HH._make(lib, 0), _make(lib, n), HH._make(lib, n)
    try:
        pb, ph = _params(lib, base), _params(lib, h)
        assert len(ph) == len(pb) + 5 * n
        for x, y in zip(pb, ph):
            assert bytes(x) == bytes(y), x.name  # names, shapes, kinds, flags, offsets and sizes
        end = pb[-1].offset + (pb[-1].size + 63) // 64 * 64
        kinds = (0, 1, 2, 3, 4)  # weight, gamma, beta, running_mean, running_var
        for i in range(n):
            for j, leaf in enumerate(LEAVES):
                p = ph[len(pb) + 5 * i + j]
                assert p.name.decode() == "hjoin.%d.%s" % (i, leaf)
                shape = (CHANNELS[i], 3) if j == 0 else (CHANNELS[i],)
                assert (p.ndim, tuple(p.shape[:p.ndim])) == (len(shape), shape), p.name
                assert p.size == int(np.prod(shape)) and p.kind == kinds[j]
                assert p.backbone == 1 and p.trainable == (1 if j < 3 else 0), p.name
                assert p.offset == end and p.offset % 64 == 0, p.name  # appended behind the last single-frame tensor
                end += (p.size + 63) // 64 * 64
        assert lib.vy_net_param_bytes(h) > lib.vy_net_param_bytes(base)
        # the conv list is the max net's, and so is every cell's frame multiplier: the join is not a conv
        assert [bytes(x) for x in HH._conv_infos(lib, h)] == [bytes(x) for x in HH._conv_infos(lib, mx)]
        for c in HH._conv_infos(lib, h):
            assert HH._tap_frames(lib, h, c.name.decode()) == HH._tap_frames(lib, mx, c.name.decode()), c.name
        assert HH._hier(lib, h) == (n, 3 ** n)
    finally:
        for x in (base, h, mx):
            lib.vy_net_destroy(x)


@pytest.mark.parametrize("hier", LISTS)
def test_tap_names_both_ways(hier):
    lib = _lib.load()
    n = hier.index(1)
    h, mx = _make(lib, n), HH._make(lib, n)
    f = ctypes.c_int32(-7)
    try:
        cells = J.join_graph(20, hier)
        assert [c["name"] for c in cells if c.get("join")] == ["hjoin.%d" % i for i in range(n)]
        for c in cells:
            assert HH._tap_frames(lib, h, c["name"]) == c["fm"], c["name"]
        for i in range(n):
            assert HH._tap_frames(lib, h, "hjoin.%d" % i) == HH._tap_frames(lib, mx, "hpool.%d" % i) == 3 ** (n - 1 - i)
            assert lib.vy_net_tap_frames(h, ("hpool.%d" % i).encode(), ctypes.byref(f)) == -1
            assert lib.vy_net_tap_frames(mx, ("hjoin.%d" % i).encode(), ctypes.byref(f)) == -1
        for name in ("hjoin.%d" % n, "hjoin.", "hjoin.00", "pool.0", "hjoin.0.0.weight"):
            assert lib.vy_net_tap_frames(h, name.encode(), ctypes.byref(f)) == -1, name
        assert f.value == -7
        # the readers of the joined planes
        by = {c["name"]: c for c in cells}
        for i, name in enumerate(hier_cells.POOL_CONSUMERS[:n]):
            assert by[name]["src"] == ["hjoin.%d" % i]
        assert by["yolo_blocks.2.body.0"]["src"] == ["transitions.1", "hjoin.3" if n == 4 else "stages.0.14.body.1"]
    finally:
        lib.vy_net_destroy(h)
        lib.vy_net_destroy(mx)


@pytest.mark.parametrize("hier,b,h,w", [([3, 1, 1, 1, 1], 2, 64, 64), ([3, 3, 1, 1, 1], 2, 96, 32), ([3, 3, 3, 3, 1], 1, 64, 64),
                                        ([3, 3, 1, 1, 1], 16, 416, 416)])
def test_workspaces_hold_the_max_nets(hier, b, h, w):
    """The inference plan is the max net's plane for plane (more parameters, so a longer fold table: never smaller); the
    training plan adds a z plane, saved statistics and partial rows per join."""
    lib = _lib.load()
    n = hier.index(1)
    cv, mx = _make(lib, n), HH._make(lib, n)
    try:
        assert lib.vy_net_workspace_bytes(cv, b, h, w) >= lib.vy_net_workspace_bytes(mx, b, h, w) > 0
        tc, tm = lib.vy_net_train_workspace_bytes(cv, b, h, w), lib.vy_net_train_workspace_bytes(mx, b, h, w)
        z = sum(4 * b * 3 ** (n - 1 - i) * (h // 2 ** i + 2) * (w // 2 ** i + 2) * CHANNELS[i] for i in range(n))
        assert tc >= tm + z, (tc, tm, z)
        # its regions carry the joins' names
        names, r, i = [], _lib.PlanRegion(), 0
        while lib.vy_net_plan_region(cv, _lib.VY_PLAN_TRAIN, b, h, w, 0, 0, i, ctypes.byref(r)) == 0:
            names.append(r.name.decode())
            i += 1
        for j in range(n):
            assert "z:hjoin.%d" % j in names
            assert ("grad:hjoin.%d" % j in names) == (j < 3)  # (the fourth joined plane is route 0's place in its concat)
        assert not any("hpool" in x for x in names)
    finally:
        lib.vy_net_destroy(cv)
        lib.vy_net_destroy(mx)


# ------------------------------------------------------------------------------------------------ the class
def test_class_is_a_new_door_and_the_factory_still_raises():
    import videoyolo_amd as vy
    assert "YOLOV3HierConv" in vy.__all__ and issubclass(vy.YOLOV3HierConv, vy.YOLOV3Hier)
    net = _conv()
    assert type(net) is vy.YOLOV3HierConv and net.h_join_type == "conv" and vy.YOLOV3Hier.h_join_type == "max"
    assert (net.hierarchical, net.frames) == ([3, 3, 1, 1, 1], 9) and net._ONE_RANK
    assert HH._hier(net._lib, net._h) == (2, 9)
    assert set(vars(vy.YOLOV3HierConv)) - set(dir(vy.YOLOV3Hier)) == {"_JOIN_RE"}  # no new public name
    with pytest.raises(NotImplementedError, match="h_join_type"):
        vy.yolo3_darknet53(C20, pretrained_base=False, new_model=True, hierarchical=[3, 3, 1, 1, 1], h_join_type="conv")
    assert "YOLOV3HierConv" in vy.yolo3_darknet53.__doc__
    with pytest.raises(ValueError, match="run of 3s"):
        vy.YOLOV3HierConv(C20, hierarchical=[3, 1, 3, 1, 1])
    with pytest.raises(ValueError, match="T = 9"):
        net(np.zeros((2, 3, 3, 64, 64), np.float32))


def test_initialize_gives_the_reference_values():
    net = _conv([3, 3, 3, 3, 1])
    net.initialize(seed=1)
    P = net.collect_params()
    for i, ch in enumerate(CHANNELS):
        w = P["hjoin.%d.0.weight" % i].data()
        assert w.shape == (ch, 3) and not w.any()  # weight_initializer='zeros', layers.py:54
        for leaf, v in (("gamma", 1), ("beta", 0), ("running_mean", 0), ("running_var", 1)):
            a = P["hjoin.%d.1.%s" % (i, leaf)].data()
            assert a.shape == (ch,) and (a == v).all(), (i, leaf)
    assert P["stages.0.0.0.weight"].data().any()
    # the cells are the single-frame net's draw: a tensor's values depend on (seed, name) only
    import videoyolo_amd as vy
    single = vy.yolo3_darknet53(C20, pretrained_base=False)
    single.initialize(seed=1)
    for k, p in single.collect_params().items():
        assert np.array_equal(P[k].data(), p.data()), k
    syn = _conv()
    syn.initialize(init="synthetic", seed=3)
    assert (syn.collect_params()["hjoin.1.0.weight"].data() == np.float32(1 / 3)).all()


def test_keys_shapes_and_files(tmp_path):
    import videoyolo_amd as vy
    key = vy.YOLOV3HierConv._key
    assert key("d_model.convs1d.0.0.weight") == "hjoin.0.0.weight"  # [UPSTREAM-RECALLED]
    assert key("d_model.convs1d.3.1.running_var") == "hjoin.3.1.running_var"
    assert key("d_model.features.15.0.weight") == "stages.1.0.0.weight" and key("hjoin.1.1.beta") == "hjoin.1.1.beta"
    rng = np.random.default_rng(4)
    net = _conv()
    net.initialize(init="synthetic", seed=2)
    w5, w2 = rng.standard_normal((32, 1, 3, 1, 1)).astype(np.float32), rng.standard_normal((64, 3)).astype(np.float32)
    g = rng.standard_normal(64).astype(np.float32)
    net.set_parameters({"d_model.convs1d.0.0.weight": w5, "hjoin.1.0.weight": w2, "d_model.convs1d.1.1.gamma": g},
                       allow_missing=True)
    P = net.collect_params()
    assert np.array_equal(P["hjoin.0.0.weight"].data(), w5.reshape(32, 3))
    assert np.array_equal(P["hjoin.1.0.weight"].data(), w2) and np.array_equal(P["hjoin.1.1.gamma"].data(), g)
    with pytest.raises(ValueError, match="shape"):
        net.set_parameters({"hjoin.0.0.weight": np.zeros((32, 3, 1), np.float32)}, allow_missing=True)
    with pytest.raises(AssertionError, match="not present in the net"):
        net.set_parameters({"hjoin.2.0.weight": np.zeros((128, 3), np.float32)}, allow_missing=True)
    # its own file round-trips, join tensors included
    f = str(tmp_path / "conv.params")
    net.save_parameters(f)
    back = _conv()
    back.load_parameters(f)
    for k, p in P.items():
        assert np.array_equal(back.collect_params()[k].data(), p.data()), k
    # a single-frame file has no join keys
    single = vy.yolo3_darknet53(C20, pretrained_base=False)
    single.initialize(init="synthetic", seed=5)
    s = str(tmp_path / "single.params")
    single.save_parameters(s)
    with pytest.raises(AssertionError, match="hjoin.0.0.weight' is missing"):
        back.load_parameters(s)
    back.load_parameters(s, allow_missing=True)
    assert np.array_equal(back.collect_params()["hjoin.0.0.weight"].data(), w5.reshape(32, 3))  # kept
    assert np.array_equal(back.collect_params()["stages.0.0.0.weight"].data(), single.collect_params()["stages.0.0.0.weight"].data())
    # ... and the max net refuses a conv net's file unless told to ignore the joins
    mx = vy.yolo3_darknet53(C20, pretrained_base=False, new_model=True, hierarchical=[3, 3, 1, 1, 1], h_join_type="max")
    with pytest.raises(AssertionError, match="not present in the net"):
        mx.load_parameters(f)
    mx.load_parameters(f, ignore_extra=True)


def test_copies_keep_the_kind_and_freeze_base_reaches_the_joins():
    import videoyolo_amd as vy
    net = _conv([3, 3, 3, 1, 1], nms_thresh=0.3)
    net.initialize(init="synthetic", seed=7)
    w = np.random.default_rng(1).standard_normal((128, 3)).astype(np.float32)
    net.collect_params()["hjoin.2.0.weight"].set_data(w)
    twin = copy.deepcopy(net)
    assert type(twin) is vy.YOLOV3HierConv and twin.hierarchical == [3, 3, 3, 1, 1] and twin.frames == 27
    assert twin.h_join_type == "conv" and twin.nms_thresh == 0.3
    assert np.array_equal(twin.collect_params()["hjoin.2.0.weight"].data(), w)
    net.reset_class(["a", "b"])
    assert type(net) is vy.YOLOV3HierConv and (net.frames, net.num_class) == (27, 2)
    assert np.array_equal(net.collect_params()["hjoin.2.0.weight"].data(), w)
    # wrappers.py:50-57: freeze_base freezes d_model whole, the joins with it
    joins = [p for k, p in net.collect_params().items() if k.startswith("hjoin.")]
    assert len(joins) == 15 and all(p.backbone for p in joins)
    assert [p.trainable for p in joins[:5]] == [True, True, True, False, False]
    for p in net.collect_params().values():
        if p.backbone:
            p.grad_req = "null"
    assert all(p.grad_req == "null" for p in joins)


# ------------------------------------------------------------------------------------------------ what it refuses
def test_python_entry_points_refuse_it():
    net = _conv([3, 1, 1, 1, 1])
    for fn in (net.extract_features, net.detect_two_streams):
        with pytest.raises(NotImplementedError, match="hierarchical"):
            fn(np.zeros((1, 3, 3, 64, 64), np.float32))
    for mode in ("split_bf16x3", "split_bf16x3_train"):
        with pytest.raises(NotImplementedError, match="exact"):
            net.set_conv_mode(mode)
    net.set_conv_mode("exact")
    assert not hasattr(net, "video")


def test_entries_it_does_not_serve_return_their_codes():
    lib = _lib.load()
    h = _make(lib, 2)
    p = ctypes.c_void_p(0x1000)
    tab = (ctypes.c_int32 * 6)(0, 1, 2, 3, 4, 5)
    try:
        for mode in (_lib.VY_CONV_SPLIT_BF16X3, _lib.VY_CONV_SPLIT_BF16X3_TRAIN):
            assert lib.vy_net_set_conv_mode(h, mode) == -4
            assert "hierarchical" in lib.vy_last_error().decode()
        assert lib.vy_net_set_conv_mode(h, _lib.VY_CONV_EXACT_FP32) == 0
        calls = [
            (lib.vy_net_forward_features, (p, p, p, p, None)),
            (lib.vy_net_forward_infer_routes, (p, p, p, p, p, p, None, None)),
            (lib.vy_net_train_forward_routes, (p, p, p, p, 1, p, p, p, p, p, p, None)),
            (lib.vy_net_train_mode_forward_routes, (p, p, p, p, p, p, p, p, None)),
            (lib.vy_net_train_backward_routes, (p, p, p, None)),
            (lib.vy_net_forward_infer_bank, (p, p, p, 6, tab, p, p, p, None, None)),
            (lib.vy_net_train_forward_bank, (p, p, p, 6, tab, p, 1, p, p, p, p, p, p, None)),
            (lib.vy_net_train_mode_forward_bank, (p, p, p, 6, tab, p, p, p, p, p, None)),
            (lib.vy_net_video_push, (p, tab, None)),
            (lib.vy_net_video_detect, (tab, p, p, p, None, None)),
            (lib.vy_net_video_read_slot, (0, p, p, p, None)),
            (lib.vy_net_bind_video, (p, 1 << 30, 4, 2, 8, 64, 64, None)),
        ]
        for fn, args in calls:
            assert fn(h, *args) == -2, fn.__name__
            assert "not bound" not in lib.vy_last_error().decode(), fn.__name__
        assert lib.vy_net_video_workspace_bytes(h, 4, 2, 8, 64, 64) == 0
        assert lib.vy_net_forward_infer(h, p, p, p, p, None, None) == -2
        assert "not bound" in lib.vy_last_error().decode()
    finally:
        lib.vy_net_destroy(h)
