"""-m "not gpu": the hierarchical net (yolo3_darknet53 with new_model=True, hierarchical=[3,..,1], h_join_type='max') on
the host — which constructor arguments give it and which keep raising, the C-ABI constructor, its tables against the
single-frame net's, the frame multiplier of every cell, the workspace sizes, the parameter-key aliases, the input check
and the entry points that refuse it.  Nothing here launches a kernel."""
import ctypes

import numpy as np
import pytest

import hier_cells
from videoyolo_amd import _lib

C20 = ["c%d" % i for i in range(20)]
LISTS = [list(v) for v in hier_cells.VALID]


def _hier(lib, h):
    n, t = ctypes.c_int32(-1), ctypes.c_int32(-1)
    _lib.check(lib.vy_net_hier(h, ctypes.byref(n), ctypes.byref(t)))
    return n.value, t.value


def _make(lib, n_pools, num_class=20):
    h = ctypes.c_void_p()
    if n_pools:
        _lib.check(lib.vy_net_create_hier(num_class, n_pools, ctypes.byref(h)))
    else:
        _lib.check(lib.vy_net_create(num_class, ctypes.byref(h)))
    return h


def _conv_infos(lib, h):
    out = []
    for i in range(lib.vy_net_num_convs(h)):
        info = _lib.ConvInfo()
        _lib.check(lib.vy_net_conv_info(h, i, ctypes.byref(info)))
        out.append(info)
    return out


def _tap_frames(lib, h, name):
    f = ctypes.c_int32(-1)
    _lib.check(lib.vy_net_tap_frames(h, name.encode(), ctypes.byref(f)))
    return f.value


# ------------------------------------------------------------------------------------------------ the constructor
@pytest.mark.parametrize("hier", LISTS)
def test_constructor_returns_the_hierarchical_net(hier):
    import videoyolo_amd as vy
    net = vy.yolo3_darknet53(C20, pretrained_base=False, new_model=True, hierarchical=hier, h_join_type="max")
    assert type(net) is vy.YOLOV3Hier and isinstance(net, vy.YOLOV3)
    n = hier.index(1)
    assert net.hierarchical == hier and net.frames == 3 ** n and net.h_join_type == "max" and net._ONE_RANK
    assert _hier(net._lib, net._h) == (n, 3 ** n)
    # the keys are the single-frame net's, offset for offset: its files load as they are
    plain = vy.yolo3_darknet53(C20, pretrained_base=False)
    assert _hier(plain._lib, plain._h) == (0, 1)
    assert [(p.name, p.shape, p.kind, p.trainable, p.backbone, p.offset) for p in net.collect_params().values()] == \
           [(p.name, p.shape, p.kind, p.trainable, p.backbone, p.offset) for p in plain.collect_params().values()]
    # a tuple is a list too
    assert type(vy.yolo3_darknet53(C20, pretrained_base=False, new_model=True, hierarchical=tuple(hier),
                                   h_join_type="max")) is vy.YOLOV3Hier


@pytest.mark.parametrize("kw,named", [
    (dict(new_model=True), "new_model"),
    (dict(hierarchical=[3, 1, 1, 1, 1]), "hierarchical"),
    (dict(hierarchical=[3, 3, 1, 1, 1], h_join_type="max"), "hierarchical"),
    (dict(new_model=True, hierarchical=[3, 1, 1, 1, 1]), "h_join_type"),
    (dict(new_model=True, hierarchical=[3, 3, 1, 1, 1], h_join_type="conv"), "h_join_type"),
    (dict(new_model=True, h_join_type="max"), "new_model"),
    (dict(h_join_type="max"), "h_join_type"),
    (dict(new_model=True, hierarchical=[3, 3, 3, 3, 3], h_join_type="max"), "hierarchical"),
    (dict(new_model=True, hierarchical=[3, 1, 3, 1, 1], h_join_type="max"), "hierarchical"),
    (dict(new_model=True, hierarchical=[1, 3, 1, 1, 1], h_join_type="max"), "hierarchical"),
    (dict(new_model=True, hierarchical=[2, 1, 1, 1, 1], h_join_type="max"), "hierarchical"),
    (dict(new_model=True, hierarchical=[9, 1, 1, 1, 1], h_join_type="max"), "hierarchical"),
    (dict(new_model=True, hierarchical=[3, 1, 1, 1], h_join_type="max"), "hierarchical"),
    (dict(new_model=True, hierarchical=[3, 3, 1, 1, 1, 1], h_join_type="max"), "hierarchical"),
    (dict(new_model=True, hierarchical=[3, 1, 1, 1, 1], h_join_type="max", k=3, k_join_type="max", k_join_pos="early"),
     "hierarchical"),
])
def test_everything_else_keeps_raising_and_names_the_option(kw, named):
    import videoyolo_amd as vy
    with pytest.raises(NotImplementedError, match=named):
        vy.yolo3_darknet53(C20, pretrained_base=False, **kw)


def test_the_class_itself_checks_its_list():
    import videoyolo_amd as vy
    for bad in ([1, 1, 1, 1, 1], [3, 3, 3, 3, 3], [3, 1, 3, 1, 1], [3, 1, 1, 1], "3,3,1,1,1"):
        with pytest.raises(ValueError, match="hierarchical"):
            vy.YOLOV3Hier(C20, hierarchical=bad)


def test_c_abi_constructor_checks_its_arguments():
    lib = _lib.load()
    h = ctypes.c_void_p()
    for args in ((20, 0), (20, 5), (20, -1), (0, 2), (1001, 2)):
        assert lib.vy_net_create_hier(*args, ctypes.byref(h)) == -1, args
        assert not h.value
    assert lib.vy_net_create_hier(20, 2, None) == -1
    assert lib.vy_net_hier(None, None, None) == -1
    h = _make(lib, 3)
    try:
        assert _hier(lib, h) == (3, 27)
        k = ctypes.c_int32(-1)
        _lib.check(lib.vy_net_window(h, ctypes.byref(k), None))
        assert k.value == 0
    finally:
        lib.vy_net_destroy(h)


# ------------------------------------------------------------------------------------------------ tables and frames
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_tables_are_the_single_frame_nets(n):
    """Parameter table byte for byte; conv list name for name, shape for shape, in the same order.  Where a cell stores its
    output is the single-frame net's too — but for the route-0 cell of a four-pool net, which writes a plane of its own
    (the pool, not the cell, writes route 0 into the stride-8 concat plane)."""
    lib = _lib.load()
    base, h = _make(lib, 0), _make(lib, n)
    try:
        assert lib.vy_net_num_params(h) == lib.vy_net_num_params(base) == 366
        for i in range(lib.vy_net_num_params(base)):
            a, b = _lib.ParamInfo(), _lib.ParamInfo()
            _lib.check(lib.vy_net_param_info(base, i, ctypes.byref(a)))
            _lib.check(lib.vy_net_param_info(h, i, ctypes.byref(b)))
            assert bytes(a) == bytes(b), a.name
        assert lib.vy_net_param_bytes(h) == lib.vy_net_param_bytes(base)
        ca, cb = _conv_infos(lib, base), _conv_infos(lib, h)
        assert len(ca) == len(cb) == 75
        moved = []
        for a, b in zip(ca, cb):
            for f in ("name", "cin", "cout", "kernel", "stride", "pad", "has_bn", "sync_bn", "residual", "upsample"):
                assert getattr(a, f) == getattr(b, f), (a.name, f)
            if bytes(a) != bytes(b):
                moved.append((b.name.decode(), b.concat_offset, b.out_channels_total))
        assert moved == ([("stages.0.14.body.1", 0, 256)] if n == 4 else [])
    finally:
        lib.vy_net_destroy(base)
        lib.vy_net_destroy(h)


@pytest.mark.parametrize("hier", LISTS)
def test_frame_multiplier_of_every_cell(hier):
    """vy_net_tap_frames of every conv and every pooled plane is the cell list's fm (tests/hier_cells.py): 3^(pools ahead)
    in the backbone, 1 from the last pool on."""
    lib = _lib.load()
    n = hier.index(1)
    h = _make(lib, n)
    try:
        cells = hier_cells.hier_graph(20, hier)
        convs = [c for c in cells if not c.get("pool")]
        assert [c["name"] for c in convs] == [i.name.decode() for i in _conv_infos(lib, h)]
        for c in cells:
            assert _tap_frames(lib, h, c["name"]) == c["fm"], c["name"]
        assert [c["name"] for c in cells if c.get("pool")] == ["hpool.%d" % i for i in range(n)]
        assert [c["fm"] for c in cells if c.get("pool")] == [3 ** (n - 1 - i) for i in range(n)]
        assert cells[0]["fm"] == 3 ** n and all(c["fm"] == 1 for c in cells if not c["name"].startswith(("stages.0", "hpool")))
        f = ctypes.c_int32()
        assert lib.vy_net_tap_frames(h, ("hpool.%d" % n).encode(), ctypes.byref(f)) == -1
        assert lib.vy_net_tap_frames(h, b"pool.0", ctypes.byref(f)) == -1
        # the consumers of the pooled planes
        by = {c["name"]: c for c in cells}
        for i, name in enumerate(hier_cells.POOL_CONSUMERS[:n]):
            assert by[name]["src"] == ["hpool.%d" % i] and by[name]["s"] == 2
        assert by["yolo_blocks.2.body.0"]["src"] == ["transitions.1", "hpool.3" if n == 4 else "stages.0.14.body.1"]
    finally:
        lib.vy_net_destroy(h)


def test_single_frame_net_has_no_pooled_taps():
    lib = _lib.load()
    h = _make(lib, 0)
    try:
        f = ctypes.c_int32()
        assert lib.vy_net_tap_frames(h, b"hpool.0", ctypes.byref(f)) == -1
        assert _tap_frames(lib, h, "stages.0.0") == 1
    finally:
        lib.vy_net_destroy(h)


@pytest.mark.parametrize("frames,h,w", [(81, 64, 64), (162, 96, 32)])
def test_workspace_shrinks_with_every_pool(frames, h, w):
    """At a fixed number of frames B * T every further pool takes frames out of the cells behind it: both workspaces are
    monotone in the number of pools, and all of them lie below the single-frame net's on the same frames."""
    lib = _lib.load()
    nets = [_make(lib, n) for n in range(5)]
    try:
        for fn in (lib.vy_net_workspace_bytes, lib.vy_net_train_workspace_bytes):
            sizes = [fn(net, frames // 3 ** n, h, w) for n, net in enumerate(nets)]
            assert all(s > 0 for s in sizes), sizes
            assert all(a > b for a, b in zip(sizes, sizes[1:])), (fn.__name__, sizes)
        # with activations kept every pooled plane has storage of its own: more than the recycled plan
        lean = lib.vy_net_workspace_bytes(nets[2], frames // 9, h, w)
        _lib.check(lib.vy_net_set_keep_activations(nets[2], 1))
        assert lib.vy_net_workspace_bytes(nets[2], frames // 9, h, w) > lean
    finally:
        for net in nets:
            lib.vy_net_destroy(net)


# ------------------------------------------------------------------------------------------------ keys, files, inputs
def test_reference_spelling_of_the_backbone_keys():
    """[UPSTREAM-RECALLED] d_model.features.N.<rest>, N over the 29 feature cells of stages.0 / 1 / 2 in order."""
    import videoyolo_amd as vy
    key = vy.YOLOV3Hier._key
    assert key("d_model.features.0.0.weight") == "stages.0.0.0.weight"
    assert key("d_model.features.14.body.1.1.gamma") == "stages.0.14.body.1.1.gamma"
    assert key("d_model.features.15.0.weight") == "stages.1.0.0.weight"
    assert key("d_model.features.23.body.0.1.running_var") == "stages.1.8.body.0.1.running_var"
    assert key("d_model.features.24.1.beta") == "stages.2.0.1.beta"
    assert key("d_model.features.28.body.1.0.weight") == "stages.2.4.body.1.0.weight"
    for same in ("d_model.features.29.0.weight", "stages.0.0.0.weight", "yolo_blocks.0.tip.0.weight", "d_model.output.weight"):
        assert key(same) == same
    single = vy.yolo3_darknet53(C20, pretrained_base=False)
    single.initialize(init="synthetic", seed=3)
    want = {n: p.data() for n, p in single.collect_params().items()}
    ours = set()
    for n in want:
        if n.startswith("stages."):
            si, j, rest = n.split(".", 3)[1:]
            ours.add("d_model.features.%d.%s" % ((0, 15, 24)[int(si)] + int(j), rest))
    spelled = {}
    for n, v in want.items():
        if n.startswith("stages."):
            si, j, rest = n.split(".", 3)[1:]
            n = "d_model.features.%d.%s" % ((0, 15, 24)[int(si)] + int(j), rest)
        spelled[n] = v
    assert len(spelled) == len(want) and len(ours) == sum(n.startswith("stages.") for n in want)
    net = vy.yolo3_darknet53(C20, pretrained_base=False, new_model=True, hierarchical=[3, 3, 1, 1, 1], h_join_type="max")
    net.set_parameters(spelled)
    for n, v in want.items():
        assert np.array_equal(net.collect_params()[n].data(), v), n
    with pytest.raises(AssertionError, match="not present in the net"):
        net.set_parameters({"d_model.features.29.0.weight": np.zeros(1, np.float32)}, allow_missing=True)


def test_single_frame_file_loads_and_copies_keep_the_kind(tmp_path):
    import copy
    import videoyolo_amd as vy
    single = vy.yolo3_darknet53(C20, pretrained_base=False)
    single.initialize(init="synthetic", seed=5)
    f = str(tmp_path / "single.params")
    single.save_parameters(f)
    net = vy.yolo3_darknet53(C20, pretrained_base=False, new_model=True, hierarchical=[3, 3, 3, 1, 1], h_join_type="max")
    net.load_parameters(f)
    for n, p in single.collect_params().items():
        assert np.array_equal(net.collect_params()[n].data(), p.data()), n
    g = str(tmp_path / "hier.params")
    net.save_parameters(g)
    back = vy.yolo3_darknet53(C20, pretrained_base=False)
    back.load_parameters(g)  # and back: the file of a hierarchical net is a single-frame file
    twin = copy.deepcopy(net)
    assert type(twin) is vy.YOLOV3Hier and twin.hierarchical == [3, 3, 3, 1, 1] and twin.frames == 27
    assert np.array_equal(twin.collect_params()["stages.0.0.0.weight"].data(), single.collect_params()["stages.0.0.0.weight"].data())
    net.reset_class(["a", "b"])
    assert type(net) is vy.YOLOV3Hier and (net.frames, net.num_class) == (27, 2)
    # freeze_base marks the backbone, as on any net
    frozen = vy.yolo3_darknet53(C20, pretrained_base=False, freeze_base=True, new_model=True, hierarchical=[3, 1, 1, 1, 1],
                                h_join_type="max")
    assert all((p.grad_req == "null") == bool(p.backbone) for p in frozen.collect_params().values() if p.trainable)


@pytest.mark.parametrize("shape", [(2, 3, 64, 64), (2, 3, 3, 64, 64), (2, 9, 1, 64, 64), (2, 27, 3, 64, 64), (9, 3, 64)])
def test_clips_are_checked_before_the_device(shape):
    import videoyolo_amd as vy
    net = vy.yolo3_darknet53(C20, pretrained_base=False, new_model=True, hierarchical=[3, 3, 1, 1, 1], h_join_type="max")
    with pytest.raises(ValueError, match="T = 9"):
        net(np.zeros(shape, np.float32))
    with pytest.raises(RuntimeError, match="not on a device"):
        net(np.zeros((2, 9, 3, 64, 64), np.float32))


# ------------------------------------------------------------------------------------------------ what it refuses
def test_python_entry_points_refuse_it():
    import videoyolo_amd as vy
    net = vy.yolo3_darknet53(C20, pretrained_base=False, new_model=True, hierarchical=[3, 1, 1, 1, 1], h_join_type="max")
    for fn in (net.extract_features, net.detect_two_streams):
        with pytest.raises(NotImplementedError, match="hierarchical"):
            fn(np.zeros((1, 3, 3, 64, 64), np.float32))
    for mode in ("split_bf16x3", "split_bf16x3_train"):
        with pytest.raises(NotImplementedError, match="exact"):
            net.set_conv_mode(mode)
    net.set_conv_mode("exact")
    assert net.two_stream_batch == 0 and not hasattr(net, "video")


def test_entries_it_does_not_serve_return_their_codes():
    """As on a window net: the split conv modes VY_ERR_UNSUPPORTED; extract_features, the video ring and the *_routes /
    *_bank entries VY_ERR_STATE, before anything is touched (the bogus device pointers are never dereferenced)."""
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
        # the entries it does serve get as far as the state of the net
        assert lib.vy_net_forward_infer(h, p, p, p, p, None, None) == -2
        assert "not bound" in lib.vy_last_error().decode()
    finally:
        lib.vy_net_destroy(h)
