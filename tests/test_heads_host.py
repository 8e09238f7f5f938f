"""-m "not gpu": the heads-only net (yolo3_no_backbone, YOLOV3_noback of the reference) on the host — its parameter and
conv tables against the full net's heads, the .params round trips, route-shape validation, and the C-ABI refusing to mix
full-net and heads-net entry points.  Nothing here launches a kernel."""
import ctypes

import numpy as np
import pytest

from videoyolo_amd import _lib

C20 = ["c%d" % i for i in range(20)]


def _convs(lib, h):
    out = []
    for i in range(lib.vy_net_num_convs(h)):
        info = _lib.ConvInfo()
        _lib.check(lib.vy_net_conv_info(h, i, ctypes.byref(info)))
        out.append((info.name.decode(), info.cin, info.cout, info.kernel, info.stride, info.has_bn, info.sync_bn,
                    info.residual, info.upsample, info.concat_offset, info.out_channels_total))
    return out


def _handles(lib, num_class=20):
    full, heads = ctypes.c_void_p(), ctypes.c_void_p()
    _lib.check(lib.vy_net_create(num_class, ctypes.byref(full)))
    _lib.check(lib.vy_net_create_heads(num_class, ctypes.byref(heads)))
    return full, heads


@pytest.mark.parametrize("num_class", [1, 20, 80])
def test_param_table_is_the_full_nets_heads(num_class):
    import videoyolo_amd as vy
    classes = ["c%d" % i for i in range(num_class)]
    full = vy.yolo3_darknet53(classes, pretrained_base=False)
    heads = vy.yolo3_no_backbone(classes)
    assert isinstance(heads, vy.YOLOV3NoBackbone) and vy.YOLOV3_noback is vy.YOLOV3NoBackbone
    want = [(p.name, p.shape, p.kind, p.trainable) for p in full.collect_params().values() if not p.backbone]
    got = [(p.name, p.shape, p.kind, p.trainable) for p in heads.collect_params().values()]
    assert got == want
    assert not any(p.backbone for p in heads.collect_params().values())
    assert all(n.startswith(("yolo_blocks.", "transitions.", "yolo_outputs.")) for n, _, _, _ in got)
    assert len(got) == 106  # 20 BatchNorm cells x 5 tensors + 3 prediction convs x 2
    # the conv graph: the full net's head rows, in the same order, with the same concat geometry
    lib = _lib.load()
    fh, hh = _handles(lib, num_class)
    try:
        fc, hc = _convs(lib, fh), _convs(lib, hh)
        assert hc == [c for c in fc if not c[0].startswith("stages.")]
        assert not any(c[6] for c in hc)  # no SyncBatchNorm cell among the heads
        # the heads plan only what the heads read: less workspace than the full net at the same image size
        for b, h, w in ((2, 416, 416), (1, 609, 611)):
            a, z = lib.vy_net_workspace_bytes(hh, b, h, w), lib.vy_net_workspace_bytes(fh, b, h, w)
            assert 0 < a < z
        assert 0 < lib.vy_net_train_workspace_bytes(hh, 4, 320, 320) < lib.vy_net_train_workspace_bytes(fh, 4, 320, 320)
        assert lib.vy_net_train_workspace_bytes(hh, 1, 416, 400) == 0  # training: multiples of 32, as the full net
        assert lib.vy_net_workspace_bytes(hh, 1, 16, 416) == 0
    finally:
        lib.vy_net_destroy(fh)
        lib.vy_net_destroy(hh)


def test_params_round_trip_and_full_model_file(tmp_path):
    import videoyolo_amd as vy
    heads = vy.yolo3_no_backbone(C20)
    heads.initialize(init="synthetic", seed=7)
    f = str(tmp_path / "heads.params")
    heads.save_parameters(f)
    back = vy.yolo3_no_backbone(C20)
    back.load_parameters(f)
    for name, p in heads.collect_params().items():
        assert np.array_equal(back.collect_params()[name].data(), p.data()), name
    # the anchors / offsets Constants ride along, as in the reference's own file
    with np.load(f) as z:
        assert "yolo_outputs.0.anchors" in z.files and "stages.0.0.0.weight" not in z.files

    full = vy.yolo3_darknet53(C20, pretrained_base=False)
    full.initialize(init="synthetic", seed=9)
    g = str(tmp_path / "full.params")
    full.save_parameters(g)
    other = vy.yolo3_no_backbone(C20)
    with pytest.raises(AssertionError, match="not present in the net"):
        other.load_parameters(g)
    other.load_parameters(g, ignore_extra=True)
    for name, p in other.collect_params().items():
        assert np.array_equal(p.data(), full.collect_params()[name].data()), name
    # and the other way: a heads file fills the heads of a full model (allow_missing)
    full.load_parameters(f, allow_missing=True)
    assert np.array_equal(full.collect_params()["transitions.1.0.weight"].data(),
                          heads.collect_params()["transitions.1.0.weight"].data())


def test_reset_class_and_deepcopy_keep_the_kind():
    import copy
    import videoyolo_amd as vy
    heads = vy.yolo3_no_backbone(C20)
    heads.initialize(init="synthetic", seed=3)
    twin = copy.deepcopy(heads)
    assert type(twin) is vy.YOLOV3NoBackbone
    assert np.array_equal(twin.collect_params()["yolo_blocks.0.tip.0.weight"].data(),
                          heads.collect_params()["yolo_blocks.0.tip.0.weight"].data())
    keep = heads.collect_params()["yolo_blocks.2.body.3.0.weight"].data()
    heads.reset_class(["a", "b", "c"])
    assert type(heads) is vy.YOLOV3NoBackbone and heads.num_class == 3
    assert heads.collect_params()["yolo_outputs.0.prediction.weight"].shape == (24, 1024, 1, 1)
    assert np.array_equal(heads.collect_params()["yolo_blocks.2.body.3.0.weight"].data(), keep)
    heads.set_nms(0.5, 200, 50)
    assert (heads.nms_thresh, heads.nms_topk, heads.post_nms) == (0.5, 200, 50)


def _routes(b, h, w):
    c8 = lambda n: -(-n // 8)  # noqa: E731
    h8, w8 = c8(h), c8(w)
    return [np.zeros((b, 256, h8, w8), np.float32), np.zeros((b, 512, -(-h8 // 2), -(-w8 // 2)), np.float32),
            np.zeros((b, 1024, -(-h8 // 4), -(-w8 // 4)), np.float32)]


@pytest.mark.parametrize("bad", [
    "batch", "channels", "stride16", "stride32", "rank", "tiny",
])
def test_route_shapes_are_checked_before_anything_runs(bad):
    import videoyolo_amd as vy
    heads = vy.yolo3_no_backbone(C20)
    f = _routes(2, 416, 416)
    if bad == "batch":
        f[1] = f[1][:1]
    elif bad == "channels":
        f[0] = np.zeros((2, 128, 52, 52), np.float32)
    elif bad == "stride16":
        f[1] = np.zeros((2, 512, 27, 26), np.float32)
    elif bad == "stride32":
        f[2] = np.zeros((2, 1024, 13, 14), np.float32)
    elif bad == "rank":
        f[2] = f[2][0]
    elif bad == "tiny":
        f = _routes(1, 24, 416)
    with pytest.raises(ValueError, match="routes"):
        heads(*f)


def test_route_shapes_of_odd_sizes_are_accepted_by_the_check():
    """609 x 611 routes (77 x 77, 39 x 39, 20 x 20) pass the shape check; the call then stops at the device check."""
    import videoyolo_amd as vy
    heads = vy.yolo3_no_backbone(C20)
    with pytest.raises(RuntimeError, match="not on a device"):
        heads(*_routes(1, 609, 611))


def test_image_entry_points_refuse_a_heads_net():
    import videoyolo_amd as vy
    heads = vy.yolo3_no_backbone(C20)
    for fn in (heads.extract_features, heads.profile):
        with pytest.raises(NotImplementedError):
            fn(np.zeros((1, 3, 64, 64), np.float32))


def test_mixing_kinds_fails_with_state_error():
    """A full-net entry on a heads net and a routes entry on a full net return VY_ERR_STATE before touching anything:
    the (bogus, non-null) device pointers below are never dereferenced, and no workspace is even bound."""
    lib = _lib.load()
    full, heads = _handles(lib)
    p = ctypes.c_void_p(0x1000)
    try:
        calls = [
            (heads, lib.vy_net_forward_infer, (p, p, p, p, None, None)),
            (heads, lib.vy_net_forward_features, (p, p, p, p, None)),
            (heads, lib.vy_net_train_forward, (p, p, 1, p, p, p, p, p, p, None)),
            (heads, lib.vy_net_train_mode_forward, (p, p, p, p, p, p, None)),
            (heads, lib.vy_net_train_backward, (p, None)),
            (full, lib.vy_net_forward_infer_routes, (p, p, p, p, p, p, None, None)),
            (full, lib.vy_net_train_forward_routes, (p, p, p, p, 1, p, p, p, p, p, p, None)),
            (full, lib.vy_net_train_mode_forward_routes, (p, p, p, p, p, p, p, p, None)),
            (full, lib.vy_net_train_backward_routes, (p, p, p, None)),
        ]
        for h, fn, args in calls:
            rc = fn(h, *args)
            assert rc == -2, (fn.__name__, rc)
            msg = lib.vy_last_error().decode()
            assert ("heads-only" in msg) if h is heads else ("full net" in msg), msg
        stats = (_lib.LaunchStat * 4)()
        n = ctypes.c_int32(4)
        assert lib.vy_net_profile_infer(heads, p, p, p, p, stats, ctypes.byref(n), None) == -2
        # the right kind with no workspace bound is a different error (state of the net, not of the entry)
        assert lib.vy_net_forward_infer_routes(heads, p, p, p, p, p, p, None, None) == -2
        assert "not bound" in lib.vy_last_error().decode()
    finally:
        lib.vy_net_destroy(full)
        lib.vy_net_destroy(heads)
