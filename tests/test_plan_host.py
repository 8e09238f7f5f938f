"""-m "not gpu": the workspace planners as pure functions of (net, settings, shape).

tests/golden/net_plan_totals.json holds vy_net_workspace_bytes, vy_net_train_workspace_bytes and
vy_net_video_workspace_bytes over a table that reaches every branch of the planner, recorded from the library as it was
before the inference plan became a value (NetPlan): the totals must stay byte for byte.  A total pins the last offset of
a plan; the offsets before it are held region by region: tests/test_ws_guard_host.py pins the region table of every plan
(ascending, disjoint, ending at the total), and tests/test_gpu_ws_guard.py shows on the device that no launch leaves the
region it was given (the bit-exact comparisons of tests/test_gpu_plan.py see a stray write only where it lands on live bytes).
Nothing here launches a kernel: the library plans without a device (vy_cu_count then answers 256, the MI355X's count).
"""
import ctypes
import json
import os

import pytest

from videoyolo_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "net_plan_totals.json")

# net kind -> (constructor, window k); clip nets (full window nets) run the exact kernels only
KINDS = {
    "full": ("vy_net_create", 0),
    "heads": ("vy_net_create_heads", 0),
    "window2": ("vy_net_create_window", 2),
    "window3": ("vy_net_create_window", 3),
    "heads_window2": ("vy_net_create_heads_window", 2),
    "heads_window3": ("vy_net_create_heads_window", 3),
}
CLASSES = (20, 80)  # 80: the prediction planes pad 255 -> 256 channels
SHAPES = ((1, 64, 64), (2, 96, 64), (1, 400, 416), (16, 416, 416), (8, 608, 608))
VIDEO = ((4, 2, 6), (16, 16, 18))  # frames, clips, ring
# (conv mode, VY_SPLIT_TRAIN): the training images of mode 2 follow the switch, read when the net is created
MODES = ((_lib.VY_CONV_EXACT_FP32, None), (_lib.VY_CONV_SPLIT_BF16X3, None), (_lib.VY_CONV_SPLIT_BF16X3_TRAIN, 0),
         (_lib.VY_CONV_SPLIT_BF16X3_TRAIN, 1), (_lib.VY_CONV_SPLIT_BF16X3_TRAIN, 2))


def _create(lib, kind, classes):
    ctor, k = KINDS[kind]
    h = ctypes.c_void_p()
    _lib.check(getattr(lib, ctor)(classes, k, _lib.VY_JOIN_MAX, ctypes.byref(h)) if k else getattr(lib, ctor)(classes, ctypes.byref(h)))
    return h


def _sizes(lib, h, kind, b, hh, ww):
    """The three queries at one shape: [workspace, training, video...] (video: window nets, one per VIDEO entry)."""
    out = [lib.vy_net_workspace_bytes(h, b, hh, ww), lib.vy_net_train_workspace_bytes(h, b, hh, ww)]
    if kind.startswith("window"):
        out += [lib.vy_net_video_workspace_bytes(h, f, c, r, hh, ww) for f, c, r in VIDEO]
    return out


def table(lib, setenv):
    """Every row of the table as (key, sizes); `setenv(name, value_or_None)` sets the environment the next net reads."""
    rows = []
    for kind in KINDS:
        clip = kind.startswith("window")
        for classes in CLASSES:
            for mode, st in MODES:
                if clip and mode != _lib.VY_CONV_EXACT_FP32:
                    continue
                setenv("VY_SPLIT_TRAIN", None if st is None else str(st))
                h = _create(lib, kind, classes)
                try:
                    _lib.check(lib.vy_net_set_conv_mode(h, mode))
                    for keep in (0, 1):
                        _lib.check(lib.vy_net_set_keep_activations(h, keep))
                        for b, hh, ww in SHAPES:
                            key = "%s c%d mode%d st%s keep%d %dx%dx%d" % (kind, classes, mode, "-" if st is None else st, keep, b, hh, ww)
                            rows.append((key, _sizes(lib, h, kind, b, hh, ww)))
                finally:
                    lib.vy_net_destroy(h)
    setenv("VY_SPLIT_TRAIN", None)
    return rows


def _queries(lib, h, kind, b, hh, ww):
    """_sizes, and as a fourth query the region tables of the same plans (vy_net_plan_region; tests/ws_guard.py)"""
    import ws_guard
    plans = [("clip", (b, hh, ww)), ("train", (b, hh, ww))] + [("video", (f, c, r, hh, ww)) for f, c, r in VIDEO if kind.startswith("window")]
    return _sizes(lib, h, kind, b, hh, ww) + [ws_guard.regions(lib, h, plan, shape) for plan, shape in plans]


def _cus_are_256():
    """The training totals depend on the CU count (the weight-gradient split-K): 256 without a device, and on an MI355X."""
    import torch
    return not torch.cuda.is_available() or torch.cuda.get_device_properties(0).multi_processor_count == 256


def test_totals_are_the_recorded_ones(monkeypatch):
    lib = _lib.load()
    with open(GOLDEN) as f:
        want = json.load(f)
    setenv = lambda n, v: monkeypatch.delenv(n, raising=False) if v is None else monkeypatch.setenv(n, v)
    got = dict(table(lib, setenv))
    assert sorted(got) == sorted(want), "the table and the fixture name the same rows"
    train_too = _cus_are_256()
    # the table reaches what it is meant to: both refusals (0) and real sizes, planes recycled or not, images or not
    assert any(v[1] == 0 for v in want.values()) and any(v[1] > 0 for v in want.values())
    assert want["full c20 mode0 st- keep0 1x64x64"][0] < want["full c20 mode0 st- keep1 1x64x64"][0]
    assert want["full c20 mode0 st- keep0 1x64x64"][0] < want["full c20 mode1 st- keep0 1x64x64"][0]
    assert len({want["full c20 mode2 st%d keep0 1x64x64" % s][1] for s in (0, 1)}) == 2
    bad = []
    for key, sizes in got.items():
        for i, (g, w) in enumerate(zip(sizes, want[key])):
            if i == 1 and not train_too:
                continue
            if g != w:
                bad.append((key, i, g, w))
        assert len(sizes) == len(want[key]), key
    assert not bad, bad[:10]


@pytest.mark.parametrize("kind", ["full", "heads", "window2"])
def test_a_query_leaves_no_trace(kind):
    """A sizing query at another shape — and a conv-mode switch and back — between two identical queries: the second
    answers what the first did, for all three queries and for the region tables of their plans."""
    lib = _lib.load()
    h = _create(lib, kind, 20)
    try:
        for keep in (0, 1):
            _lib.check(lib.vy_net_set_keep_activations(h, keep))
            for a, b in ((SHAPES[1], SHAPES[3]), (SHAPES[3], SHAPES[0])):
                first = _queries(lib, h, kind, *a)
                assert all(first), (kind, a, first)
                other = _queries(lib, h, kind, *b)
                assert other != first
                if not kind.startswith("window"):
                    for mode in (_lib.VY_CONV_SPLIT_BF16X3, _lib.VY_CONV_SPLIT_BF16X3_TRAIN):
                        _lib.check(lib.vy_net_set_conv_mode(h, mode))
                        assert _sizes(lib, h, kind, *b)[0] > other[0]  # the weight images are in the plan
                    _lib.check(lib.vy_net_set_conv_mode(h, _lib.VY_CONV_EXACT_FP32))
                assert _queries(lib, h, kind, *a) == first, (kind, keep, a, b)
    finally:
        lib.vy_net_destroy(h)
