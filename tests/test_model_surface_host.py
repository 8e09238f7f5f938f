"""-m "not gpu": the surface of the five kinds of net, pinned — the public attribute names and signatures of an instance,
the entry points each kind refuses, and the error (type and whole message) of every malformed call that is caught before
the device is touched.  The expected values are literals recorded from the model classes as they stood before their call
paths were folded into one; nothing here launches a kernel or needs a device."""
import inspect

import numpy as np
import pytest

C20 = ["c%d" % i for i in range(20)]
KINDS = ("full", "heads", "window", "hier", "heads_window")


def _net(kind, **kw):
    import videoyolo_amd as vy
    if kind == "full":
        return vy.yolo3_darknet53(C20, pretrained_base=False, **kw)
    if kind == "heads":
        return vy.yolo3_no_backbone(C20, **kw)
    if kind == "window":
        return vy.yolo3_darknet53(C20, pretrained_base=False, k=3, k_join_type="max", k_join_pos="early", **kw)
    if kind == "hier":
        return vy.yolo3_darknet53(C20, pretrained_base=False, new_model=True, hierarchical=[3, 1, 1, 1, 1], h_join_type="max",
                                  **kw)
    return vy.yolo3_no_backbone(C20, k=3, k_join_type="max", k_join_pos="early", **kw)


def _caught(fn):
    """(exception type name, whole message) of fn()."""
    try:
        fn()
    except Exception as e:  # noqa: BLE001 — the type is what is compared
        return type(e).__name__, str(e)
    return None


# ---------------------------------------------------------------- public surface
# name -> signature of a public callable, None for any other public attribute; a kind's surface is FULL updated with its own
FULL = {
    "classes": None,
    "collect_params": "(select=None)",
    "constants": "()",
    "detect": "(x, return_index=False)",
    "detect_heads": "(heads, size, return_index=False)",
    "detect_two_streams": "(x, return_index=False)",
    "extract_features": "(x)",
    "forward_train": "(*args)",
    "forward_train_mode": "(*inputs)",
    "backward": "()",
    "grad": "(name)",
    "hybridize": "(active=True, **kwargs)",
    "initialize": "(init=None, ctx=None, force_reinit=False, seed=None, **kwargs)",
    "keep_activations": "(keep=True)",
    "load_darknet53_backbone": "(filename)",
    "load_parameters": "(filename, ctx=None, allow_missing=False, ignore_extra=False)",
    "nms_thresh": None,
    "nms_topk": None,
    "num_class": None,
    "param_table": "()",
    "post_nms": None,
    "profile": "(x)",
    "read_activation": "(name)",
    "read_grad_activation": "(name)",
    "read_head": "(i)",
    "read_train_tap": "(name, which)",
    "reset_class": "(classes, reuse_weights=None)",
    "reset_ctx": "(ctx)",
    "save_parameters": "(filename, format=None)",
    "semantics": None,
    "set_conv_mode": "(mode='exact')",
    "set_nms": "(nms_thresh=0.45, nms_topk=400, post_nms=100)",
    "set_parameters": "(arrays, allow_missing=False, ignore_extra=False)",
    "set_semantics": "(*, strict_valid=None, strict_iou=None, tie_ascending=None, topk_first=None, plus_one=None, "
                     "running_var_unbiased=None)",
    "sgd_step": "(lr, momentum, wd, rescale_grad)",
    "streamk_enabled": "()",
    "summary": "(*inputs)",
    "train_conv_plan": "(name)",
    "two_stream_batch": None,
}
REFUSED = "(*args, **kwargs)"
OWN = {
    "full": {},
    "heads": {"detect": "(f1, f2, f3, return_index=False)", "extract_features": REFUSED, "detect_two_streams": REFUSED,
              "profile": REFUSED, "load_darknet53_backbone": REFUSED},
    "window": {"k": None, "k_join_type": None, "video": "(frames_per_step=16, step=1, ring=None)",
               "detect_video": "(frames, step=1, frames_per_step=16, return_index=False)",
               "extract_features": REFUSED, "detect_two_streams": REFUSED, "profile": REFUSED},
    "hier": {"hierarchical": None, "frames": None, "h_join_type": None, "extract_features": REFUSED,
             "detect_two_streams": REFUSED},
    "heads_window": {"k": None, "k_join_type": None, "detect": "(f1, f2, f3, return_index=False, table=None)",
                     "from_bank": "(f1, f2, f3, table, *args, return_index=False)",
                     "detect_video_features": "(f1, f2, f3, step=1, clips_per_step=16, return_index=False)",
                     "extract_features": REFUSED, "detect_two_streams": REFUSED, "profile": REFUSED,
                     "load_darknet53_backbone": REFUSED},
}


def _surface(net):
    out = {}
    for name in sorted(n for n in dir(net) if not n.startswith("_")):
        v = getattr(net, name)
        out[name] = str(inspect.signature(v)) if callable(v) else None
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_public_names_and_signatures(kind):
    got = _surface(_net(kind))
    want = dict(FULL, **OWN[kind])
    assert sorted(got) == sorted(want)
    assert got == want


# ---------------------------------------------------------------- refusals
_NO_IMAGE = ("NotImplementedError", "a heads-only net (yolo3_no_backbone) takes route tensors, not images")
_NOT_WINDOWED = ("NotImplementedError", "not available on a window net (yolo3_darknet53 with k > 1): use a single-frame net")
_NOT_HIER = ("NotImplementedError", "not available on a hierarchical net (yolo3_darknet53 with hierarchical=...): use a "
                                    "single-frame net")
REFUSALS = {
    "full": {},
    "heads": dict.fromkeys(("extract_features", "detect_two_streams", "profile", "load_darknet53_backbone"), _NO_IMAGE),
    "window": dict.fromkeys(("extract_features", "detect_two_streams", "profile"), _NOT_WINDOWED),
    "hier": dict.fromkeys(("extract_features", "detect_two_streams"), _NOT_HIER),
    "heads_window": dict.fromkeys(("extract_features", "detect_two_streams", "profile", "load_darknet53_backbone"), _NO_IMAGE),
}
_IMAGE_ENTRIES = ("extract_features", "detect_two_streams", "profile", "load_darknet53_backbone")


@pytest.mark.parametrize("kind", KINDS)
def test_refused_entry_points(kind):
    """Every image entry point of a kind either refuses with its kind's message — whatever it is given — or is not refused:
    then it gets as far as its own first check."""
    net = _net(kind)
    x = np.zeros((1, 3, 64, 64), np.float32)
    got = {}
    for name in _IMAGE_ENTRIES:
        seen = {_caught(lambda: getattr(net, name)(x)), _caught(lambda: getattr(net, name)()),
                _caught(lambda: getattr(net, name)(x, 1, anything=2))}
        if len(seen) == 1 and next(iter(seen))[0] == "NotImplementedError":
            got[name] = seen.pop()
    assert got == REFUSALS[kind]


# ---------------------------------------------------------------- errors before the device
def _routes(lead, h8=8, w8=8):
    return [np.zeros(tuple(lead) + (c, -(-h8 // d), -(-w8 // d)), np.float32) for c, d in ((256, 1), (512, 2), (1024, 4))]


def _swap(fs, i, shape):
    fs = list(fs)
    fs[i] = np.zeros(shape, np.float32)
    return fs


_TABLE = np.array([[0, 1, 2], [6, 6, 5]], np.int64)
_TARGETS = (1, 2, 3, 4, 5)  # five where six are due


def _record():
    from videoyolo_amd import autograd
    return autograd.record()


def _train_mode():
    from videoyolo_amd import autograd
    return autograd.train_mode()


def _under(scope, fn):
    def run():
        with scope():
            return fn()
    return run


# (kind, case) -> the call on a fresh parameter-less net of that kind with no device
CALLS = {
    # image nets: the device check comes before the shape check
    ("full", "valid"): lambda n: n(np.zeros((1, 3, 64, 64), np.float32)),
    ("full", "rank"): lambda n: n(np.zeros((3, 64, 64), np.float32)),
    ("full", "train_mode"): lambda n: _under(_train_mode, lambda: n(np.zeros((1, 3, 64, 64), np.float32)))(),
    ("full", "targets"): lambda n: _under(_record, lambda: n(np.zeros((1, 3, 64, 64), np.float32), *_TARGETS))(),
    ("full", "six targets"): lambda n: _under(_record, lambda: n(np.zeros((1, 3, 64, 64), np.float32), *_TARGETS, 6))(),
    ("full", "detect_heads"): lambda n: n.detect_heads([np.zeros((1, 75, 2, 2), np.float32)] * 3, 64),
    ("full", "extract_features"): lambda n: n.extract_features(np.zeros((1, 3, 64, 64), np.float32)),
    ("full", "detect_two_streams"): lambda n: n.detect_two_streams(np.zeros((2, 3, 64, 64), np.float32)),
    ("full", "profile"): lambda n: n.profile(np.zeros((1, 3, 64, 64), np.float32)),
    ("full", "backward"): lambda n: n.backward(),
    # clip nets: the clip's shape first, then the device
    ("window", "valid"): lambda n: n(np.zeros((2, 3, 3, 64, 64), np.float32)),
    ("window", "rank"): lambda n: n(np.zeros((6, 3, 64, 64), np.float32)),
    ("window", "k"): lambda n: n(np.zeros((2, 2, 3, 64, 64), np.float32)),
    ("window", "channels"): lambda n: n(np.zeros((2, 3, 1, 64, 64), np.float32)),
    ("window", "list"): lambda n: n([[[[[0.0] * 4] * 4] * 3] * 2] * 2),
    ("window", "train_mode"): lambda n: _under(_train_mode, lambda: n(np.zeros((2, 2, 3, 64, 64), np.float32)))(),
    ("window", "targets"): lambda n: _under(_record, lambda: n(np.zeros((2, 3, 3, 64, 64), np.float32), *_TARGETS))(),
    ("window", "video"): lambda n: n.video(),
    ("hier", "valid"): lambda n: n(np.zeros((2, 3, 3, 64, 64), np.float32)),
    ("hier", "rank"): lambda n: n(np.zeros((6, 3, 64, 64), np.float32)),
    ("hier", "frames"): lambda n: n(np.zeros((2, 9, 3, 64, 64), np.float32)),
    ("hier", "channels"): lambda n: n(np.zeros((2, 3, 4, 64, 64), np.float32)),
    ("hier", "profile"): lambda n: n.profile(np.zeros((1, 2, 3, 64, 64), np.float32)),
    ("hier", "targets"): lambda n: _under(_record, lambda: n(np.zeros((2, 3, 3, 64, 64), np.float32), *_TARGETS))(),
    ("hier", "conv mode"): lambda n: n.set_conv_mode("split_bf16x3"),
    # heads nets: the routes' shapes first, then the device
    ("heads", "valid"): lambda n: n(*_routes((2,), 77, 77)),
    ("heads", "rank"): lambda n: n(*_swap(_routes((2,)), 2, (1024, 2, 2))),
    ("heads", "scalar"): lambda n: n(1.0, *_routes((2,))[1:]),
    ("heads", "batch"): lambda n: n(*_swap(_routes((2,)), 1, (1, 512, 4, 4))),
    ("heads", "channels"): lambda n: n(*_swap(_routes((2,)), 0, (2, 128, 8, 8))),
    ("heads", "stride16"): lambda n: n(*_swap(_routes((2,), 52, 52), 1, (2, 512, 27, 26))),
    ("heads", "tiny"): lambda n: n(*_routes((1,), 3, 52)),
    ("heads", "huge"): lambda n: n(*[np.broadcast_to(np.float32(0), (1, c, -(-513 // d), 4 // d))
                                     for c, d in ((256, 1), (512, 2), (1024, 4))]),
    ("heads", "empty batch"): lambda n: n(*_routes((0,))),
    ("heads", "train_mode"): lambda n: _under(_train_mode, lambda: n(*_swap(_routes((2,)), 0, (2, 128, 8, 8))))(),
    ("heads", "targets"): lambda n: _under(_record, lambda: n(*_routes((2,)), *_TARGETS))(),
    ("heads", "six targets"): lambda n: _under(_record, lambda: n(*_routes((2,)), *_TARGETS, 6))(),
    ("heads", "backward"): lambda n: n.backward(),
    # windowed heads net, (B, k, C, h, w) routes
    ("heads_window", "valid"): lambda n: n(*_routes((2, 3))),
    ("heads_window", "rank"): lambda n: n(*_routes((6,))),
    ("heads_window", "k"): lambda n: n(*_routes((3, 2))),
    ("heads_window", "batch"): lambda n: n(*_swap(_routes((2, 3)), 2, (1, 3, 1024, 2, 2))),
    ("heads_window", "channels"): lambda n: n(*_swap(_routes((2, 3)), 0, (2, 3, 128, 8, 8))),
    ("heads_window", "sizes"): lambda n: n(*_swap(_routes((2, 3)), 1, (2, 3, 512, 4, 5))),
    ("heads_window", "tiny"): lambda n: n(*_routes((2, 3), 3, 8)),
    ("heads_window", "huge"): lambda n: n(*[np.broadcast_to(np.float32(0), (1, 3, c, -(-513 // d), 4 // d))
                                            for c, d in ((256, 1), (512, 2), (1024, 4))]),
    ("heads_window", "too many"): lambda n: n(*[np.broadcast_to(np.float32(0), (171, 3) + f.shape[2:])
                                                for f in _routes((1, 3), 4, 4)]),
    ("heads_window", "empty batch"): lambda n: n(*_routes((0, 3))),
    ("heads_window", "train_mode"): lambda n: _under(_train_mode, lambda: n(*_routes((3, 2))))(),
    ("heads_window", "targets"): lambda n: _under(_record, lambda: n(*_routes((2, 3)), *_TARGETS))(),
    ("heads_window", "six targets"): lambda n: _under(_record, lambda: n(*_routes((2, 3)), *_TARGETS, 6))(),
    # ... and banks next to a table
    ("heads_window", "bank valid"): lambda n: n.from_bank(*_routes((7,), 77, 77), _TABLE),
    ("heads_window", "bank no table"): lambda n: n.from_bank(*_routes((7,)), None),
    ("heads_window", "bank rank"): lambda n: n.from_bank(*_routes((2, 3)), _TABLE),
    ("heads_window", "bank sizes"): lambda n: n.from_bank(*_swap(_routes((7,)), 2, (7, 1024, 3, 2)), _TABLE),
    ("heads_window", "bank frames"): lambda n: n.from_bank(*_swap(_routes((7,)), 1, (6, 512, 4, 4)), _TABLE),
    ("heads_window", "bank empty"): lambda n: n.from_bank(*_routes((0,)), _TABLE),
    ("heads_window", "table dtype"): lambda n: n.from_bank(*_routes((7,)), _TABLE.astype(np.float32)),
    ("heads_window", "table flat"): lambda n: n.from_bank(*_routes((7,)), _TABLE.reshape(-1)),
    ("heads_window", "table k"): lambda n: n.from_bank(*_routes((7,)), _TABLE[:, :2]),
    ("heads_window", "table past the end"): lambda n: n.from_bank(*_routes((7,)), _TABLE + 1),
    ("heads_window", "table negative"): lambda n: n.from_bank(*_routes((7,)), _TABLE - 1),
    ("heads_window", "table 513"): lambda n: n.from_bank(*_routes((7,)), np.zeros((171, 3), np.int32)),
    ("heads_window", "table no rows"): lambda n: n.from_bank(*_routes((7,)), np.zeros((0, 3), np.int32)),
    ("heads_window", "table 510"): lambda n: n.from_bank(*_routes((5,)), np.arange(510).reshape(170, 3) % 5),
    ("heads_window", "bank train_mode"): lambda n: _under(_train_mode, lambda: n.from_bank(*_routes((7,)), _TABLE + 1))(),
    ("heads_window", "bank targets"): lambda n: _under(_record, lambda: n.from_bank(*_routes((7,)), _TABLE, *_TARGETS))(),
    ("heads_window", "bank six targets"): lambda n: _under(
        _record, lambda: n.from_bank(*_routes((7,)), _TABLE, *_TARGETS, 6))(),
    ("heads_window", "video features"): lambda n: n.detect_video_features(*_routes((5,))),
    ("heads_window", "video features rank"): lambda n: n.detect_video_features(*_routes((5, 3))),
    ("heads_window", "video features clips"): lambda n: n.detect_video_features(*_routes((5,)), clips_per_step=171),
    ("heads_window", "backward"): lambda n: n.backward(),
}

_NO_DEVICE = ("RuntimeError", "parameters are not on a device: call net.collect_params().reset_ctx(ctx)")
_NO_FORWARD = ("RuntimeError", "backward() without a recorded forward")
_TARGETS_DUE = "gt_boxes, obj_t, centers_t, scales_t, weights_t, clas_t)"


def _usage(head):
    return "ValueError", "training call: %s, %s" % (head, _TARGETS_DUE)


def _not_routes(shapes):
    return "ValueError", ("route shapes %s are not the three Darknet-53 routes of one (B, 3, H, W) batch: expected (B, 256, h, w), "
                          "(B, 512, ceil(h/2), ceil(w/2)), (B, 1024, ceil(h/4), ceil(w/4)) with h, w in [4, 512]" % shapes)


def _not_frames(shapes):
    return "ValueError", ("route shapes %s are not the three Darknet-53 routes of the same frames: expected (.., 256, h, w), "
                          "(.., 512, ceil(h/2), ceil(w/2)), (.., 1024, ceil(h/4), ceil(w/4)) with h, w in [4, 512]" % shapes)


def _not_window(shape):
    return "ValueError", "a window net takes (B, k, 3, H, W) clips with k = 3, got %s" % shape


def _not_hier(shape):
    return "ValueError", "a hierarchical net [3, 1, 1, 1, 1] takes (B, T, 3, H, W) clips with T = 3, got %s" % shape


def _bad_table(what):
    return "ValueError", "table of shape %s: expected a (B, k) integer array with k = 3" % what


ERRORS = {
    ("full", "valid"): _NO_DEVICE,
    ("full", "rank"): _NO_DEVICE,
    ("full", "train_mode"): _NO_DEVICE,
    ("full", "targets"): _usage("net(x"),
    ("full", "six targets"): _NO_DEVICE,
    ("full", "detect_heads"): _NO_DEVICE,
    ("full", "extract_features"): _NO_DEVICE,
    ("full", "detect_two_streams"): _NO_DEVICE,
    ("full", "profile"): _NO_DEVICE,
    ("full", "backward"): _NO_FORWARD,
    ("window", "valid"): _NO_DEVICE,
    ("window", "rank"): _not_window("(6, 3, 64, 64)"),
    ("window", "k"): _not_window("(2, 2, 3, 64, 64)"),
    ("window", "channels"): _not_window("(2, 3, 1, 64, 64)"),
    ("window", "list"): _not_window("(2, 2, 3, 4, 4)"),
    ("window", "train_mode"): _not_window("(2, 2, 3, 64, 64)"),
    ("window", "targets"): _usage("net(x"),
    ("window", "video"): _NO_DEVICE,
    ("hier", "valid"): _NO_DEVICE,
    ("hier", "rank"): _not_hier("(6, 3, 64, 64)"),
    ("hier", "frames"): _not_hier("(2, 9, 3, 64, 64)"),
    ("hier", "channels"): _not_hier("(2, 3, 4, 64, 64)"),
    ("hier", "profile"): _not_hier("(1, 2, 3, 64, 64)"),
    ("hier", "targets"): _usage("net(x"),
    ("hier", "conv mode"): ("NotImplementedError", "conv mode 'split_bf16x3': a hierarchical net runs the exact fp32 kernels only"),
    ("heads", "valid"): _NO_DEVICE,
    ("heads", "rank"): _not_routes("[(2, 256, 8, 8), (2, 512, 4, 4), (1024, 2, 2)]"),
    ("heads", "scalar"): _not_routes("[(), (2, 512, 4, 4), (2, 1024, 2, 2)]"),
    ("heads", "batch"): _not_routes("[(2, 256, 8, 8), (1, 512, 4, 4), (2, 1024, 2, 2)]"),
    ("heads", "channels"): _not_routes("[(2, 128, 8, 8), (2, 512, 4, 4), (2, 1024, 2, 2)]"),
    ("heads", "stride16"): _not_routes("[(2, 256, 52, 52), (2, 512, 27, 26), (2, 1024, 13, 13)]"),
    ("heads", "tiny"): _not_routes("[(1, 256, 3, 52), (1, 512, 2, 26), (1, 1024, 1, 13)]"),
    ("heads", "huge"): _not_routes("[(1, 256, 513, 4), (1, 512, 257, 2), (1, 1024, 129, 1)]"),
    ("heads", "empty batch"): _not_routes("[(0, 256, 8, 8), (0, 512, 4, 4), (0, 1024, 2, 2)]"),
    ("heads", "train_mode"): _not_routes("[(2, 128, 8, 8), (2, 512, 4, 4), (2, 1024, 2, 2)]"),
    ("heads", "targets"): _usage("net(f1, f2, f3"),
    ("heads", "six targets"): _NO_DEVICE,
    ("heads", "backward"): _NO_FORWARD,
    ("heads_window", "valid"): _NO_DEVICE,
    ("heads_window", "rank"): ("ValueError", "route shapes [(6, 256, 8, 8), (6, 512, 4, 4), (6, 1024, 2, 2)]: expected three "
                                             "(B, k, C, h, w) tensors"),
    ("heads_window", "k"): ("ValueError", "route shapes [(3, 2, 256, 8, 8), (3, 2, 512, 4, 4), (3, 2, 1024, 2, 2)]: expected "
                                          "(B, k, C, h, w) with k = 3 and one B"),
    ("heads_window", "batch"): ("ValueError", "route shapes [(2, 3, 256, 8, 8), (2, 3, 512, 4, 4), (1, 3, 1024, 2, 2)]: expected "
                                              "(B, k, C, h, w) with k = 3 and one B"),
    ("heads_window", "channels"): _not_frames("[(6, 128, 8, 8), (6, 512, 4, 4), (6, 1024, 2, 2)]"),
    ("heads_window", "sizes"): _not_frames("[(6, 256, 8, 8), (6, 512, 4, 5), (6, 1024, 2, 2)]"),
    ("heads_window", "tiny"): _not_frames("[(6, 256, 3, 8), (6, 512, 2, 4), (6, 1024, 1, 2)]"),
    ("heads_window", "huge"): _not_frames("[(3, 256, 513, 4), (3, 512, 257, 2), (3, 1024, 129, 1)]"),
    ("heads_window", "too many"): ("ValueError", "B * k = 171 x 3: between 1 and 512 table entries (they travel in the kernel "
                                                 "arguments)"),
    ("heads_window", "empty batch"): _not_frames("[(0, 256, 8, 8), (0, 512, 4, 4), (0, 1024, 2, 2)]"),
    ("heads_window", "train_mode"): ("ValueError", "route shapes [(3, 2, 256, 8, 8), (3, 2, 512, 4, 4), (3, 2, 1024, 2, 2)]: "
                                                   "expected (B, k, C, h, w) with k = 3 and one B"),
    ("heads_window", "targets"): _usage("net(f1, f2, f3"),
    ("heads_window", "six targets"): _NO_DEVICE,
    ("heads_window", "bank valid"): _NO_DEVICE,
    ("heads_window", "bank no table"): ("ValueError", "from_bank needs a (B, k) table"),
    ("heads_window", "bank rank"): ("ValueError", "route shapes [(2, 3, 256, 8, 8), (2, 3, 512, 4, 4), (2, 3, 1024, 2, 2)]: "
                                                  "expected three (T, C, h, w) banks next to a table"),
    ("heads_window", "bank sizes"): _not_frames("[(7, 256, 8, 8), (7, 512, 4, 4), (7, 1024, 3, 2)]"),
    ("heads_window", "bank frames"): _not_frames("[(7, 256, 8, 8), (6, 512, 4, 4), (7, 1024, 2, 2)]"),
    ("heads_window", "bank empty"): _not_frames("[(0, 256, 8, 8), (0, 512, 4, 4), (0, 1024, 2, 2)]"),
    ("heads_window", "table dtype"): _bad_table("(2, 3), dtype float32"),
    ("heads_window", "table flat"): _bad_table("(6,), dtype int64"),
    ("heads_window", "table k"): _bad_table("(2, 2), dtype int64"),
    ("heads_window", "table past the end"): ("ValueError", "table entries must lie in [0, 7), the frames of the bank (got 1 ... 7)"),
    ("heads_window", "table negative"): ("ValueError", "table entries must lie in [0, 7), the frames of the bank (got -1 ... 5)"),
    ("heads_window", "table 513"): ("ValueError", "B * k = 171 x 3: between 1 and 512 table entries (they travel in the kernel "
                                                  "arguments)"),
    ("heads_window", "table no rows"): ("ValueError", "B * k = 0 x 3: between 1 and 512 table entries (they travel in the kernel "
                                                      "arguments)"),
    ("heads_window", "table 510"): _NO_DEVICE,
    ("heads_window", "bank train_mode"): ("ValueError", "table entries must lie in [0, 7), the frames of the bank (got 1 ... 7)"),
    ("heads_window", "bank targets"): _usage("net.from_bank(f1, f2, f3, table"),
    ("heads_window", "bank six targets"): _NO_DEVICE,
    ("heads_window", "video features"): _NO_DEVICE,
    ("heads_window", "video features rank"): ("ValueError", "expected (T, C, h, w) routes with T >= 1, got (5, 3, 256, 8, 8)"),
    ("heads_window", "video features clips"): ("ValueError", "clips_per_step 171 x k 3: between 1 and 512 table entries"),
    ("heads_window", "backward"): _NO_FORWARD,
}


@pytest.fixture(scope="module")
def nets():
    return {kind: _net(kind) for kind in KINDS}


@pytest.mark.parametrize("kind,case", sorted(CALLS))
def test_errors_before_the_device(nets, kind, case):
    net = nets[kind]
    assert net._device is None
    assert _caught(lambda: CALLS[kind, case](net)) == ERRORS[kind, case]
    assert net._plan is None and net._device is None


# ---------------------------------------------------------------- constructor errors
CTOR_CALLS = {
    "window k": lambda vy: vy.YOLOV3Window(C20, k=1),
    "window k text": lambda vy: vy.YOLOV3Window(C20, k=3, k_join_type="cat"),
    "heads window k": lambda vy: vy.YOLOV3NoBackboneWindow(C20, k=0, k_join_type="mean"),
    "heads window join": lambda vy: vy.YOLOV3NoBackboneWindow(C20, k=2, k_join_type=None),
    "hier list": lambda vy: vy.YOLOV3Hier(C20, hierarchical=[3, 1, 3, 1, 1]),
    "hier last": lambda vy: vy.YOLOV3Hier(C20, hierarchical=(3, 3, 3, 3, 3)),
    "hier not a list": lambda vy: vy.YOLOV3Hier(C20, hierarchical=3),
    "darknet53 late join": lambda vy: vy.yolo3_darknet53(C20, pretrained_base=False, k=3, k_join_type="max", k_join_pos="late"),
    "darknet53 hier conv": lambda vy: vy.yolo3_darknet53(C20, pretrained_base=False, new_model=True,
                                                        hierarchical=[3, 1, 1, 1, 1], h_join_type="conv"),
    "no_backbone cat": lambda vy: vy.yolo3_no_backbone(C20, k=3, k_join_type="cat", k_join_pos="early"),
    "pos_iou_thresh": lambda vy: vy.YOLOV3(C20, pos_iou_thresh=0.5),
}
_NOT_BUILT = "yolo3_darknet53: option(s) %s select a temporal/two-stream research variant outside the MI355X hot path"
_BAD_HIER = "hierarchical net: hierarchical must be a run of 3s followed by 1s, five entries, the last one 1 (got %s)"
CTOR_ERRORS = {
    "window k": ("ValueError", "window net: k >= 2 and k_join_type in ['max', 'mean'] (got k=1, 'max')"),
    "window k text": ("ValueError", "window net: k >= 2 and k_join_type in ['max', 'mean'] (got k=3, 'cat')"),
    "heads window k": ("ValueError", "windowed heads net: k >= 2 and k_join_type in ['max', 'mean'] (got k=0, 'mean')"),
    "heads window join": ("ValueError", "windowed heads net: k >= 2 and k_join_type in ['max', 'mean'] (got k=2, None)"),
    "hier list": ("ValueError", _BAD_HIER % "[3, 1, 3, 1, 1]"),
    "hier last": ("ValueError", _BAD_HIER % "(3, 3, 3, 3, 3)"),
    "hier not a list": ("ValueError", _BAD_HIER % "3"),
    "darknet53 late join": ("NotImplementedError", _NOT_BUILT % "k, k_join_type, k_join_pos"),
    "darknet53 hier conv": ("NotImplementedError", _NOT_BUILT % "h_join_type"),
    "no_backbone cat": ("NotImplementedError", "yolo3_no_backbone: k=3, k_join_type='cat', k_join_pos='early' \u2014 only k >= 2 "
                                               "with k_join_type 'max' or 'mean' and k_join_pos='early' is built"),
    "pos_iou_thresh": ("NotImplementedError", "pos_iou_thresh(0.5) < 1.0 is not implemented!"),
}


@pytest.mark.parametrize("case", sorted(CTOR_CALLS))
def test_constructor_errors(case):
    import videoyolo_amd as vy
    assert _caught(lambda: CTOR_CALLS[case](vy)) == CTOR_ERRORS[case]


def test_copies_keep_the_constructor_arguments():
    """``_ctor_kwargs`` of every kind, through the two copies that use it."""
    import copy
    for kind in KINDS:
        net = _net(kind)
        twin = copy.deepcopy(net)
        assert type(twin) is type(net) and _surface(twin) == _surface(net)
        for name in ("k", "k_join_type", "hierarchical", "frames"):
            assert getattr(twin, name, None) == getattr(net, name, None)
