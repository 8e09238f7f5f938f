"""-m "not gpu": the five kinds of net at the C-ABI — which entry point serves which kind, as one table, and how many
frames per batch entry every tap of every kind holds.  Nothing is bound and nothing launches a kernel."""
import ctypes

import pytest

from videoyolo_amd import _lib

INVALID, STATE = -1, -2
KINDS = ("full", "heads", "window", "heads-window", "hier")

IMAGES = {"full", "window", "hier"}
VIDEO = {"window"}
SERVED = {
    "vy_net_forward_infer": IMAGES,
    "vy_net_train_forward": IMAGES,
    "vy_net_train_mode_forward": IMAGES,
    "vy_net_train_backward": IMAGES,
    "vy_net_profile_infer": {"full", "hier"},
    "vy_net_forward_features": {"full"},
    "vy_net_forward_infer_routes": {"heads"},
    "vy_net_train_forward_routes": {"heads"},
    "vy_net_train_mode_forward_routes": {"heads"},
    "vy_net_train_backward_routes": {"heads", "heads-window"},
    "vy_net_forward_infer_bank": {"heads-window"},
    "vy_net_train_forward_bank": {"heads-window"},
    "vy_net_train_mode_forward_bank": {"heads-window"},
    "vy_net_video_workspace_bytes": VIDEO,
    "vy_net_bind_video": VIDEO,
    "vy_net_video_push": VIDEO,
    "vy_net_video_detect": VIDEO,
    "vy_net_video_read_slot": VIDEO,
}


def _create(lib, kind, k=2, num_class=3):
    h = ctypes.c_void_p()
    if kind == "full":
        rc = lib.vy_net_create(num_class, ctypes.byref(h))
    elif kind == "heads":
        rc = lib.vy_net_create_heads(num_class, ctypes.byref(h))
    elif kind == "window":
        rc = lib.vy_net_create_window(num_class, k, _lib.VY_JOIN_MAX, ctypes.byref(h))
    elif kind == "heads-window":
        rc = lib.vy_net_create_heads_window(num_class, k, _lib.VY_JOIN_MAX, ctypes.byref(h))
    else:
        rc = lib.vy_net_create_hier(num_class, 1, ctypes.byref(h))
    _lib.check(rc)
    return h


def _call_with_nulls(lib, entry, net):
    """`entry` on `net` with null for every pointer and 0 for every number behind it."""
    _, argtypes = _lib.SIGNATURES[entry]
    rest = [0 if t in (ctypes.c_int32, ctypes.c_size_t) else None for t in argtypes[1:]]
    return getattr(lib, entry)(net, *rest)


@pytest.fixture(scope="module")
def nets():
    lib = _lib.load()
    made = {kind: _create(lib, kind) for kind in KINDS}
    yield lib, made
    for h in made.values():
        lib.vy_net_destroy(h)


@pytest.mark.parametrize("entry", sorted(SERVED))
def test_every_entry_serves_its_kinds_and_no_other(nets, entry):
    """A kind the entry does not serve is VY_ERR_STATE and the message names the entry; a kind it serves gets as far as the
    arguments, which are all null: VY_ERR_INVALID.  The backward of the *_routes entries reads nothing from the routes, so on
    a windowed heads-only net, which has none to pass, null routes get as far as the state of the net: nothing is bound."""
    lib, made = nets
    for kind in KINDS:
        rc = _call_with_nulls(lib, entry, made[kind])
        msg = lib.vy_last_error().decode()
        if entry == "vy_net_video_workspace_bytes":
            assert rc == 0, kind
            continue
        if kind not in SERVED[entry]:
            assert rc == STATE and entry in msg, (kind, rc, msg)
            assert "not bound" not in msg, (kind, msg)
        elif (entry, kind) == ("vy_net_train_backward_routes", "heads-window"):
            assert rc == STATE and "not bound" in msg, (kind, rc, msg)
        else:
            assert rc == INVALID, (kind, rc, msg)


@pytest.mark.parametrize("entry", sorted(SERVED))
def test_a_null_net_is_an_invalid_argument_everywhere(entry):
    lib = _lib.load()
    rc = _call_with_nulls(lib, entry, None)
    assert rc == (0 if entry == "vy_net_video_workspace_bytes" else INVALID)


def test_the_table_covers_every_entry_that_takes_a_kind():
    """Every forward, backward and video entry of the binding is a row of the table."""
    rows = {n for n in _lib.SIGNATURES
            if n.startswith(("vy_net_forward_", "vy_net_train_forward", "vy_net_train_mode_forward", "vy_net_train_backward",
                             "vy_net_video_", "vy_net_profile_")) or n == "vy_net_bind_video"}
    assert rows == set(SERVED)


# ------------------------------------------------------------------------------------------------ frames of a tap
def _conv_names(lib, h):
    names = []
    for i in range(lib.vy_net_num_convs(h)):
        info = _lib.ConvInfo()
        _lib.check(lib.vy_net_conv_info(h, i, ctypes.byref(info)))
        names.append(info.name.decode())
    return names


def _tap_frames(lib, h, name):
    """(return code, frames)"""
    f = ctypes.c_int32(-7)
    rc = lib.vy_net_tap_frames(h, name.encode(), ctypes.byref(f))
    return rc, f.value


@pytest.mark.parametrize("kind,k", [("full", 0), ("heads", 0), ("window", 2), ("window", 3), ("heads-window", 2),
                                    ("heads-window", 3)])
def test_tap_frames_of_every_cell_of_every_kind(kind, k):
    """Only the stem and stage cells of a window net hold k frames per batch entry — the rule `name.startswith("stages.")`
    — and every other cell of every kind one.  The pooled routes pool.0 .. pool.2 are taps of the two window kinds alone,
    one frame each; hpool.<i> of a hierarchical net alone (tests/test_hier_host.py has those)."""
    lib = _lib.load()
    h = _create(lib, kind, k=k)
    try:
        names = _conv_names(lib, h)
        assert len(names) == (23 if kind.startswith("heads") else 75)
        for name in names:
            want = k if kind == "window" and name.startswith("stages.") else 1
            assert _tap_frames(lib, h, name) == (0, want), name
        for i in range(3):
            got = _tap_frames(lib, h, "pool.%d" % i)
            assert got == ((0, 1) if k else (INVALID, -7)), (i, got)
        for name in ("pool.3", "pool.00", "pool.", "hpool.0", "stages.0.0.", "", "nothing"):
            assert _tap_frames(lib, h, name) == (INVALID, -7), name
    finally:
        lib.vy_net_destroy(h)
