"""-m "not gpu": the per-net semantics setting (vy_net_set_semantics / net.set_semantics) on the host — defaults, round trip,
validation, scope, copies — and the census of tests/semantics_cases.py: every constructed case must change under the
switches it was built for and under no other, settled on the CPU (switchable plain-Python box_nms on the CPU decode) before
any GPU test relies on it."""
import copy
import ctypes

import numpy as np
import pytest

import semantics_cases as SC
from test_mxnet_kit_sensitivity import DEFAULTS, py_box_nms
from videoyolo_amd import _lib

CLASSES = ["a", "b", "c"]
FIELDS = ("nms_valid_ge", "nms_overlap_ge", "nms_tie_descending", "nms_topk_after", "nms_iou_plus_one",
          "bn_running_var_unbiased")
# `drop_background` of the plain-Python box_nms has no counterpart: ids on this path are 0 .. C-1, no row has id -1
PY_DEFAULTS = dict({k: v for k, v in DEFAULTS.items() if k != "drop_background"}, running_var_unbiased=False)


def _nets():
    import videoyolo_amd as vy
    return [("full", lambda: vy.yolo3_darknet53(CLASSES, pretrained_base=False)),
            ("heads", lambda: vy.yolo3_no_backbone(CLASSES)),
            ("window_max", lambda: vy.yolo3_darknet53(CLASSES, pretrained_base=False, k=3, k_join_type="max", k_join_pos="early")),
            ("window_mean", lambda: vy.yolo3_darknet53(CLASSES, pretrained_base=False, k=2, k_join_type="mean", k_join_pos="early")),
            ("heads_window", lambda: vy.yolo3_no_backbone(CLASSES, k=3, k_join_type="max", k_join_pos="early"))]


NETS = _nets()


def _get(lib, h):
    s = _lib.Semantics()
    assert lib.vy_net_get_semantics(h, ctypes.byref(s)) == 0
    return [getattr(s, f) for f in FIELDS] + list(s.reserved)


def test_defaults_are_zero_and_python_names_them_like_the_reference_nms():
    lib = _lib.load()
    h = ctypes.c_void_p()
    _lib.check(lib.vy_net_create(3, ctypes.byref(h)))
    assert _get(lib, h) == [0] * 16
    lib.vy_net_destroy(h)
    assert SC.DEFAULTS == {k: DEFAULTS[k] for k in SC.SWITCHES}
    for _, make in NETS:
        assert make().semantics == PY_DEFAULTS


@pytest.mark.parametrize("kind", [n for n, _ in NETS])
def test_round_trip_on_every_kind_of_net(kind):
    net = dict(NETS)[kind]()
    lib = net._lib
    for i, kw in enumerate(PY_DEFAULTS):
        net.set_semantics(**{kw: not PY_DEFAULTS[kw]})
        want = dict(PY_DEFAULTS, **{kw: not PY_DEFAULTS[kw]})
        assert net.semantics == want
        raw = _get(lib, net._h)
        assert raw[:6] == [int(j == i) for j in range(6)] and raw[6:] == [0] * 10, (kw, raw)   # keyword i is field i
        net.set_semantics()                       # omitted keywords keep their value
        assert net.semantics == want
        net.set_semantics(**{kw: PY_DEFAULTS[kw]})
    assert net.semantics == PY_DEFAULTS
    flipped = {k: not v for k, v in PY_DEFAULTS.items()}
    net.set_semantics(**flipped)
    assert net.semantics == flipped and _get(lib, net._h)[:6] == [1] * 6
    with pytest.raises(TypeError):
        net.set_semantics(plus_one=2)
    with pytest.raises(TypeError):
        net.set_semantics(True)                   # keyword-only
    assert net.semantics == flipped


def test_invalid_structs_are_refused_and_change_nothing():
    lib = _lib.load()
    h = ctypes.c_void_p()
    _lib.check(lib.vy_net_create(3, ctypes.byref(h)))
    good = _lib.Semantics(nms_overlap_ge=1, nms_topk_after=1)
    assert lib.vy_net_set_semantics(h, ctypes.byref(good)) == 0
    before = _get(lib, h)
    assert before[:6] == [0, 1, 0, 1, 0, 0]
    bad = []
    for f in FIELDS:
        for v in (2, -1, 1 << 30):
            bad.append(_lib.Semantics(**{f: v}))
    for i in range(10):
        s = _lib.Semantics()
        s.reserved[i] = 1
        bad.append(s)
    for s in bad:
        assert lib.vy_net_set_semantics(h, ctypes.byref(s)) == -1, _get(lib, h)
        assert "vy_semantics" in lib.vy_last_error().decode()
        assert _get(lib, h) == before
    assert lib.vy_net_set_semantics(h, None) == -1 and lib.vy_net_set_semantics(None, ctypes.byref(good)) == -1
    assert lib.vy_net_get_semantics(h, None) == -1 and lib.vy_net_get_semantics(None, ctypes.byref(good)) == -1
    assert _get(lib, h) == before
    lib.vy_net_destroy(h)


def test_the_setting_is_per_net_and_needs_no_plan():
    a, b = NETS[0][1](), NETS[1][1]()
    a.set_semantics(tie_ascending=False, running_var_unbiased=True)
    b.set_semantics(plus_one=True)
    assert a.semantics == dict(PY_DEFAULTS, tie_ascending=False, running_var_unbiased=True)
    assert b.semantics == dict(PY_DEFAULTS, plus_one=True)
    assert NETS[0][1]().semantics == PY_DEFAULTS
    # sizing a plan or changing the NMS parameters leaves it alone
    assert a._lib.vy_net_workspace_bytes(a._h, 1, 64, 64) > 0
    a.set_nms(0.3, 50, 10)
    assert a.semantics == dict(PY_DEFAULTS, tie_ascending=False, running_var_unbiased=True)


@pytest.mark.parametrize("kind", [n for n, _ in NETS])
def test_deep_copy_keeps_the_setting(kind):
    net = dict(NETS)[kind]()
    net.set_semantics(strict_valid=False, topk_first=False, running_var_unbiased=True)
    twin = copy.deepcopy(net)
    assert type(twin) is type(net) and twin._h.value != net._h.value
    assert twin.semantics == net.semantics == dict(PY_DEFAULTS, strict_valid=False, topk_first=False, running_var_unbiased=True)
    twin.set_semantics(strict_valid=True)
    assert net.semantics["strict_valid"] is False


def test_reset_class_keeps_the_setting():
    net = NETS[0][1]()
    net.initialize(init="synthetic", seed=1)
    net.set_semantics(strict_iou=False, plus_one=True)
    net.reset_class(["x", "y"])
    assert net.semantics == dict(PY_DEFAULTS, strict_iou=False, plus_one=True)


def test_set_semantics_and_set_nms_drop_captured_graphs():
    net = NETS[1][1]()
    net._graphs = {"k": object()}
    net.set_semantics(plus_one=True)
    assert net._graphs == {}
    net._graphs = {"k": object()}
    net.set_nms(0.45, 400, 100)
    assert net._graphs == {}


# ---------------------------------------------------------------------------------------------------------- the census
CASES = SC.all_cases()


def test_the_cases_cover_every_launch_path_and_every_switch_on_it():
    by_path = {}
    for c in CASES:
        by_path.setdefault(c["path"], set()).update(c["flips"])
    assert set(by_path) == {"small", "big", "all", "cap", "overflow"}
    # the paths that hold a site of every choice (a top-k cut exists only where nms_topk > 0)
    assert by_path["small"] == by_path["big"] == set(SC.SWITCHES)
    assert by_path["all"] == set(SC.SWITCHES) - {"topk_first"}
    assert by_path["cap"] == set(SC.SWITCHES)
    # (with the cut after suppression a launch leaves the select path, the overflow walk with it)
    assert by_path["overflow"] == set(SC.SWITCHES) - {"topk_first"}
    for c in CASES:   # the four flags that leave the cut where it is are combined on every case, all five wherever affordable
        names = [n for n, _ in SC.settings_for(c)]
        assert "four_no_cut" in names and ("all_five" in names or c["path"] == "overflow"), c["name"]
    big = [c for c in CASES if c["path"] == "big"]
    assert all(c["heads"][0].shape[0] == SC.BIG_B and len(SC.unique_images(c)[0]) > 1 for c in big)
    rows = {c["name"]: SC.out_rows(c) for c in CASES}
    assert rows["valid_at_thresh"] == 400 and rows["valid_at_thresh/post100"] == 100 and rows["valid_at_thresh/all"] == 756
    assert rows["cap1025"] == 1025 and rows["overflow"] == 400
    assert rows["cap_pair/readback"] == 1027 > 1024 >= rows["cap_pair/lds"] == 1000


def test_the_score_at_the_threshold_has_its_bits():
    case = next(c for c in CASES if c["name"] == "valid_at_thresh")
    rows, _ = SC.decoded_rows(case)
    near = sorted(int(np.float32(s).view(np.uint32)) for s in rows[0, :, 1] if s > 1e-3)
    t = int(SC.VALID.view(np.uint32))
    assert near == [t - 1, t, t + 1], (near, t)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_every_case_changes_under_the_switches_it_names_and_no_other(case):
    base = SC.reference(case, py_box_nms, {})
    assert (base[..., 0] >= 0).any(), "nothing kept: the case shows nothing"
    changed = set()
    for name, setting in SC.settings_for(case):
        if len(setting) == 1 and not np.array_equal(base, SC.reference(case, py_box_nms, setting)):
            changed.add(name)
    want = case["flips"]
    assert not want - changed, "flipping %s does not change %s: the case would not notice" % (sorted(want - changed), case["name"])
    assert not changed - want, "flipping %s also changes %s" % (sorted(changed - want), case["name"])


def test_the_cap_case_ties_across_the_chunk_boundary():
    case = next(c for c in CASES if c["name"] == "cap1025")
    rows, _ = SC.decoded_rows(case)
    s = np.sort(rows[0, :, 1][rows[0, :, 1] > SC.VALID])[::-1]
    assert len(s) == 1512 and s[1007] > s[1008] == s[1023] == s[1024] == s[1511]
    case = next(c for c in CASES if c["name"] == "overflow")
    rows, _ = SC.decoded_rows(case)
    assert len(set(rows[0, :, 1].tolist())) == 1 and rows.shape[1] == 20160 > 16384


@pytest.mark.parametrize("name", ["cap_pair/readback", "cap_pair/lds"])
def test_the_pair_at_the_iou_threshold_is_split_by_the_chunk_boundary(name):
    """A is the best candidate, B candidate 1024 — the first of the second chunk — in either tie order; A is kept, and fewer
    rows than the output holds are kept before B, so the chunked kernel reaches the second chunk and B meets A as a kept
    row of an earlier chunk."""
    case = next(c for c in CASES if c["name"] == name)
    rows = SC.decoded_rows(case)[0][0]
    for asc in (True, False):
        order = sorted((i for i in range(len(rows)) if rows[i, 1] > SC.VALID), key=lambda i: (-float(rows[i, 1]), i if asc else -i))
        a, b = order[0], order[1024]
        assert rows[a, 0] == rows[b, 0] == 0 and len(order) == 1026
        assert (rows[b, 2:6] - rows[a, 2:6]).tolist() == [8, 0, 8, 0] and (rows[a, 4] - rows[a, 2], rows[a, 5] - rows[a, 3]) == (16, 30)
    base = SC.reference(case, py_box_nms, {})[0]
    kept = base[base[:, 0] >= 0]
    assert a in kept[:, 6] and b in kept[:, 6]          # IoU == nms_thresh: kept by default
    assert list(kept[:, 6]).index(b) < SC.out_rows(case)
    for flip in (dict(strict_iou=False), dict(plus_one=True)):
        alt = SC.reference(case, py_box_nms, flip)[0]
        assert a in alt[:, 6] and b not in alt[:, 6], flip


def test_the_overflow_walk_meets_the_valid_threshold():
    """`overflow_valid`: bucket 10 holds 80 scores one ulp above 0.01f, more than the list's 16 384 at 0.01f exactly and 80
    one ulp below; only the first are valid by default, the first two groups with `>=`."""
    case = next(c for c in CASES if c["name"] == "overflow_valid")
    s = SC.decoded_rows(case)[0][0][:, 1]
    t = int(SC.VALID.view(np.uint32))
    bits = np.ascontiguousarray(s, np.float32).view(np.uint32)
    in_bucket = (s * np.float32(1024)).astype(np.int32) == 10
    assert int((s * np.float32(1024))[bits == t][0]) == 10
    assert (bits[in_bucket] >= t - 1).all() and (bits[in_bucket] <= t + 1).all()
    assert ((bits == t + 1).sum(), (bits == t - 1).sum()) == (80, 80) and (bits == t).sum() > 16384
    assert (s > SC.VALID).sum() == 82 and (s >= SC.VALID).sum() == 82 + (bits == t).sum()
    four = dict(SC.SETTINGS)["four_no_cut"]
    assert (SC.reference(case, py_box_nms, four)[0][:, 0] >= 0).sum() > (SC.reference(case, py_box_nms, {})[0][:, 0] >= 0).sum()
