"""Constructed head tensors for the per-net semantics switches (`net.set_semantics`, include/vyolo.h vy_semantics), shared
by tests/test_semantics_host.py (the census: does every case discriminate what it was built for?) and
tests/test_gpu_semantics.py (the HIP tail against the switchable plain-Python box_nms on the CPU decode).

A case is a dict: name, heads (three (B, 3 * (5 + C), g, g) arrays, strides 32, 16, 8), size, classes, nms_thresh, nms_topk,
post_nms, path (which launch path of csrc/detect.hip it takes with the default setting) and `flips`: the keywords of
`py_box_nms` (tests/test_mxnet_kit_sensitivity.py) whose flip must change its output — no other switch may.

Launch paths (vy_launch_detect):
  small     nms_topk in [1, 1024], grid.x * B < 256: hist, select, compact_kernel<1>, refine, sort_nms
  big       the same with B = 256: compact_kernel<kItemsPerThread> (252 anchors are one block per image, so 256 images)
  all       nms_topk = -1: hist + nms_all_kernel, every valid candidate
  cap       nms_topk = 1025 (> 1024): nms_all_kernel stopped after 1025 candidates, two chunks, a tie across their boundary;
            with post_nms = -1 the output has 1025 rows and the kept rows are read back from it, not from LDS
  overflow  20 160 equal scores in one bucket, more than the bucket list (kListCap = 16 384) holds: refine_kernel walks the
            score cache; nms_topk = 400 of them pass, chosen by the tie order alone.  `overflow_valid` overflows bucket 10
            (the bucket of 0.01f) under `strict_valid=False` only: its walk has to apply the valid test
`topk_first=False` sends every path down nms_all_kernel with no candidate cut.
"""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("mxnet_ops_kit", os.path.join(HERE, "golden", "mxnet_ops_kit.py"))
KIT = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(KIT)

F32 = np.float32
SIZE = KIT.HEAD_SIZE
VALID = F32(0.01)      # yolo3.py:1199
SWITCHES = ("strict_valid", "strict_iou", "tie_ascending", "topk_first", "plus_one")
BIG_B = 256

# what flipping one switch must do to the kit's own detect_heads cases (tests/test_mxnet_kit_sensitivity.py EXPECT, plus the
# +1 convention, which that file shows separately: it lifts the 240 / 720 pair to 279 / 775, over a threshold of 1 / 3)
KIT_FLIPS = {
    "heads_iou_at_thresh": {"strict_iou", "plus_one"},
    "heads_iou_below_thresh": set(),
    "heads_duplicate_scores": {"tie_ascending"},
    "heads_topk_cuts_through_tie": {"tie_ascending"},
    "heads_same_box_three_classes": {"tie_ascending"},
    "heads_tie_across_scales": {"tie_ascending"},
}


def _case(name, heads, flips, classes=KIT.HEAD_CLASSES, nms_thresh=0.45, nms_topk=400, post_nms=-1, path="small"):
    return dict(name=name, heads=[np.ascontiguousarray(h, F32) for h in heads], size=SIZE, classes=int(classes),
                nms_thresh=float(nms_thresh), nms_topk=int(nms_topk), post_nms=int(post_nms), path=path, flips=set(flips))


def out_rows(case):
    """Rows of the library's outputs (vy_net_set_nms): post_nms, else nms_topk, else all N * C."""
    if case["post_nms"] > 0:
        return case["post_nms"]
    if case["nms_topk"] > 0:
        return case["nms_topk"]
    return 3 * sum((case["size"] // d) ** 2 for d in (32, 16, 8)) * case["classes"]


# ------------------------------------------------------------------------------------------ a score of exactly 0.01f
def _score(O, cls_logit, obj_logit):
    """The decode's class score: sigmoid(class logit) * sigmoid(objectness logit), one fp32 product (yolo3.py:172-190)."""
    s = O.sigmoid(np.array([cls_logit, obj_logit], F32))
    return F32(s[0] * s[1])


def _obj_logit_for(O, cls_logit, want_bits):
    """Directed search: an objectness logit whose score with `cls_logit` has exactly the bits `want_bits`.  The score
    rises with the logit: bisect on the value, then walk the float32 neighbours."""
    bits = lambda x: int(_score(O, cls_logit, F32(x)).view(np.uint32))
    lo, hi = -1.0, 1.0
    assert bits(lo) < want_bits < bits(hi)
    for _ in range(60):
        mid = (lo + hi) / 2
        if bits(mid) < want_bits:
            lo = mid
        else:
            hi = mid
    x = F32(hi)
    for _ in range(256):
        got = bits(x)
        if got == want_bits:
            return x
        x = np.nextafter(x, F32(1 if got < want_bits else -1), dtype=F32)
    raise AssertionError("no objectness logit gives score bits %#x with class logit %r" % (want_bits, cls_logit))


CLS_LOGIT = F32(-3.875)
_OBJ = {}


def obj_logit(ulps):
    """The objectness logit that, with the class logit CLS_LOGIT, scores 0.01f moved by `ulps` (0, +1, -1); checked."""
    if ulps not in _OBJ:
        from oracle import yolo3_oracle as O
        want = int(VALID.view(np.uint32)) + ulps
        obj = _obj_logit_for(O, CLS_LOGIT, want)
        got = _score(O, CLS_LOGIT, obj)
        assert int(got.view(np.uint32)) == want and (got == VALID) == (ulps == 0), (got, want)
        _OBJ[ulps] = obj
    return _OBJ[ulps]


def put_threshold_trio(h, classes=KIT.HEAD_CLASSES):
    """Three disjoint 10 x 13 candidates (stride 8, anchor 0) of classes 0, 1, 2 whose scores are 0.01f exactly, one ulp
    above and one ulp below.  `put` fixes the objectness at +40; here it is written by hand."""
    for (y, x, c), ulps in zip(((1, 1, 0), (1, 5, 1), (5, 3, 2)), (0, 1, -1)):
        KIT.put(h, 2, y, x, 0, {c: float(CLS_LOGIT)}, classes=classes)
        h[2][0, 4, y, x] = obj_logit(ulps)
    return h


def valid_at_thresh_heads():
    return put_threshold_trio(KIT.blank_heads())


# ------------------------------------------------------------------------------------------------------- base cases
def _kit_heads(c):
    return [c["inputs"]["head0"], c["inputs"]["head1"], c["inputs"]["head2"]]


def base_cases():
    """B = 1, 64 x 64, 3 classes (756 rows): the kit's six detect_heads cases as they are, and one case per switch that the
    kit decides only at the operator level."""
    out = []
    for c in KIT.detect_heads_cases():
        out.append(_case(c["name"], _kit_heads(c), KIT_FLIPS[c["name"]], nms_thresh=c["params"]["nms_thresh"],
                         nms_topk=c["params"]["nms_topk"]))
    out.append(_case("valid_at_thresh", valid_at_thresh_heads(), {"strict_valid"}))
    # A and B overlap (IoU 1/3 > 0.3) in one class, C is disjoint and scores lower; nms_topk = 2.  Cut first: {A, B} -> A.
    # Cut after: A, C.  (The kit's nms_topk_before_suppression through the decode.)
    h = KIT.blank_heads()
    KIT.put(h, 2, 3, 2, 1, {0: 2.0})
    KIT.put(h, 2, 3, 3, 1, {0: 1.0})
    KIT.put(h, 2, 6, 6, 0, {0: 0.5})
    out.append(_case("topk_after", h, {"topk_first"}, nms_thresh=0.3, nms_topk=2))
    # the 16 x 30 pair 8 px apart: IoU 240 / 720 = 0.333 without +1, 279 / 775 = 0.36 with; nms_thresh between the two
    h = KIT.blank_heads()
    KIT.put(h, 2, 3, 2, 1, {0: 2.0})
    KIT.put(h, 2, 3, 3, 1, {0: 1.0})
    out.append(_case("plus_one", h, {"plus_one"}, nms_thresh=0.35))
    return out


def _tiled(case):
    """The case on 256 images: the tensors tiled, a few images mirrored left-right (the same candidates in other rows, so
    the images do not all decode alike)."""
    heads = [np.tile(h, (BIG_B, 1, 1, 1)) for h in case["heads"]]
    for b in (1, 77, 255):
        for h in heads:
            h[b] = h[b, :, :, ::-1]
    return dict(case, name=case["name"] + "@B256", heads=heads, path="big")


# survivors and their order do not hang on a top-k cut in these: they keep deciding their switch with nms_topk = -1
_NO_CUT = ("valid_at_thresh", "plus_one", "heads_iou_at_thresh", "heads_duplicate_scores", "heads_same_box_three_classes",
           "heads_tie_across_scales")


def cap_heads(classes=80):
    """More than 1025 valid candidates with a tie across the chunk boundary: every anchor is a candidate (objectness +40);
    classes 0-3 score sigmoid(2) — 4 x 252 = 1008 equal scores —, classes 4 and 5 sigmoid(1) — 504 equal scores, of which
    the first chunk of 1024 takes 16 and the second the one that is left of nms_topk = 1025 —, the other classes nothing."""
    h = KIT.blank_heads(classes=classes)
    P = 5 + classes
    for t in h:
        for a in range(3):
            t[:, a * P + 4] = 40.0
            t[:, a * P + 5:(a + 1) * P] = -40.0
            t[:, a * P + 5:a * P + 9] = 2.0
            t[:, a * P + 9:a * P + 11] = 1.0
    return h


def cap_pair_heads(classes=80):
    """The chunked kernel's suppression ACROSS chunks (nms_topk = 1027): A (class 0, the best score) is kept in the first
    chunk; 1023 equal-scoring candidates of classes 1-79 fill the chunk (the 12 stride-32 anchors x 79 classes and 75
    classes of one stride-16 anchor); B — A's 16 x 30 neighbour 8 px away, IoU 240 / 720 = nms_thresh, 279 / 775 with +1 —
    is candidate 1024, the first of the second chunk, so it meets A only as a kept row of an earlier chunk: in LDS when the
    output has at most 1024 rows, read back from the output when it has 1027.  After it come the three scores around
    0.01f: the one above is candidate 1025, the one at 0.01f candidate 1026 where it is valid."""
    h = KIT.blank_heads(classes=classes)
    KIT.put(h, 2, 3, 2, 1, {0: 4.0}, classes=classes)
    KIT.put(h, 2, 3, 3, 1, {0: 1.0}, classes=classes)
    for y in range(2):
        for x in range(2):
            for a in range(3):
                KIT.put(h, 0, y, x, a, {c: 2.0 for c in range(1, 80)}, classes=classes)
    KIT.put(h, 1, 0, 0, 0, {c: 2.0 for c in range(1, 76)}, classes=classes)
    return put_threshold_trio(h, classes)


def overflow_valid_heads(classes=80):
    """The overflow walk's valid test: every class of every anchor scores 0.01f EXACTLY (class logit CLS_LOGIT, objectness
    logit obj_logit(0)) except one anchor whose 80 classes score one ulp above, one whose 80 score one ulp below — all of
    them in linear bucket 10 — and the 240 / 720 pair A, B of class 0 in higher buckets.  With `>` 82 candidates are valid;
    with `>=` 20 000 are, the bucket overflows the list and refine_kernel has to find the 318 tied rows that pass
    nms_topk = 400 by walking the score cache with the same test."""
    P = 5 + classes
    h = KIT.blank_heads(classes=classes)
    for t in h:
        for a in range(3):
            t[:, a * P + 4] = obj_logit(0)
            t[:, a * P + 5:(a + 1) * P] = CLS_LOGIT
    h[2][0, 4, 0, 7] = obj_logit(1)
    h[2][0, 4, 7, 0] = obj_logit(-1)
    KIT.put(h, 2, 3, 2, 1, {0: 2.0}, classes=classes)
    KIT.put(h, 2, 3, 3, 1, {0: 1.0}, classes=classes)
    return h


def overflow_heads(classes=80):
    """Every logit equal (0): 20 160 scores of 0.25 in one bucket."""
    return [np.zeros_like(t) for t in KIT.blank_heads(classes=classes)]


def all_cases():
    base = base_cases()
    by_name = {c["name"]: c for c in base}
    out = list(base)
    # where the row count hangs on post_nms: 100 rows instead of nms_topk = 400
    for n in ("valid_at_thresh", "heads_duplicate_scores", "plus_one"):
        out.append(dict(by_name[n], name=n + "/post100", post_nms=100))
    out += [_tiled(c) for c in base]
    for n in _NO_CUT:
        out.append(dict(by_name[n], name=n + "/all", nms_topk=-1, path="all"))          # 756 output rows
    for n in ("valid_at_thresh", "heads_duplicate_scores"):
        out.append(dict(by_name[n], name=n + "/all/post100", nms_topk=-1, post_nms=100, path="all"))
    # 1008 + 504 candidates in two score levels, boxes on every cell: the tie order picks the 17 of the lower level that
    # pass the cut, cutting after suppression lets all 504 in, and the +1 convention moves neighbouring anchors' IoUs
    # (e.g. 33 x 23 boxes 8 px apart: 0.610 -> 0.619) — with nms_thresh 0.45 no pair sits between the two, see the census
    cap = cap_heads()
    out.append(_case("cap1025", cap, {"tie_ascending", "topk_first"}, classes=80, nms_topk=1025, path="cap"))
    # (its first 100 survivors all come from the upper level: only the tie order shows in them)
    out.append(_case("cap1025/post100", cap, {"tie_ascending"}, classes=80, nms_topk=1025, post_nms=100, path="cap"))
    # a second chunk of 276 candidates — the lower-level ties left of the cut —: a chunk of more than 32 and fewer than 1024
    # keys, which the kernel's rank sort splits over several thread groups; 774 rows kept, from both score levels
    out.append(_case("cap1300", cap, {"tie_ascending", "topk_first"}, classes=80, nms_topk=1300, path="cap"))
    third = float(F32(240.0) / F32(720.0))
    pair = cap_pair_heads()
    flips = {"strict_valid", "strict_iou", "tie_ascending", "plus_one"}
    out.append(_case("cap_pair/readback", pair, flips, classes=80, nms_thresh=third, nms_topk=1027, path="cap"))
    out.append(_case("cap_pair/lds", pair, flips, classes=80, nms_thresh=third, nms_topk=1027, post_nms=1000,
                     path="cap"))
    # The cut after suppression is left out of the overflow cases wherever more than 16 384 candidates are valid (`skip`:
    # settings_for): all of them would go through suppression — nms_all_kernel, the kernel of 'all' and 'cap', not the
    # overflow walk these cases are for — and the plain-Python reference needs a minute for them.  The four other flags
    # flipped together (`four_no_cut`) stand in for `all_five` there.
    out.append(dict(_case("overflow", overflow_heads(), {"tie_ascending"}, classes=80, nms_topk=400, path="overflow"),
                    skip=lambda s: not s.get("topk_first", True)))
    out.append(dict(_case("overflow_valid", overflow_valid_heads(), {"strict_valid", "strict_iou", "tie_ascending", "plus_one"},
                          classes=80, nms_thresh=third, nms_topk=400, path="overflow"),
                    skip=lambda s: not s.get("topk_first", True) and not s.get("strict_valid", True)))
    return out


# the settings the GPU tail is compared under: the default, every single flip, all five flipped, the four that leave the
# cut where it is, and descending ties with the cut after suppression (the two that change which kernel runs and what its
# keys hold)
DEFAULTS = dict(strict_valid=True, strict_iou=True, tie_ascending=True, topk_first=True, plus_one=False)
SETTINGS = [("default", {})] + [(k, {k: not DEFAULTS[k]}) for k in SWITCHES] + [
    ("all_five", {k: not DEFAULTS[k] for k in SWITCHES}),
    ("four_no_cut", {k: not DEFAULTS[k] for k in SWITCHES if k != "topk_first"}), ("tie_desc+cut_after", dict(tie_ascending=False, topk_first=False))]


def settings_for(case):
    skip = case.get("skip", lambda s: False)
    return [(n, s) for n, s in SETTINGS if not skip(s)]


# ------------------------------------------------------------------------------------------------------ the reference
def unique_images(case):
    """(indices of one representative per distinct image, image -> representative's position): the B = 256 cases hold three
    distinct images at most, and the plain-Python reference is per image."""
    b = case["heads"][0].shape[0]
    seen, reps, where = {}, [], []
    for i in range(b):
        key = b"".join(h[i].tobytes() for h in case["heads"])
        if key not in seen:
            seen[key] = len(reps)
            reps.append(i)
        where.append(seen[key])
    return reps, where


_DECODED = {}


def decoded_rows(case):
    """The CPU decode of the case's distinct images, (U, N * C, 7): the detection tensor's six columns and the row number
    as a seventh (`py_box_nms` copies whole rows, so its output carries the kept rows' indices).  Computed once."""
    if case["name"] not in _DECODED:
        from oracle import yolo3_oracle as O
        reps, where = unique_images(case)
        rows = O.OracleYolo3(case["classes"], {}).detections_from_heads([h[reps] for h in case["heads"]])
        idx = np.broadcast_to(np.arange(rows.shape[1], dtype=F32)[None, :, None], rows.shape[:2] + (1,))
        rows = np.concatenate([rows.astype(F32), idx], -1)
        rows.setflags(write=False)
        _DECODED[case["name"]] = (rows, where)
    return _DECODED[case["name"]]


_REFERENCE = {}


def reference(case, py_box_nms, setting):
    """`py_box_nms` under `setting` (keywords of SWITCHES; missing ones at their defaults) on the decoded rows, cut to the
    library's output rows: (B, R, 7) with -1 filler.  Cached per (case, setting)."""
    key = (case["name"], tuple(sorted(setting.items())))
    if key not in _REFERENCE:
        rows, where = decoded_rows(case)
        out = py_box_nms(rows, case["nms_thresh"], float(VALID), case["nms_topk"], False, drop_background=False, **setting)
        r = out_rows(case)
        want = np.full((out.shape[0], r, 7), -1.0, F32)
        n = min(r, out.shape[1])
        want[:, :n] = out[:, :n]
        want = want[where]
        want.setflags(write=False)
        _REFERENCE[key] = want
    return _REFERENCE[key]
