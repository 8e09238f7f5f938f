"""Constructed inputs of the two entry kernels' tests: csrc/targets.hip (tests/test_gpu_targets.py) and csrc/preproc.hip
(tests/test_gpu_resize.py) on the device, and the same inputs on the CPU in tests/test_entry_cases_sensitivity.py, which
shows with planted bugs that the cases are sharp.  Pure numpy; nothing here needs a GPU.

Target cases are dicts ``name, C, H, W, gt (B,M,4), ids (B,M,1), mix (B,M,1)``; ``oracle_rows`` (edges only) lists the gt
rows the reference loop can take without an IndexError of its own, and ``kept`` the number of slots it then writes.
Every builder asserts on the ORACLE's output the property its case exists for, so a case that stops exercising its edge
fails loudly instead of passing vacuously:

  wide          64 x 160, M = 150 padded to 160: three trips of the 64-row loops, H != W
  tall          160 x 64, M = 65 unpadded: one row beyond one trip
                (both: the call with height and width exchanged gives other tensors, or raises)
  full          96 x 32, M = 1000 padded to 1024, the LDS limit: most rows lose their slot to a later one
  collisions    64 x 96, M = 140: rows 3, 67, 131 are one box with three classes and ratios (a chain over three trips: 131
                wins every field), rows 10, 11 an adjacent pair, rows 20, 100 one centre with two sizes (two anchors: both stay)
  late_padding  M = 200: the first -1 row at 64 / at 129 / at 0, valid-looking rows behind it that must not be written
  edges         64 x 64: a centre at x == W (the cell index wraps into the next row, as in the reference), at y == H (the
                index leaves the scale: dropped), a wrapped cell that is the scale's last cell plus one (dropped), the same
                on the stride-8 scale (the reference's own IndexError: not given to the oracle), a NaN coordinate (padding)

Resize cases are ``(name, src (B,h,w), dst (H,W), mode, entries)``: mode as the entry point picks it (0 same size = copy,
1 linear, 2 cubic, 3 area by table, 4 area by integer block means), entries the largest number of table entries of one
destination cell per axis (x, y) from resize_oracle.area_tab (None outside mode 3); both are asserted here.
"""
import functools

import numpy as np

F32 = np.float32
K_AREA_MAX = 12   # csrc/preproc.hip kAreaMax: table entries of one destination cell per axis
K_MAX_GT = 1024   # csrc/targets.hip kMaxGt: gt rows per image staged in LDS


# ---------------------------------------------------------------------------------------------------------------------
# targets

def boxes(rng, n, H, W):
    """n boxes with centres uniform over the H x W image, sides ~ U(min/8, min/1.5), clipped inside it (no edge centre)."""
    side = min(H, W)
    c = rng.uniform(0, (W, H), (n, 2))
    wh = rng.uniform(side / 8, side / 1.5, (n, 2))
    x1y1 = np.clip(c - wh / 2, 0, (W - 2, H - 2))
    x2y2 = np.clip(c + wh / 2, x1y1 + 1, (W - 1, H - 1))
    return np.concatenate([x1y1, x2y2], 1).astype(F32)


def _random_case(name, C, H, W, B, m, pad_to, seed):
    rng = np.random.default_rng(seed)
    gt = np.full((B, pad_to, 4), -1, F32)
    ids = np.full((B, pad_to, 1), -1, F32)
    for b in range(B):
        gt[b, :m] = boxes(rng, m, H, W)
        ids[b, :m, 0] = rng.integers(0, C, m)
    mix = rng.uniform(0.3, 1.0, (B, pad_to, 1)).astype(F32)
    return dict(name=name, C=C, H=H, W=W, gt=gt, ids=ids, mix=mix)


def _oracle(c, gt=None, ids=None, mix=None, H=None, W=None):
    from oracle import targets_oracle as T
    with np.errstate(invalid="ignore"):  # the NaN row of `edges` goes through the IoU table before the loop breaks at it
        return T.prefetch_targets(c["C"], H or c["H"], W or c["W"], c["gt"] if gt is None else gt,
                                  c["ids"] if ids is None else ids, mix)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _transposed_call_differs(c):
    try:
        other = _oracle(c, mix=c["mix"], H=c["W"], W=c["H"])
    except IndexError:
        return True
    return not _same(other, _oracle(c, mix=c["mix"]))


def _slot_of(c, box):
    """the one row of N the reference writes for `box` alone"""
    obj = _oracle(c, np.asarray(box, F32).reshape(1, 1, 4), np.zeros((1, 1, 1), F32))[0]
    (n,) = np.nonzero(obj[0, :, 0])[0]
    return int(n)


def _wide():
    c = _random_case("wide", 5, 64, 160, 2, 150, 160, seed=1)
    assert _transposed_call_differs(c)
    return c


def _tall():
    c = _random_case("tall", 5, 160, 64, 2, 65, 65, seed=2)
    assert _transposed_call_differs(c)
    # row 64, the one row of the second trip, is seen: without it the tensors differ
    assert not _same(_oracle(c), _oracle(c, c["gt"][:, :64], c["ids"][:, :64]))
    return c


def _full():
    c = _random_case("full", 4, 96, 32, 2, 1000, K_MAX_GT, seed=3)
    kept = int((_oracle(c)[0] > 0).sum())
    assert 100 < kept < 1000, kept          # of 2000 rows: fewer than half keep their slot, and more than 100 do
    return c


def _collisions():
    c = _random_case("collisions", 6, 64, 96, 1, 140, 140, seed=4)
    gt, ids, mix = c["gt"], c["ids"], c["mix"]
    chain = [70.0, 20.0, 80.0, 33.0]        # 10 x 13: the first stride-8 anchor
    for k, m in enumerate((3, 67, 131)):
        gt[0, m], ids[0, m, 0], mix[0, m, 0] = chain, k, (0.4, 0.6, 0.8)[k]
    gt[0, 10] = gt[0, 11] = [10.0, 40.0, 26.0, 56.0]
    ids[0, 10], ids[0, 11] = 4, 5
    gt[0, 20], gt[0, 100] = [40.0, 8.0, 50.0, 21.0], [37.0, 0.0, 53.0, 29.0]    # centre (45, 14.5): 10 x 13 and 16 x 29
    ids[0, 20], ids[0, 100] = 3, 4
    obj, _, _, _, cls = _oracle(c, mix=mix)
    n = _slot_of(c, chain)
    assert obj[0, n, 0] == mix[0, 131, 0] and list(cls[0, n]) == [0, 0, 1, 0, 0, 0], "row 131 must win the chained slot"
    n = _slot_of(c, gt[0, 11])
    assert obj[0, n, 0] == mix[0, 11, 0] and cls[0, n, 5] == 1
    n20, n100 = _slot_of(c, gt[0, 20]), _slot_of(c, gt[0, 100])
    assert n20 != n100 and n20 // 3 == n100 // 3, (n20, n100)      # one cell, two anchor slots
    assert obj[0, n20, 0] == mix[0, 20, 0] and obj[0, n100, 0] == mix[0, 100, 0], "rows 20 and 100 must both survive"
    return c


def _late_padding():
    c = _random_case("late_padding", 5, 96, 64, 3, 200, 200, seed=5)
    first = (64, 129, 0)
    blanked = c["gt"].copy()
    closed = c["gt"].copy()
    for b, m in enumerate(first):
        c["gt"][b, m] = blanked[b, m] = -1          # ids keep their class: the rows behind look valid
        blanked[b, m:] = -1
        closed[b, m] = closed[b, m - 1]
    want = _oracle(c, mix=c["mix"])
    assert _same(want, _oracle(c, blanked, mix=c["mix"])), "rows behind the first padded row must not be written"
    assert not _same(want, _oracle(c, closed, mix=c["mix"])), "the rows behind the padding would change the tensors"
    assert want[0][2].sum() == 0 and (want[4][2] == -1).all()
    return c


def _edges():
    nan = float("nan")
    rows = [
        ([8, 8, 40, 24], 0),           # 0 ordinary
        ([64, 10, 64, 12], 1),         # 1 centre at x == W: stride-32 cell (y 0, x 2) wraps to (y 1, x 0); written
        ([40, 64, 42, 64], 2),         # 2 centre at y == H: cell (y 2, x 1) lies behind the stride-32 scale; dropped
        ([64, 40, 64, 50], 3),         # 3 x == W in the last row: the wrapped cell is the scale's last cell plus one; dropped
        ([59, 53.5, 69, 66.5], 4),     # 4 the same on the stride-8 scale (10 x 13): the reference indexes past its tensors
        ([20, 30, 50, 60], 5),         # 5 ordinary
        ([5, nan, 20, 20], 2),         # 6 a NaN coordinate is not >= 0: padding, the loop ends here
        ([30, 30, 40, 40], 3),         # 7 looks valid, lies behind the padding
    ]
    gt = np.array([[r[0] for r in rows]], F32)
    ids = np.array([[[r[1]] for r in rows]], F32)
    mix = np.linspace(0.35, 0.95, len(rows), dtype=F32).reshape(1, -1, 1)
    c = dict(name="edges", C=6, H=64, W=64, gt=gt, ids=ids, mix=mix, oracle_rows=[0, 1, 2, 3, 5, 6, 7], kept=3)
    try:
        _oracle(c, mix=mix)
        raise AssertionError("row 4 no longer leaves the reference's tensors")
    except IndexError:
        pass
    obj, _, _, _, cls = compute_reference(c, True)
    written = np.nonzero(obj[0, :, 0])[0]
    assert len(written) == c["kept"] and (cls[0, :, 0] != -1).sum() == c["kept"]
    wrapped = (1 * 2 + 0) * 3 + 0       # stride 32 is first in N: cell (y 1, x 0), anchor slot 0
    assert obj[0, wrapped, 0] == mix[0, 1, 0] and cls[0, wrapped, 1] == 1, "the x == W row must wrap into the next row"
    return c


_BUILDERS = dict(wide=_wide, tall=_tall, full=_full, collisions=_collisions, late_padding=_late_padding, edges=_edges)
TARGET_CASE_NAMES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def target_case(name):
    return _BUILDERS[name]()


def compute_reference(c, with_mix):
    """The oracle's five tensors of a case, from the rows the reference loop can take."""
    rows = c.get("oracle_rows")
    gt, ids, mix = (c["gt"], c["ids"], c["mix"]) if rows is None else (c["gt"][:, rows], c["ids"][:, rows], c["mix"][:, rows])
    return _oracle(c, gt, ids, mix if with_mix else None)


@functools.lru_cache(maxsize=None)
def reference(name, with_mix):
    """compute_reference of a named case, computed once per (case, mix setting); treat as read-only"""
    return compute_reference(target_case(name), with_mix)


def limit_case(m):
    """m unpadded rows in one 64 x 64 image: m = K_MAX_GT runs, one more is refused"""
    return _random_case("limit%d" % m, 3, 64, 64, 1, m, m, seed=6)


# ---------------------------------------------------------------------------------------------------------------------
# resize

def smooth_frames(b, h, w, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 127 + 100 * np.sin(x / 7.0)[..., None] * np.cos(y / 5.0)[..., None] * np.array([1, 0.5, -1])
    return np.clip(base[None] + rng.normal(0, 25, (b, h, w, 3)), 0, 255).astype(np.uint8)


def noise_frames(b, h, w, seed):
    """full-range uniform noise: neighbouring pixels are unrelated, so one dropped or misplaced tap moves the result"""
    return np.random.default_rng(seed).integers(0, 256, (b, h, w, 3), dtype=np.uint8)


FRAME_KINDS = dict(smooth=smooth_frames, noise=noise_frames)


def device_mode(src_hw, dst_hw):
    """The path vy_preprocess_resize_frames takes: 0 same size (copy), 1 linear, 2 cubic, 3 area by table, 4 area by
    integer block means; None where it refuses (a fractional area factor above K_AREA_MAX - 2 on either axis)."""
    (h, w), (H, W) = src_hw, dst_hw
    if (h, w) == (H, W):
        return 0
    if H > h and W > w:
        return 2
    if H < h and W < w:
        sx, sy = float(w) / W, float(h) / H
        eps = np.finfo(np.float64).eps
        if abs(sx - round(sx)) < eps and abs(sy - round(sy)) < eps:
            return 4
        return None if sx > K_AREA_MAX - 2 or sy > K_AREA_MAX - 2 else 3
    return 1


def area_entries(ssize, dsize):
    """the largest number of table entries of one destination index (resize_oracle.area_tab)"""
    from oracle import resize_oracle as R
    return int(np.bincount([di for di, _, _ in R.area_tab(ssize, dsize)]).max())


RESIZE_CASES = [
    ("area x9.9 by x6.1", (1, 97, 395), (16, 40), 3, (11, 7)),
    ("area factor exactly 10 on x", (1, 159, 400), (16, 40), 3, (10, 11)),
    ("area integer x fractional y", (2, 100, 96), (40, 32), 3, (3, 3)),
    ("area fractional x integer y", (1, 96, 100), (32, 40), 3, (3, 3)),
    ("area integer 16 by 2", (1, 512, 96), (32, 48), 4, None),
    ("area x1.9 odd source", (1, 61, 65), (32, 33), 3, (3, 3)),
    ("cubic from 1x1", (1, 1, 1), (4, 4), 2, None),
    ("cubic from 2 rows", (2, 2, 300), (5, 301), 2, None),
    ("linear tiny", (1, 3, 300), (5, 7), 1, None),
    ("same size 75x93", (2, 75, 93), (75, 93), 0, None),
    ("same size 1x3", (1, 1, 3), (1, 3), 0, None),
    ("same size 7x9", (3, 7, 9), (7, 9), 0, None),
    ("same size 6x10", (2, 6, 10), (6, 10), 0, None),
]
# next to the acceptance bound (sx > K_AREA_MAX - 2 is refused unless both factors are integers)
REFUSED = ("area x10.075 on x", (1, 161, 403), (16, 40))
ACCEPTED_AT_THE_BOUND = RESIZE_CASES[1]
INTEGER_11 = ("area integer 11 by 11", (1, 176, 440), (16, 40), 4, None)

for _name, _src, _dst, _mode, _entries in RESIZE_CASES + [INTEGER_11]:
    assert device_mode(_src[1:], _dst) == _mode, (_name, device_mode(_src[1:], _dst))
    if _mode == 3:
        _got = (area_entries(_src[2], _dst[1]), area_entries(_src[1], _dst[0]))
        assert _got == _entries and max(_got) <= K_AREA_MAX, (_name, _got)
    if _mode == 0:
        assert (_src[1] * _src[2] % 4 != 0) or _src[2] % 4 != 0, _name   # what the 4-pixel kernel's tests never had
assert device_mode(REFUSED[1][1:], REFUSED[2]) is None
assert max(area_entries(395, 40), area_entries(159, 16)) == 11


def resize_frames(case, kind):
    name, src = case[0], case[1]
    return FRAME_KINDS[kind](*src, seed=len(name))
