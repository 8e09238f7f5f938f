"""-m "not gpu": the cases of tests/entry_cases.py are sharp, and the case lists the two GPU files had before were not.

A plain numpy restatement stands in for the device, with the checks of tests/test_gpu_targets.py (`_check`, the host-mirror
comparison, the edges' direct counts) and tests/test_gpu_resize.py (recovered uint8, then the floats) applied to it.

  targets  `scatter_model`: the host mirror (videoyolo_amd/targets.py) taken apart row by row into the three phases of
           targets_scatter_kernel — the first invalid row, a slot per row, "the last row of a slot writes" — so that a bug
           can be planted in each.  Unmutated it must equal the mirror itself, bit for bit, on every case.
  resize   oracle/resize_oracle.py with the device's table capacity: area_tab cut to K_AREA_MAX entries per destination
           index, and the entry point's choice of path (entry_cases.device_mode).

Unmutated, both pass every check on every case.  Each planted bug fails at least one named case — except
`same_size_goes_through_linear`, which CANNOT fail one: OpenCV's 8-bit linear arithmetic at scale 1 is the identity on
every value (weights (2048, 0): ((2048 * ((v * 2048) >> 4)) >> 16 + 2) >> 2 == v), so routing a same-size frame through
it is not a bug but another way to copy; the test states that as what it is, for all 256 levels and on every same-size case.
Three of the bugs pass the OLD case lists (square images of at most 50 rows; area shrinks of at most x2.1): the gap was real.
"""
import numpy as np
import pytest

import entry_cases as E
from test_gpu_targets import _check

F32 = np.float32

TARGET_MUTATIONS = ["fw_and_fh_swapped", "height_and_width_swapped_at_the_call", "first_box_of_a_slot_wins",
                    "rows_from_64_on_ignored", "collision_search_stops_at_the_trip_boundary", "padding_break_per_trip",
                    "edge_centre_clamped_into_the_row", "mix_indexed_without_the_batch"]
RESIZE_MUTATIONS = ["area_table_capped_at_8", "area_left_partial_dropped", "integer_axis_takes_block_mean",
                    "same_size_goes_through_linear", "cubic_taps_not_clamped"]


# ---------------------------------------------------------------------------------------------------------------------
# targets

def scatter_model(C, H, W, gt, ids, mix=None, mut=None):
    """targets.YOLOV3PrefetchTargetGenerator(C)(H, W, gt, ids, mix) in the kernel's structure, one 64-row trip at a time."""
    from videoyolo_amd import targets as TG
    if mut == "height_and_width_swapped_at_the_call":
        H, W = W, H
    gt, ids = np.asarray(gt, F32), np.asarray(ids, F32)
    B, M = gt.shape[:2]
    N = TG.num_anchors(H, W)
    obj, ctr, scl, wts = (np.zeros((B, N, k), F32) for k in (1, 2, 2, 2))
    cls = np.full((B, N, C), -1, F32)
    fhs, fws = [H // s for s in TG.STRIDES], [W // s for s in TG.STRIDES]
    if mut == "fw_and_fh_swapped":
        fhs, fws = fws, fhs
    base = np.concatenate([[0], np.cumsum([3 * (H // s) * (W // s) for s in TG.STRIDES])])[:3]
    gw, gh = gt[..., 2] - gt[..., 0], gt[..., 3] - gt[..., 1]
    gx, gy = gt[..., 0] + gw / F32(2), gt[..., 1] + gh / F32(2)
    with np.errstate(invalid="ignore"):
        inter = np.clip(np.minimum(gw[..., None], TG.ANCHORS[:, 0]), 0, None) * np.clip(np.minimum(gh[..., None], TG.ANCHORS[:, 1]), 0, None)
        union = gw[..., None] * gh[..., None] + TG.ANCHORS[:, 0] * TG.ANCHORS[:, 1] - inter
        match = np.where(union > 0, inter / np.where(union > 0, union, 1), 0).argmax(axis=-1)
        valid = (gt >= 0).all(axis=-1)
    seen = min(M, 64) if mut == "rows_from_64_on_ignored" else M
    for b in range(B):
        # phase 1: the first invalid row
        live = np.zeros(M, bool)
        if mut == "padding_break_per_trip":
            for m0 in range(0, seen, 64):
                trip = valid[b, m0:min(m0 + 64, seen)]
                live[m0:m0 + (len(trip) if trip.all() else int(np.argmin(trip)))] = True
        else:
            live[:seen if valid[b, :seen].all() else int(np.argmin(valid[b, :seen]))] = True
        rows = np.nonzero(live)[0]
        # phase 2: a slot per row (-1: the cell lies outside its scale)
        slot = np.full(M, -1, np.int64)
        fxy = np.zeros((M, 2))
        for m in rows:
            lay = match[b, m] // 3
            fx = float(gx[b, m]) / float(W) * float(fws[lay])
            fy = float(gy[b, m]) / float(H) * float(fhs[lay])
            lx, ly = int(fx), int(fy)
            if mut == "edge_centre_clamped_into_the_row":
                lx = min(lx, fws[lay] - 1)
            cell = ly * fws[lay] + lx
            fxy[m] = fx - int(fx), fy - int(fy)
            if 0 <= cell < fhs[lay] * fws[lay]:
                slot[m] = base[lay] + cell * 3 + match[b, m] % 3
        # phase 3: of the rows of one slot one writes — the last
        writers = []
        for m in rows:
            if slot[m] < 0:
                continue
            if mut == "first_box_of_a_slot_wins":
                later = slot[rows[rows < m]]
            elif mut == "collision_search_stops_at_the_trip_boundary":
                later = slot[rows[(rows > m) & (rows < m + 64)]]
            else:
                later = slot[rows[rows > m]]
            if not (later == slot[m]).any():
                writers.append(m)
        for m in writers[::-1]:      # where a bug leaves two writers, the earlier row's values stay
            n, a = slot[m], TG.ANCHORS[match[b, m]]
            ctr[b, n] = fxy[m]
            for j, g in enumerate((gw[b, m], gh[b, m])):
                scl[b, n, j] = np.log(g / a[j]) if g >= 1 else np.log(1.0 / float(a[j]))
            wts[b, n, :] = 2.0 - float(gw[b, m] * gh[b, m]) / W / H
            obj[b, n, 0] = 1 if mix is None else mix[0 if mut == "mix_indexed_without_the_batch" else b, m, 0]
            cls[b, n, :] = 0
            cls[b, n, int(ids[b, m, 0])] = 1
    return obj, ctr, scl, wts, cls


def _mirror(C, H, W, gt, ids, mix):
    from videoyolo_amd import targets as TG
    with np.errstate(invalid="ignore"):
        return TG.YOLOV3PrefetchTargetGenerator(C)(H, W, gt, ids, mix)


def target_failures(c, mut, mixes=(True, False)):
    """The checks of test_gpu_targets.test_device_targets_match_the_cases on the model: the names of those that fail."""
    bad = []
    for with_mix in mixes:
        mix = c["mix"] if with_mix else None
        tag = "%s%s" % (c["name"], "+mix" if with_mix else "")
        try:
            got = scatter_model(c["C"], c["H"], c["W"], c["gt"], c["ids"], mix, mut)
        except (IndexError, ValueError) as e:
            bad.append("%s: %s" % (tag, type(e).__name__))
            continue
        for what, want in (("oracle", c["want"][with_mix] if "want" in c else E.reference(c["name"], with_mix)),
                           ("mirror", _mirror(c["C"], c["H"], c["W"], c["gt"], c["ids"], mix))):
            try:
                _check(got, want)
            except AssertionError:
                bad.append("%s: %s" % (tag, what))
        if "kept" in c and not ((got[0] > 0).sum() == c["kept"] == (got[4][..., 0] != -1).sum()):
            bad.append("%s: rows written" % tag)
    return bad


def _old_target_cases():
    """test_device_targets_match_the_reference_loop's three parametrisations, from the same generator"""
    from oracle import targets_oracle as T
    for size, C, B, m, pad in [(64, 3, 3, 6, 9), (416, 20, 16, 8, 12), (608, 30, 4, 40, 50)]:
        rng = np.random.default_rng(size)
        gt, ids = T.synthetic_gt(B, size, C, m=m, seed=size, pad_to=pad)
        gt[1, 2] = gt[1, 1]
        ids[1, 2] = (ids[1, 1] + 1) % C
        mix = rng.uniform(0.3, 1.0, (B, pad, 1)).astype(F32)
        want = {True: T.prefetch_targets(C, size, size, gt, ids, mix), False: T.prefetch_targets(C, size, size, gt, ids)}
        yield dict(name="old%d" % size, C=C, H=size, W=size, gt=gt, ids=ids, mix=mix, want=want)


def test_unmutated_target_model_passes_every_check():
    for name in E.TARGET_CASE_NAMES:
        c = E.target_case(name)
        assert not target_failures(c, None), name
        for mix in (c["mix"], None):   # the model IS the mirror: bit for bit, the log targets too
            got, want = scatter_model(c["C"], c["H"], c["W"], c["gt"], c["ids"], mix), _mirror(c["C"], c["H"], c["W"], c["gt"], c["ids"], mix)
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), name
    for c in _old_target_cases():
        assert not target_failures(c, None), c["name"]


@pytest.mark.parametrize("mut", TARGET_MUTATIONS)
def test_every_planted_target_bug_fails_a_case(mut):
    bad = [f for name in E.TARGET_CASE_NAMES for f in target_failures(E.target_case(name), mut)]
    assert bad, "mutation %s passed every case" % mut
    caught = {f.split(":")[0].split("+")[0] for f in bad}
    want = {"fw_and_fh_swapped": {"wide", "tall"}, "height_and_width_swapped_at_the_call": {"wide", "tall"},
            "first_box_of_a_slot_wins": {"collisions", "full"}, "rows_from_64_on_ignored": {"tall", "wide", "full"},
            "collision_search_stops_at_the_trip_boundary": {"collisions", "full"}, "padding_break_per_trip": {"late_padding"},
            "edge_centre_clamped_into_the_row": {"edges"}, "mix_indexed_without_the_batch": {"wide", "tall", "full"}}[mut]
    assert want <= caught, (mut, sorted(caught))
    print("%s: caught by %s" % (mut, ", ".join(sorted(caught))))


@pytest.mark.parametrize("mut", ["fw_and_fh_swapped", "rows_from_64_on_ignored"])
def test_old_target_cases_miss_the_bug(mut):
    """the evidence that the gap was real: square images of at most 50 rows pass with these bugs planted"""
    for c in _old_target_cases():
        assert not target_failures(c, mut), (mut, c["name"])


# ---------------------------------------------------------------------------------------------------------------------
# resize

def resize_model(frames, dst, mut=None, cap=E.K_AREA_MAX):
    """oracle.resize_oracle.inference_transform as the device runs it: the entry point's path, a table of `cap` entries"""
    from oracle import resize_oracle as R
    H, W = dst
    mode = E.device_mode(frames.shape[1:3], dst)
    assert mode is not None
    cap = 8 if mut == "area_table_capped_at_8" else cap
    orig_area, orig_cubic = R.area_tab, R._cubic_tab

    def area_tab(ssize, dsize):
        scale = float(ssize) / float(dsize)
        out, count = [], {}
        for di, si, alpha in orig_area(ssize, dsize):
            if mut == "area_left_partial_dropped" and di not in count:
                s1 = min(int(np.ceil(di * scale)), min(int(np.floor(di * scale + scale)), ssize - 1))
                count[di] = 0
                if s1 - di * scale > 1e-3 and si == s1 - 1:
                    continue
            count[di] = count.get(di, 0) + 1
            if count[di] <= cap:
                out.append((di, si, alpha))
        return out

    def cubic_tab(dsize, ssize):
        idx, w = orig_cubic(dsize, ssize)
        s, _ = R._src_coord(dsize, ssize)
        return (s[:, None] + np.arange(-1, 3)[None, :]) % ssize, w

    def one(img):
        if mode == 0:
            return R.resize_linear(img, H, W) if mut == "same_size_goes_through_linear" else img.copy()
        if mode in (3, 4):
            h, w = img.shape[:2]
            if mut == "integer_axis_takes_block_mean" and mode == 3:
                if w % W == 0:
                    img = R.resize_area(img, h, W)
                if h % H == 0:
                    img = R.resize_area(img, H, img.shape[1])
            return R.resize_area(img, H, W) if img.shape[:2] != (H, W) else img
        return {1: R.resize_linear, 2: R.resize_cubic}[mode](img, H, W)

    R.area_tab = area_tab
    if mut == "cubic_taps_not_clamped":
        R._cubic_tab = cubic_tab
    try:
        out = np.stack([one(f) for f in frames])
    finally:
        R.area_tab, R._cubic_tab = orig_area, orig_cubic
    x = (out.astype(F32) / F32(255.0) - R.MEAN) / R.STD
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2)), out


def resize_failures(case, mut, kinds=("smooth", "noise"), frames=None):
    """The assertions of test_resize_normalize_matches_the_restated_transform on the model."""
    from oracle import resize_oracle as R
    name, src, dst = case[:3]
    bad = []
    for kind in kinds:
        f = E.resize_frames(case, kind) if frames is None else frames
        got, _ = resize_model(f, dst, mut)
        want, resized = R.inference_transform(f, dst[1], dst[0])
        back = np.rint((got.transpose(0, 2, 3, 1) * R.STD + R.MEAN) * 255.0).astype(np.int64)
        if np.abs(back - resized.astype(np.int64)).max() != 0 or not np.array_equal(got, want):
            bad.append("%s (%s)" % (name, kind))
    return bad


ALL_RESIZE = E.RESIZE_CASES + [E.INTEGER_11]


def _old_resize_cases():
    """test_gpu_resize.CASES with their frames (the smooth generator, seed = len(name))"""
    import test_gpu_resize as G
    for name, src, dst in G.CASES:
        yield (name, src, dst), E.smooth_frames(*src, seed=len(name))


def test_unmutated_resize_model_passes_every_check():
    for case in ALL_RESIZE:
        assert not resize_failures(case, None), case[0]


@pytest.mark.parametrize("mut", RESIZE_MUTATIONS)
def test_every_planted_resize_bug_fails_a_case(mut):
    from oracle import resize_oracle as R
    bad = [f for case in ALL_RESIZE for f in resize_failures(case, mut)]
    if mut == "same_size_goes_through_linear":
        # not a bug: the 8-bit linear arithmetic at scale 1 is the identity (module docstring), on every level and position
        levels = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
        assert np.array_equal(R.resize_linear(levels, 16, 16), levels) and np.array_equal(R.resize_linear(levels[:1, :3], 1, 3), levels[:1, :3])
        assert not bad
        print("%s: equals the copy on all 256 levels: no case can fail, and none does" % mut)
        return
    assert bad, "mutation %s passed every case" % mut
    want = {"area_table_capped_at_8": "area x9.9 by x6.1", "area_left_partial_dropped": "area x1.9 odd source",
            "integer_axis_takes_block_mean": "area integer x fractional y", "cubic_taps_not_clamped": "cubic from 2 rows"}[mut]
    assert any(f.startswith(want) for f in bad), (mut, bad)
    print("%s: caught by %s" % (mut, ", ".join(bad)))


def test_old_resize_cases_miss_the_capped_table():
    """the evidence that the gap was real: no old case has a cell of more than 8 entries (at most x2.1: 4)"""
    for case, frames in _old_resize_cases():
        assert not resize_failures(case, "area_table_capped_at_8", kinds=("smooth",), frames=frames), case[0]
        assert not resize_failures(case, None, kinds=("smooth",), frames=frames), case[0]
