"""Constructed inputs of the loss-kernel tests (tests/test_gpu_loss_cells.py on the device, and the same construction on
the CPU oracle in tests/test_train_cells64_sensitivity.py, which settles the census conditions before any GPU run).

The vehicle is the heads net on random-normal routes.  A case is built in two passes.  Pass 1 is a train-mode forward:
it gives the decoded boxes and the raw predictions.  Pass 2 constructs, from those boxes, the gt_boxes of the recorded
step — they feed only the dynamic ignore mask and are independent of the prefetched targets — and edits the prefetched
targets:

  ignore decision   for chosen non-positive anchors with a finite box of at least MIN_SIDE pixels a side and an
                    unsaturated objectness logit, a concentric copy of the anchor's own predicted box scaled by sqrt(r)
                    per side is one gt row, so its IoU with that anchor is r: r = thresh + 1e-3 ("above"),
                    thresh - 1e-3 ("below") and the box itself (r = 1, "one"), in turn
  mixup             obj_t of every other positive is drawn from (0.3, 1), as gt_mixratio makes it
  d == 0            scales_t of the first two positives of the batch are the device's own raw rw / rh bits
  saturated logits  come through the prediction biases (saturate): per (scale, anchor slot) the objectness and two class
                    channels at +-20, +-40, +-90, +-100, one slot's rw at 90 (exp overflows: an infinite box), one at -100
                    (a zero-area box); (stride 8, slot 2) is left as it is
"""
import functools

import numpy as np

F32 = np.float32
MIN_SIDE = 2.0     # pixels: a box this large has its IoU with a scaled copy within 1e-5 of r in fp32
OBJ_UNSAT = 30.0   # |objectness logit| below this: sigmoid is a nonzero fp32, so a negative's dpred[4] is nonzero
DELTA = 1e-3       # r = thresh +- DELTA: 1000 x `near`, far inside any sloppy compare
KINDS = ("above", "below", "one")

# (scale index 0..2 = stride 32, 16, 8; anchor slot) -> {channel: bias}; channels: 2 = rw, 4 = objectness, 5 / 6 = the
# first two classes (a one-class net has only 5)
SATURATE = {
    (0, 0): {4: 20.0, 5: -20.0, 6: 40.0},
    (0, 1): {4: -20.0, 5: 20.0, 6: -40.0},
    (0, 2): {4: 40.0, 5: -90.0, 6: 90.0},
    (1, 0): {4: -40.0, 5: 100.0, 6: -100.0},
    (1, 1): {4: 90.0, 2: 90.0},
    (1, 2): {4: -90.0, 2: -100.0},
    (2, 0): {4: 100.0, 5: 40.0, 6: -20.0},
    (2, 1): {4: -100.0, 5: -40.0, 6: 20.0},
}

# classes, label smoothing, ignore threshold, gt rows M, valid gt rows per image, batch, height, width, seed.
# C = 80 takes the 1/C side of the smoothing constant, C = 1 and 20 the 1/40 side; 64x64 is N = 252 (one block with a
# tail), 96x32 N = 189, 128x128 N = 1008 (four blocks, tail 240); B = 17 puts loss_reduce_kernel into a second block
CASES = [
    dict(C=1, smooth=False, thresh=0.7, M=1, valid=1, B=17, H=64, W=64, seed=1),
    dict(C=1, smooth=True, thresh=0.7, M=100, valid=40, B=3, H=96, W=32, seed=2),
    dict(C=20, smooth=False, thresh=0.5, M=100, valid=40, B=1, H=128, W=128, seed=3),
    dict(C=20, smooth=True, thresh=0.7, M=4, valid=3, B=17, H=96, W=32, seed=4),
    dict(C=80, smooth=False, thresh=0.7, M=100, valid=40, B=3, H=64, W=64, seed=5),
    dict(C=80, smooth=True, thresh=0.7, M=4, valid=3, B=17, H=128, W=128, seed=6),
]
# the launcher's own cap on the gt rows (vy_launch_loss, include/vyolo.h); the last row is a valid box, so that a launch
# that staged fewer rows than M decides its anchor differently
M_CAP = 4096
CAP_CASE = dict(C=20, smooth=False, thresh=0.7, M=M_CAP, valid=40, B=1, H=64, W=64, seed=7, last_row=True)


def case_id(c):
    return "C%d-%s-t%g-M%d-B%d-%dx%d" % (c["C"], "smooth" if c["smooth"] else "plain", c["thresh"], c["M"], c["B"], c["H"],
                                         c["W"])


@functools.lru_cache(maxsize=4)
def _base_params(C, seed):
    from videoyolo_amd import init
    from oracle import yolo3_oracle as O
    table = [(n, s) for n, s in O.param_shapes(C) if not n.startswith("stages.")]
    return init.synthetic_params(table, seed=seed)


def saturate(params, C):
    """a copy of `params` with SATURATE's values in the three prediction biases"""
    out = dict(params)
    for i in range(3):
        name = "yolo_outputs.%d.prediction.bias" % i
        b = out[name].copy().reshape(3, 5 + C)
        for (s, slot), chans in SATURATE.items():
            if s == i:
                for ch, v in chans.items():
                    if ch < 5 + C:
                        b[slot, ch] = v
        out[name] = b.reshape(-1)
    return out


def heads_params(C, seed=233, saturated=True):
    p = _base_params(C, seed)
    return saturate(p, C) if saturated else dict(p)


def routes(B, H, W, seed):
    """random-normal routes of a (B, 3, H, W) batch: strides 8, 16, 32"""
    rng = np.random.default_rng(1000 + seed)
    return [rng.standard_normal((B, ch, H // s, W // s)).astype(F32) for ch, s in ((256, 8), (512, 16), (1024, 32))]


def oracle_heads_forward(C, params, rts):
    """the heads' train-mode forward (batch statistics) on the CPU oracle: the three prediction planes, strides 32, 16, 8"""
    from oracle import yolo3_oracle as O
    from oracle import yolo3_train_oracle as TO
    orc = TO.OracleYolo3Train(C, dict(params))
    preds, x = [], rts[2]
    for i in range(3):
        for j in range(5):
            x = orc.cell(x, "yolo_blocks.%d.body.%d" % (i, j), 1 if j % 2 == 0 else 3, 1)
        route = x
        tip = orc.cell(route, "yolo_blocks.%d.tip" % i, 3, 1)
        preds.append(O.conv2d(tip, params["yolo_outputs.%d.prediction.weight" % i], 1, 0, None,
                              params["yolo_outputs.%d.prediction.bias" % i]))
        if i == 2:
            break
        t = orc.cell(route, "transitions.%d" % i, 1, 1)
        x = np.concatenate([t.repeat(2, axis=-1).repeat(2, axis=-2), rts[1 - i]], axis=1)
    return preds


def prefetched(case):
    """the prefetched targets of the case, from a gt list of their own (12 boxes an image)"""
    from oracle import targets_oracle as T
    boxes, ids = T.synthetic_gt(case["B"], min(case["H"], case["W"]), case["C"], m=12, seed=case["seed"])
    return [np.array(t) for t in T.prefetch_targets(case["C"], case["H"], case["W"], boxes, ids)]


def construct(case, box, scales_raw, obj_raw):
    """Pass 2: (gt_boxes (B, M, 4), the five edited targets, constructed [(b, n, kind, gt row)]) from pass 1's decoded
    boxes (B, N, 4), raw scale predictions (B, N, 2) and raw objectness (B, N, 1)."""
    B, M, thresh = case["B"], case["M"], case["thresh"]
    rng = np.random.default_rng(2000 + case["seed"])
    box = np.asarray(box, F32)
    tg = prefetched(case)
    obj_t, scales_t = tg[0], tg[2]
    pos = obj_t[..., 0] > 0
    # mixup: every other positive, in (b, n) order
    pb, pn = np.nonzero(pos)
    for b, n in list(zip(pb, pn))[1::2]:
        obj_t[b, n, 0] = F32(rng.uniform(0.3, 1.0))
    # d == 0: the first two positives' scale targets are the raw predictions themselves
    for b, n in list(zip(pb, pn))[:2]:
        scales_t[b, n] = np.asarray(scales_raw, F32)[b, n]
    # the ignore decision
    side_x, side_y = box[..., 2] - box[..., 0], box[..., 3] - box[..., 1]
    with np.errstate(invalid="ignore"):
        ok = (~pos & np.isfinite(box).all(-1) & (side_x >= MIN_SIDE) & (side_y >= MIN_SIDE)
              & (np.abs(np.asarray(obj_raw, F32)[..., 0]) < OBJ_UNSAT))
    gt = np.full((B, M, 4), -1.0, F32)
    made, turn = [], 0
    for b in range(B):
        cand = np.nonzero(ok[b])[0]
        rows = list(range(case["valid"])) + ([M - 1] if case.get("last_row") else [])
        picks = rng.choice(cand, size=len(rows), replace=False)
        for m, n in zip(rows, picks):
            kind = "one" if (case.get("last_row") and m == M - 1) else KINDS[turn % 3]
            turn += 1
            if kind == "one":
                gt[b, m] = box[b, n]
            else:
                r = thresh + DELTA if kind == "above" else thresh - DELTA
                x1, y1, x2, y2 = box[b, n].astype(np.float64)
                cx, cy, hx, hy = (x1 + x2) / 2, (y1 + y2) / 2, (x2 - x1) / 2 * np.sqrt(r), (y2 - y1) / 2 * np.sqrt(r)
                gt[b, m] = [cx - hx, cy - hy, cx + hx, cy + hy]
            made.append((b, int(n), kind, m))
    return gt, tg, made


def conditions(case, terms, made):
    """The census conditions of a constructed case (chosen seeds make them hold; they are asserted, not measured):
    at least 8 anchors each positive, ignored and plain negative, at least 4 fractional positives, at most 2 exempt
    anchors, and at least 4 constructed anchors on each side of the threshold (and one r = 1 copy) decided as constructed.
    Returns the census with the constructed counts added."""
    from oracle import train_cells64 as R
    census = R.loss_census(terms)
    want = {"above": -1, "one": -1, "below": 0}
    for kind in KINDS:
        census["as constructed, " + kind] = sum(1 for b, n, k, _ in made if k == kind and terms["decision"][b, n] == want[k])
        census["constructed, " + kind] = sum(1 for _, _, k, _ in made if k == kind)
    assert min(census["positive"], census["ignored"], census["negative"]) >= 8, census
    assert census["fractional"] >= 4 and census["exempt"] <= 2, census
    assert census["as constructed, above"] >= 4 and census["as constructed, below"] >= 4, census
    assert census["as constructed, one"] >= 1, census
    return census
