"""A plain numpy model of the per-frame mAP kernel (csrc/voc_metric.hip, frame_ap_kernel), row by row as the kernel walks
them: no sort, a row's rank is a count.  Shared by tests/test_frame_map_host.py and tests/test_gpu_frame_map.py, with
switches for planted bugs (BUGS): each must make at least one test case fail.

    frame_score(labels, scores, flags, gt_labels, gt_difficults, use_07) -> (score, classes averaged)

labels / scores / flags: the frame's R rows as vy_voc_match takes and gives them; gt_labels: the M ground-truth labels
ALREADY class-mapped, < 0 = skip; gt_difficults: M values or None."""
import numpy as np

BUGS = ("ties_higher_row_first", "ignored_as_fp", "envelope_from_left", "skip_detectionless", "gtless_as_zero",
        "padding_ranked", "thresholds_k_over_10", "difficult_in_npos", "one_over_npos")
LANES = 256


def frame_terms(labels, scores, flags, gt_labels, gt_difficults=None, use_07=False, bug=None):
    """(terms, classes): the contribution of every row to the frame's sum of class APs, (R,) float64 in row order, and the
    number of classes averaged."""
    assert bug is None or bug in BUGS
    labels = np.asarray(labels, np.float32).reshape(-1)
    scores = np.asarray(scores, np.float32).reshape(-1)
    flags = np.asarray(flags).reshape(-1).astype(np.int64)
    gl = np.asarray(gt_labels).reshape(-1).astype(np.int64)
    gd = np.zeros(len(gl), bool) if gt_difficults is None else np.asarray(gt_difficults).reshape(-1) != 0
    if bug == "difficult_in_npos":
        gd = np.zeros(len(gl), bool)
    rows = len(labels)
    cls = np.where(labels >= 0, labels, -1).astype(np.int64)
    if bug == "padding_ranked":                        # a padding row taken for a false positive of class 0
        flags = np.where(cls < 0, 0, flags)
        cls = np.maximum(cls, 0)
    counted = gl[(gl >= 0) & ~gd]
    scored = set(counted.tolist())
    n_classes = len(scored)
    if bug == "skip_detectionless":
        n_classes = len(scored & set(cls[cls >= 0].tolist()))
    if bug == "gtless_as_zero":
        n_classes = len(scored | set(cls[cls >= 0].tolist()))
    idx = np.arange(rows)
    tp, npos, lead = np.zeros(rows, np.int64), np.zeros(rows, np.int64), np.zeros(rows, bool)
    prec, rec = np.zeros(rows), np.zeros(rows)
    ahead_of, behind_of = [None] * rows, [None] * rows
    for r in range(rows):
        if cls[r] < 0:
            continue
        same, tie = cls == cls[r], scores == scores[r]
        if bug == "ties_higher_row_first":
            ahead = same & ((scores > scores[r]) | (tie & (idx >= r)))
            behind = same & ((scores < scores[r]) | (tie & (idx <= r)))
        else:
            ahead = same & ((scores > scores[r]) | (tie & (idx <= r)))
            behind = same & ((scores < scores[r]) | (tie & (idx >= r)))
        ahead_of[r], behind_of[r] = ahead, behind
        tp[r] = int((flags[ahead] == 1).sum())
        fp = int((flags[ahead] == 0).sum()) + (int((flags[ahead] == -1).sum()) if bug == "ignored_as_fp" else 0)
        npos[r] = int((counted == cls[r]).sum())
        lead[r] = int(ahead.sum()) == 1
        prec[r] = np.float64(tp[r]) / np.float64(tp[r] + fp) if tp[r] + fp > 0 else 0.0
        rec[r] = np.float64(tp[r]) / np.float64(npos[r]) if npos[r] > 0 else 0.0
    terms = np.zeros(rows)
    for r in range(rows):
        if cls[r] < 0 or npos[r] <= 0:
            continue
        if not use_07:
            if flags[r] != 1:
                continue
            top = max(0.0, prec[ahead_of[r] if bug == "envelope_from_left" else behind_of[r]].max())
            n = np.float64(npos[r])
            step = np.float64(1.0) / n if bug == "one_over_npos" else np.float64(tp[r]) / n - np.float64(tp[r] - 1) / n
            terms[r] = step * top
        elif lead[r]:
            mine = cls == cls[r]
            ap = np.float64(0.0)
            for k in range(11):
                t = np.float64(k) / 10.0 if bug == "thresholds_k_over_10" else 0.0 + np.float64(k) * 0.1
                hit = mine & (rec >= t)
                ap = ap + (prec[hit].max() if hit.any() else 0.0) / 11.0
            terms[r] = ap
    return terms, n_classes


def fixed_order_sum(terms):
    """The kernel's order: lane t adds rows t, t + 256, ...; then a tree over the 256 lanes."""
    lane = np.zeros(LANES)
    for k in range(0, len(terms), LANES):
        part = terms[k:k + LANES]
        lane[:len(part)] = lane[:len(part)] + part
    half = LANES // 2
    while half:
        lane[:half] = lane[:half] + lane[half:2 * half]
        half //= 2
    return lane[0]


def frame_score(labels, scores, flags, gt_labels, gt_difficults=None, use_07=False, bug=None):
    terms, n = frame_terms(labels, scores, flags, gt_labels, gt_difficults, use_07, bug)
    return (fixed_order_sum(terms) / np.float64(n) if n > 0 else np.float64("nan")), n


def batch_scores(labels, scores, flags, gt_labels, gt_difficults=None, use_07=False, bug=None):
    """frame_score over a batch: (B,) float64 scores and (B,) int classes.  gt_labels (B, M) mapped."""
    out = [frame_score(labels[b], scores[b], flags[b], gt_labels[b], None if gt_difficults is None else gt_difficults[b],
                       use_07, bug) for b in range(len(labels))]
    return np.array([o[0] for o in out], np.float64), np.array([o[1] for o in out], np.int64)
