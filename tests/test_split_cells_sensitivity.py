"""CPU: would the per-cell checks of the split-fp32 kernels (oracle/split_oracle.py: check_split) notice a wrong kernel?

tests/test_gpu_split_cells.py holds every launch of conv_split.hip, conv_wino.hip and wgrad_split.hip to three
conditions: (a) the hard rounding bound, (b) the product census |beta_p| <= 0.25, (c) the typical-rounding bar
T 2^-24 absum.  Here numpy fp32 mocks of the four accumulations (forward direct, forward Winograd, data gradient,
weight gradient; 16-term groups, the six products smallest first, k-split slabs added in order) stand in for the
device: the checker must accept every faithful mock and reject every mock with a fault injected, and each fault names
the condition that catches it:

  fault                                                      caught by
  one of the six products dropped (each of the six)          (b) always; (c) too from m h / h m up, (a) for h h
  one product doubled                                        (b)
  h m computed in place of m h                               (b): beta(m h) = -1 and beta(h m) = +1
  data-gradient taps not flipped                             (a), (c)
  two stride-2 parity classes swapped                        (a), (c)
  the last pixel row of the last tile left at zero           (a), (c)
  a zero-padded channel of the dz operand holding garbage    (a), (c)  (garbage that is not finite fails outright)
  Winograd U1 / U2 swapped                                   (a), (c)
  Winograd's lone last pixel taken from the second slot      (a), (c)
  a x2-replicated store written past the cropped size        the border check, and (a) at the consumer

Also here: the restatement of conv_wino.hip without the cut equals the direct float64 conv to 1e-12 (the conditioning of
the float64 transform, not a kernel tolerance), and T is re-measured and held over both mocks."""
import numpy as np
import pytest

from oracle import split_oracle as S
from oracle import train_cells64 as R

F32 = np.float32


def _leaky(v):
    return np.maximum(v, F32(0.1) * v)


def _im2col(x, k, stride, pad):
    """(B,C,H,W) -> (B*Ho*Wo, k*k*C), k order (tap, channel) as the kernels walk it"""
    B, C, H, W = x.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xp = np.zeros((B, C, H + 2 * pad, W + 2 * pad), x.dtype)
    xp[:, :, pad:pad + H, pad:pad + W] = x
    cols = [xp[:, :, kh:kh + stride * Ho:stride, kw:kw + stride * Wo:stride] for kh in range(k) for kw in range(k)]
    p = np.stack(cols, 1)  # (B, taps, C, Ho, Wo)
    return np.ascontiguousarray(p.transpose(0, 3, 4, 1, 2).reshape(B * Ho * Wo, k * k * C)), (B, Ho, Wo)


def _wmat(w):
    O, C, k, _ = w.shape
    return np.ascontiguousarray(w.transpose(0, 2, 3, 1).reshape(O, k * k * C))


def mock_conv(x, w, stride, pad, **kw):
    xk, (B, Ho, Wo) = _im2col(x, w.shape[2], stride, pad)
    acc = S.mock_accumulate(xk, _wmat(w), **kw)
    return np.ascontiguousarray(acc.reshape(B, Ho, Wo, -1).transpose(0, 3, 1, 2))


def mock_dgrad(dz, w, stride, in_hw, flip=True, **kw):
    """data gradient as the kernel runs it: a stride-1 conv over dz (zero-dilated for stride 2) with the [cout][cin]
    weights, taps flipped"""
    O, C, k, _ = w.shape
    pad = k // 2
    B, _, Ho, Wo = dz.shape
    H, W = in_hw
    d = np.zeros((B, O, H + k - 1, W + k - 1), F32)
    d[:, :, k - 1 - pad:k - 1 - pad + stride * Ho:stride, k - 1 - pad:k - 1 - pad + stride * Wo:stride] = dz
    wt = w.transpose(1, 0, 2, 3)
    if flip:
        wt = wt[:, :, ::-1, ::-1]
    return mock_conv(d, np.ascontiguousarray(wt), 1, 0, **kw)


def mock_wgrad(dz, a, k, stride, sel, **kw):
    """weight gradient: rows = output channels, columns = (tap, cin), contraction over the pixels in 16-pixel groups"""
    ak, _ = _im2col(a, k, stride, k // 2)                      # (P, taps*C)
    zk = dz[:, sel].transpose(1, 0, 2, 3).reshape(len(sel), -1)  # (O, P)
    acc = S.mock_accumulate(np.ascontiguousarray(zk), np.ascontiguousarray(ak.T), **kw)
    return np.ascontiguousarray(acc.reshape(len(sel), k, k, a.shape[1]).transpose(0, 3, 1, 2))


def mock_wino(x, w, swap_u=False, lone_from_second=False, **kw):
    """conv_wino.hip: four GEMMs over (dy, channel) on the cut U / V, then the fp32 output transform"""
    U, V = S.wino_uv(x, w)
    if swap_u:
        U = U[[0, 2, 1, 3]]
    B, C, H, W = x.shape
    wp2 = V.shape[-1]
    M = []
    for xi in range(4):
        vk = np.stack([V[xi][:, :, dy:dy + H] for dy in range(3)], 1)            # (B, 3, C, H, wp2)
        vk = np.ascontiguousarray(vk.transpose(0, 3, 4, 1, 2).reshape(B * H * wp2, 3 * C))
        uk = np.ascontiguousarray(U[xi].transpose(0, 2, 1).reshape(-1, 3 * C))   # (O, (dy, C))
        M.append(S.mock_accumulate(vk, uk, **kw).reshape(B, H, wp2, -1).transpose(0, 3, 1, 2))
    y0 = ((M[0] + M[1]).astype(F32) + M[2]).astype(F32)
    y1 = ((M[1] - M[2]).astype(F32) - M[3]).astype(F32)
    out = np.empty(y0.shape[:3] + (W,), F32)
    out[..., 0::2] = y0
    out[..., 1::2] = y1[..., :W // 2]
    if lone_from_second and W % 2:
        out[..., W - 1] = y1[..., wp2 - 1]
    return out


def store_ups2(v, Hr, Wr, crop=True):
    """the x2-replicated store of a transition cell into the zero-bordered plane of a Hr x Wr route (Hr = 2h or 2h - 1)"""
    B, C, h, w = v.shape
    plane = np.zeros((B, C, Hr + 2, Wr + 2), F32)
    for dy in (0, 1):
        for dx in (0, 1):
            ys, xs = 2 * np.arange(h) + dy, 2 * np.arange(w) + dx
            if crop:
                ys, xs = ys[ys < Hr], xs[xs < Wr]
            plane[:, :, (1 + ys)[:, None], (1 + xs)[None, :]] = v[:, :, :len(ys), :len(xs)]
    return plane


def _failing(res):
    """which of (a), (b), (c) fail"""
    return {c for c, r in zip("abc", res) if not r.ok}


def _data(seed, B, C, H, W, O, k):
    rng = np.random.default_rng(seed)
    x = _leaky(rng.standard_normal((B, C, H, W)).astype(F32))
    w = (rng.standard_normal((O, C, k, k)) * 0.05).astype(F32)
    return x, w


# ---------------------------------------------------------------- the references themselves
def test_six_parts_sum_to_the_reference_and_five_is_a_subtraction():
    x, w = _data(1, 2, 32, 6, 7, 8, 3)
    for stride in (1, 2):
        parts = S.six_parts(x, w, stride, 1)
        assert np.array_equal(sum(parts), S.conv_split_ref(x, w, stride, 1))
        five = S.conv_split_ref(x, w, stride, 1, S.FIVE)
        np.testing.assert_allclose(sum(parts) - parts[S.SIX.index((0, 2))], five, rtol=0, atol=1e-13)
        assert np.array_equal(S.absum(x, w, stride, 1), S.abs_product_sum(x, w, stride, 1))


def test_gradient_parts_sum_to_the_float64_gradients_of_the_cut_operands():
    """dgrad_parts / wgrad_parts: the six parts add up to the float64 gradient up to the three products left out (2^-25)"""
    x, w = _data(2, 2, 32, 6, 8, 8, 3)
    for stride in (1, 2):
        dz = np.random.default_rng(3).standard_normal((2, 8, 6 // stride, 8 // stride)).astype(F32)
        parts, ab = S.dgrad_parts(dz, w, stride, (6, 8))
        want, ab64 = R.dgrad64(dz, w, stride, (6, 8))
        assert np.abs(sum(parts) - want).max() <= 2.0 ** -24 * ab.max() and np.array_equal(ab, ab64)
        parts, ab = S.wgrad_parts(dz, x, 3, stride, [0, 3, 7])
        want, ab64 = R.wgrad64(dz, x, 3, stride, [0, 3, 7])
        assert np.abs(sum(parts) - want).max() <= 2.0 ** -24 * ab.max() and np.array_equal(ab, ab64)


@pytest.mark.parametrize("W", [2, 7, 8, 13])
def test_winograd_restatement_without_the_cut_is_the_direct_conv(W):
    """1e-12 relative: the conditioning of the float64 transform, not a kernel tolerance"""
    import torch
    import torch.nn.functional as F
    x, w = _data(4 + W, 2, 32, 5, W, 8, 3)
    (y,), ab = S.wino_parts(x, w, cut=False)
    ref = F.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), None, 1, 1).numpy()
    assert y.shape == ref.shape
    assert np.abs(y - ref).max() <= 1e-12 * np.abs(ref).max()
    parts, ab = S.wino_parts(x, w)   # with the cut: fp32-rounded V and U, so only close
    assert np.abs(sum(parts) - ref).max() <= 8 * 2.0 ** -24 * ab.max()


def test_T_covers_both_mocks():
    """T_TYPICAL's derivation, re-measured: twice the single-term mock's worst ratio, and the 16-term mock far inside"""
    single, grouped = S.measure_typical(1), S.measure_typical(16)
    print("\nerr / (2^-24 absum), every term added singly: %s\n16-term groups: %s\nT = %g"
          % ({k: round(v, 2) for k, v in single.items()}, {k: round(v, 2) for k, v in grouped.items()}, S.T_TYPICAL))
    assert 2.0 * max(single.values()) <= S.T_TYPICAL <= 2.0 * max(single.values()) + 1.0
    assert max(grouped.values()) <= S.T_TYPICAL / 2.0


# ---------------------------------------------------------------- forward, direct form
FWD = [  # (label, B, C, H, W, O, k, stride, slabs): K = 288 on odd sizes, K = 4608 as four k-split slabs, 1x1, stride 2
    ("K288", 2, 32, 6, 7, 8, 3, 1, 1), ("K4608k4", 1, 512, 3, 4, 24, 3, 1, 4), ("K9216k8", 1, 1024, 3, 4, 24, 3, 1, 8),
    ("1x1", 1, 64, 6, 7, 8, 1, 1, 1), ("s2", 2, 32, 7, 9, 16, 3, 2, 1)]


# how close to -1 / +1 the census of a dropped / doubled product lands on these few hundred outputs: the three small
# products are far below everything else and project cleanly; m h and h m share their large factors' signs with each
# other on so few pixels (sample correlation up to 0.3 at 12 pixels); h h moved moves values across leaky's kink, where
# the census' linearisation ends.  The condition under test is |beta| > BETA_MAX in every case.
NEAR = {(2, 0): 0.1, (0, 2): 0.1, (1, 1): 0.1, (1, 0): 0.4, (0, 1): 0.4, (0, 0): 0.5}


def _fwd_case(case, **fault):
    _, B, C, H, W, O, k, stride, slabs = case
    x, w = _data(11, B, C, H, W, O, k)
    rng = np.random.default_rng(12)
    sc, sh = (0.5 + rng.random(O)).astype(F32), rng.standard_normal(O).astype(F32)
    z = mock_conv(x, w, stride, k // 2, slabs=slabs, **fault)
    res = rng.standard_normal(z.shape).astype(F32)
    got = (_leaky(R.fmaf(z, sc.reshape(1, -1, 1, 1), sh.reshape(1, -1, 1, 1))) + res).astype(F32)
    ep = S.Epilogue(sc, sh, leaky=True, addends=[res])
    n = 6 * C * k * k + slabs
    return S.check_split("forward", case[0], got, S.six_parts(x, w, stride, k // 2), S.absum(x, w, stride, k // 2), n, ep)


@pytest.mark.parametrize("case", FWD, ids=lambda c: c[0])
def test_forward_mock_is_accepted_and_every_product_fault_rejected(case):
    res = _fwd_case(case)
    assert not _failing(res), res
    assert max(abs(b) for b in res[1].betas) <= 0.1, res[1].betas
    for i, p in enumerate(S.SIX):
        dropped = _fwd_case(case, products=tuple(q for q in S.SIX if q != p))
        assert "b" in _failing(dropped), (p, dropped)
        # missing: -1 (h h dropped moves every value across leaky's kink, where the census' linearisation ends)
        assert abs(dropped[1].betas[i] + 1.0) <= NEAR[p], (p, dropped[1].betas)
        if p in ((1, 0), (0, 1), (0, 0)):
            assert "c" in _failing(dropped), (p, dropped)
        if p == (0, 0):
            assert "a" in _failing(dropped), dropped
        doubled = _fwd_case(case, products=S.SIX + (p,))
        assert "b" in _failing(doubled) and abs(doubled[1].betas[i] - 1.0) <= NEAR[p], (p, doubled[1].betas)
    swapped = _fwd_case(case, products=tuple((0, 1) if q == (1, 0) else q for q in S.SIX))  # h m in place of m h
    b = swapped[1].betas
    assert "b" in _failing(swapped) and b[S.SIX.index((1, 0))] < -0.5 and b[S.SIX.index((0, 1))] > 0.5, b


def test_last_pixel_row_of_the_last_tile_left_at_zero():
    _, B, C, H, W, O, k, stride, slabs = FWD[0]
    x, w = _data(11, B, C, H, W, O, k)
    got = mock_conv(x, w, 1, 1)
    args = (S.six_parts(x, w, 1, 1), S.absum(x, w, 1, 1), 6 * C * 9)
    assert not _failing(S.check_split("forward", "tail", got, *args))
    got[-1, :, -1, -1] = 0.0    # pixel M - 1, every channel
    assert {"a", "c"} <= _failing(S.check_split("forward", "tail", got, *args))
    got[-1, :, -1, -1] = np.nan  # ... or never written, over memory that holds no number
    assert {"a", "b", "c"} <= _failing(S.check_split("forward", "tail", got, *args))


# ---------------------------------------------------------------- Winograd
@pytest.mark.parametrize("W", [2, 7, 8])
def test_winograd_mock_is_accepted_and_its_faults_rejected(W):
    x, w = _data(21, 2, 32, 6, W, 8 if W > 2 else 16, 3)   # (W = 2, the Winograd minimum: 16 channels for the census)
    parts, ab = S.wino_parts(x, w)
    assert parts[0].size >= S.MIN_CENSUS
    n = 6 * 9 * 32 + 2

    def check(got):
        return S.check_split("winograd", "W%d" % W, got, parts, ab, n)
    assert not _failing(check(mock_wino(x, w)))
    assert {"a", "c"} <= _failing(check(mock_wino(x, w, swap_u=True)))
    if W % 2:
        assert {"a", "c"} <= _failing(check(mock_wino(x, w, lone_from_second=True)))
    for i, p in enumerate(S.SIX):
        dropped = check(mock_wino(x, w, products=tuple(q for q in S.SIX if q != p)))
        assert "b" in _failing(dropped) and abs(dropped[1].betas[i] + 1.0) <= 0.1, (p, dropped[1].betas)


# ---------------------------------------------------------------- data gradient
def _dgrad_case(stride, **fault):
    O, C, k, H, W = 32, 32, 3, 8, 8
    rng = np.random.default_rng(31 + stride)
    w = (rng.standard_normal((O, C, k, k)) * 0.05).astype(F32)
    dz = rng.standard_normal((2, O, H // stride, W // stride)).astype(F32)
    post = fault.pop("post", None)
    got = mock_dgrad(dz, w, stride, (H, W), **fault)
    if post:
        got = post(got)
    skip = rng.standard_normal(got.shape).astype(F32)
    got = (got + skip).astype(F32)   # accumulated into a skip gradient
    parts, ab = S.dgrad_parts(dz, w, stride, (H, W))
    return S.check_split("data gradient", "s%d" % stride, got, parts, ab, 6 * O * k * k, S.Epilogue(addends=[skip]))


@pytest.mark.parametrize("stride", [1, 2])
def test_data_gradient_mock_is_accepted_and_its_faults_rejected(stride):
    assert not _failing(_dgrad_case(stride))
    assert {"a", "c"} <= _failing(_dgrad_case(stride, flip=False))
    for i, p in enumerate(S.SIX):
        dropped = _dgrad_case(stride, products=tuple(q for q in S.SIX if q != p))
        assert "b" in _failing(dropped) and abs(dropped[1].betas[i] + 1.0) <= 0.1, (p, dropped[1].betas)
    if stride == 2:
        def swap(g):   # parity classes (0, 1) and (1, 0) written to each other's pixels
            g = g.copy()
            g[:, :, 0::2, 1::2], g[:, :, 1::2, 0::2] = g[:, :, 1::2, 0::2].copy(), g[:, :, 0::2, 1::2].copy()
            return g
        assert {"a", "c"} <= _failing(_dgrad_case(stride, post=swap))


def test_garbage_in_a_zero_padded_dz_channel():
    """A prediction conv's data gradient contracts over cout padded to a multiple of 32 (75 -> 96); both operands'
    padding must be zero.  Garbage in dz's padding channels shows as soon as the weight image's padding rows are not
    zero either, and at once where the garbage is not a finite number."""
    O, Op, C, H, W = 75, 96, 32, 5, 7
    rng = np.random.default_rng(41)
    w = (rng.standard_normal((O, C, 1, 1)) * 0.05).astype(F32)
    dz = rng.standard_normal((2, O, H, W)).astype(F32)
    parts, ab = S.dgrad_parts(dz, w, 1, (H, W))

    def run(dz_pad, w_pad):
        dzp = np.concatenate([dz, np.full((2, Op - O, H, W), dz_pad, F32)], 1)
        wp = np.concatenate([w, np.full((Op - O, C, 1, 1), w_pad, F32)], 0)
        return S.check_split("data gradient", "75->96", mock_dgrad(dzp, wp, 1, (H, W)), parts, ab, 6 * Op)
    assert not _failing(run(0.0, 0.0))
    assert not _failing(run(3.0, 0.0))            # finite garbage times a zero weight row: harmless
    assert {"a", "c"} <= _failing(run(3.0, 0.01))
    assert {"a", "b", "c"} <= _failing(run(np.nan, 0.0))


# ---------------------------------------------------------------- weight gradient
def test_weight_gradient_mock_is_accepted_and_its_faults_rejected():
    B, C, H, W, O, k = 2, 32, 9, 7, 16, 3
    rng = np.random.default_rng(51)
    a = _leaky(rng.standard_normal((B, C, H, W)).astype(F32))
    dz = rng.standard_normal((B, O, H, W)).astype(F32)
    sel = [0, 1, 4, 7, 9, 12, 14, 15]
    parts, ab = S.wgrad_parts(dz, a, k, 1, sel)
    assert parts[0].size == 8 * 9 * C >= S.MIN_CENSUS
    n = 6 * B * H * W + 2

    def check(**kw):
        return S.check_split("weight gradient", "3x3", mock_wgrad(dz, a, k, 1, sel, **kw), parts, ab, n)
    assert not _failing(check()) and not _failing(check(slabs=2))
    for i, p in enumerate(S.SIX):
        dropped = check(slabs=2, products=tuple(q for q in S.SIX if q != p))
        assert "b" in _failing(dropped) and abs(dropped[1].betas[i] + 1.0) <= 0.1, (p, dropped[1].betas)
    doubled = check(products=S.SIX + ((2, 0),))
    assert "b" in _failing(doubled)
    got = mock_wgrad(dz[:1], a[:1], k, 1, sel)   # the last image's pixels never summed
    assert {"a", "c"} <= _failing(S.check_split("weight gradient", "3x3", got, parts, ab, n))


# ---------------------------------------------------------------- the x2-replicated store
@pytest.mark.parametrize("Hr,Wr", [(9, 13), (10, 13), (9, 14)])
def test_x2_store_past_the_cropped_size(Hr, Wr):
    """A transition's output at 5 x 7 stored x2 into a 9 x 13 / 10 x 13 / 9 x 14 route: the crop keeps the border zero.  A
    store past it lands in the border, which the next conv reads as its padding."""
    x, w = _data(61, 1, 32, 5, 7, 8, 1)
    v = mock_conv(x, w, 1, 0)
    good, bad = store_ups2(v, Hr, Wr), store_ups2(v, Hr, Wr, crop=False)
    assert R.border_zero("borders", "transition", good).ok and not R.border_zero("borders", "transition", bad).ok
    # at the consumer: a 3x3 conv that reads the plane, border included; its reference pads the interior with zeros
    w2 = (np.random.default_rng(62).standard_normal((32, 8, 3, 3)) * 0.05).astype(F32)
    inner = np.ascontiguousarray(good[:, :, 1:-1, 1:-1])
    args = (S.six_parts(inner, w2, 1, 1), S.absum(inner, w2, 1, 1), 6 * 72)
    assert not _failing(S.check_split("forward", "consumer", mock_conv(inner, w2, 1, 1), *args))
    got = mock_conv(bad, w2, 1, 0)   # the device reads the plane as it is
    assert {"a", "c"} <= _failing(S.check_split("forward", "consumer", got, *args))
    # and the reference of the transition itself on the cropped replicate
    want = R.upsample2(v)[:, :, :Hr, :Wr]
    assert np.array_equal(inner, want)
