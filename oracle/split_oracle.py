"""CPU restatement of the OPT-IN split-fp32 conv arithmetic of videoyolo_amd/csrc/conv_split.hip — TEST INFRASTRUCTURE,
like everything under oracle/: only tests/ may import it; the product never does.

This is not a restatement of the reference (the reference has no such mode: mxnet hands `Conv2D`,
models/definitions/layers.py:63-70, to cuDNN / MKL-DNN); it pins what the kernel claims to compute, independently of
the kernel: every fp32 operand is cut into three bf16 numbers by round-to-nearest-even,

    h = bf16(x),   m = bf16(x - h),   l = bf16(x - h - m)                 (both differences are exact in fp32)

and a product x * w is taken as the six partial products  l h + h l + m m + m h + h m + h h  (the three left out are
below 2^-25 |x w|).  `conv_split_ref` evaluates exactly those six products in float64 — so the only thing the GPU result
may differ by is the rounding of its fp32 accumulation; `conv_split_ref(..., products=FIVE)` drops `h_x l_w`, which is how
the tests show that they would notice a missing product.  Parity status of this file: checked against float64 and against
its own exactness properties (tests/test_split_oracle.py); there is nothing in the reference to pin it to.
"""
import numpy as np

SIX = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))   # (plane of x, plane of w); plane 0 = h, 1 = m, 2 = l
FIVE = tuple(p for p in SIX if p != (0, 2))


def bf16_rne(x):
    """fp32 -> the nearest bf16 value (ties to even), returned as fp32.  Same integer formula as
    split_weights_kernel; finite inputs only."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32).reshape(np.shape(x))


def split3(x):
    """x (fp32) -> (h, m, l), each holding bf16 values, with h + m + l == x exactly."""
    x = np.ascontiguousarray(x, np.float32)
    h = bf16_rne(x)
    r = (x - h).astype(np.float32)      # exact: h is x rounded to 8 significant bits
    m = bf16_rne(r)
    l = bf16_rne((r - m).astype(np.float32))
    return h, m, l


def conv_split_ref(x, w, stride, pad, products=SIX):
    """The sum of the selected partial products of conv2d(x, w) in float64.  x (B,Cin,H,W), w (Cout,Cin,k,k) fp32."""
    import torch
    import torch.nn.functional as F
    xs = [torch.from_numpy(np.ascontiguousarray(p, np.float64)) for p in split3(x)]
    ws = [torch.from_numpy(np.ascontiguousarray(p, np.float64)) for p in split3(w)]
    out = None
    with torch.no_grad():
        for px, pw in products:
            t = F.conv2d(xs[px], ws[pw], None, stride, pad)
            out = t if out is None else out + t
    return out.numpy()


def abs_product_sum(x, w, stride, pad):
    """sum_k |x_k w_k| per output (float64): the scale the fp32 accumulation error is relative to."""
    import torch
    import torch.nn.functional as F
    with torch.no_grad():
        return F.conv2d(torch.from_numpy(np.abs(x).astype(np.float64)), torch.from_numpy(np.abs(w).astype(np.float64)),
                        None, stride, pad).numpy()


# ================================================================ per-kernel references and checks
# Everything below serves tests/test_split_cells_sensitivity.py (CPU) and tests/test_gpu_split_cells.py (GPU): the split
# kernels (conv_split.hip on three tiles, splitk_finish_kernel, conv_wino.hip, wgrad_split.hip, the data-gradient use of
# conv_split_kernel) held element by element to the six-products reference, on the tensors the device itself read.
#
# THE HARD BOUND, condition (a).  Every term the kernel adds is an exact bf16 x bf16 product (16 significand bits: exact
# in fp32).  A cell's output is the sum of the 6 K such terms of its K-long contraction, accumulated in fp32 in SOME
# order (the matrix core's own tree inside a 16-term group, the groups and the six products in program order, the k-split
# slabs in index order, the Winograd output transform last).  Any summation order of n fp32 additions with unit roundoff
# u satisfies |fl(sum) - sum| <= gamma_n sum|terms|, gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability, 4.4), so
#     |got - six| <= gamma'_n absum,   n = 6 K + (k-split slabs) + (output-transform adds),   u' = 2^-23.
# u' is the unit roundoff of an fp32 adder that TRUNCATES (2^-24 if it rounds to nearest): nobody has measured which the
# matrix core's accumulator does, and the bound must hold either way.  The epilogue adds one rounding each, a full ulp
# (2^-23 relative) of the value it rounds: the affine fmaf, leaky's product 0.1f * v, the residual add, the bias add,
# every addend accumulated into a gradient plane.  Leaky is 1-Lipschitz: it passes an error on at most unchanged, kink
# or no kink, so no element is exempt.
U_HARD = 2.0 ** -23
U32 = 2.0 ** -24
# THE TYPICAL-ROUNDING BAR, condition (c): err <= T_TYPICAL 2^-24 absum + the same epilogue roundings.  T is measured, on
# the CPU, not chosen: `mock_accumulate(..., group=1)` adds every one of the 6 K terms singly in fp32, round to nearest —
# no hardware order accumulates more roundings than that — on leaky(N(0,1)) activations and N(0, 0.05^2) weights for
# K in {32, 288, 1024, 4608, 9216}, two seeds of 384 outputs each (measure_typical below), against the float64
# six-products sum.  Worst err / (2^-24 absum) per K, seed 0 | seed 1:
#     K = 32: 5.05 | 6.51    288: 4.42 | 3.65    1024: 4.99 | 5.26    4608: 4.51 | 3.80    9216: 8.21 | 4.37
# (the ratio does not grow with K: the random walk's sqrt(6 K) is offset by absum's lead of K / sqrt(K) over the running
# sum; it is a maximum, so it moves with the draw).  The 16-term-group mock stays at 1.2 ... 2.3.  T is twice the worst,
# 2 x 8.21 = 16.4, rounded up to a whole number: the device run takes its maximum over ~1e5 elements per cell where the
# mock has a few hundred.  tests/test_split_cells_sensitivity.py::test_T_covers_both_mocks re-measures and asserts that
# the single-term mock stays under T_TYPICAL / 2 and the 16-term-group mock under it too.
T_TYPICAL = 17.0
BETA_MAX = 0.25      # condition (b): present 0, missing -1, doubled +1
MIN_CENSUS = 256     # outputs a product census needs at least
PRODUCT_NAMES = tuple("%s_x %s_w" % ("hml"[a], "hml"[b]) for a, b in SIX)


def gamma_hard(n):
    n = np.asarray(n, np.float64)
    return n * U_HARD / (1.0 - n * U_HARD)


def _t64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


def _planes(a):
    return [_t64(p) for p in split3(a)]


def six_parts(x, w, stride, pad):
    """The six partial products of conv2d(x, w) separately, float64, in the order of SIX: a list of six (B,Cout,Ho,Wo)
    arrays.  conv_split_ref(x, w, stride, pad) is their sum; "five products" is the sum minus one part."""
    import torch
    import torch.nn.functional as F
    xs, ws = _planes(x), _planes(w)
    with torch.no_grad():
        return [F.conv2d(xs[px], ws[pw], None, stride, pad).numpy() for px, pw in SIX]


def absum(x, w, stride, pad):
    """sum_k |x_k| |w_k| per output, float64 (|h + m + l| products: within 2^-8 of the sum of the six |parts|' terms)"""
    return abs_product_sum(x, w, stride, pad)


def dgrad_parts(dz, w, stride, in_hw):
    """The six partial products of the data gradient conv2d_input(dz, w) on the split planes of dz and w (the x planes
    of SIX are dz's: dz is the kernel's activation operand, w its pre-split [cout][cin] image) -> (parts, absum)."""
    import torch
    k = w.shape[2]
    shape = (dz.shape[0], w.shape[1], int(in_hw[0]), int(in_hw[1]))
    zs, ws = _planes(dz), _planes(w)
    with torch.no_grad():
        parts = [torch.nn.grad.conv2d_input(shape, ws[pw], zs[pz], stride=stride, padding=k // 2).numpy() for pz, pw in SIX]
        ab = torch.nn.grad.conv2d_input(shape, _t64(np.abs(w)), _t64(np.abs(dz)), stride=stride, padding=k // 2).numpy()
    return parts, ab


def wgrad_parts(dz, a, k, stride, sel):
    """The six partial products of the weight gradient conv2d_weight(a, dz) for the output channels `sel` (as
    train_cells64.wgrad64 restricts it); the x planes of SIX are dz's (the kernel's A operand), the w planes a's ->
    (parts, absum), each (len(sel), Cin, k, k)."""
    import torch
    shape = (len(sel), a.shape[1], k, k)
    zs, as_ = _planes(dz[:, sel]), _planes(a)
    with torch.no_grad():
        parts = [torch.nn.grad.conv2d_weight(as_[pa], shape, zs[pz], stride=stride, padding=k // 2).numpy() for pz, pa in SIX]
        ab = torch.nn.grad.conv2d_weight(_t64(np.abs(a)), shape, _t64(np.abs(dz[:, sel])), stride=stride, padding=k // 2).numpy()
    return parts, ab


def wino_uv(x, w, cut=True):
    """conv_wino.hip's operands.  U (4, Cout, Cin, 3[dy]) from w (Cout, Cin, 3, 3) with wino_weights_kernel's own fp32
    expression; V (4, B, Cin, H + 2, ceil(W / 2)) as fp32 sums / differences of two pixels of the zero-bordered plane (the
    pixel past an odd width is the border's zero; d3 of the lone last pair lies past it and is taken as zero: it feeds
    only the discarded Y(x0 + 1)).  cut=False: the same transforms in float64, nothing rounded."""
    ft = np.float32 if cut else np.float64
    g0, g1, g2 = [np.ascontiguousarray(w[:, :, :, i], ft) for i in range(3)]
    half = ft(0.5)
    U = np.stack([g0, (((g0 + g1).astype(ft) + g2).astype(ft) * half).astype(ft),
                  (((g0 - g1).astype(ft) + g2).astype(ft) * half).astype(ft), g2])
    B, C, H, W = x.shape
    wp2 = (W + 1) // 2
    xp = np.zeros((B, C, H + 2, 2 * wp2 + 2), ft)
    xp[:, :, 1:H + 1, 1:W + 1] = x
    d = [xp[:, :, :, j:j + 2 * wp2:2] for j in range(4)]   # d_j of pair xp: padded column 2 xp + j
    V = np.stack([(d[0] - d[2]).astype(ft), (d[1] + d[2]).astype(ft), (d[2] - d[1]).astype(ft), (d[1] - d[3]).astype(ft)])
    return U, V


def wino_parts(x, w, cut=True):
    """conv_wino.hip restated up to accumulation order: U and V formed and rounded in fp32 (wino_uv), both cut with
    split3, the six parts of every M_xi as float64 sums over (dy, channel), Y(x0) = M0 + M1 + M2 and
    Y(x0 + 1) = M1 - M2 - M3 -> (parts: six (B,Cout,H,W) arrays, absum: the sum over the xi used of sum |V| |U|).
    cut=False: one "part", the float64 transform without any rounding or cut (== the direct float64 conv up to the
    conditioning of the transform)."""
    import torch
    import torch.nn.functional as F
    B, C, H, W = x.shape
    U, V = wino_uv(x, w, cut)
    prods = SIX if cut else ((0, 0),)
    M = [[None] * len(prods) for _ in range(4)]
    A = []
    with torch.no_grad():
        for xi in range(4):
            vs = _planes(V[xi]) if cut else [_t64(V[xi])]
            us = [t.unsqueeze(-1) for t in (_planes(U[xi]) if cut else [_t64(U[xi])])]   # (Cout, Cin, 3, 1): taps along y
            for i, (pv, pu) in enumerate(prods):
                M[xi][i] = F.conv2d(vs[pv], us[pu]).numpy()
            A.append(F.conv2d(_t64(np.abs(V[xi])), _t64(np.abs(U[xi])).unsqueeze(-1)).numpy())

    def weave(y0, y1):
        out = np.empty(y0.shape[:3] + (W,), np.float64)
        out[..., 0::2] = y0
        out[..., 1::2] = y1[..., :W // 2]
        return out
    parts = [weave(M[0][i] + M[1][i] + M[2][i], M[1][i] - M[2][i] - M[3][i]) for i in range(len(prods))]
    return parts, weave(A[0] + A[1] + A[2], A[1] + A[2] + A[3])


class Epilogue:
    """What follows the accumulation, applied in float64 to the six-products sum: affine (scale, shift per channel;
    scale None with a shift: a bias), leaky (slope float32(0.1), as vy_leaky holds it), addends (a residual, a skip
    gradient, the gradient plane a data gradient accumulates into; each may carry its own error bound), and exact terms
    (float64 references of contributions the EXACT kernel computed into the same plane, with their gamma bound).
    `axis` is the channel axis of the checked tensor."""

    def __init__(self, scale=None, shift=None, leaky=False, addends=(), axis=1):
        self.scale, self.shift, self.leaky, self.addends, self.axis = scale, shift, leaky, list(addends), axis

    def _b(self, v, ndim):
        shape = [1] * ndim
        shape[self.axis] = -1
        return np.asarray(v, np.float64).reshape(shape)

    def apply(self, z, bound):
        """(reference output, |d out / d z|, error bound of the output) from the pre-epilogue reference z and the bound
        on the accumulation error; every rounding adds one ulp (2^-23 relative) of the largest value it can round."""
        gain = np.ones_like(z)
        y = z
        if self.scale is not None:
            sc, sh = self._b(self.scale, z.ndim), self._b(self.shift, z.ndim)
            y = y * sc + sh
            gain = gain * np.abs(sc)
            bound = bound * np.abs(sc)
            bound = bound + U_HARD * (np.abs(y) + bound)
        elif self.shift is not None:
            y = y + self._b(self.shift, z.ndim)
            bound = bound + U_HARD * (np.abs(y) + bound)
        if self.leaky:
            slope = np.float64(np.float32(0.1))
            neg = y <= 0
            y = np.where(neg, slope * y, y)
            gain = np.where(neg, slope * gain, gain)
            bound = bound + U_HARD * (np.abs(y) + bound)   # (the product 0.1f * v is rounded; 1-Lipschitz otherwise)
        for a in self.addends:
            y = y + np.asarray(a, np.float64)
            bound = bound + U_HARD * (np.abs(y) + bound)
        return y, gain, bound


def check_split(kind, name, got, parts, absum_, n_terms, epilogue=None, exact_terms=(), launches=None):
    """The three conditions on one tensor the split kernels produced -> [Result (a), Result (b), Result (c)]
    (train_cells64.Result: `ratio` <= 1 passes; kinds '<kind> hard bound', '<kind> product census', '<kind> typical bar').

    got: the device tensor.  parts: the six float64 partial products (or a list of such lists, one per split launch
    that accumulated into this tensor: several consumers of one gradient plane); absum_: sum |x| |w| of all of them.
    n_terms: the fp32 additions of the accumulation, 6 K + slabs + transform adds (summed over the launches).
    exact_terms: [(want64, absum64, n)] contributions of the exact kernel to the same plane, each within
    gamma_n(u = 2^-24) absum (train_cells64.gamma).  launches: names for the census' detail.

    (a) |got - ref| <= gamma'_n absum + epilogue roundings (module comment), non-finite values fail;
    (b) |beta_p| <= BETA_MAX for each of the six products of each launch,
        beta_p = <got - ref, P_p g> / <P_p g, P_p g> over the checked outputs, g = d out / d z of the epilogue;
    (c) |got - ref| <= T_TYPICAL 2^-24 absum + epilogue roundings."""
    from .train_cells64 import Result, gamma
    epilogue = epilogue or Epilogue()
    groups = parts if isinstance(parts[0], (list, tuple)) else [parts]
    z = sum(sum(g) for g in groups)
    extra_hard = np.zeros_like(z)
    for want, ab, n in exact_terms:
        z = z + want
        extra_hard = extra_hard + gamma(n) * ab
    got = np.asarray(got, np.float64)
    assert got.shape == z.shape, (name, got.shape, z.shape)
    # launches accumulated into one plane: each join is one rounding of a partial sum, itself within the absolute sum
    if len(groups) + len(exact_terms) > 1:
        total = absum_ + sum(ab for _, ab, _ in exact_terms)
        extra_hard = extra_hard + (len(groups) + len(exact_terms) - 1) * U_HARD * total
    want_a, gain, bound_a = epilogue.apply(z, gamma_hard(n_terms) * absum_ + extra_hard)
    _, _, bound_c = epilogue.apply(z, T_TYPICAL * U32 * absum_ + extra_hard)
    d = got - want_a
    err = np.abs(d)
    bad = ~np.isfinite(got)
    out = []
    for label, bound in (("hard bound", bound_a), ("typical bar", bound_c)):
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / bound)
            h = np.where(err == 0, 0.0, err / (U32 * absum_ * gain))
        r, h = np.where(bad, np.inf, r), np.where(bad | ~np.isfinite(h), 0.0, h)
        out.append(Result("%s %s" % (kind, label), name, r.max(initial=0.0), h.max(initial=0.0),
                          np.where(bad, np.inf, err).max(initial=0.0), np.abs(want_a).max(initial=0.0),
                          "%d non-finite" % int(bad.sum()) if bad.any() else ""))
    betas, detail = [], []
    dd = np.where(bad, 0.0, d)
    for gi, g in enumerate(groups):
        for pi, p in enumerate(g):
            pg = p * gain
            den = float((pg * pg).sum())
            b = float((dd * pg).sum()) / den if den > 0 else 0.0
            betas.append(b)
            if abs(b) > BETA_MAX:
                detail.append("%s%s beta %.2f" % ((launches[gi] + " ") if launches else "", PRODUCT_NAMES[pi], b))
    worst = max(abs(b) for b in betas)
    ratio = worst / BETA_MAX
    if got.size < MIN_CENSUS or bad.any():
        ratio = np.inf
        detail.append("%d outputs (%d non-finite): no census" % (got.size, int(bad.sum())))
    census = Result("%s product census" % kind, name, ratio, worst, err.max(initial=0.0), np.abs(want_a).max(initial=0.0),
                    "; ".join(detail))
    census.betas, census.n_out = betas, int(got.size)
    return [out[0], census, out[1]]


def sample_channels(cout, name, pixels=None):
    """Output channels a cell is checked on: all of them up to 64, else the first, the last and one (drawn from the
    cell's name) out of each of m equal runs, m = 32 — every 32-column group of every tile of a launch is met — or as
    many as the product census needs where the cell has only `pixels` checked pixels per channel"""
    import zlib
    m = 32 if not pixels else max(32, -(-MIN_CENSUS // pixels))
    if cout <= max(64, m):
        return list(range(cout))
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    return sorted({0, cout - 1} | {i * cout // m + int(rng.integers(max(1, cout // m))) for i in range(m)})


def mock_accumulate(xk, wk, group=16, products=SIX, slabs=1):
    """fp32 mock of the kernels' accumulation: xk (P, K), wk (O, K) fp32 operands in the kernel's k order -> (P, O) fp32.
    Per group of `group` consecutive k and per product in SIX's order (smallest first), the group's exact sum is added
    to the fp32 accumulator with one rounding (group=16: the matrix core's 16-term instruction; group=1: every term
    added singly, the order with the most roundings).  slabs > 1: K in that many contiguous ranges, each accumulated
    from zero, the slabs then added in index order (split-K)."""
    xs = [np.asarray(p, np.float64) for p in split3(xk)]
    ws = [np.asarray(p, np.float64) for p in split3(wk)]
    K = xk.shape[1]
    total = np.zeros((xk.shape[0], wk.shape[0]), np.float32)
    for s in range(slabs):
        lo, hi = s * K // slabs, (s + 1) * K // slabs
        acc = np.zeros_like(total)
        for g0 in range(lo, hi, group):
            g1 = min(hi, g0 + group)
            for px, pw in products:
                acc = (acc.astype(np.float64) + xs[px][:, g0:g1] @ ws[pw][:, g0:g1].T).astype(np.float32)
        total = acc if slabs == 1 else (total + acc).astype(np.float32)
    return total


def measure_typical(group, seeds=(0, 1), ks=(32, 288, 1024, 4608, 9216), P=48, O=8):
    """{K: worst err / (2^-24 absum)} of mock_accumulate(group) against the float64 six-products sum, on the inputs
    T_TYPICAL's derivation names (leaky(N(0, 1)) activations, N(0, 0.05^2) weights, P x O outputs per seed)"""
    out = {}
    for K in ks:
        worst = 0.0
        for seed in seeds:
            rng = np.random.default_rng(1000 * seed + K)
            x = rng.standard_normal((P, K)).astype(np.float32)
            x = np.maximum(x, np.float32(0.1) * x)
            w = (rng.standard_normal((O, K)) * 0.05).astype(np.float32)
            xs = [p.astype(np.float64) for p in split3(x)]
            ws = [p.astype(np.float64) for p in split3(w)]
            six = sum(xs[a] @ ws[b].T for a, b in SIX)
            ab = np.abs(x).astype(np.float64) @ np.abs(w).astype(np.float64).T
            worst = max(worst, float((np.abs(mock_accumulate(x, w, group=group) - six) / (U32 * ab)).max()))
        out[K] = worst
    return out
