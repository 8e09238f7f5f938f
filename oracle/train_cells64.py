"""Per-cell float64 reference of the training step, fed the tensors the HIP step itself
used.

TEST INFRASTRUCTURE ONLY.  End-to-end gradient comparisons cannot be tight: a last-bit change in the forward moves
gradients by up to 2e-2 through the LeakyReLU kinks.  Here every kernel of the step is checked on its own: it gets
the exact inputs the device gave it (tapped z / dz planes, BatchNorm statistics, input views, output gradients), the
same operation is recomputed in float64, and each element must lie within a worst-case rounding bound

    |got - want| <= gamma_n * sum|terms|,   gamma_n = n u / (1 - n u),  u = 2^-24,

where n is the fp32 accumulation depth the device's plan uses (any summation order of that depth satisfies it, so
the bound never fails a correct kernel).  Forward convolutions (pinned summation order, include/vy_math.h) and the
BatchNorm forward apply are bit-exact; the batch statistics are within 1 ulp of their float64 value rounded the way
the finalize rounds it.

A SyncBatchNorm cell's statistics are those of the global batch: the other ranks' contribution to the all-reduce is one
more input of the cell (`peer`, `world` of stats64 / check_stats / check_running / bn_backward64 / check_bn_backward;
check_sync_sums for the sums the exchange is handed; sync_peer constructs a peer).  Without a peer every check is the
per-device one, bit for bit.

The graph walked here mirrors OracleYolo3Train.forward_raw / backward: routes, concat order (the upsampled
transition first), x2 transition gradients summed over 2x2, residual skips, planes with several consumers.

Every check returns a Result; `ratio` is the worst error / bound (a pass is <= 1), `headroom` the worst
error / (u sqrt(n) sum|terms|), the size of the error against a typical (random-walk) rounding error.
"""
import numpy as np
import torch

from . import yolo3_oracle as O

U = 2.0 ** -24
F32 = np.float32


U64 = 2.0 ** -53


def gamma(n, u=U):
    n = np.asarray(n, np.float64)
    return n * u / (1.0 - n * u)


class Result:
    def __init__(self, kind, name, ratio, headroom, err_max=0.0, want_max=0.0, detail=""):
        self.kind, self.name, self.ratio, self.headroom = kind, name, float(ratio), float(headroom)
        self.err_max, self.want_max = float(err_max), float(want_max)
        self.detail = detail
        self.extra = {}  # conditions on the inputs a check found on the way (not part of the verdict)

    @property
    def ok(self):
        return self.ratio <= 1.0

    @property
    def old_bar_ok(self):
        """would the end-to-end bar, max|got - want| < 2e-3 max|want| over the tensor, have passed?"""
        return self.err_max < 2e-3 * self.want_max or self.err_max == 0.0

    @staticmethod
    def merge(parts):
        """one Result of a tensor checked in pieces (channel blocks)"""
        w = max(parts, key=lambda r: r.ratio)
        r = Result(w.kind, w.name, w.ratio, max(p.headroom for p in parts), max(p.err_max for p in parts),
                   max(p.want_max for p in parts), "; ".join(sorted(set(p.detail for p in parts if p.detail))))
        return r

    def __repr__(self):
        return "%s %s: err/bound %.3g, err/(u sqrt(n) S) %.3g%s" % (self.kind, self.name, self.ratio, self.headroom,
                                                                  (" " + self.detail) if self.detail else "")


def _bounded(kind, name, got, want, absum, n, detail="", u=U):
    """got (fp32) vs want (float64) elementwise, bar gamma_n * absum (n scalar or per element; u: the unit roundoff of
    the accumulation, 2^-24 unless the device sums in double)."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - want)
    bound = gamma(n, u) * absum
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
        h = np.where(err == 0, 0.0, err / (u * np.sqrt(n) * absum))
    return Result(kind, name, r.max(initial=0.0), h.max(initial=0.0), err.max(initial=0.0),
                  np.abs(want).max(initial=0.0), detail)


def _exact(kind, name, got, want):
    bad = got != want
    if got.dtype.kind == "f":
        bad &= ~(np.isnan(got) & np.isnan(want))
    nbad = int(np.count_nonzero(bad))
    scale = np.abs(want.astype(np.float64)).max(initial=0.0)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)).max(initial=0.0) if nbad else 0.0
    return Result(kind, name, np.inf if nbad else 0.0, 0.0, err, scale, "%d elements differ" % nbad if nbad else "")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


def fmaf(a, b, c):
    """fp32 fmaf(a, b, c) exactly: a*b is exact in float64; s = fl64(a*b + c) plus its TwoSum error is the exact sum,
    and rounding s to fp32 is only wrong when s sits exactly on an fp32 rounding midpoint (then the error's sign
    decides)."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c, p.shape).astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = s.astype(F32)
    rd = r.astype(np.float64)
    # the fp32 neighbour on the other side of s, and whether s is their midpoint
    other = np.where(s > rd, np.nextafter(r, F32(np.inf)), np.nextafter(r, F32(-np.inf))).astype(np.float64)
    mid = (s != rd) & ((rd + other) * 0.5 == s)
    fix = mid & (e != 0)
    if np.any(fix):
        up = e > 0
        r = np.where(fix, np.where(up, np.maximum(r, other.astype(F32)), np.minimum(r, other.astype(F32))), r)
    return r.astype(F32)


def leaky(v):
    return np.maximum(v, F32(0.1) * v)  # vy_leaky


def upsample2(a):
    return a.repeat(2, axis=-1).repeat(2, axis=-2)


def interior(p):
    return p[:, :, 1:-1, 1:-1]


def border_zero(kind, name, p):
    m = np.ones(p.shape[2:], bool)
    m[1:-1, 1:-1] = False
    nz = int(np.count_nonzero(p[:, :, m]))
    return Result(kind, name, np.inf if nz else 0.0, 0.0, 0.0, 0.0, "%d nonzero border values" % nz if nz else "")


# ---------------------------------------------------------------- the graph
ROUTE_CHANNELS = (256, 512, 1024)  # strides 8, 16, 32


def graph(num_class, k=1, heads_only=False):
    """Cells in forward order: dict(name, k, s, cin, cout, bn, ups, src, skip, fm).  `src`: the producers whose
    outputs, concatenated in this order, are the cell's input ("image" for the stem); `skip`: the producer whose output
    is added to this cell's (residual blocks); `fm`: the frame multiplier (PlaneT::fm), the cell runs on B * fm frames.

    k > 1 is the window net: the stem and the stages run on the B * k frames (fm = k), and three pool nodes
    "pool.0" .. "pool.2" (strides 8, 16, 32; dict(name, pool=True, src=[route cell], cout, fm=1)) stand between the
    per-frame route cells and the head cells that read the routes; stages.1.0 / stages.2.0 keep reading the per-frame
    routes.  heads_only is the heads net: the head cells alone, their route inputs named "route.0" .. "route.2"."""
    if heads_only and k != 1:
        raise ValueError("the heads net has no frames to pool")
    cells = []

    def add(name, k_, s, cin, cout, src, bn=True, ups=1, skip=None, fm=1):
        cells.append(dict(name=name, k=k_, s=s, cin=cin, cout=cout, bn=bn, ups=ups, src=list(src), skip=skip, fm=fm))

    if heads_only:
        routes = ["route.%d" % i for i in range(3)]
        chans = dict(zip(routes, ROUTE_CHANNELS))
    else:
        feats = O.darknet_feature_cells()
        prev, routes = "image", []
        for si, (lo, hi) in enumerate(O.STAGE_SLICES):
            for j, f in enumerate(feats[lo:hi]):
                pre = "stages.%d.%d" % (si, j)
                if f[0] == "conv":
                    add(pre, f[3], f[4], f[1], f[2], [prev], fm=k)
                    prev = pre
                else:
                    c = f[1]
                    add(pre + ".body.0", 1, 1, c, c // 2, [prev], fm=k)
                    add(pre + ".body.1", 3, 1, c // 2, c, [pre + ".body.0"], skip=prev, fm=k)
                    prev = pre + ".body.1"
            routes.append(prev)
        chans = {c["name"]: c["cout"] for c in cells}
        if k > 1:
            for i, r in enumerate(routes):
                cells.append(dict(name="pool.%d" % i, pool=True, src=[r], cin=chans[r], cout=chans[r], fm=1, skip=None))
                chans["pool.%d" % i] = chans[r]
            routes = ["pool.%d" % i for i in range(3)]
    x = [routes[2]]
    for i, ch in enumerate(O.HEAD_CHANNELS):
        cin = sum(chans[p] for p in x)
        for j in range(5):
            oc, kk = (ch, 1) if j % 2 == 0 else (2 * ch, 3)
            name = "yolo_blocks.%d.body.%d" % (i, j)
            add(name, kk, 1, cin, oc, x)
            x, cin = [name], oc
        route = x[0]
        add("yolo_blocks.%d.tip" % i, 3, 1, ch, 2 * ch, [route])
        add("yolo_outputs.%d.prediction" % i, 1, 1, 2 * ch, 3 * (5 + num_class), ["yolo_blocks.%d.tip" % i], bn=False)
        if i == 2:
            break
        add("transitions.%d" % i, 1, 1, ch, ch // 2, [route], ups=2)
        chans["transitions.%d" % i] = ch // 2
        x = ["transitions.%d" % i, routes[1 - i]]
        chans.update({c["name"]: c["cout"] for c in cells})
    return cells


def is_pool(c):
    return bool(c.get("pool"))


def consumers(cells):
    """producer name -> [(consumer, channel offset of the producer inside the consumer's input)] and
    producer name -> [cells whose skip it is].  A consumer is a conv cell or a pool node (is_pool); the producers are
    cells, pool nodes, "image" and the heads net's imported routes "route.i"."""
    width = {c["name"]: c["cout"] for c in cells}
    width["image"] = 3
    width.update({"route.%d" % i: ch for i, ch in enumerate(ROUTE_CHANNELS)})
    cons, skips = {}, {}
    for c in cells:
        off = 0
        for p in c["src"]:
            cons.setdefault(p, []).append((c, off))
            off += width[p]
        if c["skip"]:
            skips.setdefault(c["skip"], []).append(c)
    return cons, skips


# ---------------------------------------------------------------- temporal pooling (temporal.hip)
def pool_forward(frames, k, join):
    """TemporalPooling 'direct' over each clip's k frames (frame t of clip b is frame b*k + t) in temporal.hip's pinned
    fp32 arithmetic: max is strict > in frame order (ties keep the earliest frame's bits), mean is
    acc = x0; acc += x1; ...; acc / float32(k)."""
    f = np.asarray(frames, F32)
    f = f.reshape((-1, k) + f.shape[1:])
    acc = f[:, 0].copy()
    for t in range(1, k):
        v = f[:, t]
        if join == "max":
            m = v > acc
            acc[m] = v[m]
        else:
            acc = (acc + v).astype(F32)
    if join == "mean":
        acc = (acc / F32(k)).astype(F32)
    return acc


def pool_backward(g_pooled, frames, pooled, k, join):
    """Per-frame route gradients (B*k, ...) window_pool_bwd writes: mean gives g / float32(k) to every frame, max gives g
    to every frame with x_t == pooled (IEEE equality: every tied frame gets the full g) and +0 to the others."""
    g = np.asarray(g_pooled, F32)
    f = np.asarray(frames, F32)
    f = f.reshape((-1, k) + f.shape[1:])
    if join == "mean":
        out = np.repeat((g / F32(k)).astype(F32)[:, None], k, axis=1)
    else:
        out = np.where(f == np.asarray(pooled, F32)[:, None], g[:, None], F32(0.0)).astype(F32)
    return np.ascontiguousarray(out.reshape((-1,) + f.shape[2:]))


def check_pool_forward(name, frames, k, join, pooled_got):
    """the pooled route on the device's own per-frame route values: bit-equal"""
    return _exact("pool forward", name, pooled_got, pool_forward(frames, k, join))


def pool_wins(frames, k):
    """(wins, ties) of (B*k, ...) per-frame values: wins[t] = the number of elements where frame t alone holds the
    clip's maximum, ties = the number of elements where more than one frame holds it"""
    f = np.asarray(frames, F32)
    f = f.reshape((-1, k) + f.shape[1:])
    hold = f == f.max(axis=1, keepdims=True)
    n_hold = hold.sum(axis=1, keepdims=True)
    wins = [int(np.count_nonzero(hold[:, t:t + 1] & (n_hold == 1))) for t in range(k)]
    return wins, int(np.count_nonzero(n_hold > 1))


def check_pool_backward(name, g_pooled, frames, pooled, k, join, got):
    """window_pool_bwd's output on the device's own pooled gradient, per-frame route values and pooled values:
    bit-equal.  Returns (Result, wins, ties) with pool_wins' counts of one route."""
    res = _exact("pool backward", name, got, pool_backward(g_pooled, frames, pooled, k, join))
    wins, ties = pool_wins(frames, k)
    return res, wins, ties


# ---------------------------------------------------------------- per-kernel checks
def check_forward_conv(name, a, w, stride, z_got):
    """raw conv output (no BN) on HIP's own input: bit-equal to the pinned-order oracle conv"""
    k = w.shape[2]
    return _exact("forward conv", name, z_got, O.conv2d(a, w, stride, k // 2))


def stats64(z, peer=None, world=1):
    """(mean, biased variance, count) of a cell in float64: the sums of the tapped z, plus — SyncBatchNorm — the peer
    ranks' [2][C] contribution to the all-reduce (an exact input of the cell, as recorded), over world * n samples"""
    z64 = z.astype(np.float64)
    n = z.shape[0] * z.shape[2] * z.shape[3]
    s1, s2 = z64.sum(axis=(0, 2, 3)), (z64 * z64).sum(axis=(0, 2, 3))
    if peer is not None:
        s1, s2 = s1 + peer[0], s2 + peer[1]
    n = n * world
    mean = s1 / n
    return mean, np.maximum(s2 / n - mean * mean, 0.0), n


def check_stats(name, z, mean_got, invstd_got, gamma_p, beta_p, scale_got, shift_got, eps=1e-5, peer=None, world=1):
    """saved mean / invstd within 1 ulp of the float64 statistics rounded in the finalize's form; scale / shift as the
    finalize forms them from those.  peer, world: a synchronised cell's statistics are those of the global batch
    (stats64)"""
    mean, var, _ = stats64(z, peer, world)
    mf, vf = mean.astype(F32), var.astype(F32)
    inv = (F32(1.0) / np.sqrt(vf + F32(eps))).astype(F32)
    e_m = np.abs(mean_got.astype(np.float64) - mf) / np.spacing(np.abs(mf)).astype(np.float64)
    e_i = np.abs(invstd_got.astype(np.float64) - inv) / np.spacing(np.abs(inv)).astype(np.float64)
    ulps = float(max(e_m.max(), e_i.max()))
    r = Result("forward stats", name, ulps, ulps, np.abs(mean_got - mf).max(), np.abs(mf).max(), "%.2g ulp" % ulps)
    sc = (gamma_p * invstd_got).astype(F32)
    sh = fmaf(-mean_got, sc, beta_p)
    if not (np.array_equal(sc, scale_got) and np.array_equal(sh, shift_got)):
        r.ratio, r.detail = np.inf, r.detail + ", scale/shift differ from the finalize's form"
    return r


def check_apply(name, z, scale, shift, out_got, res=None, ups=1):
    """forward apply: leaky(fmaf(z, scale, shift)) (+ skip) (x2 replicated), fp32, bit-equal"""
    v = leaky(fmaf(z, scale.reshape(1, -1, 1, 1), shift.reshape(1, -1, 1, 1)))
    if res is not None:
        v = (v + res).astype(F32)
    if ups == 2:
        v = upsample2(v)
    return _exact("forward apply", name, out_got, v)


def sync_cells(cells):
    """names of the SyncBatchNorm cells of a graph, in forward order: the stem and the five stride-2 convs of the stages
    (is_sync_layer, csrc/net_internal.h) — the statistics exchange runs for them in this order forward, reversed
    backward"""
    return [c["name"] for c in cells if c.get("bn") and c["name"].startswith("stages.") and ".body." not in c["name"]]


def sync_peer(index, local, n, world, forward, seed=0):
    """The constructed peer of one statistics exchange: what the other world - 1 ranks add to the [2][C] sums `local`
    (float64) of a rank with n samples, drawn from a generator keyed by (seed, index of the call in the step).
    Forward: the sums of (world - 1) n samples whose per-channel mean is the local mean shifted by +-[0.25, 1] local
    standard deviations and whose variance is the local variance times 2^[-1, 1] — the global variance stays positive
    and every channel's global mean differs from the local one (the variance too, but for a chance cancellation of the
    two shifts; tests/test_train_cells64_sensitivity.py holds both at the counts the GPU test uses).  Backward: a per-channel multiple in [-1, 2] of the
    local sum plus an offset of +-[0.25, 1] times the call's largest |local sum| (never zero), times world - 1.
    world = 1: zeros, the all-reduce over one rank."""
    local = np.asarray(local, np.float64)
    C = local.shape[1]
    if world == 1:
        return np.zeros_like(local)
    rng = np.random.default_rng([seed, index])
    sign = lambda shape: rng.choice([-1.0, 1.0], shape)  # noqa: E731
    m = float((world - 1) * n)
    if forward:
        mu = local[0] / n
        var = np.maximum(local[1] / n - mu * mu, 0.0)
        mp = mu + rng.uniform(0.25, 1.0, C) * sign(C) * np.sqrt(var)
        vp = var * 2.0 ** rng.uniform(-1.0, 1.0, C)
        return np.stack([m * mp, m * (vp + mp * mp)])
    a = rng.uniform(-1.0, 2.0, (2, C))
    b = rng.uniform(0.25, 1.0, (2, C)) * sign((2, C))
    return (world - 1) * (a * local + b * np.abs(local).max())


def _fsum_channels(a):
    """per-channel sums of (B, C, H, W) float64 values, correctly rounded (math.fsum)"""
    import math
    rows = np.ascontiguousarray(a.transpose(1, 0, 2, 3)).reshape(a.shape[1], -1)
    return np.array([math.fsum(r) for r in rows], np.float64)


def check_sync_sums(name, local_got, z=None, bwd=None, rows_per_chunk=None):
    """The [2][C] double sums a synchronised cell hands to the all-reduce (reduce_partials_kernel's output, as the
    callback received it), against the sums of the cell's own tensors.

    Forward (z: the tapped z): [sum z, sum z^2].  Every term is exact in double (z is fp32, z^2 has 48 significant
    bits) and every add on the device is a double add: the conv epilogue sums a tile's rows per thread, across the two
    half-waves and across the tile's waves; the stem sums its block's rows; reduce_partials_kernel<double> adds the
    per-tile rows in 32 row groups and the groups in order.  The tile shape depends on the launch form, but whatever it
    is the whole is one summation tree over the cell's n local samples, so
        |got - want| <= gamma_n(2^-53) sum|terms|,
    n - 1 adds on the device plus the one rounding of the reference, which is the correctly rounded sum (math.fsum).

    Backward (bwd: bn_backward64's dict; rows_per_chunk: the plan's): [sum dy, sum dy xhat].  bn_bwd_reduce_kernel sums
    one chunk of rows_per_chunk image rows of W pixels per channel in fp32 (two accumulator sets per lane, the lanes in a
    fixed tree: a tree of depth <= rows_per_chunk W - 1), each term rounded on the way: the slope product 0.1f da (1,
    and 0.1f is 0.1 (1 + 0.25 u)), xhat = (z - mean) invstd (2; the product dy xhat enters through an fma); the x2
    transitions' 2x2 sum (2) never meets a synchronised cell but is covered.  The chunk partials are then added as
    doubles (reduce_partials_kernel<float>: 2^-53 per add, under one more u).  So
        |got - want| <= gamma_d sum|terms|,  d = rows_per_chunk W + 8,
    the bar dgamma / dbeta are held to (check_bn_backward), here on the sums before their cast to fp32."""
    local_got = np.asarray(local_got, np.float64)
    if z is not None:
        z64 = z.astype(np.float64)
        n = z.shape[0] * z.shape[2] * z.shape[3]
        sq = z64 * z64
        want = np.stack([_fsum_channels(z64), _fsum_channels(sq)])
        absum = np.stack([np.abs(z64).sum(axis=(0, 2, 3)), sq.sum(axis=(0, 2, 3))])
        return _bounded("sync sums forward", name, local_got, want, absum, n, u=U64)
    d = rows_per_chunk * bwd["dz"].shape[3] + 8
    return _bounded("sync sums backward", name, local_got, np.stack([bwd["dbeta"], bwd["dgamma"]]),
                    np.stack([bwd["s1"], bwd["s2"]]), d)


def check_running(name, z, mean_got, before, after, peer=None, world=1, unbiased=False, momentum=0.9):
    """running_mean / running_var ([2][C] fp32, `before` and `after` the step) in bn_finalize_channel's fp32 operation
    order, r' = r * momentum + s * (1.0f - momentum), every operation rounded (-ffp-contract=off).
    The mean takes s = the saved mean: bit-equal given the saved mean the device holds.  The variance takes s = the fp32
    variance, times — running_var_unbiased — (float)(N / max(N - 1, 1)) with N = world n formed in double; the fp32
    variance is not saved, the statistics check allows it 1 ulp around the float64 variance of the global batch rounded
    once, so the result must be bit-equal to the formula at that value or at one of its two fp32 neighbours.  The ratio
    is the distance in ulp of the variance that matched (0 or 1; inf: none did, or the mean differs)."""
    _, var, N = stats64(z, peer, world)
    mom = F32(momentum)
    om = F32(1.0) - mom
    want_m = ((before[0] * mom).astype(F32) + (mean_got.astype(F32) * om).astype(F32)).astype(F32)
    bad_m = int(np.count_nonzero(want_m != after[0]))
    vf = var.astype(F32)
    fac = F32(np.float64(N) / max(np.float64(N) - 1.0, 1.0)) if unbiased else None
    ulps = np.full(vf.shape, np.inf)
    for dist, v in ((1, np.nextafter(vf, F32(np.inf))), (1, np.nextafter(vf, F32(-np.inf))), (0, vf)):
        rv = (v * fac).astype(F32) if unbiased else v
        r = ((before[1] * mom).astype(F32) + (rv * om).astype(F32)).astype(F32)
        ulps = np.where(r == after[1], dist, ulps)
    bad_v = int(np.count_nonzero(np.isinf(ulps)))
    ratio = np.inf if bad_m or bad_v else float(ulps.max(initial=0.0))
    detail = "%d means, %d variances differ" % (bad_m, bad_v) if bad_m or bad_v else "variance at %d ulp" % ratio
    err = max(np.abs(want_m.astype(np.float64) - after[0]).max(initial=0.0), 0.0)
    return Result("running stats", name, ratio, ratio, err, np.abs(want_m).max(initial=0.0), detail)


def bn_backward64(z, g_out, bn, gamma_p, ups, peer=None, world=1):
    """float64 BN + leaky backward from the tapped z, output gradient (interior, at the stored resolution) and
    [mean, invstd, scale, shift]: dict of the references and their absolute-value sums.  peer, world (a synchronised
    cell): dbeta / dgamma stay the LOCAL sums; the coefficients c2, c3 of dz are (local + peer) / (world n), the means
    over the global batch; dz_local is dz with the local-only coefficients (what a kernel that missed the exchange
    would give)."""
    mean, inv, sc, sh = [bn[i].astype(np.float64).reshape(1, -1, 1, 1) for i in range(4)]
    z64 = z.astype(np.float64)
    g = g_out.astype(np.float64)
    if ups == 2:
        B, C, H2, W2 = g.shape
        g4 = g.reshape(B, C, H2 // 2, 2, W2 // 2, 2)
        da, da_abs = g4.sum(axis=(3, 5)), np.abs(g4).sum(axis=(3, 5))
    else:
        da, da_abs = g, np.abs(g)
    # the mask: sign of fmaf(z, scale, shift) — z*scale is exact in float64 and one rounding keeps the sign
    slope = np.where(z64 * sc + sh > 0, 1.0, 0.1)
    dy, dy_abs = da * slope, da_abs * slope
    xh = (z64 - mean) * inv
    n = z.shape[0] * z.shape[2] * z.shape[3]
    dbeta, s1 = dy.sum(axis=(0, 2, 3)), dy_abs.sum(axis=(0, 2, 3))
    dgamma, s2 = (dy * xh).sum(axis=(0, 2, 3)), (dy_abs * np.abs(xh)).sum(axis=(0, 2, 3))
    c1 = gamma_p.astype(np.float64).reshape(1, -1, 1, 1) * inv
    N = n * world
    g1, g2 = (dbeta, dgamma) if peer is None else (dbeta + peer[0], dgamma + peer[1])
    c2, c3 = (g1 / N).reshape(1, -1, 1, 1), (g2 / N).reshape(1, -1, 1, 1)
    dz = c1 * (dy - c2 - xh * c3)
    r = dict(dbeta=dbeta, s1=s1, dgamma=dgamma, s2=s2, dz=dz, c1=c1, c2=c2, c3=c3, dy_abs=dy_abs, xh=xh, n=n, N=N)
    if peer is not None:
        r["dz_local"] = c1 * (dy - (dbeta / n).reshape(1, -1, 1, 1) - xh * (dgamma / n).reshape(1, -1, 1, 1))
    return r


def check_bn_backward(name, z, g_out, bn, gamma_p, ups, rows_per_chunk, dgamma_got, dbeta_got, dz_got, peer=None,
                      world=1, local_got=None):
    """dgamma / dbeta: fp32 partial sums over one chunk of rows_per_chunk image rows (then float64), each term rounded
    a few times on the way (2x2 sum, slope, xhat); dz = c1 ((dy - c2) - xhat c3) from the fp32 coefficients.

    A synchronised cell (peer: the recorded [2][C] contribution of the other ranks, world: their number plus one):
    dgamma / dbeta are the LOCAL sums, to the same bar (the gradients are all-reduced later with every other one).  The
    coefficients are the global means: the device forms c2 = fl32((L^ + P) / N), N = world n, from its own local sum L^
    and the peer P.  P is an input, exact on both sides, and |L^ - L| <= gamma_d s1 (check_sync_sums), so
        |c2_dev - c2| <= gamma_d s1 / N + (u + 2 u64) |c2|
    (the double add and divide, u64 = 2^-53 each, then the cast): only the local partial sums' rounding enters, divided
    by the GLOBAL count; the same for c3 with s2.  These are e2, e3 below; with world = 1 and no peer they are the
    per-device terms unchanged.  local_got (the [2][C] sums the callback received) adds check_sync_sums' backward
    Result.  The dz Result of a cell with a peer carries extra["local_only_differs"]: whether dz_local is more than
    TWICE the bar away from dz in some element of EVERY channel of this block, so that a device that used local coefficients (within one bar
    of dz_local) could not pass."""
    r = bn_backward64(z, g_out, bn, gamma_p, ups, peer, world)
    d = rows_per_chunk * z.shape[3] + 8
    out = [_bounded("bn backward dbeta", name, dbeta_got, r["dbeta"], r["s1"], d),
           _bounded("bn backward dgamma", name, dgamma_got, r["dgamma"], r["s2"], d)]
    if local_got is not None:
        out.append(check_sync_sums(name, local_got, bwd=r, rows_per_chunk=rows_per_chunk))
    uc = U if peer is None else U + 2 * U64
    e2 = gamma(d) * r["s1"].reshape(1, -1, 1, 1) / r["N"] + uc * np.abs(r["c2"])
    e3 = gamma(d) * r["s2"].reshape(1, -1, 1, 1) / r["N"] + uc * np.abs(r["c3"])
    absum = r["dy_abs"] + np.abs(r["c2"]) + np.abs(r["xh"] * r["c3"])
    # bar = |c1| (e2 + |xhat| e3 + gamma_10 absum), written as gamma_10 * S_eff for _bounded
    s_eff = np.abs(r["c1"]) * ((e2 + np.abs(r["xh"]) * e3) / gamma(10) + absum)
    out.append(_bounded("bn backward dz", name, dz_got, r["dz"], s_eff, 10))
    if peer is not None:
        far = np.abs(r["dz_local"] - r["dz"]) > 2 * gamma(10) * s_eff
        out[-1].extra["local_only_differs"] = bool(far.any(axis=(0, 2, 3)).all())
    return out


def local_mean_differs(z, peer, world):
    """per channel: does the fp32 mean of the local samples alone lie more than 1 ulp from the fp32 global mean (so that
    a finalize that missed the exchange, or the count, fails check_stats)?"""
    lm = stats64(z)[0].astype(F32)
    gm = stats64(z, peer, world)[0].astype(F32)
    return np.abs(lm.astype(np.float64) - gm) > np.spacing(np.abs(gm)).astype(np.float64)


def wgrad64(dz, a, k, stride, sel):
    """sum_p dz[p, o] a[p*stride + tap, c] for the output channels `sel`, and the same over |dz| |a|"""
    shape = (len(sel), a.shape[1], k, k)
    dzs = _t(dz[:, sel])
    at = _t(a)
    want = torch.nn.grad.conv2d_weight(at, shape, dzs, stride=stride, padding=k // 2).numpy()
    absum = torch.nn.grad.conv2d_weight(at.abs(), shape, dzs.abs(), stride=stride, padding=k // 2).numpy()
    return want, absum


def check_wgrad(name, dz, a, k, stride, sel, got, splits, k_per_split, kind="weight gradient"):
    """split-K over the pixels: fp32 within a split of k_per_split pixels, the slabs added in fp32"""
    want, absum = wgrad64(dz, a, k, stride, sel)
    return _bounded(kind, name, got, want, absum, k_per_split + splits + 2,
                    "(%d splits x %d px)" % (splits, k_per_split))


def check_bias_grad(name, dpred, got, chunk=64):
    d = dpred.astype(np.float64)
    return _bounded("bias gradient", name, got, d.sum(axis=(0, 2, 3)), np.abs(d).sum(axis=(0, 2, 3)), chunk + 2)


def dgrad64(dz, w, stride, in_hw):
    k = w.shape[2]
    shape = (dz.shape[0], w.shape[1], in_hw[0], in_hw[1])
    want = torch.nn.grad.conv2d_input(shape, _t(w), _t(dz), stride=stride, padding=k // 2).numpy()
    absum = torch.nn.grad.conv2d_input(shape, _t(np.abs(w)), _t(np.abs(dz)), stride=stride, padding=k // 2).numpy()
    return want, absum


def check_dgrad(name, got, terms, addends=()):
    """gradient plane of a producer: sum over its consumers of convT(dz, W) restricted to the producer's channels
    [lo, lo + C), plus the skip addends.  terms: [(dz, w, stride, lo)]"""
    C, hw = got.shape[1], got.shape[2:]
    want = np.zeros(got.shape, np.float64)
    absum = np.zeros(got.shape, np.float64)
    n = 2
    for dz, w, stride, lo in terms:
        wv, av = dgrad64(dz, w[:, lo:lo + C], stride, hw)
        want += wv
        absum += av
        n += w.shape[0] * w.shape[2] * w.shape[3]
    for a in addends:
        want += a.astype(np.float64)
        absum += np.abs(a.astype(np.float64))
        n += 1
    return _bounded("data gradient", name, got, want, absum, n)


# ---------------------------------------------------------------- loss gradient
def head_grads(num_class, preds, gt_boxes, targets, ignore_iou_thresh=0.7, label_smooth=False, near=1e-6):
    """d(loss)/d(pred) by the oracle's merge_targets + loss on the device's own raw predictions (fp32 oracle math,
    float64 where it sums).  Returns (dpreds in the (B, A*P, H, W) head layout, exempt masks of the same shapes: the
    positions whose ignore-IoU decision lies within `near` of the threshold)."""
    from .yolo3_train_oracle import OracleYolo3Train
    orc = OracleYolo3Train(num_class, {}, ignore_iou_thresh=ignore_iou_thresh, label_smooth=label_smooth)
    pr = orc.split_preds(preds)
    tg = orc.merge_targets(pr["box"], gt_boxes, *targets)
    _, g = orc.loss(pr, tg)
    ious_max = O.batch_iou(pr["box"], gt_boxes).max(axis=-1, keepdims=True)
    close = (np.abs(ious_max.astype(np.float64) - ignore_iou_thresh) < near) & ~(targets[0] > 0)  # (B, N, 1)
    A, P = 3, 5 + num_class
    out, ex, n0 = [], [], 0
    for pred in preds:
        B, _, H, W = pred.shape
        n1 = n0 + H * W * A
        d = np.concatenate([g["xy"][:, n0:n1], g["wh"][:, n0:n1], g["obj"][:, n0:n1], g["cls"][:, n0:n1]], -1)
        out.append(np.ascontiguousarray(d.reshape(B, H * W, A * P).transpose(0, 2, 1).reshape(B, A * P, H, W)))
        m = np.broadcast_to(close[:, n0:n1].reshape(B, H * W, A, 1), (B, H * W, A, P)).reshape(B, H * W, A * P)
        ex.append(np.ascontiguousarray(m.transpose(0, 2, 1).reshape(B, A * P, H, W)))
        n0 = n1
    return out, ex


def check_head_grad(name, got, want, exempt, ulps=4):
    """d(loss)/d(pred): a few ulp of the terms it is formed from (sigmoid(x) - t, weighted; sign(x - t), weighted)"""
    got64, want64 = got.astype(np.float64), want.astype(np.float64)
    err = np.where(exempt, 0.0, np.abs(got64 - want64))
    bound = ulps * U * (np.abs(want64) + 2.0)  # sigmoid and targets are O(1), the box weights <= 2
    r = (err / bound).max(initial=0.0)
    return Result("loss gradient", name, r, r, err.max(initial=0.0), np.abs(want64).max(initial=0.0),
                  "%d exempt (IoU within 1e-6 of the threshold)" % int(np.count_nonzero(exempt)))


# ---------------------------------------------------------------- loss values (loss_kernel, loss_reduce_kernel)
# Rounding counts of one anchor's term, read off train_kernels.hip (bce_logits, loss_kernel) with -ffp-contract=off, in
# units of u times the term's absolute sum A.  vy_expf is pinned to 2 ulp = 4u relative (test_vy_math_against_libm);
# vy_logf on [1, 2], the only arguments the loss gives it, is within 5u relative by its code (m - 1 exact, m + 1, the
# divide, s^2, the last fma of the polynomial, p * s: 5 roundings that reach the result at full weight, the earlier
# polynomial steps are damped by s^2 <= 0.03; fe * ln2 is 0 or one exact-constant fma pair below log 2) —
# tests/test_train_cells64_sensitivity.py holds both figures on a dense grid.
#   BCE term ((relu(x) - x z) + log(1 + exp(-|x|))) * mask, A = (relu(x) + |x z| + log 2) * mask:
#     on relu(x) + |x z|:  x*z (1), the subtraction (1)                                            = 2
#     on log 2:            exp, 4u e / (1 + e) <= 2u = 2.89 u log 2; the add 1 + e, u = 1.45 u log 2;
#                          vy_logf 5u log(1 + e) <= 5 u log 2                                      <= 9.34
#     on the whole:        the outer add (1), the product with the mask (1)                        = 2
#     -> 12 (the log 2 part is the worst).  log(1 + e) -> 0 where 1 + e rounds to 1 and e -> 0 at the exp cut-off drop
#     at most u, far inside u log 2.
#   objectness: the mask is 1, 0 or obj_t itself                                                   T = 12
#   centre:     mask = weights_t * obj_t (1), two terms added (1)                                  T = 14
#   class:      mask = 1 * obj_t (exact), C terms accumulated in the thread (C - 1)                T = 11 + C
#   scale term |raw - t| * w, A = (|raw| + |t|) * w: the difference (1), w = weights_t * obj_t (1), the product (1),
#               two terms added (1)                                                                T = 4
# The label-smoothed class target is formed in fp32 exactly as the kernel forms it (one correctly rounded divide and
# subtraction of constants), so both sides hold the same z.
TREE_LEVELS = 9  # 256-term block tree: six shuffles, two adds over the four waves; and the final cast of the double sum


def loss_counts(num_class):
    """(objectness, centre, scale, class) rounding counts T of one anchor's term (derivation above)"""
    return (12, 14, 4, 11 + num_class)


def bce64(x, z):
    """the true relu(x) - x z + log1p(exp(-|x|)) in float64"""
    x, z = np.asarray(x, np.float64), np.asarray(z, np.float64)
    return np.maximum(x, 0.0) - x * z + np.log1p(np.exp(-np.abs(x)))


def _bce_abs(x, z):
    x, z = np.asarray(x, np.float64), np.asarray(z, np.float64)
    return np.maximum(x, 0.0) + np.abs(x * z) + np.log(2.0)


def smoothed_class_targets(clas_t, num_class, label_smooth):
    """class targets as loss_kernel forms them, in fp32: smooth = min(1/C, 1/40); 1 -> 1 - smooth, 0 -> smooth, -1 kept"""
    ct = np.asarray(clas_t, F32)
    if not label_smooth:
        return ct
    sm = min(F32(1.0) / F32(num_class), F32(1.0) / F32(40.0))
    ct = np.where(ct > F32(0.5), (ct - sm).astype(F32), ct)
    return np.where((ct < F32(-0.5)) | (ct > F32(0.5)), ct, sm).astype(F32)


def loss_terms64(num_class, preds, gt_boxes, targets, ignore_iou_thresh=0.7, label_smooth=False, near=1e-6):
    """Per-anchor float64 terms of the four losses on the device's own raw predictions (net.read_head(i)), targets and
    gt_boxes.  dict: terms / absum (4, B, N) in the order objectness, centre, scale, class (absum: a BCE term's
    (relu(x) + |x z| + log 2) mask, a scale term's (|raw| + |target|) weight); decision (B, N): 1 positive, -1 ignored, 0
    negative; exempt (B, N): not positive and the max IoU within `near` of the threshold without being the fp32 threshold
    itself; exempt_term (B, N): what the
    objectness term of an exempt anchor can be at most (its value as a plain negative; 0 as an ignored one);
    fractional (B, N): positives with obj_t < 1; counts: loss_counts.  The ignore decision is O.batch_iou's, in fp32 on
    the oracle's fp32 decode, as head_grads takes it; everything after it is float64 on the fp32 inputs."""
    from .yolo3_train_oracle import OracleYolo3Train
    f64 = np.float64
    orc = OracleYolo3Train(num_class, {}, ignore_iou_thresh=ignore_iou_thresh, label_smooth=label_smooth)
    obj_t, centers_t, scales_t, weights_t, clas_t = [np.asarray(t, F32) for t in targets]
    with np.errstate(invalid="ignore", over="ignore"):  # a saturated rw / rh decodes to an infinite box
        pr = orc.split_preds(preds)
        ious = O.batch_iou(pr["box"], np.asarray(gt_boxes, F32))
    ious_max = np.fmax.reduce(ious, axis=-1, keepdims=True, initial=F32(-1.0))  # fmaxf from best = -1: a NaN never wins
    pos = obj_t > 0
    ign = ~pos & (ious_max > F32(ignore_iou_thresh))
    # exempt as head_grads exempts, but for an IoU that IS the fp32 threshold bit for bit: both sides evaluate the same
    # pinned fp32 sequence on bit-equal boxes, and that value is the one point where `>` and `>=` part
    exempt = ~pos & (np.abs(ious_max.astype(f64) - ignore_iou_thresh) < near) & (ious_max != F32(ignore_iou_thresh))
    o64 = np.where(pos, obj_t, 0).astype(f64)
    hard = np.where(pos, 1.0, np.where(ign, -1.0, 0.0))
    omask = np.where(pos, o64, np.where(ign, 0.0, 1.0))
    w = weights_t.astype(f64) * o64
    ct = smoothed_class_targets(clas_t, num_class, label_smooth)
    cm = np.where(ct >= 0, 1.0, 0.0) * o64
    xo, xy, wh, xc = [pr[k].astype(f64) for k in ("obj", "xy", "wh", "cls")]
    ct64, st64 = centers_t.astype(f64), scales_t.astype(f64)
    terms = np.stack([(bce64(xo, hard) * omask).sum(-1), (bce64(xy, ct64) * w).sum(-1),
                      (np.abs(wh - st64) * w).sum(-1), (bce64(xc, ct) * cm).sum(-1)])
    absum = np.stack([(_bce_abs(xo, hard) * omask).sum(-1), (_bce_abs(xy, ct64) * w).sum(-1),
                      ((np.abs(wh) + np.abs(st64)) * w).sum(-1), (_bce_abs(xc, ct) * cm).sum(-1)])
    return dict(terms=terms, absum=absum, decision=np.where(pos, 1, np.where(ign, -1, 0))[..., 0].astype(np.int8),
                exempt=exempt[..., 0], exempt_term=np.where(exempt, bce64(xo, 0.0), 0.0)[..., 0],
                fractional=(pos & (obj_t < 1))[..., 0], counts=loss_counts(num_class), ious_max=ious_max[..., 0])


LOSS_NAMES = ("objectness", "centre", "scale", "class")


def check_losses(name, got, terms):
    """The (4, B) loss values against the float64 sums of the per-anchor terms: per image and per loss
        |got - sum terms| <= gamma(T + 9) sum A_i + sum_exempt |term|,
    T = loss_counts (one term's roundings), 9 = TREE_LEVELS: every term passes the eight add levels of its block's
    256-term tree, and the sum over the blocks, taken in double, is rounded once by the final cast.  A NaN or an
    infinite loss fails (its ratio is NaN / inf).  One Result per loss, the worst image."""
    got = np.asarray(got, np.float64)
    out = []
    for q in range(4):
        want = terms["terms"][q].sum(axis=-1)
        absum = terms["absum"][q].sum(axis=-1)
        n = terms["counts"][q] + TREE_LEVELS
        allow = terms["exempt_term"].sum(axis=-1) if q == 0 else 0.0
        err = np.abs(got[q] - want)
        bound = gamma(n) * absum + allow
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / bound)
            h = np.where(err == 0, 0.0, err / (U * np.sqrt(n) * absum + allow))
        bad = ~np.isfinite(got[q])
        r, h = np.where(bad, np.inf, r), np.where(bad, np.inf, h)
        out.append(Result("loss value", "%s %s" % (name, LOSS_NAMES[q]), r.max(initial=0.0), h.max(initial=0.0),
                          err.max(initial=0.0), np.abs(want).max(initial=0.0)))
    return out


def loss_census(terms):
    """how many anchors took each branch of the decision, how many are exempt, how many positives are fractional"""
    d = terms["decision"]
    return dict(positive=int(np.count_nonzero(d == 1)), ignored=int(np.count_nonzero(d == -1)),
                negative=int(np.count_nonzero(d == 0)), exempt=int(np.count_nonzero(terms["exempt"])),
                fractional=int(np.count_nonzero(terms["fractional"])))


# ---------------------------------------------------------------- raw predictions (raw_preds_kernel)
# Rounding count of a decoded box corner, from raw_preds_kernel: the centre (sigmoid(r) + x) * stride — exp 4u of e,
# 1 + e (1), the divide (1): sigmoid within 6u; the add of the cell offset (1); the stride is a power of two — is within
# 7u |centre|; the half extent exp(r) * anchor / 2 — exp 4u, the product (1), the halving exact — within 5u |half|;
# the corner centre -+ half adds one rounding of the result: 8u (|centre| + |half extent|) bounds both.
T_BOX = 8


def exp64_cut(x):
    """exp in float64 with vy_expf's cut-offs, which are part of the operation (vy_math.h): +inf above 88.5, 0 below -86"""
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        return np.where(x > 88.5, np.inf, np.where(x >= -86.0, np.exp(np.clip(x, -100.0, 100.0)), 0.0))


def raw_layout(preds, num_class):
    """the head planes (B, A*P, H, W), strides 32, 16, 8, as the (B, N, P) rows raw_preds_kernel walks: scale -> cell ->
    anchor; and each row's cell x, y, stride and anchor size"""
    A, P = 3, 5 + num_class
    rows, geo = [], []
    for i, pred in enumerate(preds):
        B, _, H, W = pred.shape
        rows.append(pred.reshape(B, A, P, H * W).transpose(0, 3, 1, 2).reshape(B, H * W * A, P))
        cell = np.repeat(np.arange(H * W), A)
        anc = np.tile(np.array(O.ANCHORS[::-1][i], np.float64).reshape(A, 2), (H * W, 1))
        geo.append(np.stack([cell % W, cell // W, np.full(cell.shape, float(O.STRIDES[::-1][i])), anc[:, 0], anc[:, 1]], -1))
    return np.concatenate(rows, 1), np.concatenate(geo, 0)


def check_raw_preds(name, preds, box, centers, scales, objness, class_pred):
    """The train-mode tensors of raw_preds_kernel against the head planes `preds` of the same forward: the four raw
    tensors bit-equal to the planes in the stride 32 -> 16 -> 8, cell, anchor order; every box corner within
    gamma(T_BOX) (|centre| + |half extent|) of a float64 decode of the device's raw values (exp64_cut); an infinite
    extent (the exp's cut-off, or exp(r) * anchor beyond fp32) infinite with the same sign on both sides; no NaN."""
    C = class_pred.shape[-1]
    rows, geo = raw_layout([np.asarray(p, F32) for p in preds], C)
    bits = lambda a: np.ascontiguousarray(a, F32).view(np.int32)  # noqa: E731
    out = []
    for label, got, want in (("centers", centers, rows[..., 0:2]), ("scales", scales, rows[..., 2:4]),
                             ("objness", objness, rows[..., 4:5]), ("class_pred", class_pred, rows[..., 5:])):
        got = np.asarray(got, F32)
        if got.shape != want.shape:
            out.append(Result("raw predictions", "%s %s" % (name, label), np.inf, 0.0, detail="shape %s" % (got.shape,)))
            continue
        out.append(_exact("raw predictions", "%s %s" % (name, label), bits(got), bits(want)))
    r64 = rows.astype(np.float64)
    gx, gy, stride, aw, ah = [geo[:, i][None] for i in range(5)]
    cx = (1.0 / (1.0 + exp64_cut(-r64[..., 0])) + gx) * stride
    cy = (1.0 / (1.0 + exp64_cut(-r64[..., 1])) + gy) * stride

    def half(r, anchor):
        """the extent exp(r) * anchor overflows fp32 before it is halved: beyond FLT_MAX it is infinite on the device; within
        the exp's 4u + 1 of FLT_MAX either is right (second value: that band)"""
        ext, top = exp64_cut(r) * anchor, float(np.finfo(F32).max)
        edge = np.abs(ext / top - 1.0) <= gamma(5)
        return np.where(ext > top, np.inf, ext) / 2.0, edge

    (hw, ex), (hh, ey) = half(r64[..., 2], aw), half(r64[..., 3], ah)
    want = np.stack([cx - hw, cy - hh, cx + hw, cy + hh], -1)
    scale = np.stack([np.abs(cx) + hw, np.abs(cy) + hh] * 2, -1)
    edge = np.stack([ex, ey] * 2, -1)
    got = np.asarray(box, np.float64)
    inf = np.isinf(want)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.where(inf | edge, 0.0, np.abs(got - want))
        ratio = np.where(err == 0, 0.0, err / (gamma(T_BOX) * scale))
    bad = (inf & ~edge & (got != want)) | np.isnan(got)
    ratio = np.where(bad, np.inf, ratio)
    out.append(Result("decoded boxes", name, ratio.max(initial=0.0), ratio.max(initial=0.0) * np.sqrt(T_BOX),
                      np.nanmax(err, initial=0.0), np.abs(want[~inf]).max(initial=0.0),
                      "%d infinite corners" % int(np.count_nonzero(inf))))
    return out


# ---------------------------------------------------------------- SGD (sgd_kernel)
# One element of sgd_kernel: gg = g * rescale + wd_k * w; m' = momentum * m - lr_k * gg; w' = w + m', with
# lr_k = lr * lr_mult and wd_k = wd * wd_mult formed in fp32 in the kernel.  Roundings on the way to m', per addend:
#   wd_k w:  wd_k (1), the product (1), the add to gg (1), lr_k (1), lr_k * gg (1), the subtraction (1)   = 6
#   g r:     the product (1), the add (1), lr_k (1), lr_k * gg (1), the subtraction (1)                    = 5
#   mu m:    the product (1), the subtraction (1)                                                          = 2
# so c = 6 covers every addend.  The build pins -ffp-contract=off; had the compiler fused g * rescale + (wd_k w) or
# mu m - (lr_k gg) into fmas, each fusion would drop one rounding, so the count holds either way.  lr, momentum, wd
# and rescale reach the kernel as fp32 arguments: the reference takes their fp32 values.
C_SGD = 6


class SgdRef:
    """Float64 carrier of one parameter's momentum across steps: m_0 = 0, b_0 = 0;
        m_t = mu m_{t-1} - lr_k (g r + wd_k w_{t-1}),   w_{t-1} the device's own bits,
        b_t = mu b_{t-1} + gamma(C_SGD) (mu |m_{t-1}| + lr_k (|g r| + |wd_k w_{t-1}|))
    bounds the device momentum's distance from m_t, and the step must satisfy |w_t - (w_{t-1} + m_t)| <= b_t + u |w_t|
    (the last add is rounded once).  A disabled step (grad_req 'null') leaves m, b and w as they are: bit-equal.
    lr_mult = 0 moves m only by mu m, and from m = 0 the parameter stays bit-equal."""

    def __init__(self, shape):
        self.m = np.zeros(shape, np.float64)
        self.b = np.zeros(shape, np.float64)

    def step(self, name, w_before, g, w_after, lr, momentum, wd, rescale, lr_mult, wd_mult, enabled):
        if not enabled:
            return _exact("sgd frozen", name, w_after, w_before)
        f = lambda v: np.float64(F32(v))  # noqa: E731
        mu, lr_k, wd_k, r = f(momentum), f(lr) * f(lr_mult), f(wd) * f(wd_mult), f(rescale)
        w0, g64 = w_before.astype(np.float64), g.astype(np.float64)
        m_new = mu * self.m - lr_k * (g64 * r + wd_k * w0)
        self.b = mu * self.b + gamma(C_SGD) * (mu * np.abs(self.m) + lr_k * (np.abs(g64 * r) + np.abs(wd_k * w0)))
        self.m = m_new
        w1 = w_after.astype(np.float64)
        err = np.abs(w1 - (w0 + m_new))
        bound = self.b + U * np.abs(w1)
        if lr_mult == 0 and not np.any(m_new):
            return _exact("sgd lr_mult 0", name, w_after, w_before)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound)
        ratio = np.where(np.isfinite(w1), ratio, np.inf)
        return Result("sgd step", name, ratio.max(initial=0.0), ratio.max(initial=0.0), err.max(initial=0.0),
                      np.abs(m_new).max(initial=0.0))


def summarize(results):
    """per kernel class: the worst err/bound and err/(u sqrt(n) S)"""
    by = {}
    for r in results:
        w = by.setdefault(r.kind, [-1.0, 0.0, "", 0])
        w[3] += 1
        if r.ratio > w[0]:
            w[0], w[2] = r.ratio, r.name
        w[1] = max(w[1], r.headroom)
    return {k: dict(worst_ratio=v[0], worst_cell=v[2], worst_headroom=v[1], checks=v[3]) for k, v in sorted(by.items())}
