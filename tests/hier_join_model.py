"""The numpy model of one learned join of a hierarchical net (YOLOV3HierConv; hier.hip's hier_join_* kernels), in the
arithmetic the kernels pin, and the checks the tests hold the device to.  Pooled frame n of the flat frame axis is made of
frames 3n, 3n + 1, 3n + 2; w is the library's (C, 3).

  forward   z = fmaf(w2, x2, fmaf(w1, x1, fl32(w0 x0)))                       fp32, bit for bit (R.fmaf)
  apply     y = leaky(fmaf(z, scale, shift))                                   fp32, bit for bit
  data      gx_t = fl32(w_t dz), written to frame 3n + t                       fp32, bit for bit
  weight    dw[c, t] = sum over (n, y, x) of x_t dz                            float64, with sum |x_t dz|
  BatchNorm statistics and backward are a cell's: R.stats64 / R.check_stats / R.check_bn_backward on the join's taps.

The weight gradient's bar.  hier_join_bwd_kernel forms every product x_t dz in double (two fp32 factors: exact), adds a
block's pixels in lane order in double, and the per-block rows go through the ordered column sum in double
(reduce_partials_kernel<double>: 32 row groups, then the groups in order); one cast to fp32 ends it.  The longest addition
path — pixels of a block + rows of a group + 32 — is made of double adds, 2^-53 each: for any plane this library can hold
(below 2^31 positions) the whole tree stays under 2^-22 of one fp32 unit roundoff times sum |x_t dz|.  What counts in fp32
is the cast alone, so the path has no fp32 addition and n = 0 + 1, plus one for the tree's double roundings: DW_N = 2."""
import numpy as np

import hier_cells
from oracle import train_cells64 as R

F32 = np.float32
DW_N = 2
EPS = 1e-5
_pool_graph = hier_cells.hier_graph  # (bound here: a test may put join_graph in its place for the max net's walkers)


def _triples(pre):
    pre = np.asarray(pre, F32)
    assert pre.shape[0] % 3 == 0, pre.shape
    return pre.reshape((-1, 3) + pre.shape[1:])


def _w(w, t):
    return np.asarray(w, F32)[:, t].reshape(1, -1, 1, 1)


def join_z(pre, w):
    """(3n, C, H, W) pre-pool frames -> (n, C, H, W) raw join output"""
    f = _triples(pre)
    p0 = (_w(w, 0) * f[:, 0]).astype(F32)
    return R.fmaf(_w(w, 2), f[:, 2], R.fmaf(_w(w, 1), f[:, 1], p0))


def fold(gamma, beta, mean, var, eps=EPS):
    """the eval-mode scale / shift in float32 numpy, as vy_bn_scale / vy_bn_shift (include/vy_math.h) define them"""
    gamma, beta, mean, var = [np.asarray(v, F32) for v in (gamma, beta, mean, var)]
    scale = (gamma / np.sqrt((var + F32(eps)).astype(F32)).astype(F32)).astype(F32)
    return scale, R.fmaf(-mean, scale, beta)


def join_apply(z, scale, shift):
    return R.leaky(R.fmaf(np.asarray(z, F32), np.asarray(scale, F32).reshape(1, -1, 1, 1), np.asarray(shift, F32).reshape(1, -1, 1, 1)))


def join_gx(dz, w):
    """(n, C, H, W) dz -> the (3n, C, H, W) gradient of the pre-pool frames"""
    dz = np.asarray(dz, F32)
    out = np.stack([(_w(w, t) * dz).astype(F32) for t in range(3)], axis=1)
    return np.ascontiguousarray(out.reshape((-1,) + dz.shape[1:]))


def join_dw64(pre, dz):
    """-> (dw (C, 3) float64, sum |x_t dz| (C, 3))"""
    f = _triples(pre).astype(np.float64)
    d = np.asarray(dz, np.float64)[:, None]
    p = f * d
    return p.sum(axis=(0, 3, 4)).T, np.abs(p).sum(axis=(0, 3, 4)).T


def bn_bwd_rows_per_chunk(frames, H, C):
    """image rows per partial row of bn_bwd_reduce on a join's z plane: vy_bn_bwd_rows_per_chunk (train_kernels.hip) at the
    join's geometry — ~1024 partial rows per group of 64 channel quads"""
    cq = C // 4
    groups = -(-cq // min(cq, 64))
    want = max(1024 // groups, 1)
    return -(-(frames * H) // want)


# ---------------------------------------------------------------- checks
def check_forward(name, pre, w, z_got):
    return R._exact("join forward", name, np.asarray(z_got, F32), join_z(pre, w))


def check_apply(name, z, scale, shift, out_got):
    return R._exact("join apply", name, np.asarray(out_got, F32), join_apply(z, scale, shift))


def check_data_grad(name, dz, w, gx_got):
    return R._exact("join data gradient", name, np.asarray(gx_got, F32), join_gx(dz, w))


def check_weight_grad(name, pre, dz, dw_got, n=DW_N):
    want, absum = join_dw64(pre, dz)
    return R._bounded("join weight gradient", name, dw_got, want, absum, n)


# ---------------------------------------------------------------- the cell list
def join_graph(num_class, hierarchical):
    """tests/hier_cells.py's cell list with every pool node turned into a join node "hjoin.i": still a pool node to
    R.consumers and R.is_pool (one producer in, a third of the frames out, no conv), with `join` and `bn` set — so that
    test_gpu_train_cells._record taps its z between the forward and the backward — and every reader renamed with it."""
    out, renamed = [], {}
    for c in _pool_graph(num_class, hierarchical):
        c = dict(c)
        if R.is_pool(c):
            new = c["name"].replace("hpool.", "hjoin.")
            renamed[c["name"]] = new
            c.update(name=new, join=True, bn=True)
        c["src"] = [renamed.get(p, p) for p in c["src"]]
        out.append(c)
    return out
