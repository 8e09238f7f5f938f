"""-m gpu: the SyncBatchNorm statistics exchange, cell by cell, against float64 (oracle/train_cells64.py).

With a statistics callback installed the six synchronised cells (the stem and the five stride-2 convs) leave the path
tests/test_gpu_train_cells.py walks: the ordered reduce into the local sums (reduce_partials_kernel, double forward,
fp32 backward), the copy the callback receives, the count times the world size, bn_finalize_kernel (saved and running
statistics from the global sums over the global count) and bn_bwd_finalize_kernel (dgamma / dbeta from the LOCAL sums,
the three coefficient rows of dz from the GLOBAL sums over the global count).

A cell-level check needs no second process: the result of the all-reduce is an input of the cell.  One net runs one
recorded step to bind its workspace; the running statistics are read (the "before" values); a ctypes callback is
installed (vy_net_set_sync_bn) that copies the [2][C] doubles it is handed to the host ("local"), draws the other
ranks' contribution from a generator keyed by the call index (R.sync_peer: a different mean and variance in every
channel forward, a per-channel multiple plus a nonzero offset backward), writes local + peer back and returns 0.  The
checked step is the next recorded one.  The walker of test_gpu_train_cells.py then holds every synchronised cell to:
zero borders; check_sync_sums on what the callback received, forward and backward; check_stats on the global batch (1
ulp); the forward apply (bit-equal); check_running (running mean bit-equal given the saved mean, running variance
through the fp32 formula at the variance or an fp32 neighbour, the unbiased factor from the global count); dgamma /
dbeta against the local sums and dz with the global coefficients.  The first case also runs the whole unfiltered walk:
every downstream kernel meets its bar on the activations and gradients the global statistics produce.

Not vacuous: with world > 1, in every channel of every synchronised cell the float64 dz with local-only coefficients
lies more than twice the dz bar from the true one in some element, and the local-only fp32 mean lies more than 1 ulp
from the global one — conditions on the inputs, asserted from the references (at world 1 the peer is zero and they
cannot hold).  The worst err/bound per check kind of one run: profiles/syncbn_cells.txt."""
import time
import traceback

import numpy as np
import pytest

import test_gpu_train_cells as T

pytestmark = pytest.mark.gpu

# (classes, batch, height, width, world, running_var_unbiased, the whole walk as well): 2 frames of 64x64 — the
# 1024-channel cell has 2*2*2 local samples; one frame at world 3 — 4 local samples at stride 32, a hard-coded 2 or a
# count left local fails; 32-wide frames (the row chunks of the backward reduce) with the unbiased factor; a non-square
# frame; world 1 with a callback (the forced-collectives path: the all-reduce is the identity, the peer zero)
CASES = [(3, 2, 64, 64, 2, False, True), (1, 1, 64, 64, 3, False, False), (3, 3, 96, 32, 2, True, False),
         (4, 2, 128, 224, 2, False, False), (3, 2, 64, 64, 1, False, False)]
# (join, k, clips, height, width, world): the statistics count is B * k * Ho * Wo * world
WINDOW_CASE = ("max", 2, 2, 64, 64, 2)
SEED = 3


def _running(net, names):
    p = net.collect_params()
    return {n: np.stack([p[net._key(n + ".1.running_mean")].data(), p[net._key(n + ".1.running_var")].data()])
            for n in names}


def _sync_step(st, world, unbiased, H, W):
    """The checked step of a bound net `st` (a builder's dict after its first recorded step): the callback installed, one
    more recorded step on the same inputs; st gets the new taps and st["sync"]."""
    import torch
    from videoyolo_amd import _lib
    from oracle import train_cells64 as R
    net, cells = st["net"], st["cells"]
    names = R.sync_cells(cells)
    by_name = {c["name"]: c for c in cells}
    n_local = []  # local samples of each exchange, in call order
    for i, n in enumerate(names):  # the stem at stride 1, the i-th stride-2 conv at stride 2^i
        n_local.append(st["B"] * by_name[n]["fm"] * (H >> i) * (W >> i))
    n_local = n_local + n_local[::-1]
    if unbiased:
        net.set_semantics(running_var_unbiased=True)
    before = _running(net, names)
    calls, errors = [], []

    def cb(user, ptr, count):
        try:
            off = int(ptr) - net._ws.data_ptr()
            assert 0 <= off and off + 8 * count <= net._ws.numel() and count % 2 == 0, (off, count)
            view = net._ws[off:off + 8 * count].view(torch.float64)
            local = view.cpu().numpy().reshape(2, count // 2).copy()
            i = len(calls)
            peer = R.sync_peer(i, local, n_local[i], world, forward=i < len(names), seed=SEED)
            view.add_(torch.from_numpy(np.ascontiguousarray(peer.reshape(-1))).to(view.device))
            back = view.cpu().numpy().reshape(2, count // 2)
            assert np.array_equal(back, local + peer), "the write-back is not local + peer"
            calls.append(dict(local=local, peer=peer))
            return 0
        except Exception:  # surfaced as a library error: an exception cannot cross the C frame
            errors.append(traceback.format_exc())
            return 1

    keep = _lib.ALLREDUCE_CB(cb)
    net._cb_keep.append(keep)
    _lib.check(net._lib.vy_net_set_sync_bn(net._h, world, keep, None))
    x = st["frames"] if st["k"] == 1 else st["frames"].reshape((st["B"], st["k"]) + st["frames"].shape[1:])
    try:
        z_fwd, losses = T._record(net, cells, (x,), st["gt_boxes"], st["tg"])
    finally:
        assert not errors, errors[0]
    st.update(z_fwd=z_fwd, losses=losses,
              sync=dict(world=world, calls=calls, before=before, after=_running(net, names), unbiased=unbiased))
    # the call order identifies the cell: six exchanges forward, the same six reversed backward
    order = [2 * by_name[n]["cout"] for n in names]
    assert order == [64, 128, 256, 512, 1024, 2048] and [q["local"].size for q in calls] == order + order[::-1]
    assert n_local[:6] == [z_fwd[n].shape[0] * (z_fwd[n].shape[2] - 2) * (z_fwd[n].shape[3] - 2) for n in names]
    return names


def _check(st, names, world, title, full):
    t0 = time.time()
    res, _ = T._walk(st, only=set(names))
    kinds = {r.kind for r in res}
    assert kinds == {"borders", "sync sums forward", "forward stats", "forward apply", "running stats",
                     "bn backward dbeta", "bn backward dgamma", "sync sums backward", "bn backward dz"}, kinds
    assert len([r for r in res if r.kind == "bn backward dz"]) == 6
    nv = st["sync"]["nonvacuous"]
    assert sorted(nv) == sorted(names)
    if world > 1:  # (world 1: the peer is zero and global == local by construction)
        for n in names:
            assert all(b["mean"] and b["dz"] for b in nv[n]), (n, nv[n])
    assert all(r.ratio == 0 for r in res if r.kind == "forward apply")
    T._report(title, res, t0)
    if full:
        t0 = time.time()
        st["z_fwd"] = dict(st["z_keep"])
        res, _ = T._walk(st)
        T._report(title + ", every cell", res, t0, census=st["census"])


@pytest.mark.parametrize("C,B,H,W,world,unbiased,full", CASES)
def test_every_synchronised_cell_against_float64(C, B, H, W, world, unbiased, full):
    st = T._step(C, B, H, W)
    names = _sync_step(st, world, unbiased, H, W)
    st["z_keep"] = dict(st["z_fwd"])  # (the walk pops the taps it uses)
    _check(st, names, world, "SyncBN world %d, %dx%d batch %d, %d classes%s"
           % (world, H, W, B, C, ", unbiased running_var" if unbiased else ""), full)


def test_every_synchronised_window_cell_against_float64():
    join, k, B, H, W, world = WINDOW_CASE
    st = T._step_window(join, k, B, H, W, C=3)
    names = _sync_step(st, world, False, H, W)
    _check(st, names, world, "SyncBN world %d, window %s k=%d, %d clips of %dx%d" % (world, join, k, B, H, W), False)
