"""-m gpu: a hierarchical net over a whole video (hier_detect_video on YOLOV3Hier / YOLOV3HierConv: every level once per frame
position, the joins dilated; hier.hip) against the clip path of the same net, which is already pinned.

Eval-mode BatchNorm is per frame and a conv's result does not depend on the batch it sits in, so every comparison is bit
equality: detections and head tensors against `net(frames[window_indices(N, T, step)])`, every joined tap against the numpy
join of its own source tap (oracle.train_cells64's max, tests/hier_join_model.py's conv join) at the dilated operands, the
clip and training plans of the same net around a hier_detect_video call, and the bytes outside the plan's regions.

Both joins, and both forms of the dilated kernels (the chain walk, and three reads per frame under VY_HIER_CHAIN=0).  The
conv join has random weights and non-default BatchNorm tensors (test_gpu_hier_conv.join_params).  Shapes: the smallest that
reach every pool point, one non-square, one odd-sized, a video shorter than the clip, steps 1 and 2."""
import ctypes

import numpy as np
import pytest

import hier_cells
import hier_join_model as J
import test_gpu_hier as TH
import test_gpu_hier_conv as THC
import ws_guard as G

pytestmark = pytest.mark.gpu


def hier_detect_video(net, frames, **kw):
    import videoyolo_amd as vy
    return vy.hier_detect_video(net, frames, **kw)

C, CLASSES, OUT = TH.C, TH.CLASSES, TH.OUT
_host, _same = TH._host, TH._same
params = TH.params  # the module fixture: the single-frame synthetic parameters

# (hierarchical, frames of the video N, step, frames per step F, height, width)
CASES = [([3, 1, 1, 1, 1], 7, 1, 4, 64, 64), ([3, 3, 1, 1, 1], 23, 1, 4, 96, 32), ([3, 3, 1, 1, 1], 11, 2, 4, 40, 72),
         ([3, 3, 3, 1, 1], 9, 1, 4, 64, 64), ([3, 3, 3, 3, 1], 5, 1, 2, 64, 64)]
JOINS = ["max", "conv"]
TAP_CASES = [CASES[2], CASES[4]]  # step 2 on an odd size; four pools: the fourth writes route 0 into the concat plane
_REF = {}


def _id(case):
    return "%s-N%d-s%d-F%d-%dx%d" % (("".join(str(v) for v in case[0]),) + tuple(case[1:]))


def _net(params, join, hier, keep=False):
    return (THC._conv if join == "conv" else TH._hier)(params, hier, keep=keep)


def _video(n, h, w, seed=31):
    return np.random.default_rng(seed + n + h + w).standard_normal((n, 3, h, w)).astype(np.float32)


def _clip_outputs(net, frames, step, chunk=4):
    """net(frames[window_indices]) in chunks of clips, on the clip plan"""
    import torch
    from videoyolo_amd import window_indices
    idx = window_indices(len(frames), net.frames, step)
    outs = [net(frames[idx[i:i + chunk]], return_index=True) for i in range(0, len(idx), chunk)]
    return tuple(torch.cat(ts, 0).cpu() for ts in zip(*outs))


def _reference(params, join, case):
    """The clip path of a case, computed once: the video, the four outputs, and a non-vacuity check of them"""
    key = (join, _id(case))
    if key not in _REF:
        hier, n, step, f, h, w = case
        frames = _video(n, h, w)
        want = _clip_outputs(_net(params, join, hier), frames, step)
        ids = want[0].numpy()
        valid = int(((ids >= 0).any(axis=(1, 2))).sum())
        distinct = any(not np.array_equal(want[1][i].numpy(), want[1][j].numpy()) for i in range(n) for j in range(i))
        print("%s %s: %d of %d frames hold a valid row, frames differ: %s" % (key + (valid, n, distinct)))
        assert 2 * valid >= n, "the reference clip outputs hold a valid row on %d of %d frames only" % (valid, n)
        assert distinct or n == 1, "every frame's reference output is the same: equality would be vacuous"
        _REF[key] = (frames, want)
    return _REF[key]


def _equal(got, want, what):
    for name, g, r in zip(OUT, got, want):
        assert _same(g.cpu(), r.cpu()), (what, name)


# ---------------------------------------------------------------------------------------------- 1. video = clip net
@pytest.mark.parametrize("join", JOINS)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_video_equals_the_clip_net(params, join, case):
    from videoyolo_amd import window_indices
    hier, n, step, f, h, w = case
    frames, want = _reference(params, join, case)
    x0 = frames.copy()
    net = _net(params, join, hier)
    got = hier_detect_video(net, frames, step=step, frames_per_step=f, return_index=True)
    assert np.array_equal(frames, x0), "the caller's input was written"
    assert all(g.shape[0] == n for g in got)
    _equal(got, want, "host video")
    # the heads of the last chunk are the clip net's on the same centres
    heads = [net.read_head(i).clone() for i in range(3)]
    last = list(range((n - 1) // f * f, n))
    assert all(t.shape[0] == f for t in heads)
    net(frames[window_indices(n, net.frames, step)[last]])
    for i in range(3):
        assert _same(heads[i][:len(last)], net.read_head(i)), ("head", i)
    # a device video is read in place, and without return_index the first three come back
    import torch
    xd = torch.from_numpy(frames).cuda()
    plain = hier_detect_video(net, xd, step=step, frames_per_step=f)
    assert len(plain) == 3
    _equal(plain, want[:3], "device video")
    assert np.array_equal(xd.cpu().numpy(), x0), "the caller's device input was written"


# ---------------------------------------------------------------------------------------------- 2. every dilated join
@pytest.mark.parametrize("chain", [0, 1], ids=["three-read", "chain-walk"])
@pytest.mark.parametrize("join", JOINS)
@pytest.mark.parametrize("case", TAP_CASES, ids=_id)
def test_every_joined_tap_is_the_dilated_join_of_its_source_tap(monkeypatch, params, join, case, chain):
    from oracle import train_cells64 as R
    from videoyolo_amd import video
    hier, n, step, f, h, w = case
    monkeypatch.setenv("VY_HIER_CHAIN", str(chain))  # (read when the net is created)
    pools = hier_cells.n_pools(hier)
    frames, want = _reference(params, join, case)
    net = _net(params, join, hier, keep=True)
    got = hier_detect_video(net, frames, step=step, frames_per_step=f, return_index=True)
    _equal(got, want, "kept planes, chain %d" % chain)
    _, counts = video.hier_video_chunks(n, pools, step, f)
    jp = THC.join_params(pools)
    nodes = [c for c in hier_cells.hier_graph(C, hier) if R.is_pool(c)]
    assert len(nodes) == pools
    for i, c in enumerate(nodes):
        name = ("hjoin.%d" if join == "conv" else "hpool.%d") % i
        src, pooled = _host(net.read_activation(c["src"][0])), _host(net.read_activation(name))
        d, p = step * 3 ** i, counts[i + 1]
        assert src.shape[0] == counts[i] == p + 2 * d and pooled.shape == (p, c["cout"]) + src.shape[2:], (name, src.shape)
        triples = np.ascontiguousarray(np.stack([src[:p], src[d:d + p], src[2 * d:2 * d + p]], axis=1).reshape((3 * p,) + src.shape[1:]))
        if join == "max":
            r = R.check_pool_forward(name, triples, 3, "max", pooled)
            assert r.ok, r
            wins, ties = R.pool_wins(triples, 3)
            print("  %s: elements won by operand position alone %s, tied %d" % (name, wins, ties))
            assert len(wins) == 3 and min(wins) > 0, (name, wins, ties)  # every operand position wins elements on its own
        else:
            sc, sh = J.fold(*[jp["%s.1.%s" % (name, leaf)] for leaf in ("gamma", "beta", "running_mean", "running_var")])
            wj = jp[name + ".0.weight"]
            r = J.check_apply(name, J.join_z(triples, wj), sc, sh, pooled)
            assert r.ok, r
            # the operand order is visible: the same join on the operands reversed is another plane
            rev = np.ascontiguousarray(triples.reshape((p, 3) + src.shape[1:])[:, ::-1].reshape(triples.shape))
            assert not np.array_equal(J.join_apply(J.join_z(rev, wj), sc, sh), pooled), name
    assert tuple(net.read_activation("stages.0.0").shape) == (f + step * (3 ** pools - 1), 32, h, w)
    # the profile entry times the same launches under the same labels, the joins with their algorithmic bytes
    import torch
    x = torch.from_numpy(frames[video.hier_video_chunks(n, pools, step, f)[0][0][1]]).cuda()
    prof = {name: by for name, _, _, by in net._profile_video_chunk(x, step)}
    for i, c in enumerate(nodes):
        name = ("hjoin.%d" if join == "conv" else "hpool.%d") % i
        hh, ww = -(-h // 2 ** i), -(-w // 2 ** i)
        assert prof[name] == 4.0 * (counts[i] + counts[i + 1]) * c["cout"] * hh * ww, name
    assert "decode_nms" in prof and "stages.0.0" in prof
    assert net.read_head(0).shape[0] == f


# ---------------------------------------------------------------------------------------------- 3. chunk sizes, one frame
@pytest.mark.parametrize("join", JOINS)
def test_same_bits_for_every_chunk_size_and_for_one_frame(monkeypatch, params, join):
    case = CASES[2]
    hier, n, step, _, h, w = case
    frames, want = _reference(params, join, case)
    net = _net(params, join, hier)
    for f in (1, 4, 16):
        _equal(hier_detect_video(net, frames, step=step, frames_per_step=f, return_index=True), want, "F = %d" % f)
    one = frames[3:4]
    got = hier_detect_video(net, one, step=step, return_index=True)
    assert got[0].shape[0] == 1
    _equal(got, _clip_outputs(net, one, step), "N = 1")
    monkeypatch.setenv("VY_HIER_CHAIN", "0")
    base = _net(params, join, hier)
    for f in (1, 16):
        _equal(hier_detect_video(base, frames, step=step, frames_per_step=f, return_index=True), want, "three reads, F = %d" % f)


# ---------------------------------------------------------------------------------------------- 4. the other plans around it
@pytest.mark.parametrize("join", JOINS)
def test_clip_and_training_calls_bind_their_own_plans_again(params, join):
    from videoyolo_amd import _lib, autograd
    from oracle import targets_oracle as T
    hier, b, h, w = [3, 3, 1, 1, 1], 2, 64, 64
    net = _net(params, join, hier)
    clips = TH._clips(hier, b, h, w, seed=2)
    c0 = clips.copy()
    first = net(clips, return_index=True)
    frames = _video(6, h, w)
    v0 = frames.copy()
    video_out = hier_detect_video(net, frames, frames_per_step=4, return_index=True)
    # the library itself refuses the clip entry while the hier-video plan is bound
    p = ctypes.c_void_p(0x1000)
    assert net._lib.vy_net_forward_infer(net._h, p, p, p, p, None, None) == -2
    assert "vy_net_bind_hier_video" in net._lib.vy_last_error().decode()
    gt_boxes, gt_ids = T.synthetic_gt(b, min(h, w), C, m=3, seed=2, pad_to=5)
    tg = T.prefetch_targets(C, h, w, gt_boxes, gt_ids)
    with autograd.record():
        losses = net(clips, gt_boxes, *tg)
        autograd.backward([losses[0] + losses[1] + losses[2] + losses[3]])
    assert all(np.isfinite(_host(l)).all() for l in losses)
    # ... and a video entry on a clip plan
    out = net._detect_outputs(4, net._out_rows(), True)
    with pytest.raises(_lib.VyError) as e:
        _lib.check(net._lib.vy_net_hier_video_detect(net._h, p, *[ctypes.c_void_p(t.data_ptr()) for t in out], None))
    assert e.value.code == -2
    # the recorded forward moved the BatchNorm running statistics (nothing else: no optimizer step); with them put back the
    # clip call is the first one's, on a plan of its own again
    key = "stages.0.0.1.running_mean"
    assert not np.array_equal(net.collect_params()[key].data(), params[key])
    net.set_parameters(dict(params, **(THC.join_params(2) if join == "conv" else {})))
    _equal(net(clips, return_index=True), first, "the clip call after hier_detect_video and a training step")
    _equal(hier_detect_video(net, frames, frames_per_step=4, return_index=True), video_out, "hier_detect_video again")
    assert np.array_equal(clips, c0) and np.array_equal(frames, v0), "an input was written"
    # set_semantics reaches the shared tail: the video path follows the clip path
    net.set_semantics(strict_valid=False, tie_ascending=False)
    _equal(hier_detect_video(net, frames, frames_per_step=4, return_index=True), _clip_outputs(net, frames, 1), "semantics")


# ---------------------------------------------------------------------------------------------- 5. no stray byte
def _regions(net, centres, step, h, w):
    from videoyolo_amd import _lib
    table, r = [], _lib.PlanRegion()
    while True:
        rc = net._lib.vy_net_plan_region(net._h, _lib.VY_PLAN_HIER_VIDEO, centres, h, w, step, 0, len(table), ctypes.byref(r))
        if rc == _lib.VY_ERR_RANGE:
            break
        _lib.check(rc)
        table.append((r.name.decode(), int(r.offset), int(r.bytes), int(r.span)))
    G.check_table(table, int(net._lib.vy_net_hier_video_workspace_bytes(net._h, centres, step, h, w)))
    return table


@pytest.mark.parametrize("chain", [0, 1], ids=["three-read", "chain-walk"])
@pytest.mark.parametrize("join", JOINS)
@pytest.mark.parametrize("case", TAP_CASES, ids=_id)
def test_no_byte_outside_the_plans_regions_is_written(monkeypatch, params, join, case, chain):
    import torch
    hier, n, step, f, h, w = case
    frames, want = _reference(params, join, case)
    monkeypatch.setenv("VY_PLAN_GUARD", str(G.GUARD))
    monkeypatch.setenv("VY_HIER_CHAIN", str(chain))
    net = _net(params, join, hier)
    need = int(net._lib.vy_net_hier_video_workspace_bytes(net._h, f, step, h, w))
    assert need > 0
    buf, view = G.banded(need)
    net._ws = view
    with torch.cuda.device(net._device):
        net._ensure_hier_video(f, step, h, w)
    assert net._ws.data_ptr() == view.data_ptr(), "the net let go of the banded workspace"
    table = _regions(net, f, step, h, w)
    assert G.gap_bytes(table) >= G.GUARD * len(table)
    G.poison(view, table)
    got = hier_detect_video(net, frames, step=step, frames_per_step=f, return_index=True)  # every chunk on the one binding
    assert net._ws.data_ptr() == view.data_ptr()
    torch.cuda.synchronize()
    bad = G.violations(buf.cpu().numpy(), table, G.BAND)
    assert not bad, "bytes outside a region were written (region, first offset behind its used end, bytes): %s" % bad[:8]
    _equal(got, want, "guarded")
