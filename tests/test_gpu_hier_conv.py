"""-m gpu: the hierarchical net with the learned join (YOLOV3HierConv; hier.hip's hier_join_* kernels) against the numpy
model of tests/hier_join_model.py and against what is already pinned.

Everything around a join is the max net's, so the walkers of tests/test_gpu_hier.py run here unchanged, on this net and
on the cell list of hier_join_model.join_graph: the test swaps in the net builder and the cell list, and — for the
training walk — the two pool checks of oracle.train_cells64 for the join's apply and data-gradient checks; every conv cell
keeps R's bounds at its B * fm frames.  What a join adds is checked here: z, statistics, apply, BatchNorm backward, running
statistics, the three frames' gradients and the weight gradient, borders, run-to-run identity.

Shapes are tests/test_gpu_hier.py's.  Join weights are random normal, their BatchNorm tensors random with var > 0."""
import time

import numpy as np
import pytest

import hier_cells
import hier_join_model as J
import test_gpu_hier as TH
import test_gpu_train_cells as TC

pytestmark = pytest.mark.gpu

TRAIN_CASES, INFER_CASES = TH.TRAIN_CASES, TH.INFER_CASES
C, CLASSES, OUT = TH.C, TH.CLASSES, TH.OUT
_host, _same, _id = TH._host, TH._same, TH._id
params = TH.params  # the module fixture: the single-frame synthetic parameters


def join_params(n, seed=17):
    rng = np.random.default_rng(seed)
    out = {}
    for i in range(n):
        ch = (32, 64, 128, 256)[i]
        out["hjoin.%d.0.weight" % i] = rng.standard_normal((ch, 3)).astype(np.float32)
        out["hjoin.%d.1.gamma" % i] = rng.uniform(0.5, 1.5, ch).astype(np.float32)
        out["hjoin.%d.1.beta" % i] = (0.3 * rng.standard_normal(ch)).astype(np.float32)
        out["hjoin.%d.1.running_mean" % i] = (0.3 * rng.standard_normal(ch)).astype(np.float32)
        out["hjoin.%d.1.running_var" % i] = rng.uniform(0.5, 2.0, ch).astype(np.float32)
    return out


def _conv(params, hier, keep=False, classes=CLASSES, joins=None, **kw):
    import videoyolo_amd as vy
    net = vy.YOLOV3HierConv(classes, hierarchical=hier, **kw)
    net.set_parameters(dict(params, **(join_params(hier_cells.n_pools(hier)) if joins is None else joins)))
    net.collect_params().reset_ctx("cuda:0")
    if keep:
        net.keep_activations()
    return net


@pytest.fixture
def as_conv_net(monkeypatch):
    """tests/test_gpu_hier.py's helpers build the conv-join net and walk its cell list"""
    monkeypatch.setattr(TH, "_hier", lambda prm, hier, keep=False, classes=CLASSES, **kw: _conv(prm, hier, keep, classes, **kw))
    monkeypatch.setattr(hier_cells, "hier_graph", J.join_graph)


# ---------------------------------------------------------------------------------------------- 1. inference
@pytest.mark.parametrize("case", INFER_CASES, ids=_id)
def test_stem_and_every_join_forward(params, case):
    from oracle import yolo3_oracle as O
    hier, b, h, w = case
    n = hier_cells.n_pools(hier)
    t = 3 ** n
    x = TH._clips(hier, b, h, w)
    x0 = x.copy()
    jp = join_params(n)
    net = _conv(params, hier, keep=True)
    got = net(x, return_index=True)
    assert np.array_equal(x, x0), "the caller's input was written"
    single = TH._single(params, keep=True)
    single(x.reshape((b * t, 3, h, w)))
    stem = net.read_activation("stages.0.0")
    assert tuple(stem.shape) == (b * t, 32, h, w) and _same(stem, single.read_activation("stages.0.0"))
    joins = [c for c in J.join_graph(C, hier) if c.get("join")]
    assert [c["name"] for c in joins] == ["hjoin.%d" % i for i in range(n)]
    for c, reader in zip(joins, hier_cells.POOL_CONSUMERS):
        name = c["name"]
        pre, pooled = _host(net.read_activation(c["src"][0])), _host(net.read_activation(name))
        assert pre.shape[0] == 3 * b * c["fm"] and pooled.shape == (b * c["fm"], c["cout"]) + pre.shape[2:], (name, pre.shape)
        sc, sh = J.fold(*[jp["%s.1.%s" % (name, leaf)] for leaf in ("gamma", "beta", "running_mean", "running_var")])
        r = J.check_apply(name, J.join_z(pre, jp[name + ".0.weight"]), sc, sh, pooled)
        assert r.ok, r
        assert len(np.unique(pooled)) > pooled.size // 4, name  # not a constant plane
        # the border of the joined plane is zero: the stride-2 conv that reads it is the oracle's zero-padded conv, bit for bit
        fsc, fsh = O.bn_fold(*[params["%s.1.%s" % (reader, leaf)] for leaf in ("gamma", "beta", "running_mean", "running_var")])
        want = O.conv2d(pooled, params[reader + ".0.weight"], 2, 1, fsc, fsh, leaky=True)
        assert np.array_equal(_host(net.read_activation(reader)), want), (name, reader)
    # the plan that recycles planes computes the same
    for name, g, r in zip(OUT, _conv(params, hier)(x, return_index=True), got):
        assert _same(g, r), ("recycled", name)


@pytest.mark.parametrize("case", INFER_CASES, ids=_id)
def test_inference_cells_behind_the_last_join(as_conv_net, params, case):
    """tests/test_gpu_hier.py's check on this net: every cell behind the last join bit-equal to the pinned-order oracle on
    its own input — with four pools the transition that shares the stride-8 concat plane with the joined route 0, and the
    head cell that reads both — and the detection tail vy_net_detect_heads' on the net's own heads."""
    TH.test_inference_cells_behind_the_last_pool(params, case)


# ---------------------------------------------------------------------------------------------- 2. the identity pin
def test_identity_join_is_leaky_of_the_first_frame(params):
    """w = (1, 0, 0), gamma 1, beta 0, mean 0, var = 1 - eps: scale is exactly 1 and shift exactly 0 in fp32
    (tests/test_hier_join_sensitivity.py), so every join is leaky(x_0).  On clips of identical frames the model is the
    single-frame chain with leaky() applied again at each join point, run cell by cell through the pinned-order oracle
    conv; its three head tensors go through the single-frame net's detection tail."""
    from oracle import train_cells64 as R
    from oracle import yolo3_oracle as O
    hier, b, h, w = [3, 3, 1, 1, 1], 1, 64, 64
    n, one = 2, np.float32(1)
    ident = {}
    for i in range(n):
        ch = (32, 64)[i]
        wt = np.zeros((ch, 3), np.float32)
        wt[:, 0] = 1
        ident.update({"hjoin.%d.0.weight" % i: wt, "hjoin.%d.1.gamma" % i: np.ones(ch, np.float32),
                      "hjoin.%d.1.beta" % i: np.zeros(ch, np.float32), "hjoin.%d.1.running_mean" % i: np.zeros(ch, np.float32),
                      "hjoin.%d.1.running_var" % i: np.full(ch, one - np.float32(1e-5), np.float32)})
    sc, sh = J.fold(ident["hjoin.0.1.gamma"], ident["hjoin.0.1.beta"], ident["hjoin.0.1.running_mean"], ident["hjoin.0.1.running_var"])
    assert (sc == 1).all() and not sh.any()
    x1 = np.random.default_rng(13).standard_normal((b, 3, h, w)).astype(np.float32)
    clips = np.ascontiguousarray(np.repeat(x1[:, None], 9, axis=1))
    net = _conv(params, hier, joins=ident)
    got = net(clips, return_index=True)
    act = {"image": x1}
    for c in J.join_graph(C, hier):
        a = np.concatenate([act[p] for p in c["src"]], axis=1)
        if c.get("join"):
            act[c["name"]] = R.leaky(a)
            continue
        pre = c["name"]
        if c["bn"]:
            fsc, fsh = O.bn_fold(*[params["%s.1.%s" % (pre, leaf)] for leaf in ("gamma", "beta", "running_mean", "running_var")])
            v = O.conv2d(a, params[pre + ".0.weight"], c["s"], c["k"] // 2, fsc, fsh, leaky=True)
            if c["skip"]:
                v = (v + act[c["skip"]]).astype(np.float32)
            if c["ups"] == 2:
                v = R.upsample2(v)
        else:
            v = O.conv2d(a, params[pre + ".weight"], 1, 0, None, params[pre + ".bias"], leaky=False)
        act[pre] = v
    assert not np.array_equal(act["hjoin.0"], act["stages.0.0"])  # leaky twice is not leaky once: the join is visible
    heads = [act["yolo_outputs.%d.prediction" % i] for i in range(3)]
    for i in range(3):
        assert np.array_equal(_host(net.read_head(i)), heads[i]), i
    want = TH._single(params).detect_heads(heads, (h, w), return_index=True)
    for name, g, r in zip(OUT, got, want):
        assert _same(g, r), name


# ---------------------------------------------------------------------------------------------- 3. one training step
def _rec(net, x, gt_boxes, tg):
    from videoyolo_amd import autograd
    with autograd.record():
        losses = net(x, gt_boxes, *tg)
        autograd.backward([losses[0] + losses[1] + losses[2] + losses[3]])
    return losses


def _join_grads(net, n):
    return {k: net.grad(k) for i in range(n) for k in ("hjoin.%d.0.weight" % i, "hjoin.%d.1.gamma" % i, "hjoin.%d.1.beta" % i)}


def _step(hier, B, H, W, classes=3, seed=7):
    """As tests/test_gpu_hier.py's _step, on the conv-join net — after one step on OTHER frames, so that every gradient plane
    holds an earlier step's values when the recorded step writes it."""
    n = hier_cells.n_pools(hier)
    T = 3 ** n
    prm, gt_boxes, tg = TC._inputs(classes, B, H, W, seed)
    prm = dict(prm, **join_params(n))
    rng = np.random.default_rng(seed + H + W + T)
    x, earlier = [rng.standard_normal((B, T, 3, H, W)).astype(np.float32) for _ in range(2)]
    net = _conv(prm, hier, classes=["c%d" % i for i in range(classes)], joins={})
    _rec(net, earlier, gt_boxes, tg)
    stale = _host(net.read_train_tap("stages.0.0", "grad")).copy()
    running = {"hjoin.%d" % i: np.stack([net.collect_params()["hjoin.%d.1.%s" % (i, leaf)].data()
                                         for leaf in ("running_mean", "running_var")]) for i in range(n)}
    cells = J.join_graph(classes, hier)
    z_fwd, losses = TC._record(net, cells, (x,), gt_boxes, tg)
    return dict(net=net, params=prm, cells=cells, frames=x.reshape((B * T, 3, H, W)), gt_boxes=gt_boxes, tg=tg, z_fwd=z_fwd,
                losses=losses, C=classes, B=B, T=T, x=x, running=running, stale=stale)


@pytest.mark.parametrize("case", TRAIN_CASES, ids=_id)
def test_every_training_cell_and_join_against_float64(monkeypatch, case):
    from oracle import train_cells64 as R
    hier, B, H, W = case
    n = hier_cells.n_pools(hier)
    t0 = time.time()
    st = _step(hier, B, H, W)
    net, prm = st["net"], st["params"]
    jz = {c["name"]: _host(st["z_fwd"][c["name"]]) for c in st["cells"] if c.get("join")}  # z, tapped before the backward

    def tap(name, which):
        return _host(net.read_train_tap(name, which))

    # the two pool checks of TH._walk, on a join: the apply pass into the joined plane, and the three frames' gradients
    def apply_check(name, pre, k, join, pooled):
        bn = tap(name, "bn")
        return J.check_apply(name, R.interior(jz[name]), bn[2], bn[3], pooled)

    def data_grad_check(name, g_pool, pre, pooled, k, join, gx):
        return J.check_data_grad(name, R.interior(tap(name, "z")), prm[name + ".0.weight"], gx), [1, 1, 1], 0

    monkeypatch.setattr(R, "check_pool_forward", apply_check)
    monkeypatch.setattr(R, "check_pool_backward", data_grad_check)
    res, pools = TH._walk(st)
    monkeypatch.undo()
    assert sorted(pools) == ["hjoin.%d" % i for i in range(n)]
    for c in st["cells"]:
        if not c.get("join"):
            continue
        name = c["name"]
        frames = B * c["fm"]
        pre = R.interior(tap(name, "input"))
        zf_pad, dz_pad = jz[name], tap(name, "z")
        assert zf_pad.shape == dz_pad.shape == (frames, c["cout"], pre.shape[2] + 2, pre.shape[3] + 2), (name, zf_pad.shape)
        res.append(R.border_zero("borders", name + " z", zf_pad))
        res.append(R.border_zero("borders", name + " dz", dz_pad))
        z, dz = np.ascontiguousarray(R.interior(zf_pad)), np.ascontiguousarray(R.interior(dz_pad))
        wj, gam, bet = prm[name + ".0.weight"], prm[name + ".1.gamma"], prm[name + ".1.beta"]
        res.append(J.check_forward(name, pre, wj, z))
        bn = tap(name, "bn")
        res.append(R.check_stats(name, z, bn[0], bn[1], gam, bet, bn[2], bn[3]))  # the count is B * fm * H * W
        res.append(R.check_apply(name, z, bn[2], bn[3], _host(net.read_activation(name))))
        g = _host(net.read_grad_activation(name))
        rpc = J.bn_bwd_rows_per_chunk(frames, z.shape[2], c["cout"])
        res += R.check_bn_backward(name, z, g, bn, gam, 1, rpc, net.grad(name + ".1.gamma"), net.grad(name + ".1.beta"), dz)
        after = np.stack([net.collect_params()["%s.1.%s" % (name, leaf)].data() for leaf in ("running_mean", "running_var")])
        assert not np.array_equal(after, st["running"][name]), name
        res.append(R.check_running(name, z, bn[0], st["running"][name], after))
        # gx_t = fl32(w_t dz) for all three frames: written over the earlier step's gradient plane (checked in the walk);
        # dw within DW_N roundings of float64
        res.append(J.check_weight_grad(name, pre, dz, net.grad(name + ".0.weight")))
        assert np.count_nonzero(dz) and np.count_nonzero(net.grad(name + ".0.weight")), name
    TC._report("hier conv %s, %d clips of %dx%d" % (hier, B, H, W), res, t0, census=st["census"])
    assert np.count_nonzero(R.interior(st["stale"])), "the earlier step left no gradient in the first pre-pool plane"
    kinds = {}
    for r in res:
        kinds.setdefault(r.kind, set()).add(r.name)
    want = {"hjoin.%d" % i for i in range(n)}
    for kind in ("join forward", "join apply", "join data gradient", "join weight gradient", "forward stats", "forward apply",
                 "bn backward dz", "bn backward dgamma", "bn backward dbeta", "running stats"):
        assert want <= kinds.get(kind, set()), (kind, kinds.get(kind))
    assert {"forward conv", "data gradient", "weight gradient", "loss value"} <= set(kinds)
    assert bool(st.get("route0_sum")) == (n == 4)
    # the same step again: the joins' gradients bit for bit
    first = _join_grads(net, n)
    _rec(net, st["x"], st["gt_boxes"], st["tg"])
    for k, v in _join_grads(net, n).items():
        assert np.array_equal(v, first[k]), k


# ---------------------------------------------------------------------------------------------- 4. defaults, optimizer
def _targets(b, h, w):
    from oracle import targets_oracle as T
    gt_boxes, gt_ids = T.synthetic_gt(b, min(h, w), C, m=3, seed=2, pad_to=5)
    return gt_boxes, T.prefetch_targets(C, h, w, gt_boxes, gt_ids)


def test_default_initialisation_joins_are_constant_planes_with_live_gradients():
    """initialize(): zero join weights (the reference's choice), so z = 0, the batch statistics are (0, 0) and the joined
    plane is leaky(beta) everywhere — while the weight gradient, sum x_t dz, is not zero."""
    import videoyolo_amd as vy
    from oracle import train_cells64 as R
    hier, b, h, w = [3, 1, 1, 1, 1], 2, 64, 64
    net = vy.YOLOV3HierConv(CLASSES, hierarchical=hier)
    net.initialize(seed=3)
    beta = (0.3 * np.random.default_rng(5).standard_normal(32)).astype(np.float32)
    net.collect_params()["hjoin.0.1.beta"].set_data(beta)
    net.collect_params().reset_ctx("cuda:0")
    gt_boxes, tg = _targets(b, h, w)
    losses = _rec(net, TH._clips(hier, b, h, w, seed=3), gt_boxes, tg)
    assert all(np.isfinite(_host(l)).all() for l in losses)
    pooled = _host(net.read_activation("hjoin.0"))
    want = np.broadcast_to(R.leaky(beta).reshape(1, -1, 1, 1), pooled.shape)
    assert np.array_equal(pooled, want)
    for k in net.collect_params():
        if net.collect_params()[k].trainable:
            assert np.isfinite(net.grad(k)).all(), k
    assert np.count_nonzero(net.grad("hjoin.0.0.weight"))


def test_the_optimizer_moves_the_joins_and_freeze_base_holds_them(params):
    import videoyolo_amd as vy
    hier, b, h, w = [3, 3, 1, 1, 1], 2, 64, 64
    x = TH._clips(hier, b, h, w, seed=3)
    gt_boxes, tg = _targets(b, h, w)
    prm = dict(params, **join_params(2))
    net = _conv(params, hier)
    trainer = vy.Trainer(net.collect_params(), "sgd", {"learning_rate": 1e-3, "wd": 5e-4, "momentum": 0.9})
    assert all(np.isfinite(_host(l)).all() for l in _rec(net, x, gt_boxes, tg))
    trainer.step(b)
    P = net.collect_params()
    for i in range(2):
        for leaf in ("0.weight", "1.gamma", "1.beta", "1.running_mean", "1.running_var"):
            key = "hjoin.%d.%s" % (i, leaf)
            assert not np.array_equal(P[key].data(), prm[key]), key
    assert not np.array_equal(P["stages.0.1.0.weight"].data(), prm["stages.0.1.0.weight"])
    frozen = _conv(params, hier)
    for p in frozen.collect_params().values():  # wrappers.py:55-57, what freeze_base=True does
        if p.backbone:
            p.grad_req = "null"
    trainer = vy.Trainer(frozen.collect_params(), "sgd", {"learning_rate": 1e-3, "wd": 5e-4, "momentum": 0.9})
    _rec(frozen, x, gt_boxes, tg)
    trainer.step(b)
    for key, p in frozen.collect_params().items():
        if p.backbone and p.trainable:
            assert np.array_equal(p.data(), prm[key]), key
    assert sum(k.startswith("hjoin.") and p.trainable for k, p in frozen.collect_params().items()) == 6
    assert not np.array_equal(frozen.collect_params()["yolo_blocks.0.tip.0.weight"].data(), prm["yolo_blocks.0.tip.0.weight"])


# ---------------------------------------------------------------------------------------------- 5. the workspace guard
@pytest.mark.parametrize("hier,shape", [([3, 1, 1, 1, 1], (2, 64, 64)), ([3, 3, 3, 3, 1], (1, 64, 64))], ids=str)
def test_no_launch_leaves_its_region(monkeypatch, hier, shape):
    """tests/test_gpu_ws_guard.py's case frame on the conv-join net: inference under the clip plan and one training step
    under the training plan, with a poisoned gap behind every region — the joins' z planes among them."""
    import test_gpu_ws_guard as WG
    b, h, w = shape
    n = hier_cells.n_pools(hier)

    def make():
        return _conv(WG._synthetic(20), hier)

    g = WG._run_case("hier conv %s" % hier, monkeypatch, {}, make, shape, [WG._normal((b, 3 ** n, 3, h, w), 11)],
                     tg=WG._targets(20, b, h, w), train=True)
    assert any(r[0] == "z:hjoin.0" for r in g.table) and g.checked > 0
