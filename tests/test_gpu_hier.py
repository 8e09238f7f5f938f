"""-m gpu: the hierarchical net (yolo3_darknet53 with new_model=True, hierarchical=[3,..,1], h_join_type='max'; hier.hip)
against what is already pinned.

The conv list is the single-frame net's and every launch has the geometry of a single-frame net at B * fm frames, so
the bars are the project's own: bit-equality wherever the arithmetic is pinned (identical frames against the single-frame
net, the stem, every pool forward and backward against oracle.train_cells64's numpy pool on the device's own planes, the
inference cells behind the last pool against the pinned-order CPU oracle on their own inputs, the detection tail against
vy_net_detect_heads) and oracle/train_cells64.py's float64 bounds, unchanged, for every kernel of one training step, cell
by cell, each cell at its own B * fm frames.  The cell list is tests/hier_cells.py's.

Shapes: the smallest that reach every pool point and both situations of route 0 (a cell's output with one, two or three
pools; the fourth pooled plane itself with four), one of them non-square, one with odd sizes (inference only: the cropped
upsample)."""
import time
import zlib

import numpy as np
import pytest

import hier_cells
import test_gpu_train_cells as TC

pytestmark = pytest.mark.gpu

# (hierarchical, clips, height, width)
TRAIN_CASES = [([3, 1, 1, 1, 1], 2, 64, 64), ([3, 3, 1, 1, 1], 2, 96, 32), ([3, 3, 3, 3, 1], 1, 64, 64)]
INFER_CASES = TRAIN_CASES + [([3, 3, 1, 1, 1], 1, 40, 72)]
C = 20
CLASSES = ["c%d" % i for i in range(C)]
OUT = ("ids", "scores", "bboxes", "keep_idx")


def _id(case):
    return "%s-%dx%dx%d" % ("".join(str(v) for v in case[0]), case[1], case[2], case[3])


def _host(t):
    return t.detach().cpu().numpy()


def _bits(t):
    import torch
    return t.detach().contiguous().view(torch.int32).cpu()


def _same(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def params():
    from videoyolo_amd import init
    from oracle import yolo3_oracle as O
    return init.synthetic_params(O.param_shapes(C), seed=233)


def _single(params, keep=False, classes=CLASSES):
    import videoyolo_amd as vy
    net = vy.yolo3_darknet53(classes, pretrained_base=False)
    net.set_parameters(params)
    net.collect_params().reset_ctx("cuda:0")
    if keep:
        net.keep_activations()
    return net


def _hier(params, hier, keep=False, classes=CLASSES, **kw):
    import videoyolo_amd as vy
    net = vy.yolo3_darknet53(classes, pretrained_base=False, new_model=True, hierarchical=hier, h_join_type="max", **kw)
    assert isinstance(net, vy.YOLOV3Hier)
    net.set_parameters(params)  # a single-frame parameter dict, as it is
    net.collect_params().reset_ctx("cuda:0")
    if keep:
        net.keep_activations()
    return net


def _clips(hier, b, h, w, seed=5):
    t = 3 ** hier_cells.n_pools(hier)
    return np.random.default_rng(seed + h + w + t).standard_normal((b, t, 3, h, w)).astype(np.float32)


# ---------------------------------------------------------------------------------------------- 1. identical frames
@pytest.mark.parametrize("case", INFER_CASES, ids=_id)
def test_identical_frames_detect_as_the_single_frame_net(params, case):
    """T copies of a frame: every max returns its (earliest) operand, so the detections and the three head tensors are the
    single-frame net's bits — in the recycled-plane plan, the one inference runs by default."""
    hier, b, h, w = case
    t = 3 ** hier_cells.n_pools(hier)
    x1 = np.random.default_rng(9 + h).standard_normal((b, 3, h, w)).astype(np.float32)
    clips = np.ascontiguousarray(np.repeat(x1[:, None], t, axis=1))
    single, net = _single(params), _hier(params, hier)
    want = single(x1, return_index=True)
    got = net(clips, return_index=True)
    for name, g, r in zip(OUT, got, want):
        assert _same(g, r), name
    for i in range(3):
        assert _same(net.read_head(i), single.read_head(i)), i


# ---------------------------------------------------------------------------------------------- 2-3. stem, pools
@pytest.mark.parametrize("case", INFER_CASES, ids=_id)
def test_stem_and_every_pool_forward(params, case):
    from oracle import train_cells64 as R
    hier, b, h, w = case
    n = hier_cells.n_pools(hier)
    t = 3 ** n
    x = _clips(hier, b, h, w)
    x0 = x.copy()
    net = _hier(params, hier, keep=True)
    got = net(x, return_index=True)
    assert np.array_equal(x, x0), "the caller's input was written"
    # the stem at B * T frames is the single-frame net's on the same frames
    single = _single(params, keep=True)
    single(x.reshape((b * t, 3, h, w)))
    stem = net.read_activation("stages.0.0")
    assert tuple(stem.shape) == (b * t, 32, h, w)
    assert _same(stem, single.read_activation("stages.0.0"))
    cells = hier_cells.hier_graph(C, hier)
    pools = [c for c in cells if R.is_pool(c)]
    assert [c["name"] for c in pools] == ["hpool.%d" % i for i in range(n)]
    for c in pools:
        pre, pooled = _host(net.read_activation(c["src"][0])), _host(net.read_activation(c["name"]))
        assert pre.shape[0] == 3 * b * c["fm"] and pooled.shape == (b * c["fm"],) + pre.shape[1:], (c["name"], pre.shape)
        assert pooled.shape[1] == c["cout"]
        r = R.check_pool_forward(c["name"], pre, 3, "max", pooled)
        assert r.ok, r
        wins, ties = R.pool_wins(pre, 3)
        assert len(wins) == 3 and min(wins) > 0, (c["name"], wins, ties)  # every frame position wins elements on its own
    # the plan that recycles planes computes the same
    for name, g, r in zip(OUT, _hier(params, hier)(x, return_index=True), got):
        assert _same(g, r), ("recycled", name)


# ---------------------------------------------------------------------------------------------- 4. the inference tail
@pytest.mark.parametrize("case", INFER_CASES, ids=_id)
def test_inference_cells_behind_the_last_pool(params, case):
    """From the last pooled plane on the net is the single-frame net on B clips: every cell behind the last pool is
    bit-equal to the pinned-order CPU oracle's cell (folded BatchNorm, leaky, residual add, x2 upsample cropped to its
    route) on the very planes the device's taps return as its input, and the detection tail is vy_net_detect_heads' on
    the net's own three head tensors."""
    from oracle import train_cells64 as R
    from oracle import yolo3_oracle as O
    hier, b, h, w = case
    x = _clips(hier, b, h, w, seed=11)
    net = _hier(params, hier, keep=True)
    outs = net(x, return_index=True)
    cells = hier_cells.hier_graph(C, hier)
    last = max(i for i, c in enumerate(cells) if R.is_pool(c))
    act = {}

    def tap(name):
        if name not in act:
            act[name] = _host(net.read_activation(name))
        return act[name]

    checked = 0
    for c in cells[last + 1:]:
        assert c["fm"] == 1, c["name"]
        a = np.concatenate([tap(p) for p in c["src"]], axis=1)
        assert a.shape[0] == b and a.shape[1] == c["cin"], (c["name"], a.shape)
        got = tap(c["name"])
        if c["bn"]:
            pre = c["name"]
            sc, sh = O.bn_fold(params[pre + ".1.gamma"], params[pre + ".1.beta"], params[pre + ".1.running_mean"],
                               params[pre + ".1.running_var"])
            want = O.conv2d(a, params[pre + ".0.weight"], c["s"], c["k"] // 2, sc, sh, leaky=True)
            if c["skip"]:
                want = (want + tap(c["skip"])).astype(np.float32)
            if c["ups"] == 2:
                want = R.upsample2(want)[:, :, :got.shape[2], :got.shape[3]]
        else:
            want = O.conv2d(a, params[c["name"] + ".weight"], 1, 0, None, params[c["name"] + ".bias"], leaky=False)
        r = R._exact("inference cell", c["name"], got, np.ascontiguousarray(want))
        assert r.ok, r
        checked += 1
    assert checked == len(cells) - last - 1 >= 49
    heads = [net.read_head(i) for i in range(3)]
    for i in range(3):
        assert np.array_equal(_host(heads[i]), tap("yolo_outputs.%d.prediction" % i)), i
    again = net.detect_heads(heads, (h, w), return_index=True)
    for name, g, r in zip(OUT, again, outs):
        assert _same(g, r), name


# ---------------------------------------------------------------------------------------------- 5. one training step
def _step(hier, B, H, W, classes=3, seed=7, x=None):
    """One recorded step of the hierarchical net on B clips (random-normal frames unless given), in the dict the walker of
    tests/test_gpu_train_cells.py builds for its nets."""
    import videoyolo_amd as vy
    T = 3 ** hier_cells.n_pools(hier)
    prm, gt_boxes, tg = TC._inputs(classes, B, H, W, seed)
    if x is None:
        x = np.random.default_rng(seed + H + W + T).standard_normal((B, T, 3, H, W)).astype(np.float32)
    net = vy.yolo3_darknet53(["c%d" % i for i in range(classes)], pretrained_base=False, new_model=True, hierarchical=hier,
                             h_join_type="max")
    net.set_parameters(prm)
    net.collect_params().reset_ctx("cuda:0")
    cells = hier_cells.hier_graph(classes, hier)
    z_fwd, losses = TC._record(net, [c for c in cells if not c.get("pool")], (x,), gt_boxes, tg)
    return dict(net=net, params=prm, cells=cells, frames=x.reshape((B * T, 3, H, W)), gt_boxes=gt_boxes, tg=tg, z_fwd=z_fwd,
                losses=losses, C=classes, B=B, T=T)


def _walk(st):
    """Every check of one recorded step: the checks of tests/test_gpu_train_cells.py's walker with its bounds, each cell
    at B * fm frames (so the statistics count is B * fm * H * W), and for the pool nodes: forward and backward bit-equal
    to the numpy pool on the device's own planes, the borders of the pooled plane and of both gradient planes zero, the
    pooled plane's gradient held as the sum of its consumers' data gradients.  -> (results, {pool: (wins, ties)})"""
    from oracle import train_cells64 as R
    net, params, cells, z_fwd = st["net"], st["params"], st["cells"], st["z_fwd"]
    C_, B = st["C"], st["B"]
    by_name = {c["name"]: c for c in cells}
    cons, skips = R.consumers(cells)
    res, pools = [], {}

    def tap(name, which):
        return _host(net.read_train_tap(name, which))

    def act(name):
        return _host(net.read_activation(name))

    for c in cells:
        name = c["name"]
        if R.is_pool(c):
            pre_pad = tap(name, "input")  # the pre-pool plane, border included
            pre, pooled = R.interior(pre_pad), act(name)
            assert pre.shape[0] == 3 * B * c["fm"] and pooled.shape[0] == B * c["fm"], (name, pre.shape, pooled.shape)
            res.append(R._exact("pre-pool view", name, pre, act(c["src"][0])))
            res.append(R.border_zero("borders", name + " pre-pool", pre_pad))
            res.append(R.check_pool_forward(name, pre, 3, "max", pooled))
            g_pad = tap(name, "grad")  # the pooled plane's gradient (route 0 of four pools: its channels of the concat)
            res.append(R.border_zero("borders", name + " grad", g_pad))
            g_pool = _host(net.read_grad_activation(name))
            res.append(R._exact("pooled gradient view", name, R.interior(g_pad), g_pool))
            assert np.count_nonzero(g_pool), name + ": the pooled gradient is zero everywhere"
            # hier_pool_bwd: the whole pre-pool gradient plane, written (never accumulated: nothing else writes it)
            r, wins, ties = R.check_pool_backward(name, g_pool, pre, pooled, 3, "max", R.interior(tap(c["src"][0], "grad")))
            res.append(r)
            pools[name] = (wins, ties)
            continue
        kk, s = c["k"], c["s"]
        sel_img = TC._sel(B, c["fm"])
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        sel_o = sorted({0, c["cout"] - 1} | set(rng.choice(c["cout"], size=min(6, c["cout"]), replace=False).tolist()))
        g_pad = tap(name, "grad")
        assert g_pad.shape[0] == B * c["fm"], (name, g_pad.shape)
        res.append(R.border_zero("borders", name + " grad", g_pad))
        g = R.interior(g_pad)
        if c["src"] == ["image"]:
            a = st["frames"]
        else:
            a_pad = tap(name, "input")
            res.append(R.border_zero("borders", name + " input", a_pad))  # a pooled plane's border among them
            a = np.ascontiguousarray(R.interior(a_pad))
            off = 0
            for p in c["src"]:  # the view a conv reads of a pooled plane holds the pool's bits
                if p.startswith("hpool."):
                    src = act(p)
                    res.append(R._exact("pooled view", name + " <- " + p, a[:, off:off + src.shape[1]], src))
                off += by_name[p]["cout"]
        assert a.shape[0] == B * c["fm"], (name, a.shape)
        wname = name + (".0.weight" if c["bn"] else ".weight")
        w = params[wname]
        plan = net.train_conv_plan(name)
        if not c["bn"]:
            res.append(R.check_bias_grad(name, g, net.grad(name + ".bias")))
            res.append(R.check_wgrad(name, g, a, kk, s, sel_o, net.grad(wname)[sel_o], plan[0], plan[1]))
            continue
        zf_pad = _host(z_fwd.pop(name))
        dz_pad = tap(name, "z")
        res.append(R.border_zero("borders", name + " z", zf_pad))
        res.append(R.border_zero("borders", name + " dz", dz_pad))
        z, dz = np.ascontiguousarray(R.interior(zf_pad)), np.ascontiguousarray(R.interior(dz_pad))
        assert z.shape[0] == B * c["fm"], (name, z.shape)  # the statistics count is B * fm * H * W
        bn = tap(name, "bn")
        gam, bet = params[name + ".1.gamma"], params[name + ".1.beta"]
        out = act(name)
        skip = act(c["skip"]) if c["skip"] else None
        res.append(R.check_forward_conv(name, a[sel_img], w, s, z[sel_img]))
        res.append(R.check_stats(name, z, bn[0], bn[1], gam, bet, bn[2], bn[3]))
        res.append(R.check_apply(name, z, bn[2], bn[3], out, skip, c["ups"]))
        res += R.check_bn_backward(name, z, g, bn, gam, c["ups"], plan[2], net.grad(name + ".1.gamma"),
                                   net.grad(name + ".1.beta"), dz)
        if c["src"] == ["image"]:
            res.append(R.check_wgrad(name, dz, a, kk, s, list(range(c["cout"])), net.grad(wname), plan[0], plan[1],
                                     kind="stem weight gradient"))
        else:
            res.append(R.check_wgrad(name, dz, a, kk, s, sel_o, net.grad(wname)[sel_o], plan[0], plan[1]))

    # data gradients: every producer's gradient plane as the sum of its conv consumers' (a pre-pool plane's only consumer
    # is the pool: checked bit for bit above), first and last clip, all fm frames of each
    for c in cells:
        name = c["name"]
        if name not in cons or all(R.is_pool(q) for q, _ in cons[name]):
            continue
        assert not any(R.is_pool(q) for q, _ in cons[name]), name
        sel_img = TC._sel(B, c["fm"])
        if R.is_pool(c):
            got = _host(net.read_grad_activation(name))[sel_img]
        else:
            got = R.interior(tap(name, "grad"))[sel_img]
        adds = [R.interior(tap(q["name"], "grad"))[sel_img] for q in skips.get(name, [])]
        terms = []
        for q, lo in cons[name]:
            dzq = R.interior(tap(q["name"], "z" if q["bn"] else "grad"))[sel_img]
            terms.append((dzq, params[q["name"] + (".0.weight" if q["bn"] else ".weight")], q["s"], lo))
        res.append(R.check_dgrad(name, got, terms, adds))
        if R.is_pool(c) and len(terms) == 2:
            # route 0 of a four-pool net: stages.1.0's data gradient PLUS the stride-8 head's, held above as the sum of both
            # consumers' terms with both depths in the bound (the device adds the second onto the first in place, so neither
            # is available on its own as an exact addend).  An overwrite either way — one consumer's term missing — must fail
            for i in (0, 1):
                alone = R.check_dgrad(name, got, [terms[i]])
                assert not alone.ok, "an overwrite by %s would pass: %r" % (cons[name][i][0]["name"], alone)
            st["route0_sum"] = True

    preds = [_host(net.read_head(i)) for i in range(3)]
    targets = [np.asarray(t) for t in st["tg"]]
    want, exempt = R.head_grads(C_, preds, st["gt_boxes"], targets)
    for i in range(3):
        name = "yolo_outputs.%d.prediction" % i
        res.append(R.check_head_grad(name, R.interior(tap(name, "grad")), want[i], exempt[i]))
    terms = R.loss_terms64(C_, preds, st["gt_boxes"], targets)
    res += R.check_losses("losses", st["losses"], terms)
    st["census"] = R.loss_census(terms)
    return res, pools


@pytest.mark.parametrize("case", TRAIN_CASES, ids=_id)
def test_every_training_cell_against_float64(case):
    hier, B, H, W = case
    t0 = time.time()
    st = _step(hier, B, H, W)
    res, pools = _walk(st)
    n = hier_cells.n_pools(hier)
    TC._report("hier %s, %d clips of %dx%d" % (hier, B, H, W), res, t0, census=st["census"])
    for name, (wins, ties) in sorted(pools.items()):
        print("  %s: elements won by frame position t alone %s, tied %d" % (name, wins, ties))
    # not vacuous: every pool ran both ways, and every frame position wins elements at every pool point (a gradient sent
    # to the wrong frame, or to all three, cannot pass)
    assert sorted(pools) == ["hpool.%d" % i for i in range(n)]
    for name, (wins, ties) in pools.items():
        assert len(wins) == 3 and min(wins) > 0, (name, wins, ties)
    kinds = {r.kind for r in res}
    assert {"pool forward", "pool backward", "forward stats", "data gradient", "weight gradient", "loss value"} <= kinds
    assert bool(st.get("route0_sum")) == (n == 4)


# ---------------------------------------------------------------------------------------------- 6. ties
def test_tied_frames_both_get_the_full_gradient():
    """Frames 0 and 1 of every triple identical, the third distinct: at the first pool hier_pool_bwd gives the full pooled
    gradient to BOTH tied frames wherever they hold the max, and +0 to the third there — bit-equal to pool_backward."""
    from oracle import train_cells64 as R
    hier, B, H, W = [3, 3, 1, 1, 1], 1, 64, 64
    x = np.random.default_rng(21).standard_normal((B, 9, 3, H, W)).astype(np.float32)
    x[:, 1::3] = x[:, 0::3]
    st = _step(hier, B, H, W, x=x)
    net = st["net"]
    pre = _host(net.read_activation("stages.0.0"))
    pooled = _host(net.read_activation("hpool.0"))
    g_pool = _host(net.read_grad_activation("hpool.0"))
    got = _host(net.read_grad_activation("stages.0.0"))
    assert pre.shape[0] == 9 and got.shape == pre.shape and np.count_nonzero(g_pool)
    f = pre.reshape((3, 3) + pre.shape[1:])
    assert np.array_equal(f[:, 0], f[:, 1]) and not np.array_equal(f[:, 0], f[:, 2])
    r = R._exact("pool backward", "hpool.0", got, R.pool_backward(g_pool, pre, pooled, 3, "max"))
    assert r.ok, r
    g = got.reshape(f.shape)
    tied = (f[:, 0] > f[:, 2]) & (g_pool != 0)   # the tied pair holds the max
    assert np.count_nonzero(tied) > 1000
    assert np.array_equal(g[:, 0][tied], g_pool[tied]) and np.array_equal(g[:, 1][tied], g_pool[tied])
    third = g[:, 2][tied]
    assert not third.any() and not np.signbit(third).any()  # +0
    lone = (f[:, 2] > f[:, 0]) & (g_pool != 0)
    assert np.count_nonzero(lone) > 1000 and np.array_equal(g[:, 2][lone], g_pool[lone])
    assert not g[:, 0][lone].any() and not g[:, 1][lone].any()
    # the forward kept the earliest frame's bits (the same bits here) and the second pool saw no such ties
    assert np.array_equal(pooled, np.maximum(f[:, 0], f[:, 2]))


# ---------------------------------------------------------------------------------------------- 7. running statistics
def test_running_statistics_and_the_optimizer(params):
    import videoyolo_amd as vy
    from videoyolo_amd import autograd
    from oracle import targets_oracle as T
    hier, b, h, w = [3, 3, 1, 1, 1], 2, 64, 64
    x = _clips(hier, b, h, w, seed=3)
    gt_boxes, gt_ids = T.synthetic_gt(b, min(h, w), C, m=3, seed=2, pad_to=5)
    tg = T.prefetch_targets(C, h, w, gt_boxes, gt_ids)

    def step(net):
        with autograd.record():
            losses = net(x, gt_boxes, *tg)
            autograd.backward([losses[0] + losses[1] + losses[2] + losses[3]])
        return losses

    net = _hier(params, hier)
    trainer = vy.Trainer(net.collect_params(), "sgd", {"learning_rate": 1e-3, "wd": 5e-4, "momentum": 0.9})
    losses = step(net)
    assert all(np.isfinite(_host(l)).all() for l in losses)
    # the stem saw B * T frames: its running statistics are the single-frame net's train-mode forward on those frames
    single = _single(params)
    with autograd.train_mode():
        single(x.reshape((b * 9, 3, h, w)))
    for leaf in ("running_mean", "running_var"):
        key = "stages.0.0.1." + leaf
        assert not np.array_equal(net.collect_params()[key].data(), params[key]), key
        assert np.array_equal(net.collect_params()[key].data(), single.collect_params()[key].data()), key
    # ... and a cell behind the first pool did NOT see what the single-frame net saw
    key = "stages.0.1.1.running_mean"
    assert not np.array_equal(net.collect_params()[key].data(), single.collect_params()[key].data())
    backbone = ["stages.0.0.0.weight", "stages.0.1.0.weight", "stages.0.4.body.1.1.gamma", "stages.2.4.body.1.0.weight"]
    trainer.step(b)
    for key in backbone + ["yolo_blocks.0.tip.0.weight"]:
        assert not np.array_equal(net.collect_params()[key].data(), params[key]), key

    frozen = _hier(params, hier, freeze_base=True)
    trainer = vy.Trainer(frozen.collect_params(), "sgd", {"learning_rate": 1e-3, "wd": 5e-4, "momentum": 0.9})
    step(frozen)
    trainer.step(b)
    for key, p in frozen.collect_params().items():
        if p.backbone and p.trainable:
            assert np.array_equal(p.data(), params[key]), key
    assert not np.array_equal(frozen.collect_params()["yolo_blocks.0.tip.0.weight"].data(), params["yolo_blocks.0.tip.0.weight"])
    # label smoothing and the recalled semantics are set as on any net
    frozen._target_generator._label_smooth = True
    frozen.set_semantics(strict_valid=False)
    assert all(np.isfinite(_host(l)).all() for l in step(frozen))
