"""-m gpu: every kernel of one training step, cell by cell, against float64 (oracle/train_cells64.py), on the three
nets that train: the single-frame net, the heads net (routes in) and the k-frame window net.

One fresh step per case.  z is tapped after the forward; after the backward every cell's dz, output gradient, input
view and BatchNorm state are tapped, and each kernel is recomputed from exactly the tensors the device gave it:
forward conv (bit-equal, first and last image), batch statistics (<= 1 ulp), forward apply (bit-equal), BN + leaky
backward (dgamma, dbeta, dz: per element, gamma_d from the plan's chunking), weight gradients (output channels 0,
Cout-1 and 6 random ones; gamma from the split-K plan), every producer's data gradient (first and last image, all
channels, summed over its consumers plus the skip addend), prediction-conv bias gradients, the stem's weight
gradient, d(loss)/d(pred) (a few ulp), the four loss values per image (R.check_losses: gamma(T + 9) times the absolute
sum of the per-anchor float64 terms; the census of the ignore decision is printed) and the zero borders of every z / dz /
gradient / input plane.  The constructed branches of the loss kernel, the raw predictions and the SGD step are
tests/test_gpu_loss_cells.py's.  Large cells are
checked in channel blocks so that the host never holds more than a few float64 copies of one block.

One walker serves all three: a builder makes the net, runs the step and names the graph (R.graph).  A cell runs on
B * fm frames (fm = k for the window net's stem and stages, else 1); the image-sampled checks take the first and last
clip, all fm frames of each, which puts the b*k + t frame order under test.  The window net adds the pool nodes: pool
forward bit-equal on all three routes (whole batch), window_pool_bwd bit-equal at stride 32 (the route gradient has no
other contributor), and at strides 8 / 16 the route cell's gradient plane within the data-gradient bound of the next
stage's first conv with the pool backward (numpy fp32, temporal.hip's arithmetic) as an addend.  The pooled planes'
own gradients are checked as producers of their head consumers, at their channel offset inside the concat.  The heads
net adds: each first consumer's input view is bit-equal to the caller's route in its channel range ("route view"),
borders zero, and the caller's tensors are unchanged.  (The walker runs "route view" on the window net too, where it
only ties the input tap to the pooled plane it aliases: there the pool forward check is the one that bites.)"""
import resource
import time
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (classes, batch, height, width): the bench's training headline (stream-K forward launches at this shape), the two
# ends of the multi-scale sizes (608 at batch 8: host memory), and the small shapes where edges sit — one class on one
# 64x64 frame, 32-wide frames (BatchNorm-backward row chunks), a non-square frame
CASES = [(20, 16, 416, 416), (20, 8, 608, 608), (20, 16, 320, 320), (1, 1, 64, 64), (3, 3, 96, 32), (4, 2, 128, 224)]
# (join, k, clips, height, width): DESIGN §11's measured shape with both joins (every backbone launch has the geometry
# of a full net at 48 frames, which no other test runs), and small shapes with both joins: one clip, k = 2 on 32-wide
# frames, k = 4 non-square, a multi-scale size
WINDOW_CASES = [("max", 3, 16, 416, 416), ("mean", 3, 16, 416, 416), ("max", 3, 1, 64, 64), ("mean", 2, 3, 96, 32),
                ("max", 4, 2, 128, 224), ("mean", 3, 2, 320, 320)]
WINDOW_CLASSES = 20
HEADS_CASES = [(20, 16, 416, 416), (3, 3, 96, 32)]
CH_BLOCK = 1 << 24  # elements per channel block of the full-batch checks


def _host(t):
    return t.detach().cpu().numpy()


def _inputs(C, B, H, W, seed):
    from videoyolo_amd import init
    from oracle import targets_oracle as T
    from oracle import yolo3_oracle as O
    params = init.synthetic_params(O.param_shapes(C), seed=seed)
    gt_boxes, gt_ids = T.synthetic_gt(B, min(H, W), C, m=3, seed=seed, pad_to=4)
    tg = T.prefetch_targets(C, H, W, gt_boxes, gt_ids)
    return params, gt_boxes, tg


def _record(net, cells, inputs, gt_boxes, tg):
    """One recorded step; z of every BatchNorm cell is tapped between the forward and the backward.  Returns the taps and
    the four (B,) loss tensors as one (4, B) array."""
    from videoyolo_amd import autograd
    with autograd.record():
        losses = net(*inputs, gt_boxes, *tg)
        z_fwd = {c["name"]: net.read_train_tap(c["name"], "z").clone() for c in cells if c.get("bn")}
        autograd.backward([losses[0] + losses[1] + losses[2] + losses[3]])
    return z_fwd, np.stack([_host(l) for l in losses])


def _step(C, B, H, W, seed=7, mode=None):
    """The single-frame net (mode: a conv mode to train in, tests/test_gpu_split_cells.py; default: the exact path)."""
    import videoyolo_amd as vy
    from oracle import train_cells64 as R
    params, gt_boxes, tg = _inputs(C, B, H, W, seed)
    rng = np.random.default_rng(seed + H + W)
    x = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    net = vy.yolo3_darknet53(["c%d" % i for i in range(C)], pretrained_base=False)
    net.set_parameters(params)
    net.collect_params().reset_ctx("cuda:0")
    if mode:
        net.set_conv_mode(mode)
    cells = R.graph(C)
    z_fwd, losses = _record(net, cells, (x,), gt_boxes, tg)
    return dict(net=net, params=params, cells=cells, frames=x, gt_boxes=gt_boxes, tg=tg, z_fwd=z_fwd, losses=losses, C=C, B=B, k=1)


def _step_window(join, k, B, H, W, C=WINDOW_CLASSES, seed=7):
    """The window net on B clips of k random-normal frames (distinct frames: one frame wins almost every element)."""
    import videoyolo_amd as vy
    from oracle import train_cells64 as R
    params, gt_boxes, tg = _inputs(C, B, H, W, seed)
    rng = np.random.default_rng(seed + H + W + k)
    x = rng.standard_normal((B, k, 3, H, W)).astype(np.float32)
    net = vy.yolo3_darknet53(["c%d" % i for i in range(C)], pretrained_base=False, k=k, k_join_type=join,
                             k_join_pos="early")
    assert isinstance(net, vy.YOLOV3Window)
    net.set_parameters(params)
    net.collect_params().reset_ctx("cuda:0")
    cells = R.graph(C, k=k)
    z_fwd, losses = _record(net, cells, (x,), gt_boxes, tg)
    return dict(net=net, params=params, cells=cells, frames=x.reshape((B * k, 3, H, W)), gt_boxes=gt_boxes, tg=tg,
                z_fwd=z_fwd, losses=losses, C=C, B=B, k=k, join=join)


def _step_heads(C, B, H, W, seed=7):
    """The heads net on the routes a full net's extract_features gives for a random-normal batch."""
    import torch
    import videoyolo_amd as vy
    from oracle import train_cells64 as R
    params, gt_boxes, tg = _inputs(C, B, H, W, seed)
    rng = np.random.default_rng(seed + H + W)
    x = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    classes = ["c%d" % i for i in range(C)]
    full = vy.yolo3_darknet53(classes, pretrained_base=False)
    full.set_parameters(params)
    full.collect_params().reset_ctx("cuda:0")
    routes = full.extract_features(x)
    before = [_host(r).copy() for r in routes]
    net = vy.yolo3_no_backbone(classes)
    net.set_parameters({n: v for n, v in params.items() if not n.startswith("stages.")})
    net.collect_params().reset_ctx("cuda:0")
    cells = R.graph(C, heads_only=True)
    z_fwd, losses = _record(net, cells, routes, gt_boxes, tg)
    torch.cuda.synchronize()
    res = [R._exact("caller's route", "route.%d" % i, _host(r), b0) for i, (r, b0) in enumerate(zip(routes, before))]
    del full
    return dict(net=net, params=params, cells=cells, frames=None, gt_boxes=gt_boxes, tg=tg, z_fwd=z_fwd, losses=losses, C=C,
                B=B, k=1, routes={"route.%d" % i: b0 for i, b0 in enumerate(before)}, res=res)


def _blocks(C, per_channel):
    step = max(4, min(C, CH_BLOCK // max(per_channel, 1)))
    return [(lo, min(C, lo + step)) for lo in range(0, C, step)]


def _sel(B, fm):
    """first and last clip (image, fm = 1), all fm frames of each: frame t of clip b is frame b*fm + t"""
    return sorted(set(range(fm)) | set(range((B - 1) * fm, B * fm)))


def _walk(st, split=None, only=None):
    """Every check of one recorded step `st` (a builder's dict) -> (results, pool counts {route: (wins, ties, clips counted)}).
    The loss census (R.loss_census) of the step is left in st["census"].

    st["sync"] (tests/test_gpu_syncbn_cells.py): the step ran with a SyncBatchNorm statistics callback — dict(world,
    calls=[dict(local, peer)] in call order, before / after={cell: [2][C] running statistics}, unbiased).  The
    synchronised cells (R.sync_cells) are then checked against the statistics of the global batch: check_stats and
    check_bn_backward with the recorded peer, check_sync_sums on what the callback received, check_running; what each
    block's inputs could tell apart is left in st["sync"]["nonvacuous"][cell].

    only: a set of cell names — the BatchNorm-side checks (borders, statistics, apply, BN backward) of those cells
    alone; no convolution, gradient-plane or loss check runs.

    split (tests/test_gpu_split_cells.py): the launches of the step that ran on the split-fp32 kernels, from its label
    log — dict(fwd={cell: k-split}, dgrad={cell: k-split}, wgrad={cell: splits}).  For those launches three checks are
    replaced by their split counterparts (oracle/split_oracle.py: check_split, three Results each): "forward conv
    bit-equal", the data gradient and the weight gradient; a consumer the exact kernel served keeps its exact term inside
    the same gradient plane's sum.  Every other check runs unchanged."""
    from oracle import split_oracle as S
    from oracle import train_cells64 as R
    split = split or dict(fwd={}, dgrad={}, wgrad={})
    net, params, cells, z_fwd = st["net"], st["params"], st["cells"], st["z_fwd"]
    C, B, k, join = st["C"], st["B"], st["k"], st.get("join")
    by_name = {c["name"]: c for c in cells}
    cons, skips = R.consumers(cells)
    res = list(st.get("res", []))
    pools = {}

    def tap(name, which):
        return _host(net.read_train_tap(name, which))

    def grad(pname):
        return net.grad(net._key(pname))

    def act(name):
        """forward value of a producer: a cell's or pool node's output, or the caller's route"""
        return st["routes"][name] if name in st.get("routes", {}) else _host(net.read_activation(name))

    sync, sync_at = st.get("sync"), {}
    if sync:  # the statistics exchanges of the step: forward in cell order, backward reversed; [2][C] doubles each
        names = R.sync_cells(cells)
        counts = [2 * by_name[n]["cout"] for n in names]
        assert [q["local"].size for q in sync["calls"]] == counts + counts[::-1], [q["local"].size for q in sync["calls"]]
        sync_at = {n: (sync["calls"][i], sync["calls"][2 * len(names) - 1 - i]) for i, n in enumerate(names)}
        sync["nonvacuous"] = {}

    for c in cells:
        if only is not None and (R.is_pool(c) or c["name"] not in only or not c["bn"]):
            continue
        if R.is_pool(c):  # pool forward on the device's own per-frame route, whole batch
            frames = act(c["src"][0])
            assert frames.shape[0] == B * k, (c["name"], frames.shape)
            res.append(R.check_pool_forward(c["name"], frames, k, join, act(c["name"])))
            continue
        name, kk, s = c["name"], c["k"], c["s"]
        sel_img = _sel(B, c["fm"])
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        sel_o = sorted({0, c["cout"] - 1} | set(rng.choice(c["cout"], size=min(6, c["cout"]), replace=False).tolist()))
        g_pad = tap(name, "grad")
        assert g_pad.shape[0] == B * c["fm"], (name, g_pad.shape)
        res.append(R.border_zero("borders", name + " grad", g_pad))
        g = R.interior(g_pad)
        del g_pad
        if only is not None:
            a = None
        elif c["src"] == ["image"]:
            a = st["frames"]
        else:
            a_pad = tap(name, "input")
            res.append(R.border_zero("borders", name + " input", a_pad))
            a = np.ascontiguousarray(R.interior(a_pad))
            del a_pad
            off = 0
            for p in c["src"]:  # a pooled or imported route: the view the conv reads holds the producer's bits
                if p.startswith(("pool.", "route.")):
                    src = act(p)
                    res.append(R._exact("route view", name + " <- " + p, a[:, off:off + src.shape[1]], src))
                    off += src.shape[1]
                else:
                    off += by_name[p]["cout"]
        assert only is not None or a.shape[0] == B * c["fm"], (name, a.shape)
        wname = name + (".0.weight" if c["bn"] else ".weight")
        w = params[wname]
        plan = net.train_conv_plan(name)
        def wgrad_check(dz_):
            if name in split["wgrad"]:  # 16-pixel groups of six products within a slab, the slabs added in order
                assert split["wgrad"][name] == plan[0], (name, split["wgrad"][name], plan)
                parts, ab = S.wgrad_parts(dz_, a, kk, s, sel_o)
                return S.check_split("split weight gradient", name, grad(wname)[sel_o], parts, ab, 6 * plan[1] + plan[0] + 2)
            return [R.check_wgrad(name, dz_, a, kk, s, sel_o, grad(wname)[sel_o], plan[0], plan[1])]

        if not c["bn"]:  # prediction conv: dz is the loss kernel's head gradient
            res.append(R.check_bias_grad(name, g, grad(name + ".bias")))
            res += wgrad_check(g)
            continue
        zf_pad = _host(z_fwd.pop(name))
        dz_pad = tap(name, "z")
        res.append(R.border_zero("borders", name + " z", zf_pad))
        res.append(R.border_zero("borders", name + " dz", dz_pad))
        z, dz = np.ascontiguousarray(R.interior(zf_pad)), np.ascontiguousarray(R.interior(dz_pad))
        del zf_pad, dz_pad
        assert z.shape[0] == B * c["fm"], (name, z.shape)  # the statistics count is B * fm * H * W
        bn = tap(name, "bn")
        gam, bet = params[name + ".1.gamma"], params[name + ".1.beta"]
        out = _host(net.read_activation(name))
        skip = _host(net.read_activation(c["skip"])) if c["skip"] else None
        if only is not None:
            pass
        elif name in split["fwd"]:  # the raw conv on conv_split_kernel: no epilogue, per-tile statistics, never k-split
            ch = S.sample_channels(c["cout"], name, z[sel_img][:, 0].size)
            a_s = np.ascontiguousarray(a[sel_img])
            res += S.check_split("split forward conv", name, z[sel_img][:, ch], S.six_parts(a_s, w[ch], s, kk // 2),
                                 S.absum(a_s, w[ch], s, kk // 2), 6 * kk * kk * c["cin"] + split["fwd"][name])
            del a_s
        else:
            res.append(R.check_forward_conv(name, a[sel_img], w, s, z[sel_img]))
        dgam, dbet = grad(name + ".1.gamma"), grad(name + ".1.beta")
        per = z.shape[0] * z.shape[2] * z.shape[3]
        parts = {}
        for lo, hi in _blocks(c["cout"], per * c["ups"] ** 2):
            cs = slice(lo, hi)
            kw_f, kw_b = {}, {}
            if name in sync_at:  # the statistics of the global batch: the recorded peer is an input of the cell
                fwd, bwd = sync_at[name]
                kw_f = dict(peer=fwd["peer"][:, cs], world=sync["world"])
                kw_b = dict(peer=bwd["peer"][:, cs], world=sync["world"], local_got=bwd["local"][:, cs])
                parts.setdefault("sync", []).append(R.check_sync_sums(name, fwd["local"][:, cs], z=z[:, cs]))
                parts.setdefault("running", []).append(R.check_running(
                    name, z[:, cs], bn[0, cs], sync["before"][name][:, cs], sync["after"][name][:, cs],
                    unbiased=sync["unbiased"], **kw_f))
                sync["nonvacuous"].setdefault(name, []).append(
                    dict(mean=bool(R.local_mean_differs(z[:, cs], **kw_f).all())))
            parts.setdefault("stats", []).append(R.check_stats(name, z[:, cs], bn[0, cs], bn[1, cs], gam[cs], bet[cs],
                                                              bn[2, cs], bn[3, cs], **kw_f))
            parts.setdefault("apply", []).append(R.check_apply(
                name, z[:, cs], bn[2, cs], bn[3, cs], out[:, cs], None if skip is None else skip[:, cs], c["ups"]))
            for r in R.check_bn_backward(name, z[:, cs], g[:, cs], bn[:, cs], gam[cs], c["ups"], plan[2], dgam[cs],
                                         dbet[cs], dz[:, cs], **kw_b):
                parts.setdefault(r.kind, []).append(r)
                if "local_only_differs" in r.extra:
                    sync["nonvacuous"][name][-1]["dz"] = r.extra["local_only_differs"]
        res += [R.Result.merge(p) for p in parts.values()]
        del out, skip, z
        if only is not None:
            continue
        if c["src"] == ["image"]:
            res.append(R.check_wgrad(name, dz, a, kk, s, list(range(c["cout"])), grad(wname), plan[0], plan[1],
                                     kind="stem weight gradient"))
        else:
            res += wgrad_check(dz)
        del dz, a

    if only is not None:
        return res, pools

    # data gradients: every producer's gradient plane, first and last clip
    for c in cells:
        name = c["name"]
        if name not in cons:
            continue
        sel_img = _sel(B, c["fm"])
        if R.is_pool(c):  # the pooled plane's own gradient: its head consumer's data gradient at the concat offset
            got = _host(net.read_grad_activation(name))
            assert got.shape[0] == B and np.count_nonzero(got), name + ": the pooled gradient is zero everywhere"
            got = got[sel_img]
        else:
            got = R.interior(tap(name, "grad"))[sel_img]
        terms, adds = [], [R.interior(tap(q["name"], "grad"))[sel_img] for q in skips.get(name, [])]
        for q, lo in cons[name]:
            if R.is_pool(q):
                # window_pool_bwd writes the per-frame route gradient before the next stage's first conv accumulates on it
                g_pool, pooled = _host(net.read_grad_activation(q["name"])), act(q["name"])
                frames, sel_b = act(name), _sel(B, 1)
                if len(cons[name]) == 1:  # stride 32: no other contributor, every element of the batch bit-equal
                    r, wins, ties = R.check_pool_backward(q["name"], g_pool, frames, pooled, k, join,
                                                          R.interior(tap(name, "grad")))
                    res.append(r)
                else:
                    wins, ties = R.pool_wins(frames[sel_img], k)
                    adds.append(R.pool_backward(g_pool[sel_b], frames[sel_img], pooled[sel_b], k, join))
                pools[q["name"]] = (wins, ties, "all %d clips" % B if len(cons[name]) == 1 else
                                    "the first and last clip")  # the clips whose route gradient is checked
                continue
            dzq = R.interior(tap(q["name"], "z" if q["bn"] else "grad"))[sel_img]
            wq = params[q["name"] + (".0.weight" if q["bn"] else ".weight")]
            terms.append((dzq, wq, q["s"], lo, q["name"]))
        if terms and not any(t[4] in split["dgrad"] for t in terms):
            res.append(R.check_dgrad(name, got, [t[:4] for t in terms], adds))
        elif terms:
            # consumers on conv_split_kernel ([cout][cin] images, flipped taps, one launch per parity class at stride 2,
            # cout zero-padded to a multiple of 32): their six products each; consumers on the exact kernel: their
            # float64 term and its own bound; the skip addends and the accumulation into the plane: one rounding each
            C_, hw = got.shape[1], got.shape[2:]
            groups, names, exact, ab_all, n = [], [], [], 0.0, 0
            for dzq, wq, sq, lo, qname in terms:
                wv = np.ascontiguousarray(wq[:, lo:lo + C_])
                if qname in split["dgrad"]:
                    parts, ab = S.dgrad_parts(dzq, wv, sq, hw)
                    groups.append(parts)
                    names.append(qname)
                    ab_all = ab_all + ab
                    n += 6 * ((wq.shape[0] + 31) // 32 * 32) * wq.shape[2] * wq.shape[3] + split["dgrad"][qname]
                else:
                    want, ab = R.dgrad64(dzq, wv, sq, hw)
                    exact.append((want, ab, wq.shape[0] * wq.shape[2] * wq.shape[3] + 2))
            res += S.check_split("split data gradient", name, got, groups, ab_all, n, S.Epilogue(addends=adds),
                                 exact_terms=exact, launches=names)

    # d(loss)/d(pred) on the device's own raw predictions
    preds = [_host(net.read_head(i)) for i in range(3)]
    opts = dict(ignore_iou_thresh=st.get("thresh", 0.7), label_smooth=st.get("label_smooth", False))
    targets = [np.asarray(t) for t in st["tg"]]
    want, exempt = R.head_grads(C, preds, st["gt_boxes"], targets, **opts)
    for i in range(3):
        name = "yolo_outputs.%d.prediction" % i
        res.append(R.check_head_grad(name, R.interior(tap(name, "grad")), want[i], exempt[i]))
    # the four loss values, per image, against the float64 sums of the per-anchor terms
    terms = R.loss_terms64(C, preds, st["gt_boxes"], targets, **opts)
    res += R.check_losses("losses", st["losses"], terms)
    st["census"], st["terms"] = R.loss_census(terms), terms
    return res, pools


def _check_net(C, B, H, W):
    st = _step(C, B, H, W)
    return _walk(st)[0], st["census"]


def _report(title, res, t0, pools=None, census=None):
    from oracle import train_cells64 as R
    print("\n%s: %d checks in %.0f s, peak host RSS %.1f GiB"
          % (title, len(res), time.time() - t0, resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2.0 ** 20))
    for kind, v in R.summarize(res).items():
        print("  %-22s worst err/bound %.3g (%s), worst err/(u sqrt(n) S) %.3g, %d checks"
              % (kind, v["worst_ratio"], v["worst_cell"], v["worst_headroom"], v["checks"]))
    for name, (wins, ties, scope) in sorted((pools or {}).items()):
        print("  %s, %s: elements won by frame t alone %s, elements with tied frames %d" % (name, scope, wins, ties))
    for r in res:
        if r.kind in ("loss gradient", "loss value"):
            print("  ", r)
    if census is not None:
        print("   anchors by decision: %(positive)d positive (%(fractional)d fractional), %(ignored)d ignored, %(negative)d "
              "negative; %(exempt)d exempt" % census)
    bad = [r for r in res if not r.ok]
    assert not bad, "\n".join(repr(r) for r in bad[:40])


@pytest.mark.parametrize("C,B,H,W", CASES)
def test_every_training_cell_against_float64(C, B, H, W):
    t0 = time.time()
    res, census = _check_net(C, B, H, W)
    _report("%dx%d batch %d, %d classes" % (H, W, B, C), res, t0, census=census)


@pytest.mark.parametrize("join,k,B,H,W", WINDOW_CASES)
def test_every_window_cell_against_float64(join, k, B, H, W):
    t0 = time.time()
    st = _step_window(join, k, B, H, W)
    res, pools = _walk(st)
    _report("window %s k=%d, %d clips of %dx%d, %d classes" % (join, k, B, H, W, WINDOW_CLASSES), res, t0, pools,
            st["census"])
    # not vacuous: all three routes were pooled and back-propagated; with max, every frame index of the checked clips
    # wins elements of every route on its own (a gradient sent to the wrong frame, or to all of them, cannot pass)
    assert sorted(pools) == ["pool.0", "pool.1", "pool.2"], sorted(pools)
    if join == "max":
        for name, (wins, ties, _) in pools.items():
            assert len(wins) == k and min(wins) > 0, (name, wins, ties)


@pytest.mark.parametrize("C,B,H,W", HEADS_CASES)
def test_every_heads_cell_against_float64(C, B, H, W):
    t0 = time.time()
    st = _step_heads(C, B, H, W)
    res, _ = _walk(st)
    _report("heads net, routes of %dx%d batch %d, %d classes" % (H, W, B, C), res, t0, census=st["census"])
    views = [r for r in res if r.kind == "route view"]
    assert len(views) == 3 and len([r for r in res if r.kind == "caller's route"]) == 3
