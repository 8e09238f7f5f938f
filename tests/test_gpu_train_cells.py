"""-m gpu: every kernel of one training step, cell by cell, against float64 (oracle/train_cells64.py).

One fresh step per case.  z is tapped after the forward; after the backward every cell's dz, output gradient, input
view and BatchNorm state are tapped, and each kernel is recomputed from exactly the tensors the device gave it:
forward conv (bit-equal, first and last image), batch statistics (<= 1 ulp), forward apply (bit-equal), BN + leaky
backward (dgamma, dbeta, dz: per element, gamma_d from the plan's chunking), weight gradients (output channels 0,
Cout-1 and 6 random ones; gamma from the split-K plan), every producer's data gradient (first and last image, all
channels, summed over its consumers plus the skip addend), prediction-conv bias gradients, the stem's weight
gradient, d(loss)/d(pred) (a few ulp) and the zero borders of every z / dz / gradient / input plane.  Large cells are
checked in channel blocks so that the host never holds more than a few float64 copies of one block."""
import time
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (classes, batch, height, width): the bench's training headline (stream-K forward launches at this shape), the two
# ends of the multi-scale sizes (608 at batch 8: host memory), and the small shapes where edges sit — one class on one
# 64x64 frame, 32-wide frames (BatchNorm-backward row chunks), a non-square frame
CASES = [(20, 16, 416, 416), (20, 8, 608, 608), (20, 16, 320, 320), (1, 1, 64, 64), (3, 3, 96, 32), (4, 2, 128, 224)]
CH_BLOCK = 1 << 24  # elements per channel block of the full-batch checks


def _host(t):
    return t.detach().cpu().numpy()


def _step(C, B, H, W, seed=7):
    import videoyolo_amd as vy
    from videoyolo_amd import autograd, init
    from oracle import targets_oracle as T
    from oracle import yolo3_oracle as O
    params = init.synthetic_params(O.param_shapes(C), seed=seed)
    rng = np.random.default_rng(seed + H + W)
    x = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    gt_boxes, gt_ids = T.synthetic_gt(B, min(H, W), C, m=3, seed=seed, pad_to=4)
    tg = T.prefetch_targets(C, H, W, gt_boxes, gt_ids)
    net = vy.yolo3_darknet53(["c%d" % i for i in range(C)], pretrained_base=False)
    net.set_parameters(params)
    net.collect_params().reset_ctx("cuda:0")
    with autograd.record():
        losses = net(x, gt_boxes, *tg)
        z_fwd = {}
        for name, p in net.collect_params().items():
            if name.endswith(".1.gamma"):
                cell = name[:-len(".1.gamma")]
                z_fwd[cell] = net.read_train_tap(cell, "z").clone()
        autograd.backward([losses[0] + losses[1] + losses[2] + losses[3]])
    return net, params, x, gt_boxes, tg, z_fwd


def _blocks(C, per_channel):
    step = max(4, min(C, CH_BLOCK // max(per_channel, 1)))
    return [(lo, min(C, lo + step)) for lo in range(0, C, step)]


def _check_net(C, B, H, W):
    from oracle import train_cells64 as R
    net, params, x, gt_boxes, tg, z_fwd = _step(C, B, H, W)
    cells = R.graph(C)
    cons, skips = R.consumers(cells)
    sel_img = sorted({0, B - 1})
    res = []

    def tap(name, which):
        return _host(net.read_train_tap(name, which))

    for c in cells:
        name, k, s = c["name"], c["k"], c["s"]
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        sel_o = sorted({0, c["cout"] - 1} | set(rng.choice(c["cout"], size=min(6, c["cout"]), replace=False).tolist()))
        g_pad = tap(name, "grad")
        res.append(R.border_zero("borders", name + " grad", g_pad))
        g = R.interior(g_pad)
        del g_pad
        if c["src"] == ["image"]:
            a = x
        else:
            a_pad = tap(name, "input")
            res.append(R.border_zero("borders", name + " input", a_pad))
            a = np.ascontiguousarray(R.interior(a_pad))
            del a_pad
        wname = name + (".0.weight" if c["bn"] else ".weight")
        w = params[wname]
        plan = net.train_conv_plan(name)
        if not c["bn"]:  # prediction conv: dz is the loss kernel's head gradient
            res.append(R.check_bias_grad(name, g, net.grad(name + ".bias")))
            res.append(R.check_wgrad(name, g, a, k, s, sel_o, net.grad(wname)[sel_o], plan[0], plan[1]))
            continue
        zf_pad = _host(z_fwd.pop(name))
        dz_pad = tap(name, "z")
        res.append(R.border_zero("borders", name + " z", zf_pad))
        res.append(R.border_zero("borders", name + " dz", dz_pad))
        z, dz = np.ascontiguousarray(R.interior(zf_pad)), np.ascontiguousarray(R.interior(dz_pad))
        del zf_pad, dz_pad
        bn = tap(name, "bn")
        gam, bet = params[name + ".1.gamma"], params[name + ".1.beta"]
        out = _host(net.read_activation(name))
        skip = _host(net.read_activation(c["skip"])) if c["skip"] else None
        res.append(R.check_forward_conv(name, a[sel_img], w, s, z[sel_img]))
        dgam, dbet = net.grad(name + ".1.gamma"), net.grad(name + ".1.beta")
        per = z.shape[0] * z.shape[2] * z.shape[3]
        parts = {}
        for lo, hi in _blocks(c["cout"], per * c["ups"] ** 2):
            cs = slice(lo, hi)
            parts.setdefault("stats", []).append(R.check_stats(name, z[:, cs], bn[0, cs], bn[1, cs], gam[cs], bet[cs],
                                                              bn[2, cs], bn[3, cs]))
            parts.setdefault("apply", []).append(R.check_apply(
                name, z[:, cs], bn[2, cs], bn[3, cs], out[:, cs], None if skip is None else skip[:, cs], c["ups"]))
            for r in R.check_bn_backward(name, z[:, cs], g[:, cs], bn[:, cs], gam[cs], c["ups"], plan[2], dgam[cs],
                                         dbet[cs], dz[:, cs]):
                parts.setdefault(r.kind, []).append(r)
        res += [R.Result.merge(p) for p in parts.values()]
        del out, skip, z
        if c["src"] == ["image"]:
            res.append(R.check_wgrad(name, dz, a, k, s, list(range(c["cout"])), net.grad(wname), plan[0], plan[1],
                                     kind="stem weight gradient"))
        else:
            res.append(R.check_wgrad(name, dz, a, k, s, sel_o, net.grad(wname)[sel_o], plan[0], plan[1]))
        del dz, a

    # data gradients: every producer's gradient plane, first and last image
    for c in cells:
        name = c["name"]
        if name not in cons:
            continue
        got = R.interior(tap(name, "grad"))[sel_img]
        terms = []
        for q, lo in cons[name]:
            dzq = R.interior(tap(q["name"], "z" if q["bn"] else "grad"))[sel_img]
            wq = params[q["name"] + (".0.weight" if q["bn"] else ".weight")]
            terms.append((dzq, wq, q["s"], lo))
        adds = [R.interior(tap(q["name"], "grad"))[sel_img] for q in skips.get(name, [])]
        res.append(R.check_dgrad(name, got, terms, adds))

    # d(loss)/d(pred) on the device's own raw predictions
    preds = [_host(net.read_head(i)) for i in range(3)]
    want, exempt = R.head_grads(C, preds, gt_boxes, [np.asarray(t) for t in tg])
    for i in range(3):
        name = "yolo_outputs.%d.prediction" % i
        res.append(R.check_head_grad(name, R.interior(tap(name, "grad")), want[i], exempt[i]))
    return res


@pytest.mark.parametrize("C,B,H,W", CASES)
def test_every_training_cell_against_float64(C, B, H, W):
    from oracle import train_cells64 as R
    t0 = time.time()
    res = _check_net(C, B, H, W)
    print("\n%dx%d batch %d, %d classes: %d checks in %.0f s" % (H, W, B, C, len(res), time.time() - t0))
    for kind, v in R.summarize(res).items():
        print("  %-22s worst err/bound %.3g (%s), worst err/(u sqrt(n) S) %.3g, %d checks"
              % (kind, v["worst_ratio"], v["worst_cell"], v["worst_headroom"], v["checks"]))
    for r in res:
        if r.kind == "loss gradient":
            print("  ", r)
    bad = [r for r in res if not r.ok]
    assert not bad, "\n".join(repr(r) for r in bad[:40])
