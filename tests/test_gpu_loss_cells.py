"""-m gpu: the two ends of the training step, element by element: the loss values and raw predictions
(loss_kernel, loss_reduce_kernel, raw_preds_kernel) on constructed inputs that reach every branch, and sgd_kernel over
four steps with changing multipliers.  The references and the derived bounds are oracle/train_cells64.py's
(loss_terms64 / check_losses / check_raw_preds / SgdRef: gamma(count) or count * u times an absolute sum, the counts
read off the kernels there); the constructed content is tests/loss_cases.py's, whose census conditions
tests/test_train_cells64_sensitivity.py settles on the CPU oracle.  Nothing here is a measured tolerance.

The census of every case and the worst err/bound observed per kind are recorded in profiles/loss_sgd_cells.txt, not
asserted.

The vehicle is the heads net (yolo3_no_backbone) on random-normal routes: no backbone, and the loss kernel is the one
every net ends its step with."""
import time

import numpy as np
import pytest

import loss_cases as L

pytestmark = pytest.mark.gpu


def _host(t):
    return t.detach().cpu().numpy()


def _net(case, params):
    import videoyolo_amd as vy
    net = vy.yolo3_no_backbone(["c%d" % i for i in range(case["C"])], ignore_iou_thresh=case["thresh"])
    net._target_generator._label_smooth = case["smooth"]
    net.set_parameters(params)
    net.collect_params().reset_ctx("cuda:0")
    return net


def _print(results):
    for r in results:
        print("  ", r)


def _two_passes(case, net=None):
    """Pass 1 (train-mode forward, raw predictions checked), the construction, pass 2 (the recorded step) -> dict"""
    from videoyolo_amd import autograd
    from oracle import train_cells64 as R
    C = case["C"]
    net = net or _net(case, L.heads_params(C))
    rts = L.routes(case["B"], case["H"], case["W"], case["seed"])
    with autograd.train_mode():
        out = net(*rts)
    box, ctr, scl, obj, cls = [_host(out[i]) for i in (0, 4, 5, 6, 7)]
    heads1 = [_host(net.read_head(i)) for i in range(3)]
    res = R.check_raw_preds("pass 1", heads1, box, ctr, scl, obj, cls)
    gt, tg, made = L.construct(case, box, scl, obj)
    with autograd.record():
        losses = net(*rts, gt, *tg)
        autograd.backward([losses[0] + losses[1] + losses[2] + losses[3]])
    heads2 = [_host(net.read_head(i)) for i in range(3)]
    for a, b in zip(heads1, heads2):  # the recorded forward ran on the same batch statistics
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), "the recorded forward's heads differ from pass 1's"
    grads = [_host(net.read_train_tap("yolo_outputs.%d.prediction" % i, "grad")) for i in range(3)]
    return dict(net=net, res=res, gt=gt, tg=tg, made=made, heads=heads2, grads=grads, box=box,
                losses=np.stack([_host(l) for l in losses]))


def _check_case(case, st):
    from oracle import train_cells64 as R
    C = case["C"]
    res, grads = st["res"], st["grads"]
    opts = dict(ignore_iou_thresh=case["thresh"], label_smooth=case["smooth"])
    terms = R.loss_terms64(C, st["heads"], st["gt"], st["tg"], **opts)
    census = L.conditions(case, terms, st["made"])
    print("\n%s: %s" % (L.case_id(case), census))
    res += R.check_losses("losses", st["losses"], terms)
    want, exempt = R.head_grads(C, st["heads"], st["gt"], st["tg"], **opts)
    for i in range(3):
        name = "yolo_outputs.%d.prediction" % i
        res.append(R.border_zero("borders", name + " grad", grads[i]))
        res.append(R.check_head_grad(name, R.interior(grads[i]), want[i], exempt[i]))
    _print(res)
    # saturated logits and an infinite box: no NaN or infinity in any loss or gradient
    assert np.isfinite(st["losses"]).all(), st["losses"]
    assert all(np.isfinite(g).all() for g in grads)
    assert np.isinf(st["box"]).any() and not np.isnan(st["box"]).any()
    # every constructed anchor is decided as the reference decides it (as constructed, unless another gt row decides first):
    # ignored -> dpred[4] == 0 exactly, not ignored -> dpred[4] != 0 (its objectness logit is unsaturated)
    dp4 = R.raw_layout([R.interior(g) for g in grads], C)[0][..., 4]
    for b, n, kind, m in st["made"]:
        ignored = terms["decision"][b, n] == -1
        assert (dp4[b, n] == 0) == ignored, (b, n, kind, m, dp4[b, n], terms["ious_max"][b, n])
    # d == 0: the two constructed positives have a zero scale gradient
    rows = R.raw_layout([R.interior(g) for g in grads], C)[0]
    pb, pn = np.nonzero(st["tg"][0][..., 0] > 0)
    for b, n in list(zip(pb, pn))[:2]:
        assert rows[b, n, 2] == 0 and rows[b, n, 3] == 0, (b, n, rows[b, n, 2:4])
    bad = [r for r in res if not r.ok]
    assert not bad, "\n".join(repr(r) for r in bad)


@pytest.mark.parametrize("case", L.CASES, ids=L.case_id)
def test_losses_and_raw_predictions_at_every_branch(case):
    t0 = time.time()
    _check_case(case, _two_passes(case))
    print("   %.1f s" % (time.time() - t0))


def test_gt_rows_at_the_launchers_cap():
    """M at vy_launch_loss's cap: 64 KiB of dynamic LDS next to the kernel's 64 static bytes, inside the 160 KiB a
    workgroup may hold on this chip (the device's sharedMemPerBlock, printed).  The losses are correct at the cap — the
    last row is a valid box that decides its anchor — and one row more is an error return."""
    import torch
    from videoyolo_amd import _lib, autograd
    case = L.CAP_CASE
    prop = torch.cuda.get_device_properties(0)
    print("\nLDS a block may hold: %s bytes; the launch asks for %d" % (
        getattr(prop, "shared_memory_per_block", "?"), case["M"] * 16 + 64))
    st = _two_passes(case)
    assert any(m == case["M"] - 1 for _, _, _, m in st["made"])
    _check_case(case, st)
    rts = L.routes(case["B"], case["H"], case["W"], case["seed"])
    gt = np.full((case["B"], case["M"] + 1, 4), -1.0, np.float32)
    with pytest.raises(_lib.VyError):
        with autograd.record():
            st["net"](*rts, gt, *st["tg"])


# ---------------------------------------------------------------------------------------------- sgd_kernel
LR, MOMENTUM, WD = 1e-3, 0.9, 5e-4


def _spread(names):
    """lr_mult in {0, 0.1, 1, 10} and wd_mult in {0, 1} over the parameters, by position"""
    return {n: ((0.0, 0.1, 1.0, 10.0)[i % 4], float((i // 4) % 2)) for i, n in enumerate(names)}


@pytest.mark.parametrize("C", [2, 1])
def test_sgd_steps_element_by_element(C):
    """Four recorded steps with Trainer.step on the heads net at 64x64 (prediction biases of 21 / 18 elements and weights of
    21 / 18 x 1024: not multiples of 4, 5 1/4 / 4 1/2 chunks of VY_SGD_CHUNK, the segments behind them off a 16-byte
    boundary).  Every parameter and gradient is read at every step; the host carries the momentum in float64 (R.SgdRef)."""
    import videoyolo_amd as vy
    from videoyolo_amd import autograd
    from oracle import train_cells64 as R
    case = dict(C=C, smooth=False, thresh=0.7, M=4, valid=3, B=2, H=64, W=64, seed=11 + C)
    net = _net(case, L.heads_params(C, saturated=False))
    rts = L.routes(case["B"], case["H"], case["W"], case["seed"])
    gt, tg, _ = L.construct(case, *_raw(net, rts))
    params = net.collect_params()
    train = [n for n, p in params.items() if p.trainable]
    stats = [n for n, p in params.items() if not p.trainable]
    assert any(params[n].size % 4 for n in train) and stats
    mult = _spread(train)
    frozen_first, frozen_later = "yolo_blocks.1.body.2.0.weight", "yolo_outputs.0.prediction.bias"
    mult[frozen_first] = (1.0, 1.0)
    for n, (lm, wm) in mult.items():
        params[n].lr_mult, params[n].wd_mult = lm, wm
    params[frozen_first].grad_req = 'null'
    trainer = vy.Trainer(params, 'sgd', {'learning_rate': LR, 'wd': WD, 'momentum': MOMENTUM})
    refs = {n: R.SgdRef(params[n].shape) for n in train}
    start = {n: params[n].data().copy() for n in (frozen_first, frozen_later)}
    res = []
    for step in range(1, 5):
        if step == 3:  # some multipliers change, the frozen cell thaws (from momentum 0), another one freezes
            for i, n in enumerate(train):
                if i % 3 == 0 and n not in (frozen_first, frozen_later):
                    mult[n] = ((10.0, 0.0, 0.1, 1.0)[i % 4], float(1 - (i // 4) % 2))
                    params[n].lr_mult, params[n].wd_mult = mult[n]
            params[frozen_first].grad_req = 'write'
            params[frozen_later].grad_req = 'null'
        with autograd.record():
            losses = net(*rts, gt, *tg)
            autograd.backward([losses[0] + losses[1] + losses[2] + losses[3]])
        before = {n: params[n].data().copy() for n in train}
        stats_before = {n: params[n].data().copy() for n in stats}
        g = {n: net.grad(n) for n in train}
        trainer.step(case["B"])
        for n in train:
            enabled = params[n].grad_req != 'null'
            res.append(R.SgdRef.step(refs[n], "%s step %d" % (n, step), before[n], g[n], params[n].data(), LR, MOMENTUM, WD,
                                     1.0 / case["B"], mult[n][0], mult[n][1], enabled))
        for n in stats:  # the step never touches the running statistics
            assert np.array_equal(params[n].data().view(np.int32), stats_before[n].view(np.int32)), (n, step)
        if step == 2:
            assert np.array_equal(params[frozen_first].data(), start[frozen_first])
            start[frozen_later] = params[frozen_later].data().copy()
    assert not np.array_equal(params[frozen_first].data(), start[frozen_first]), "the thawed cell did not move"
    assert np.array_equal(params[frozen_later].data(), start[frozen_later]), "the cell frozen before step 3 moved"
    kinds = {}
    for r in res:
        w = kinds.setdefault(r.kind, [0, 0.0, ""])
        w[0] += 1
        if r.ratio >= w[1]:
            w[1], w[2] = r.ratio, r.name
    print("\nC = %d: %s" % (C, {k: "%d checks, worst err/bound %.3g (%s)" % tuple(v) for k, v in kinds.items()}))
    assert kinds["sgd step"][0] and kinds["sgd frozen"][0] and kinds["sgd lr_mult 0"][0], kinds
    bad = [r for r in res if not r.ok]
    assert not bad, "\n".join(repr(r) for r in bad[:40])


def _raw(net, rts):
    from videoyolo_amd import autograd
    with autograd.train_mode():
        out = net(*rts)
    return _host(out[0]), _host(out[5]), _host(out[6])
