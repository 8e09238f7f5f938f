"""-m gpu: no launch leaves the region of the workspace it was given — for every region of every plan, every kind of net and
every launch form the suite knows how to reach, whatever the neighbouring region holds.

One case builds two nets from the same parameters under the same launch switches: a plain one, and one created under
VY_PLAN_GUARD (a gap behind every region: include/vyolo.h, vy_net_plan_region) whose workspace — and, where it trains,
gradient and momentum buffers — are views inside larger buffers (tests/ws_guard.py).  After every bind of the guarded net
the gaps, the rounding slack behind each region's used bytes and the bands around the buffer are filled with one quiet-NaN
pattern; then both nets run the same calls.  Asserted:

  (a) every gap, slack and band byte is still the pattern: no launch wrote outside its region;
  (b) every output of every call is bit-equal to the plain net's.  Results do not depend on where the workspace lies
      (tests/test_gpu_plan.py, tests/test_gpu_multiscale.py), so a difference — the NaN itself, as a rule — is a read
      past a region's end that reached a result;
  (c) the caller's input tensors are bit-unchanged;
  (d) the stream-K flag words are all zero.

A read outside a region whose value is discarded does not show, and is not looked for.  The parameter buffer and the
inference outputs are allocated where a test cannot put bands around them; they are not covered.

Shapes are the smallest at which each form occurs, all of them met elsewhere in the suite.  The table of one run —
case, regions checked, gap / slack / band bytes checked, conv forms served, result — is profiles/ws_guard.txt, written by
the last test of the file when every case has run in the process."""
import ctypes
import itertools
import os

import numpy as np
import pytest

import conv_forms as F
import ws_guard as G

pytestmark = pytest.mark.gpu

GUARD, WIDE = G.GUARD, 262144  # WIDE: a stray that jumps a whole row, not a few bytes
SWITCHES = sorted(set(F.SWITCHES) | {"VY_SPLIT_ALWAYS", "VY_SPLIT_WINO", "VY_SPLIT_TRAIN", "VY_SPLIT_WGRAD", "VY_SPLIT_FORCE",
                                     "VY_PLAN_GUARD"})
A, B, C = (1, 1, 64, 64), (3, 3, 96, 32), (4, 2, 128, 224)  # (classes, batch, height, width): test_gpu_train_cell_forms.py
TABLE = {}  # case -> (regions, bytes checked, forms, result)
_serial = itertools.count()
_params = {}


def _ids(v):
    return v if isinstance(v, str) else "x".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


def _synthetic(classes):
    if classes not in _params:
        from videoyolo_amd import init
        from oracle import yolo3_oracle as O
        _params[classes] = init.synthetic_params(O.param_shapes(classes), seed=233)
    return _params[classes]


def _setenv(monkeypatch, env, guard):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if guard:
        monkeypatch.setenv("VY_PLAN_GUARD", str(guard))


def _names(classes):
    return ["c%d" % i for i in range(classes)]


def _on_device(net, params, heads_only=False):
    net.set_parameters({k: v for k, v in params.items() if not (heads_only and k.startswith("stages."))})
    net.collect_params().reset_ctx("cuda:0")
    return net


def _full(classes, **kw):
    import videoyolo_amd as vy
    return _on_device(vy.yolo3_darknet53(_names(classes), pretrained_base=False, **kw), _synthetic(classes))


def _heads(classes, **kw):
    import videoyolo_amd as vy
    return _on_device(vy.yolo3_no_backbone(_names(classes), **kw), _synthetic(classes), heads_only=True)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _normal(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def _targets(classes, b, h, w, seed=7):
    from oracle import targets_oracle as T
    gt_boxes, gt_ids = T.synthetic_gt(b, min(h, w), classes, m=3, seed=seed, pad_to=4)
    return [gt_boxes] + list(T.prefetch_targets(classes, h, w, gt_boxes, gt_ids))


def _host(t):
    import torch
    t = t.detach().contiguous()
    return (t.view(torch.uint8) if t.dtype != torch.uint8 else t).cpu().numpy()


# ---------------------------------------------------------------- the guarded buffers of one net
class Guarded:
    """A workspace view inside a banded buffer, for the handle `h`: `view` is what the caller hands to the bind (net._ws,
    session._ws, a twin's ws); with train, net._grads and net._mom are set to banded, zeroed views as well."""

    def __init__(self, net, plans, h=None, train=False):
        import torch
        self.net, self.lib, self.h = net, net._lib, h or net._h
        need = max(G.plan_bytes(self.lib, self.h, p, s) for p, s in plans)
        assert need > 0, plans
        self.buf, self.view = G.banded(need)
        self.params = {}
        if train:
            n = int(self.lib.vy_net_param_bytes(self.h))
            for name in ("_grads", "_mom"):
                buf, view = G.banded(n, zero=True)
                setattr(net, name, view.view(torch.float32))
                self.params[name] = (buf, n)
        self.table, self.regions, self.checked = None, 0, 0

    def bound(self, plan, shape):
        """The library has just bound `plan` in the view (or still holds it: the holes are poisoned again)"""
        self.table = G.regions(self.lib, self.h, plan, shape)
        assert self.table[-1][1] + self.table[-1][3] <= self.view.numel()
        G.poison(self.view, self.table)

    def check(self, what):
        import torch
        torch.cuda.synchronize()
        host = self.buf.cpu().numpy()
        bad = G.violations(host, self.table, G.BAND)
        assert not bad, "%s: bytes outside a region were written (region, first offset behind its used end, bytes): %s" % (what, bad[:8])
        _, off, used, _ = next(r for r in self.table if r[0] == "sk.flags")
        assert not host[G.BAND + off:G.BAND + off + used].any(), "%s: a stream-K flag is up" % what
        self.regions += len(self.table)
        self.checked += G.gap_bytes(self.table) + 2 * G.BAND + self.view.numel() - (self.table[-1][1] + self.table[-1][3])
        for name, (buf, n) in self.params.items():
            bad = G.violations(buf.cpu().numpy(), [(name, 0, n, n)], G.BAND)
            assert not bad, "%s: bytes around the %s buffer were written: %s" % (what, name, bad)
            self.checked += 2 * G.BAND


def _bind(net, g, plan, shape):
    """The bind the next call would make, made now, so that the holes can be poisoned in between"""
    import torch
    assert net._ws.data_ptr() == g.view.data_ptr(), "the net let go of the banded workspace"
    with torch.cuda.device(net._device):
        net._ensure_plan(*shape, train=plan == "train")
    assert net._ws.data_ptr() == g.view.data_ptr() and net._ws.numel() == g.view.numel()
    g.bound(plan, shape)


def _equal(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), \
            "%s: %s differs from the plain net's (%d of %d bytes)" % (what, k, int((got[k] != want[k]).sum()), want[k].size)


def _unchanged(inputs, what):
    for i, (dev, host) in enumerate(inputs):
        assert _host(dev).tobytes() == host.view(np.uint8).tobytes(), "%s: input %d was written" % (what, i)


def _log(case, gs, forms, result="ok"):
    TABLE[case] = (sum(g.regions for g in gs), sum(g.checked for g in gs), forms, result)
    assert TABLE[case][1] > 0


# ---------------------------------------------------------------- the calls of a case
def _detect(net, call, inputs):
    """One inference call -> its outputs, keep indices included"""
    outs = call(*[d for d, _ in inputs], return_index=True)
    return {"detect.%d" % i: _host(t) for i, t in enumerate(outs)}


def _train_step(net, call, inputs, tg, batch):
    """Recorded forward, backward, Trainer.step, train-mode forward -> losses, every gradient, momentum, parameters, the
    train-mode tensors"""
    import videoyolo_amd as vy
    from videoyolo_amd import autograd
    trainer = vy.Trainer(net.collect_params(), 'sgd', {'learning_rate': 1e-3, 'wd': 5e-4, 'momentum': 0.9})
    dev = [d for d, _ in inputs]
    with autograd.record():
        losses = call(*dev, *tg)
        autograd.backward([losses[0] + losses[1] + losses[2] + losses[3]])
    out = {"loss.%d" % i: _host(l) for i, l in enumerate(losses)}
    out["grads"] = _host(net._grads)
    trainer.step(batch)
    out["momentum"] = _host(net._mom)
    out["params"] = _host(net._dev_params)
    with autograd.train_mode():
        tm = call(*dev)
    for i in (0, 4, 5, 6, 7):
        out["train_mode.%d" % i] = _host(tm[i])
    return out


def _pair(monkeypatch, env, guard, make, labels=None):
    """(plain net, guarded net): the same constructor under the same switches, the second with the guard — and with
    VY_TRAIN_LABELS=labels, so that the launch labels of a step are the guarded net's"""
    _setenv(monkeypatch, env, 0)
    plain = make()
    _setenv(monkeypatch, dict(env, VY_TRAIN_LABELS=labels) if labels else env, guard)
    guarded = make()
    _setenv(monkeypatch, env, 0)
    return plain, guarded


def _run_case(case, monkeypatch, env, make, shape, inputs, tg=None, infer=True, train=False, guard=GUARD, call=None, labels=None,
              setup=None):
    """The frame of most cases: one inference call under the clip plan, then (train) one training step under the training
    plan, on both nets; (a)-(d) after each.  shape: (batch, height, width) of the plans; inputs: [numpy] the caller's
    tensors; call(net): the entry (default: the net itself); setup(net): settings between creation and the first plan.
    Returns the guarded net's Guarded."""
    plain, net = _pair(monkeypatch, env, guard, make, labels)
    for n in (plain, net):
        if setup:
            setup(n)
    call = call or (lambda n: n)
    plans = ([("clip", shape)] if infer else []) + ([("train", shape)] if train else [])
    g = Guarded(net, plans, train=train)
    net._ws = g.view
    held = [(_dev(a), a) for a in inputs]
    for plan, _ in plans:
        what = "%s, %s plan" % (case, plan)
        run = (lambda n: _detect(n, call(n), held)) if plan == "clip" else (lambda n: _train_step(n, call(n), held, tg, shape[0]))
        want = run(plain)
        _bind(net, g, plan, shape)
        got = run(net)
        g.check(what)
        _equal(got, want, what)
        _unchanged(held, what)
    return g


# ---------------------------------------------------------------- single-frame inference, default plan
INFER = [("c1", 1, (3, 64, 64), {}), ("c20", 20, (2, 96, 64), {}), ("c80", 80, (1, 100, 136), {}), ("c200", 200, (3, 33, 47), {}),
         ("keep_activations", 20, (1, 100, 136), dict(keep=True)), ("nms_off", 20, (3, 33, 47), dict(nms=(1.0, 400, 100))),
         ("topk_all", 20, (2, 96, 64), dict(nms=(0.45, -1, 100)))]


@pytest.mark.parametrize("name,classes,shape,opt", INFER, ids=_ids)
def test_single_frame_inference(monkeypatch, name, classes, shape, opt):
    def setup(net):
        if opt.get("keep"):
            net.keep_activations()
        if "nms" in opt:
            net.set_nms(*opt["nms"])
    case = "infer %s %s" % (name, _ids(shape))
    g = _run_case(case, monkeypatch, {}, lambda: _full(classes), shape, [_normal((shape[0], 3) + shape[1:], 5)], setup=setup)
    _log(case, [g], "")


def test_a_write_planted_on_the_device_is_reported(monkeypatch):
    """The device side of the checker — poison after the bind, the copy of the whole buffer, the scan — sees one word
    written behind a plane, one in the middle of the detection list's gap and one at the first byte of the back band,
    each against its region, after a forward that itself leaves no trace.  (The host side: tests/test_ws_guard_host.py.)"""
    shape = (1, 100, 136)  # (15 x 19 padded pixels at stride 8: the 96-channel prediction plane ends between 256-byte lines)
    g = _run_case("planted", monkeypatch, {}, lambda: _full(20), shape, [_normal((shape[0], 3) + shape[1:], 5)])
    plane = next(r for r in g.table if r[0].startswith("plane:") and r[3] - r[2] > GUARD)
    det = next(r for r in g.table if r[0] == "det.list")
    last = g.table[-1]
    for name, at in ((plane[0], plane[1] + plane[2]), (det[0], det[1] + det[3] - GUARD // 2), (last[0], last[1] + last[3])):
        g.bound("clip", shape)
        g.buf[G.BAND + at:G.BAND + at + 4] = 0
        with pytest.raises(AssertionError, match="bytes outside a region were written") as err:
            g.check("planted")
        assert "('%s', %d, 4)" % (name, at - next(r[1] + r[2] for r in g.table if r[0] == name)) in str(err.value), str(err.value)
        G._fill(g.buf, G.BAND + at, G.BAND + at + 4)  # (the band is not the bind's to poison again)
    g.bound("clip", shape)
    g.check("planted, poisoned again")


def test_detect_heads_on_the_overflow_heads(monkeypatch):
    """The tail alone on 20 160 equal scores: the bucket list at its cap, refine_kernel walking the score cache"""
    import semantics_cases as SC
    sc = next(c for c in SC.all_cases() if c["name"] == "overflow")
    size = sc["size"]
    h, w = (size, size) if isinstance(size, int) else size
    shape = (int(sc["heads"][0].shape[0]), h, w)

    def setup(net):
        net.set_nms(sc["nms_thresh"], sc["nms_topk"], sc["post_nms"])
    case = "detect_heads overflow %s" % _ids(shape)
    g = _run_case(case, monkeypatch, {}, lambda: _heads(sc["classes"]), shape, [np.asarray(t, np.float32) for t in sc["heads"]],
                  setup=setup, call=lambda n: (lambda *a, **kw: n.detect_heads(a, (h, w), **kw)))
    _log(case, [g], "")


def test_two_stream_batch_split(monkeypatch):
    """detect_two_streams: the halves on the net and on its twin, each in a banded workspace of its own"""
    import torch
    from videoyolo_amd import _lib
    classes, (b, h, w) = 20, (2, 96, 64)
    half = (b // 2, h, w)
    case = "infer two streams %s" % _ids((b, h, w))
    plain, net = _pair(monkeypatch, {}, GUARD, lambda: _full(classes))
    x = _normal((b, 3, h, w), 5)
    held = [(_dev(x), x)]
    want = _detect(plain, plain.detect_two_streams, held)
    _setenv(monkeypatch, {}, GUARD)  # (a twin is created inside the first call: the guarded net's under the guard)
    g = Guarded(net, [("clip", half)])
    net._ws = g.view
    _detect(net, net.detect_two_streams, held)  # creates the twin and binds both
    tw = net._twin
    assert tw is not None and net._ws.data_ptr() == g.view.data_ptr()
    g2 = Guarded(net, [("clip", half)], h=tw["h"])
    with torch.cuda.device(net._device):
        _lib.check(net._lib.vy_net_bind_workspace(tw["h"], ctypes.c_void_p(g2.view.data_ptr()), g2.view.numel(), *half, net._stream()))
    tw["ws"], tw["plan"] = g2.view, half
    g.bound("clip", half)
    g2.bound("clip", half)
    got = _detect(net, net.detect_two_streams, held)
    assert tw["ws"].data_ptr() == g2.view.data_ptr() and tw["plan"] == half
    for gg in (g, g2):
        gg.check(case)
    _equal(got, want, case)
    _unchanged(held, case)
    _log(case, [g, g2], "")


# ---------------------------------------------------------------- every forced form of the exact conv kernel
def _forced_cases():
    import test_gpu_train_cell_forms as TF
    assert (TF.A, TF.B, TF.C) == (A, B, C)
    assert {e for e, _ in TF.NET_CASES} == set(F.FORCED)
    for tile in ("128x128", "128x64", "128x32", "64x64"):  # the 32-wide shape of the BatchNorm-backward overflow, on every tile
        assert any(F.FORCED[e].get("VY_CONV_FORCE") == tile and s == B for e, s in TF.NET_CASES), tile
    return list(TF.NET_CASES)


@pytest.mark.parametrize("envname,shape", _forced_cases(), ids=_ids)
def test_forced_form_inference_and_training_step(monkeypatch, tmp_path, envname, shape):
    from oracle import train_cells64 as R
    classes, b, h, w = shape
    labels = str(tmp_path / ("labels_%d.txt" % next(_serial)))  # a fresh path: the library fills each path once
    case = "forced %s %s" % (envname, _ids(shape))
    g = _run_case(case, monkeypatch, F.FORCED[envname], lambda: _full(classes), (b, h, w), [_normal((b, 3, h, w), 7 + h + w)],
                  tg=_targets(classes, b, h, w), train=True, labels=labels)
    convs, wgrads = F.read_labels(labels, R.graph(classes))
    os.remove(labels)
    F.check_served(envname, convs, wgrads)
    _log(case, [g], " ".join("%s:%s" % f for f in sorted(F.forms_of(convs))))


# ---------------------------------------------------------------- the split-fp32 modes
SPLIT_INFER = [("wino0", {"VY_SPLIT_ALWAYS": "1", "VY_SPLIT_WINO": "0"}, (3, 33, 47)), ("wino0", {"VY_SPLIT_ALWAYS": "1", "VY_SPLIT_WINO": "0"}, (2, 64, 64)),
               ("wino2", {"VY_SPLIT_ALWAYS": "1", "VY_SPLIT_WINO": "2"}, (3, 33, 47)), ("wino2", {"VY_SPLIT_ALWAYS": "1", "VY_SPLIT_WINO": "2"}, (2, 64, 64)),
               ("force128x64k4", {"VY_SPLIT_ALWAYS": "1", "VY_SPLIT_WINO": "0", "VY_SPLIT_FORCE": "128x64k4"}, (3, 96, 32))]


@pytest.mark.parametrize("name,env,shape", SPLIT_INFER, ids=_ids)
def test_split_inference(monkeypatch, name, env, shape):
    case = "split_bf16x3 %s %s" % (name, _ids(shape))
    x = _normal((shape[0], 3) + shape[1:], 9)
    g = _run_case(case, monkeypatch, env, lambda: _full(20), shape, [x], setup=lambda n: n.set_conv_mode("split_bf16x3"))
    assert {r[0].split(":")[0] for r in g.table} >= {"wsplit", "wino"}
    # the kernels the case is about really served it: the labels of one profiled forward of the guarded net
    forms = sorted({row[0].split("|")[1] for row in g.net.profile(x) if "|split" in row[0] or "|wino" in row[0]})
    assert any(f.startswith("split") for f in forms), forms
    assert any(f.startswith("wino") for f in forms) == (env["VY_SPLIT_WINO"] == "2"), forms
    if "VY_SPLIT_FORCE" in env:
        assert "split" + env["VY_SPLIT_FORCE"] in forms, forms
    _log(case, [g], " ".join("infer:" + f for f in forms))


def test_split_training_step(monkeypatch, tmp_path):
    classes, b, h, w = B
    case = "split_bf16x3_train %s" % _ids(B)
    labels = str(tmp_path / ("labels_%d.txt" % next(_serial)))
    g = _run_case(case, monkeypatch, {"VY_SPLIT_ALWAYS": "1"}, lambda: _full(classes), (b, h, w), [_normal((b, 3, h, w), 9)],
                  tg=_targets(classes, b, h, w), infer=False, train=True, setup=lambda n: n.set_conv_mode("split_bf16x3_train"),
                  labels=labels)
    assert {r[0].split(":")[0] for r in g.table} >= {"wsplit", "dgrad_image"}
    # forward, data gradients and weight gradients of the step really ran on the split kernels: the step's own labels
    kinds, last = {}, None
    with open(labels) as f:
        for line in f:
            t = line.split()
            if t and t[0] != "#":
                last = t[0]
            elif t and "split" in t[2]:
                kinds.setdefault(last, set()).add(t[2] if last == "wgrad" else " ".join(t[2:5]).replace(" ", ""))
    os.remove(labels)
    assert sorted(kinds) == ["dgrad", "fwd", "wgrad"], kinds
    _log(case, [g], " ".join("%s:%s" % (k, v) for k in sorted(kinds) for v in sorted(kinds[k])))


# ---------------------------------------------------------------- SyncBatchNorm: the sums and slices regions
def test_syncbn_step_with_a_simulated_peer(monkeypatch):
    """World 2 with test_gpu_train_parity's stand-in for the all-reduce: the [2][C] sums doubled in place"""
    import torch
    from videoyolo_amd import _lib, autograd
    classes, b, s = 3, 2, 64
    case = "syncbn world 2 %s" % _ids((classes, b, s, s))
    plain, net = _pair(monkeypatch, {}, GUARD, lambda: _full(classes))
    x = _normal((b, 3, s, s), 9)
    held, tg = [(_dev(x), x)], _targets(classes, b, s, s)
    g = Guarded(net, [("train", (b, s, s))], train=True)
    net._ws = g.view
    calls = {}

    def hook(n):
        def cb(user, ptr, count):
            off = int(ptr) - n._ws.data_ptr()
            n._ws[off:off + 8 * count].view(torch.float64).mul_(2.0)
            calls[id(n)] = calls.get(id(n), 0) + 1
            return 0
        keep = _lib.ALLREDUCE_CB(cb)
        n._cb_keep.append(keep)
        with torch.cuda.device(n._device):
            n._ensure_plan(b, s, s, train=True)  # plan + bind first: the callback needs the workspace
        _lib.check(n._lib.vy_net_set_sync_bn(n._h, 2, keep, None))

    hook(plain)
    want = _train_step(plain, plain, held, tg, b)
    hook(net)
    _bind(net, g, "train", (b, s, s))
    got = _train_step(net, net, held, tg, b)
    g.check(case)
    assert calls[id(net)] == calls[id(plain)] >= 12, calls
    sums = next(r for r in g.table if r[0] == "train.sums")
    assert sums[2] == 2 * 2 * 1024 * 8
    _equal(got, want, case)
    _unchanged(held, case)
    _log(case, [g], "")


# ---------------------------------------------------------------- the other kinds of net
def _window(classes, k, join):
    return _full(classes, k=k, k_join_type=join, k_join_pos="early")


def _hier(classes, hier):
    return _full(classes, new_model=True, hierarchical=hier, h_join_type="max")


KINDS = {
    "window max k3": (lambda: _window(20, 3, "max"), 20, (1, 64, 64), 3),
    "window mean k2": (lambda: _window(20, 2, "mean"), 20, (3, 96, 32), 2),
    "hier 3,1,1,1,1": (lambda: _hier(20, [3, 1, 1, 1, 1]), 20, (2, 64, 64), 3),
    "hier 3,3,3,3,1": (lambda: _hier(20, [3, 3, 3, 3, 1]), 20, (1, 64, 64), 81),
}


def _kind_case(monkeypatch, name, guard):
    make, classes, (b, h, w), frames = KINDS[name]
    case = "%s %s%s" % (name, _ids((b, h, w)), " guard %d" % guard if guard != GUARD else "")
    g = _run_case(case, monkeypatch, {}, make, (b, h, w), [_normal((b, frames, 3, h, w), 11)], tg=_targets(classes, b, h, w), train=True,
                  guard=guard)
    _log(case, [g], "")


@pytest.mark.parametrize("name", sorted(KINDS))
def test_clip_nets_inference_and_training_step(monkeypatch, name):
    _kind_case(monkeypatch, name, GUARD)


def _routes(classes, b, h, w):
    full = _full(classes)
    routes = [t.cpu().numpy() for t in full.extract_features(_normal((b, 3, h, w), 13))]
    del full
    return routes


def _heads_case(monkeypatch, guard):
    classes, b, h, w = B
    case = "heads %s%s" % (_ids((b, h, w)), " guard %d" % guard if guard != GUARD else "")
    _setenv(monkeypatch, {}, 0)
    g = _run_case(case, monkeypatch, {}, lambda: _heads(classes), (b, h, w), _routes(classes, b, h, w), tg=_targets(classes, b, h, w),
                  train=True, guard=guard)
    _log(case, [g], "")


def test_heads_net_inference_and_training_step(monkeypatch):
    _heads_case(monkeypatch, GUARD)


def _bank(t, h, w, seed):
    h8, w8 = -(-h // 8), -(-w // 8)
    return [_normal(s, seed + i) for i, s in enumerate(((t, 256, h8, w8), (t, 512, -(-h8 // 2), -(-w8 // 2)), (t, 1024, -(-h8 // 4), -(-w8 // 4))))]


def _heads_window_case(monkeypatch, guard):
    """A bank of 5 frames and a full table: 128 clips x 4 frames = VY_VIDEO_TABLE_MAX entries"""
    from videoyolo_amd import _lib
    classes, k, s = 3, 4, 64
    b = _lib.VY_VIDEO_TABLE_MAX // k
    table = np.random.default_rng(0).integers(0, 5, (b, k))
    case = "heads window full table %s%s" % (_ids((b, s, s)), " guard %d" % guard if guard != GUARD else "")
    g = _run_case(case, monkeypatch, {}, lambda: _heads(classes, k=k, k_join_type="max", k_join_pos="early"), (b, s, s), _bank(5, s, s, 3),
                  tg=_targets(classes, b, s, s), train=True, guard=guard,
                  call=lambda n: (lambda f1, f2, f3, *a, **kw: n.from_bank(f1, f2, f3, table, *a, **kw)))
    _log(case, [g], "")


def test_heads_window_net_from_a_bank_with_a_full_table(monkeypatch):
    _heads_window_case(monkeypatch, GUARD)


def _video_case(monkeypatch, guard):
    """Frames 4, clips 2, ring 6 on a k = 3 window net: 11 frames pushed in three parts (the ring wraps), then the flush's
    detects, then every slot read back.  The ring's gap and the back band are the checks."""
    from videoyolo_amd.video import VideoSession
    classes, k, (f, c, r), (h, w) = 20, 3, (4, 2, 6), (64, 64)
    case = "video %s %s%s" % (_ids((f, c, r)), _ids((h, w)), " guard %d" % guard if guard != GUARD else "")
    plain, net = _pair(monkeypatch, {}, guard, lambda: _window(classes, k, "max"))
    x = _normal((11, 3, h, w), 17)
    held = [(_dev(x), x)]

    def run(n, g=None):
        session = VideoSession(n, frames_per_step=f, ring=r, clips_per_step=c)
        if g is not None:
            session._ws = g.view
            session._ensure_bound(h, w)
            assert session._ws.data_ptr() == g.view.data_ptr()
            g.bound("video", (f, c, r, h, w))
        out, dev = {}, held[0][0]
        for i, (lo, hi) in enumerate(((0, 3), (3, 7), (7, 11))):
            for j, t in enumerate(session.push(dev[lo:hi], return_index=True)):
                out["push%d.%d" % (i, j)] = _host(t)
        for j, t in enumerate(session.flush(return_index=True)):
            out["flush.%d" % j] = _host(t)
        for slot in range(r):
            for j, t in enumerate(session.read_slot(slot)):
                out["slot%d.%d" % (slot, j)] = _host(t)
        return out

    want = run(plain)
    g = Guarded(net, [("video", (f, c, r, h, w))])
    got = run(net, g)
    g.check(case)
    assert g.table[-1][0] == "ring"
    _equal(got, want, case)
    _unchanged(held, case)
    _log(case, [g], "")


def test_video_plan_until_the_ring_wraps(monkeypatch):
    _video_case(monkeypatch, GUARD)


# ---------------------------------------------------------------- re-binding on one buffer
def test_size_sequence_on_one_buffer(monkeypatch):
    """test_gpu_multiscale.py's first sequence of training sizes, on one banded buffer sized for the largest: every bind
    lays the workspace out anew; poison and check after each"""
    import videoyolo_amd as vy
    from videoyolo_amd import autograd
    classes, b, seq = 20, 2, (96, 160, 64, 128, 96, 160, 160, 64)
    case = "size sequence %s batch %d" % ("-".join(str(s) for s in seq), b)
    plain, net = _pair(monkeypatch, {}, GUARD, lambda: _full(classes))
    g = Guarded(net, [("train", (b, s, s)) for s in set(seq)], train=True)
    net._ws = g.view
    trainers = {id(n): vy.Trainer(n.collect_params(), 'sgd', {'learning_rate': 1e-3, 'wd': 5e-4, 'momentum': 0.9}) for n in (plain, net)}

    def step(n, dev, tg):
        with autograd.record():
            losses = n(dev, *tg)
            autograd.backward([losses[0] + losses[1] + losses[2] + losses[3]])
        out = {"loss.%d" % i: _host(l) for i, l in enumerate(losses)}
        out["grads"] = _host(n._grads)
        trainers[id(n)].step(b)
        out["params"] = _host(n._dev_params)
        return out

    last = None
    for i, s in enumerate(seq):
        what = "%s, step %d (size %d)" % (case, i, s)
        x, tg = _normal((b, 3, s, s), 40 + i), _targets(classes, b, s, s, seed=41 + i)
        held = [(_dev(x), x)]
        want = step(plain, held[0][0], tg)
        if s != last:
            _bind(net, g, "train", (b, s, s))
        got = step(net, held[0][0], tg)
        g.check(what)
        _equal(got, want, what)
        _unchanged(held, what)
        last = s
    _log(case, [g], "")


# ---------------------------------------------------------------- one case per kind of net with a gap of 256 KiB
WIDE_CASES = {"full": None, "window": "window mean k2", "hier": "hier 3,1,1,1,1", "heads": None, "heads window": None, "video": None}


@pytest.mark.parametrize("kind", sorted(WIDE_CASES))
def test_a_gap_of_a_quarter_mebibyte(monkeypatch, kind):
    if kind == "full":
        classes, b, h, w = B
        case = "full %s guard %d" % (_ids(B), WIDE)
        g = _run_case(case, monkeypatch, {}, lambda: _full(classes), (b, h, w), [_normal((b, 3, h, w), 7)], tg=_targets(classes, b, h, w),
                      train=True, guard=WIDE)
        _log(case, [g], "")
    elif kind == "heads":
        _heads_case(monkeypatch, WIDE)
    elif kind == "heads window":
        _heads_window_case(monkeypatch, WIDE)
    elif kind == "video":
        _video_case(monkeypatch, WIDE)
    else:
        _kind_case(monkeypatch, WIDE_CASES[kind], WIDE)


# ---------------------------------------------------------------- the table
def test_zz_the_table_of_this_run():
    """Every FORCED form and every kind of net is in the table with bytes checked; written to profiles/ws_guard.txt when
    the whole file has run in this process (a selection of cases leaves the committed table alone)"""
    n_cases = (len(INFER) + 2 + len(_forced_cases()) + len(SPLIT_INFER) + 1 + 1 + len(KINDS) + 3 + 1 + len(WIDE_CASES))
    if len(TABLE) < n_cases:
        print("\n%d of %d cases ran in this process: the table is written by a run of the whole file" % (len(TABLE), n_cases))
        return
    for envname in F.FORCED:
        assert any(c.startswith("forced %s " % envname) and v[1] > 0 and v[2] for c, v in TABLE.items()), envname
    for kind in ("infer", "heads ", "heads window", "window", "hier", "video", "split_bf16x3 ", "split_bf16x3_train", "syncbn"):
        assert any(c.startswith(kind) and v[1] > 0 for c, v in TABLE.items()), kind
    lines = ["# tests/test_gpu_ws_guard.py: case | regions checked | gap, slack and band bytes checked | conv forms served | result"]
    for c in sorted(TABLE):
        lines.append("%s | %d | %d | %s | %s" % ((c,) + TABLE[c]))
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ws_guard.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
