"""-m gpu: every launch of the split-fp32 kernels, cell by cell, against the six-products reference
(oracle/split_oracle.py: check_split) on the tensors the device itself read.

conv_split.hip (conv_split_kernel on its three tiles, splitk_finish_kernel), conv_wino.hip, wgrad_split.hip and the
data-gradient use of conv_split_kernel were held only end to end (tests/test_gpu_split.py: heads within 3e-5, gradients
within 2e-3 of a tensor's maximum).  Here every cell that ran on one of them must meet three conditions per element:
(a) the hard rounding bound gamma'_n absum, (b) the product census |beta_p| <= 0.25 for each of the six partial
products, (c) the typical-rounding bar T 2^-24 absum — all derived in oracle/split_oracle.py, and shown to reject wrong
kernels by tests/test_split_cells_sensitivity.py.  VY_SPLIT_ALWAYS=1 sends every supported launch to the split kernels.

Inference ('split_bf16x3', keep_activations; VY_SPLIT_WINO=0: direct form everywhere, =2: Winograd wherever supported):
each walked cell's input is assembled from the device's own taps (concat inputs from train_cells64.graph's src lists),
the epilogue (folded BatchNorm, leaky, residual) is applied in float64, first and last frame, sampled output channels.
A transition cell's stored plane must also be the bit-exact x2 replicate of its own even pixels, cropped to the route.
NOT covered on the GPU: a x2 replicate written PAST the crop.  It would land in the zero border of the concat plane, which
cannot be read back after an inference forward (only training plans have padded taps, and the training forward has no x2
epilogue), and the only cells that read those planes are 1x1, which never touch the border.  What is held here is every
value inside the crop, at both odd route sizes, for conv_split_kernel's ups2 epilogue and splitk_finish_kernel's dx / dy
guards alike.  tests/test_split_cells_sensitivity.py shows only that a border check WOULD reject the fault.
  2 x 64 x 64      stride 32 leaves 8 pixels in a 128-row tile; LW = 2, the Winograd minimum
  3 x 96 x 32      LW = 1 at stride 32: Winograd declines, the direct form serves
  1 x 72 x 104     routes 9x13, 5x7, 3x4: odd widths (the lone Winograd pixel), both crops of the x2 store, one frame
  2 x 128 x 224    80 classes

Training ('split_bf16x3_train'; default routing, and VY_SPLIT_TRAIN=3: forward exact): test_gpu_train_cells' walker
with its three conv checks replaced, for the launches the step's label log names, by their split counterparts.

The census takes the labels of the product's own plans (no VY_SPLIT_ALWAYS) at the bench's shapes and asserts that every
split form they choose — (pass, kernel and tile, k1 or k>1) — is among the walked ones."""
import itertools
import os
import time

import numpy as np
import pytest

import conv_forms as F
import test_gpu_train_cells as TC

pytestmark = pytest.mark.gpu

SWITCHES = sorted(set(F.SWITCHES) | {"VY_SPLIT_ALWAYS", "VY_SPLIT_WINO", "VY_SPLIT_TRAIN", "VY_SPLIT_WGRAD", "VY_SPLIT_FORCE"})
# (frames, height, width, classes)
INFER_CASES = [(2, 64, 64, 20), (3, 96, 32, 20), (1, 72, 104, 20), (2, 128, 224, 80)]
# (classes, batch, height, width); the last: the prediction convs' 255 -> 256 padding
TRAIN_CASES = [(1, 1, 64, 64), (3, 3, 96, 32), (20, 2, 128, 224), (80, 1, 64, 64)]
ROUTING = {"default": {}, "forward_exact": {"VY_SPLIT_TRAIN": "3"}}
# VY_SPLIT_FORCE: under VY_SPLIT_ALWAYS the cost model gives the small shapes above 128x64 (k1 and k-split) and 128x128
# k-split only; the product's plans at the bench's shapes also choose 128x128 k1 and the 256x64 tile (the census below).
# Every tile with k1 and with 4 slabs, forced, at two small shapes each way.
FORCED = ["128x128k1", "128x128k4", "128x64k1", "128x64k4", "256x64k1", "256x64k4"]
FORCED_INFER = {f: ((2, 64, 64, 20) if f.endswith("k1") else (3, 96, 32, 20)) for f in FORCED}
FORCED_TRAIN = {f: ((1, 1, 64, 64) if f.endswith("k1") else (3, 3, 96, 32)) for f in FORCED}
INFER_PLANS = [(64, 608), (1, 608), (16, 416), (1, 416)]
TRAIN_PLAN = (20, 16, 416, 416)

WALKED = {}     # (pass, kernel + tile, "k1" | "k>1") -> {where}
_params = {}
_serial = itertools.count()


def _setenv(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _record(where, forms):
    for f in forms:
        WALKED.setdefault(f, set()).add(where)


def _kk(ks):
    return "k1" if ks == 1 else "k>1"


def _summary(title, res, t0):
    """per check kind: worst err/bound of (a) and (c), worst err/(u absum), the beta range"""
    print("\n%s: %d checks in %.0f s" % (title, len(res), time.time() - t0))
    kinds = sorted({r.kind.rsplit(" ", 2)[0] for r in res if r.kind.endswith(("hard bound", "typical bar", "product census"))})
    for kind in kinds:
        a = [r for r in res if r.kind == kind + " hard bound"]
        c = [r for r in res if r.kind == kind + " typical bar"]
        cen = [r for r in res if r.kind == kind + " product census"]
        b = [x for r in cen for x in r.betas]
        wa, wc, wb = max(a, key=lambda r: r.ratio), max(c, key=lambda r: r.ratio), max(cen, key=lambda r: r.ratio)
        print("  %-24s %3d cells: (a) worst err/bound %.3g (%s); (c) worst err/(T u absum) %.3g (%s), err/(u absum) %.3g; "
              "(b) beta in [%.3f, %.3f] (%s, %d outputs)" % (kind, len(a), wa.ratio, wa.name, wc.ratio, wc.name,
                                                          max(r.headroom for r in c), min(b), max(b), wb.name, wb.n_out))
    bad = [r for r in res if not r.ok]
    assert not bad, "\n".join(repr(r) for r in bad[:40])


# ---------------------------------------------------------------- inference
def _infer_params(ncls):
    if ncls not in _params:
        from videoyolo_amd import init
        from oracle import yolo3_oracle as O
        _params[ncls] = init.synthetic_params(O.param_shapes(ncls), seed=233)
    return _params[ncls]


def _infer_net(ncls):
    import videoyolo_amd as vy
    net = vy.yolo3_darknet53(["c%d" % i for i in range(ncls)], pretrained_base=False)
    net.set_parameters(_infer_params(ncls))
    net.collect_params().reset_ctx("cuda:0")
    net.set_conv_mode("split_bf16x3")
    return net


def _infer_labels(net, x):
    """cell -> ('split' | 'wino', tile, k-split) of the launches of one profiled forward that ran on the split kernels"""
    out = {}
    for label in (r[0] for r in net.profile(x)):
        if "|split" in label:
            cell, form = label.split("|split")
            tile, _, ks = form.partition("k")
            out[cell] = ("split", tile, int(ks) if ks else 1)
        elif "|wino" in label:
            cell, form = label.split("|wino")
            out[cell] = ("wino", form, 1)
    return out


def _walk_infer(net, x, labels, ncls):
    from oracle import split_oracle as S
    from oracle import train_cells64 as R
    from oracle import yolo3_oracle as O
    params = _infer_params(ncls)
    B = x.shape[0]
    sel_img = sorted({0, B - 1})
    cache = {}

    def act(name):
        if name not in cache:
            cache[name] = net.read_activation(name).cpu().numpy()[sel_img]
        return cache[name]

    res, widths = [], {}
    for c in R.graph(ncls):
        name = c["name"]
        if name not in labels:
            continue
        kernel, tile, ks = labels[name]
        a = np.ascontiguousarray(np.concatenate([act(p) for p in c["src"]], 1))
        assert a.shape[1] == c["cin"], (name, a.shape)
        out_all = act(name)
        ch = S.sample_channels(c["cout"], name, out_all[:, 0, ::c["ups"], ::c["ups"]].size)
        w = np.ascontiguousarray(params[name + ".0.weight"][ch])
        sc, sh = O.bn_fold(params[name + ".1.gamma"], params[name + ".1.beta"], params[name + ".1.running_mean"],
                           params[name + ".1.running_var"])
        got = out_all[:, ch]
        if c["ups"] == 2:   # stored x2-replicated, cropped to the route it is concatenated with
            base = np.ascontiguousarray(got[:, :, ::2, ::2])
            res.append(R._exact("x2 store", name, got, R.upsample2(base)[:, :, :got.shape[2], :got.shape[3]]))
            got = base
        ep = S.Epilogue(sc[ch], sh[ch], leaky=True, addends=[act(c["skip"])[:, ch]] if c["skip"] else [])
        k, K = c["k"], c["k"] * c["k"] * c["cin"]
        if kernel == "wino":
            parts, ab = S.wino_parts(a, w)
            res += S.check_split("winograd", name, got, parts, ab, 6 * K + 2, ep)
            widths.setdefault(a.shape[3] % 2, set()).add(name)
        else:
            res += S.check_split("direct %s %s" % (tile, _kk(ks)), name, got, S.six_parts(a, w, c["s"], k // 2),
                                 S.absum(a, w, c["s"], k // 2), 6 * K + ks, ep)
    return res, widths


def _infer_forms(labels):
    return {("infer", kernel + tile, _kk(ks)) for kernel, tile, ks in labels.values()}


def _infer_where(case, wino, force=None):
    return "infer %dx%dx%d, %d classes, VY_SPLIT_WINO=%s%s" % (case[:3] + (case[3], wino, ", VY_SPLIT_FORCE=" + force if force else ""))


def _infer_env(wino, force=None):
    env = {"VY_SPLIT_ALWAYS": "1", "VY_SPLIT_WINO": wino}
    if force:
        env["VY_SPLIT_FORCE"] = force
    return env


INFER_RUNS = [(c, w, None) for c in INFER_CASES for w in ("0", "2")] + [(FORCED_INFER[f], "0", f) for f in FORCED]


@pytest.mark.parametrize("case,wino,force", INFER_RUNS, ids=lambda v: "%dx%dx%d-%d" % v if isinstance(v, tuple) else str(v))
def test_every_split_inference_cell_against_six_products(monkeypatch, case, wino, force):
    t0 = time.time()
    B, H, W, ncls = case
    _setenv(monkeypatch, _infer_env(wino, force))
    x = np.random.default_rng(H * 1000 + W).standard_normal((B, 3, H, W)).astype(np.float32)
    net = _infer_net(ncls)
    net.keep_activations()
    labels = _infer_labels(net, x)
    net(x)
    assert len(labels) == 70, sorted(labels)   # all but the stem, the 64 -> 32 bottleneck and the prediction convs
    res, widths = _walk_infer(net, x, labels, ncls)
    n_wino = sum(1 for v in labels.values() if v[0] == "wino")
    print("\nforms: %s; Winograd cells %d (odd input width %d, even %d)"
          % (sorted(_infer_forms(labels)), n_wino, len(widths.get(1, ())), len(widths.get(0, ()))))
    from oracle import train_cells64 as R
    by_name = {c["name"]: c for c in R.graph(ncls)}
    can = {c["name"] for c in R.graph(ncls) if c.get("k") == 3 and c["s"] == 1 and c["cout"] % 128 == 0 and c["cin"] % 32 == 0}
    assert len(can) == 31
    if (H, W) == (96, 32):   # LW = 1 at stride 32: Winograd declines those cells, the direct form serves them
        can = {n for n in can if not n.startswith(("stages.2", "yolo_blocks.0"))}
    assert {n for n, v in labels.items() if v[0] == "wino"} == (can if wino == "2" else set())
    if wino == "2" and (H, W) == (72, 104):
        assert widths.get(1) and widths.get(0), widths   # the lone last pixel, and pairs only
    if force:   # the forced form served every launch it can serve (a k-split: as far as the k-steps and the scratch allow)
        tile, ks = force.split("k")
        for n, v in labels.items():
            assert v[1] == tile or by_name[n]["cout"] % int(tile.split("x")[1]), (n, v)
            assert v[2] <= int(ks), (n, v)
        assert any(v[1] == tile and (v[2] > 1) == (int(ks) > 1) for v in labels.values()), sorted(set(labels.values()))
    _summary(_infer_where(case, wino, force), res, t0)
    _record(_infer_where(case, wino, force), _infer_forms(labels))
    for odd in widths:
        _record(_infer_where(case, wino, force), {("infer", "wino64x128 %s width" % ("odd" if odd else "even"), "k1")})


def test_inference_cases_cover_every_tile_with_and_without_k_split_and_both_winograd_widths(monkeypatch):
    """From the launch labels of the walked cases alone (profile only where a case has not run in this process)"""
    met = _infer_met(monkeypatch)
    for tile in ("split128x128", "split128x64", "split256x64"):
        for kk in ("k1", "k>1"):
            assert ("infer", tile, kk) in met, "no walked inference launch ran as %s %s: %s" % (tile, kk, sorted(met))
    assert ("infer", "wino64x128 odd width", "k1") in met and ("infer", "wino64x128 even width", "k1") in met, sorted(met)


def _infer_met(monkeypatch):
    met = {f: set(w) for f, w in WALKED.items() if f[0] == "infer"}
    for case, wino, force in INFER_RUNS:
        where = _infer_where(case, wino, force)
        if any(where in w for w in met.values()):
            continue
        B, H, W, ncls = case
        _setenv(monkeypatch, _infer_env(wino, force))
        net = _infer_net(ncls)
        net.keep_activations()
        labels = _infer_labels(net, np.zeros((B, 3, H, W), np.float32))
        forms = _infer_forms(labels)
        for n, v in labels.items():   # (a stride-1 cell: its input is as wide as its output)
            if v[0] == "wino":
                forms.add(("infer", "wino64x128 %s width" % ("odd" if net.read_activation(n).shape[3] % 2 else "even"), "k1"))
        for f in forms:
            met.setdefault(f, set()).add(where + " (profile only in this run)")
    return met


# ---------------------------------------------------------------- training
def read_split_labels(path, uniform=True):
    """The label file of one training step -> dict(fwd={cell: k-split}, dgrad={cell: k-split}, wgrad={cell: splits}) of
    the launches that ran on the split kernels, and the set of forms (pass, kernel + tile, k1 | k>1).  A stride-2 conv's
    data gradient is four launches (parity classes of 1, 2, 2 and 4 taps, each with the k-split its own K gets): all four
    must have gone to the same kernel, and the cell's entry is the largest k-split (a pixel belongs to one class, so
    its addition count is at most that class's).  uniform=False (the census: the cost model routes launch by launch):
    forms only, a cell may have launches on both kernels."""
    fwd, dgrad, wgrad, forms, last = {}, {}, {}, set(), None
    routed = {}
    with open(path) as f:
        for line in f:
            t = line.split()
            if not t:
                continue
            if t[0] != "#":
                last = (t[0], t[1])
                continue
            kind, name = last
            if kind == "wgrad":
                if t[2] == "wgrad_split_kernel":
                    wgrad[name] = int(t[4])
                    forms.add(("wgrad", "wgrad_split_kernel", _kk(int(t[4]))))
                continue
            routed.setdefault((kind, name), set()).add(t[2])
            if t[2] != "split":
                continue
            ks = int(t[4][1:])
            if kind == "fwd":
                fwd[name] = ks
            else:
                dgrad[name] = max(dgrad.get(name, 1), ks)
            forms.add((kind, "split" + t[3], _kk(ks)))
    mixed = [k for k, v in routed.items() if len(v) > 1]
    assert not (uniform and mixed), "launches of one cell on both kernels: %s" % mixed
    return dict(fwd=fwd, dgrad=dgrad, wgrad=wgrad), forms


TRAIN_RUNS = [(s, r, None) for s in TRAIN_CASES for r in sorted(ROUTING)] + [(FORCED_TRAIN[f], "default", f) for f in FORCED]


def _train_step(monkeypatch, tmp_path, routing, shape, always=True, force=None):
    """One recorded step in conv mode 'split_bf16x3_train' -> (the builder's dict, the split launches, their forms)"""
    env = dict(ROUTING[routing])
    if always:
        env["VY_SPLIT_ALWAYS"] = "1"
    if force:
        env["VY_SPLIT_FORCE"] = force
    labels = str(tmp_path / ("labels_%d.txt" % next(_serial)))
    env["VY_TRAIN_LABELS"] = labels
    _setenv(monkeypatch, env)
    st = TC._step(*shape, mode="split_bf16x3_train")
    split, forms = read_split_labels(labels, uniform=always)
    os.remove(labels)
    return st, split, forms


def _train_where(routing, shape, force=None):
    return "train %s %s%s" % ("x".join(str(v) for v in shape), routing, ", VY_SPLIT_FORCE=" + force if force else "")


@pytest.mark.parametrize("shape,routing,force", TRAIN_RUNS, ids=lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v))
def test_every_split_training_cell_against_six_products(monkeypatch, tmp_path, shape, routing, force):
    t0 = time.time()
    st, split, forms = _train_step(monkeypatch, tmp_path, routing, shape, force=force)
    by_name = {c["name"]: c for c in st["cells"]}
    print("\nsplit launches: %d forward, %d data gradients, %d weight gradients; forms %s"
          % (len(split["fwd"]), len(split["dgrad"]), len(split["wgrad"]), sorted(forms)))
    # the launches this test is about really ran on the split kernels
    assert (len(split["fwd"]) == 70) == (routing == "default") and (routing == "default" or not split["fwd"])
    dg = split["dgrad"]
    assert any(by_name[n]["s"] == 2 for n in dg), "no stride-2 data gradient on the split kernel"
    assert all("yolo_outputs.%d.prediction" % i in dg for i in range(3)), "a prediction conv's data gradient stayed exact"
    assert any(n.endswith(".body.0") and n.startswith("stages.") for n in dg), "no split data gradient into a skip gradient"
    assert split["wgrad"], "no weight gradient on wgrad_split_kernel"
    res, _ = TC._walk(st, split)
    kinds = {r.kind for r in res}
    assert {"split data gradient hard bound", "split weight gradient product census"} <= kinds
    assert ("split forward conv typical bar" in kinds) == (routing == "default")
    assert "forward conv" in kinds   # the stem, the 64 -> 32 bottleneck (and everything under forward_exact): bit-equal
    if force:   # forward launches carry statistics and are never k-split
        tile, want = "split" + force.split("k")[0], "k1" if force.endswith("k1") else "k>1"
        assert all(f[2] == "k1" for f in forms if f[0] == "fwd" or want == "k1" and f[0] == "dgrad"), sorted(forms)
        assert ("fwd", tile, "k1") in forms and ("dgrad", tile, want) in forms, sorted(forms)
    _summary(_train_where(routing, shape, force), res, t0)
    TC._report(_train_where(routing, shape, force), res, t0, census=st["census"])
    _record(_train_where(routing, shape, force), forms)


def _train_met(monkeypatch, tmp_path):
    import torch
    met = {f: set(w) for f, w in WALKED.items() if f[0] != "infer"}
    for shape, routing, force in TRAIN_RUNS:
        where = _train_where(routing, shape, force)
        if any(where in w for w in met.values()):
            continue
        st, _, forms = _train_step(monkeypatch, tmp_path, routing, shape, force=force)
        torch.cuda.synchronize()
        del st
        for f in forms:
            met.setdefault(f, set()).add(where + " (labels only in this run)")
    return met


def test_training_cases_cover_a_k_split_data_gradient(monkeypatch, tmp_path):
    met = _train_met(monkeypatch, tmp_path)
    assert any(f[0] == "dgrad" and f[2] == "k>1" for f in met), sorted(met)
    # weight gradients with more than one slab: stated by the census below, whichever way it falls
    print("\nwalked wgrad_split_kernel forms: %s" % sorted(f for f in met if f[0] == "wgrad"))


# ---------------------------------------------------------------- the census
def test_census_every_split_form_the_products_plans_choose_is_walked(monkeypatch, tmp_path):
    """Labels only, no walk, of the product's own plans (no VY_SPLIT_ALWAYS): inference at 64 x 608^2, 1 x 608^2,
    16 x 416^2, 1 x 416^2, training at 416 x 416 batch 16, 20 classes.  (Winograd's form is one: its odd / even width
    rows are the walked cases' own.)"""
    import torch
    met = _infer_met(monkeypatch)
    met.update(_train_met(monkeypatch, tmp_path))
    chosen = {}
    _setenv(monkeypatch, {})
    for batch, size in INFER_PLANS:
        net = _infer_net(20)
        for f in _infer_forms(_infer_labels(net, np.zeros((batch, 3, size, size), np.float32))):
            chosen.setdefault(f, set()).add("infer %dx%d batch %d" % (size, size, batch))
        del net
        torch.cuda.empty_cache()
    st, _, forms = _train_step(monkeypatch, tmp_path, "default", TRAIN_PLAN, always=False)
    torch.cuda.synchronize()
    del st
    for f in forms:
        chosen.setdefault(f, set()).add("train %dx%d batch %d" % (TRAIN_PLAN[2], TRAIN_PLAN[3], TRAIN_PLAN[1]))
    print("\nsplit forms the product's plans choose -> where every element is checked")
    for f in sorted(chosen):
        where = sorted(met.get(f, ()))
        print("  %-8s %-20s %-4s chosen at %s\n      %s" % (f + ("; ".join(sorted(chosen[f])), "; ".join(where[:3]) + (
            " (+%d more)" % (len(where) - 3) if len(where) > 3 else "") if where else "NOT CHECKED")))
    print("walked, chosen by no plan of the census: %s" % sorted(set(met) - set(chosen)))
    missing = sorted(set(chosen) - set(met))
    assert not missing, "chosen by a plan of the product, walked by no per-cell test: %s" % missing
