"""Launch forms of the exact conv kernel (conv_igemm.hip), as the GPU tests name them.

A form is (pass, tile + schedule):
  pass      "fwd"     training forward of a BatchNorm cell, per-tile statistics sums
            "pred"    training forward of a prediction conv (bias, no statistics)
            "dgrad"   data gradient of a stride-1 conv
            "dgrad/2" one parity-class launch of a stride-2 conv's data gradient
            "infer"   inference forward
  tile      128x128, 128x64, 128x32, 64x64 (two LDS stages), 64x64s4 (four)
  schedule  ""  plain, "sk" stream-K, "ks<S>" split-K over the S runs of K, "ck<S>" one workgroup running the S runs in
            turn with parked chains, "ck<S>sk" stream-K pieces of those

The training step writes the form of every launch itself (VY_TRAIN_LABELS, the '# via exact <tile><schedule>' lines:
train.hip's LabelLog, from the plan the launch executed: vy_conv_plan_label of conv_launch.h).  The inference profile's
label is the same plan in its shorter style, the tile and sk / ks<S> only; infer_form() adds the stages and the parked
chains by RESTATING two rules of the plan (the four-stage condition of vy_conv_plan_exact in conv_launch.h and
vy_conv_runs of include/vy_math.h) — a restatement, to be kept in step by hand.

FORCED lists the switch settings under which the per-cell tests run; names are the test ids."""
import re

# name -> environment (read by a net at its creation)
FORCED = {
    "plain128x128": {"VY_CONV_SK": "0", "VY_CONV_FORCE": "128x128"},
    "plain128x64": {"VY_CONV_SK": "0", "VY_CONV_FORCE": "128x64"},
    "plain128x32": {"VY_CONV_SK": "0", "VY_CONV_FORCE": "128x32"},
    "plain64x64": {"VY_CONV_SK": "0", "VY_CONV_FORCE": "64x64"},
    "sk5_128x128": {"VY_CONV_SK": "1", "VY_CONV_SK_SLOTS": "5", "VY_CONV_FORCE": "128x128"},
    "sk13_64x64": {"VY_CONV_SK": "1", "VY_CONV_SK_SLOTS": "13", "VY_CONV_FORCE": "64x64"},
    "sk24_128x64": {"VY_CONV_SK": "1", "VY_CONV_SK_SLOTS": "24", "VY_CONV_FORCE": "128x64"},
    "sk13": {"VY_CONV_SK": "1", "VY_CONV_SK_SLOTS": "13"},
    "parked": {"VY_CONV_KSPLIT": "0"},
    "parked_sk13": {"VY_CONV_KSPLIT": "0", "VY_CONV_SK": "1", "VY_CONV_SK_SLOTS": "13"},
    "main_stream_wgrad": {"VY_TRAIN_SIDE_STREAM": "0"},
}
SWITCHES = sorted({k for env in FORCED.values() for k in env} | {"VY_TRAIN_LABELS"})

_FORM = re.compile(r"^(128x128|128x64|128x32|64x64)(s4)?(sk|ks\d+|ck\d+(?:sk)?)?$")


def split_form(form):
    """'64x64s4ck4sk' -> ('64x64s4', 'ck4sk'); raises on anything the launcher cannot have written"""
    m = _FORM.match(form)
    assert m, "not a conv form: %r" % form
    return m.group(1) + (m.group(2) or ""), m.group(3) or ""


def read_labels(path, cells):
    """The label file of one training step -> (conv launches [(pass, cell, form, M, N, K)], weight gradients
    [(cell, kernel, splits, reduce, stream)]).  `cells`: oracle.train_cells64.graph(...) of the net that ran."""
    by_name = {c["name"]: c for c in cells if "k" in c}
    convs, wgrads, last = [], [], None
    with open(path) as f:
        for line in f:
            t = line.split()
            if not t:
                continue
            if t[0] != "#":
                last = (t[0], t[1], int(t[3]), int(t[4]), int(t[5]))
                continue
            assert t[1] == "via" and last is not None, line
            kind, name, M, N, K = last
            last = None
            c = by_name[name]
            if kind == "wgrad":
                assert t[3] == "splits" and t[5] == "reduce" and t[7] == "stream", line
                wgrads.append((name, t[2], int(t[4]), t[6], t[8]))
                continue
            assert t[2] in ("exact", "split"), line
            if t[2] != "exact":
                continue
            split_form(t[3])
            p = ("fwd" if c["bn"] else "pred") if kind == "fwd" else ("dgrad" if c["s"] == 1 else "dgrad/2")
            convs.append((p, name, t[3], M, N, K))
    assert last is None, "a launch line without its '# via' line: %r" % (last,)
    return convs, wgrads


def forms_of(convs):
    return {(p, form) for p, _, form, _, _, _ in convs}


def check_served(envname, convs, wgrads):
    """The launches of a step under FORCED[envname] are what the name says — else the test that walked them checked
    something else.  A stream-K form must have served a data gradient and a training forward with statistics."""
    env = FORCED.get(envname, {})
    parts = [(p,) + split_form(form) for p, _, form, _, _, _ in convs]
    assert parts and wgrads, "the step wrote no launch labels"
    tile = env.get("VY_CONV_FORCE")
    if tile:
        assert {t.replace("s4", "") for _, t, _ in parts} == {tile}, sorted({t for _, t, _ in parts})
    sk = {p for p, _, sched in parts if sched.endswith("sk")}
    if env.get("VY_CONV_SK_SLOTS"):
        assert "fwd" in sk and sk & {"dgrad", "dgrad/2"}, "stream-K served %s only" % sorted(sk)
    if env.get("VY_CONV_SK") == "0":
        assert not sk and not any(sched.startswith("ks") for _, _, sched in parts)
        assert any(p == "fwd" and sched.startswith("ck") for p, _, sched in parts)    # K in runs: parked, never split
    if env.get("VY_CONV_KSPLIT") == "0":
        assert not any(sched.startswith("ks") for _, _, sched in parts)
        want = "sk" if env.get("VY_CONV_SK_SLOTS") else ""
        assert any(p == "fwd" and re.match(r"ck\d+%s$" % want, sched) for p, _, sched in parts), sorted(set(parts))
    streams = {w[4] for w in wgrads}
    assert streams == ({"main"} if env.get("VY_TRAIN_SIDE_STREAM") == "0" else {"side"}), streams


# What the per-cell tests have walked in this process: (pass, form) -> {where}; the census reads it and runs (labels or
# profile only) whatever case is missing, so it gives the same table when it runs alone.
WALKED = {}


def record(where, forms):
    for f in forms:
        WALKED.setdefault(f, set()).add(where)


def infer_form(label, flops, cin, cout, k):
    """('infer', form) of one row of net.profile(): '<cell>|<tile>[sk|ks<S>]' plus the stages and the parked chains.
    RESTATES the launcher: four stages where a 64x64 launch has at most 512 tiles and at least 8 k-steps; K is summed
    in 4 runs where K >= 4096 and the k-steps divide by 16, and a launch that is not split-K parks them."""
    form = label.split("|")[1]
    tile, sched = split_form(form)
    kc = (cin + 31) // 32 * 32
    T = k * k * kc // 32
    M = int(round(flops / (2.0 * cout * k * k * kc)))
    if tile == "64x64" and -(-M // 64) * -(-cout // 64) <= 512 and T >= 8:
        tile += "s4"
    runs = 4 if (T * 32 >= 4096 and T % 16 == 0) else 1
    if runs > 1 and not sched.startswith("ks"):
        sched = "ck%d%s" % (runs, sched)
    return ("infer", tile + sched)


def conv_info(net):
    """cell name -> (cin, cout, k) of every conv of a net"""
    import ctypes
    from videoyolo_amd import _lib
    out = {}
    for i in range(net._lib.vy_net_num_convs(net._h)):
        info = _lib.ConvInfo()
        _lib.check(net._lib.vy_net_conv_info(net._h, i, ctypes.byref(info)))
        out[info.name.decode()] = (info.cin, info.cout, info.kernel)
    return out


def infer_forms(net, x):
    """[(cell, ('infer', form))] of the exact conv launches of one profiled forward (the stem has its own kernel)"""
    info = conv_info(net)
    out = []
    for label, _, flops, _ in net.profile(x):
        if "|" not in label:
            continue
        cell = label.split("|")[0]
        out.append((cell, infer_form(label, flops, *info[cell])))
    return out
