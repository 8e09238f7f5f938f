"""The bits a training step leaves, one sha256 per item: what two builds of the library are compared by.

The float64 cell tests hold every training kernel to a tolerance, and a changed summation order passes a tolerance.  This
tool holds the bits: run it on a checkout of the commit to compare with and on the change, and `diff` the two outputs.

    python tools/train_bits.py [--only NAME ...] > bits.txt

For every configuration a fresh child process runs, on seeded parameters, frames and targets, two recorded steps
(forward, backward) each followed by Trainer.step, and prints `configuration item sha256` over the raw bytes of: the four
loss vectors of both steps; every parameter gradient and every running mean and variance after step 1 (before its
Trainer.step); every parameter after step 2.  The `raw` configuration runs the train-mode, non-recording forward instead
and hashes its five device outputs (the per-anchor tensors of raw_preds_kernel).

Run-to-run equality on ONE build is the precondition of comparing two, and it is what train_kernels.hip's header
promises: the child runs its configuration twice, on two fresh nets, and fails, naming the items, if the runs differ.

Configurations: the full net at the bench's training shape and at a small 32-wide one, each in conv modes exact and
split_bf16x3_train; the full net with a statistics callback installed (world 1, the exchange is the identity: the
reduce_partials + bn_finalize / bn_bwd_finalize path of the synchronised cells); the window net; the heads net on the
routes of a full net; the raw predictions at the bench's shape.
"""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 7
# name -> (kind, shape, conv mode); shape = (classes, batch, height, width), the window net's (join, k, clips, height, width)
CONFIGS = {
    "full416_exact": ("full", (20, 16, 416, 416), "exact"),
    "full416_split": ("full", (20, 16, 416, 416), "split_bf16x3_train"),
    "full96x32_exact": ("full", (3, 3, 96, 32), "exact"),
    "full96x32_split": ("full", (3, 3, 96, 32), "split_bf16x3_train"),
    "sync64_world1": ("sync", (3, 2, 64, 64), "exact"),
    "window_max_k2": ("window", ("max", 2, 2, 64, 64), "exact"),
    "heads96x32": ("heads", (3, 3, 96, 32), "exact"),
    "raw416": ("raw", (20, 16, 416, 416), "exact"),
}
WINDOW_CLASSES = 3
CHILD_TIMEOUT_S = 900
RUNS_DIFFER = 3  # the child's exit status when its two runs differ


def _sha(a):
    import numpy as np
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _host(t):
    return t.detach().cpu().numpy()


def run_once(kind, shape, mode):
    """One pass over a fresh net: the list of (item, sha256)."""
    import numpy as np
    import videoyolo_amd as vy
    from videoyolo_amd import _lib, autograd, init
    from oracle import targets_oracle as T
    from oracle import yolo3_oracle as O

    if kind == "window":
        join, k, B, H, W = shape
        C = WINDOW_CLASSES
    else:
        (C, B, H, W), k = shape, 1
    classes = ["c%d" % i for i in range(C)]
    params = init.synthetic_params(O.param_shapes(C), seed=SEED)
    gt_boxes, gt_ids = T.synthetic_gt(B, min(H, W), C, m=3, seed=SEED, pad_to=4)
    tg = T.prefetch_targets(C, H, W, gt_boxes, gt_ids)
    rng = np.random.default_rng(SEED + H + W + k)
    x = rng.standard_normal((B, 3, H, W) if k == 1 else (B, k, 3, H, W)).astype(np.float32)

    def full_net(**kw):
        net = vy.yolo3_darknet53(classes, pretrained_base=False, **kw)
        net.set_parameters(params)
        net.collect_params().reset_ctx("cuda:0")
        return net

    if kind == "heads":
        routes = full_net().extract_features(x)
        net = vy.yolo3_no_backbone(classes)
        net.set_parameters({n: v for n, v in params.items() if not n.startswith("stages.")})
        net.collect_params().reset_ctx("cuda:0")
        inputs = tuple(routes)
    elif kind == "window":
        net = full_net(k=k, k_join_type=join, k_join_pos="early")
        inputs = (x,)
    else:
        net = full_net()
        inputs = (x,)
    if mode != "exact":
        net.set_conv_mode(mode)

    if kind == "raw":
        with autograd.train_mode():
            out = net(*inputs)
        names = {0: "box", 4: "centers", 5: "scales", 6: "objness", 7: "class_pred"}  # (items 1-3 are host constants)
        return [("raw_preds." + names[i], _sha(_host(out[i]))) for i in sorted(names)]

    def recorded():
        with autograd.record():
            losses = net(*inputs, gt_boxes, *tg)
            autograd.backward([losses[0] + losses[1] + losses[2] + losses[3]])
        return [_host(l) for l in losses]

    if kind == "sync":
        # as tests/test_gpu_syncbn_cells.py installs one: after a first recorded step has bound the workspace.  World 1,
        # the all-reduce is the identity: the callback leaves the sums as they are
        recorded()
        keep = _lib.ALLREDUCE_CB(lambda user, ptr, count: 0)
        net._cb_keep.append(keep)
        _lib.check(net._lib.vy_net_set_sync_bn(net._h, 1, keep, None))

    trainer = vy.Trainer(net.collect_params(), "sgd", {"learning_rate": 1e-3, "wd": 5e-4, "momentum": 0.9})
    items = []
    ps = list(net.collect_params().values())
    for step in (1, 2):
        for q, l in zip(("obj", "center", "scale", "cls"), recorded()):
            items.append(("step%d.loss.%s" % (step, q), _sha(l)))
        if step == 1:
            items += [("step1.grad." + p.name, _sha(net.grad(p.name))) for p in ps if p.trainable]
            items += [("step1." + p.name, _sha(p.data())) for p in ps if p.kind in ("running_mean", "running_var")]
        trainer.step(B)
    items += [("step2.param." + p.name, _sha(p.data())) for p in ps]
    return items


def child(name):
    kind, shape, mode = CONFIGS[name]
    first, second = run_once(kind, shape, mode), run_once(kind, shape, mode)
    differ = [a[0] for a, b in zip(first, second) if a != b]
    if differ or len(first) != len(second):
        sys.stderr.write("%s: two runs on one build differ in %d of %d items: %s\n"
                         % (name, len(differ), len(first), " ".join(differ[:20])))
        return RUNS_DIFFER
    for item, h in first:
        print("%s %s %s" % (name, item, h))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="+", choices=sorted(CONFIGS), help="these configurations only")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    status = 0
    for name in args.only or CONFIGS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], cwd=ROOT, stdout=subprocess.PIPE,
                               universal_newlines=True, timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            sys.exit("%s did not finish within %d s" % (name, CHILD_TIMEOUT_S))
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode == RUNS_DIFFER:
            print("%s FAILED the run-twice precondition" % name)
            status = 1
        elif p.returncode:  # the child failed or crashed: nothing more is started on the device
            sys.exit("%s: child ended with status %d" % (name, p.returncode))
    return status


if __name__ == "__main__":
    sys.exit(main())
