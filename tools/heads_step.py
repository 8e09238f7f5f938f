"""Heads-only training step vs the full step (yolo3_no_backbone vs yolo3_darknet53 with freeze_base=True), ms per step at
416x416 batch 16 by default: recorded forward + backward + Trainer.step, timed with events over K steps after W warm-up
steps, in a fresh child process.  The heads step's routes are extracted once, as the reference's features workflow does.

    python tools/heads_step.py [--size 416] [--batch 16] [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(args):
    import torch
    import videoyolo_amd as vy
    from videoyolo_amd import autograd, targets

    dev = torch.device("cuda", 0)
    classes = ["c%d" % i for i in range(20)]
    full = vy.yolo3_darknet53(classes, pretrained_base=False, freeze_base=True)
    full.initialize(init="synthetic", seed=233)
    full.collect_params().reset_ctx(dev)
    heads = vy.yolo3_no_backbone(classes)
    heads.set_parameters({p.name: p.data() for p in full.collect_params().values() if not p.backbone})
    heads.collect_params().reset_ctx(dev)
    x = torch.randn((args.batch, 3, args.size, args.size), generator=torch.Generator().manual_seed(0)).to(dev)
    gt_boxes, gt_ids = targets.synthetic_gt(args.batch, args.size, len(classes), m=8, seed=1)
    fixed = targets.YOLOV3PrefetchTargetGenerator(len(classes))(args.size, args.size, gt_boxes, gt_ids, device=dev)
    gt = torch.as_tensor(gt_boxes).to(dev)
    routes = full.extract_features(x)

    def timed(net, inputs):
        tr = vy.Trainer(net.collect_params(), "sgd", {"learning_rate": 1e-4, "wd": 5e-4, "momentum": 0.9})

        def step():
            with autograd.record():
                l = net(*inputs, gt, *fixed)
                autograd.backward([l[0] + l[1] + l[2] + l[3]])
            tr.step(args.batch)
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    full_ms = timed(full, (x,))
    heads_ms = timed(heads, routes)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.warmup):
        full.extract_features(x)
    e0.record()
    for _ in range(args.steps):
        full.extract_features(x)
    e1.record()
    torch.cuda.synchronize()
    extract_ms = e0.elapsed_time(e1) / args.steps
    return {"size": args.size, "batch": args.batch, "steps": args.steps, "warmup": args.warmup,
            "full_step_ms": round(full_ms, 3), "heads_step_ms": round(heads_ms, 3),
            "heads_over_full": round(heads_ms / full_ms, 3), "flop_estimate": round(16.4 / 65.4, 3),
            "extract_features_ms": round(extract_ms, 3),
            "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args)))
        return
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:], cwd=ROOT,
                       stdout=subprocess.PIPE, universal_newlines=True)
    if p.returncode != 0:
        sys.exit(p.returncode)
    print(p.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    main()
