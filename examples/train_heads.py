"""The reference's features workflow on synthetic frames: extract_base_features.py:120-160 runs Darknet-53 once over the
dataset and keeps the three route tensors of every frame; train_yolov3.py --features_dir then trains and validates the
heads alone (yolo3_no_backbone, train_yolov3.py:238-250, 335-343, 444-460, 595-606).  The backbone never runs again.

    python examples/train_heads.py [--size 416] [--batch 16] [--frames 64] [--steps 10] [--out DIR]
"""
import argparse
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None, help="where the <id>_F1/F2/F3.npy files go (default: a temporary directory)")
    args = ap.parse_args()

    import torch
    import videoyolo_amd as vy
    from videoyolo_amd import autograd, metrics, targets

    dev = torch.device("cuda", 0)
    classes = ["c%d" % i for i in range(20)]
    rng = np.random.default_rng(1)
    frames = rng.standard_normal((args.frames, 3, args.size, args.size)).astype(np.float32)
    gt_boxes, gt_ids = targets.synthetic_gt(args.frames, args.size, len(classes), m=4, seed=7)

    # ---- 1. extract_base_features.py: the backbone once over the dataset, three .npy files per frame
    backbone = vy.yolo3_darknet53(classes, pretrained_base=False)
    backbone.initialize(init="synthetic", seed=233)
    backbone.collect_params().reset_ctx(dev)
    out = args.out or tempfile.mkdtemp(prefix="features_")
    os.makedirs(out, exist_ok=True)
    for s in range(0, args.frames, args.batch):
        f = backbone.extract_features(frames[s:s + args.batch])
        for i in range(len(f[0])):
            for k in range(3):
                np.save(os.path.join(out, "%06d_F%d.npy" % (s + i, k + 1)), f[k][i].cpu().numpy())
    print("extracted %d frames x 3 routes into %s" % (args.frames, out))

    def load(ids):
        return [torch.as_tensor(np.stack([np.load(os.path.join(out, "%06d_F%d.npy" % (i, k))) for i in ids])).to(dev)
                for k in (1, 2, 3)]

    # ---- 2. train_yolov3.py --features_dir: the heads alone, initialised from the same model's heads
    net = vy.yolo3_no_backbone(classes)                                            # get_net, :335-343
    backbone_file = os.path.join(out, "full.params")
    backbone.save_parameters(backbone_file)
    net.load_parameters(backbone_file, ignore_extra=True)
    net.collect_params().reset_ctx(dev)
    for p in net.collect_params(".*beta|.*gamma|.*bias").values():                 # --no_wd
        p.wd_mult = 0.0
    trainer = vy.Trainer(net.collect_params(), "sgd", {"learning_rate": 1e-3, "wd": 5e-4, "momentum": 0.9})
    gen = targets.YOLOV3PrefetchTargetGenerator(len(classes))
    for step in range(args.steps):
        ids = [(step * args.batch + i) % args.frames for i in range(args.batch)]
        f1, f2, f3 = load(ids)
        fixed = gen(args.size, args.size, gt_boxes[ids], gt_ids[ids], device=dev)
        with autograd.record():                                                    # :595-606
            obj, ctr, scl, cls = net(f1, f2, f3, torch.as_tensor(gt_boxes[ids]).to(dev), *fixed)
            autograd.backward([obj + ctr + scl + cls])
        trainer.step(args.batch)
        print("step %d  obj %.3f  center %.3f  scale %.3f  cls %.3f" % (
            step, obj.mean().item(), ctr.mean().item(), scl.mean().item(), cls.mean().item()))

    # ---- 3. validation on the same features (:444-460: net(f1, f2, f3) -> ids, scores, bboxes)
    metric = metrics.VOCMApMetric(iou_thresh=0.5, class_names=classes)
    net.set_nms(nms_thresh=0.45, nms_topk=400)
    for s in range(0, args.frames, args.batch):
        ids = list(range(s, min(s + args.batch, args.frames)))
        det_ids, scores, bboxes = [t.cpu().numpy() for t in net(*load(ids))]
        gb = gt_boxes[ids]
        gl = gt_ids[ids]
        metric.update(np.clip(bboxes, 0, args.size), det_ids, scores, gb, gl)
    names, values = metric.get()
    print("%s = %.4f (synthetic weights against random boxes: a plumbing check, not a score)" % (names[-1], values[-1]))


if __name__ == "__main__":
    main()
