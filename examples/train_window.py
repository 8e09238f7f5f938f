"""The reference's temporal window on synthetic clips: train_yolov3.py --window k --k_join_type max --k_join_pos early
(train_yolov3.py:133, 384-392) builds a YOLOV3T whose Darknet-53 stages see every frame of a k-frame clip and whose heads
see the routes pooled over the clip; the labels are the clip's sample frame's (datasets/imgnetvid.py:190-224).  A few
training steps from a single-frame model's parameters, then a validation pass with detect_yolo3.py's surface.

    python examples/train_window.py [--size 416] [--clips 8] [--k 3] [--join max] [--steps 5]
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
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--join", default="max", choices=("max", "mean"))
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()

    import torch
    import videoyolo_amd as vy
    from videoyolo_amd import autograd, metrics, targets

    dev = torch.device("cuda", 0)
    classes = ["c%d" % i for i in range(20)]
    n = 2 * args.clips
    rng = np.random.default_rng(1)
    clips = rng.standard_normal((n, args.k, 3, args.size, args.size)).astype(np.float32)
    gt_boxes, gt_ids = targets.synthetic_gt(n, args.size, len(classes), m=4, seed=7)  # one label set per clip

    # start from a single-frame model's file: its stage keys lack TimeDistributed's '.model.', the tensors are the same
    single = vy.yolo3_darknet53(classes, pretrained_base=False)
    single.initialize(init="synthetic", seed=233)
    path = os.path.join(tempfile.mkdtemp(prefix="window_"), "single.params")
    single.save_parameters(path)
    net = vy.yolo3_darknet53(classes, pretrained_base=False, k=args.k, k_join_type=args.join, k_join_pos="early")
    net.load_parameters(path, ctx=dev)
    for p in net.collect_params(".*beta|.*gamma|.*bias").values():                 # --no_wd
        p.wd_mult = 0.0
    trainer = vy.Trainer(net.collect_params(), "sgd", {"learning_rate": 1e-3, "wd": 5e-4, "momentum": 0.9})
    gen = targets.YOLOV3PrefetchTargetGenerator(len(classes))
    for step in range(args.steps):
        ids = [(step * args.clips + i) % n for i in range(args.clips)]
        fixed = gen(args.size, args.size, gt_boxes[ids], gt_ids[ids], device=dev)
        with autograd.record():
            obj, ctr, scl, cls = net(clips[ids], torch.as_tensor(gt_boxes[ids]).to(dev), *fixed)
            autograd.backward([obj + ctr + scl + cls])
        trainer.step(args.clips)
        print("step %d  obj %.3f  center %.3f  scale %.3f  cls %.3f" % (
            step, obj.mean().item(), ctr.mean().item(), scl.mean().item(), cls.mean().item()))

    metric = metrics.VOCMApMetric(iou_thresh=0.5, class_names=classes)
    net.set_nms(nms_thresh=0.45, nms_topk=400)
    for s in range(0, n, args.clips):
        ids = list(range(s, min(s + args.clips, n)))
        det_ids, scores, bboxes = [t.cpu().numpy() for t in net(clips[ids])]
        metric.update(np.clip(bboxes, 0, args.size), det_ids, scores, gt_boxes[ids], gt_ids[ids])
    names, values = metric.get()
    print("%s = %.4f (synthetic weights against random boxes: a plumbing check, not a score)" % (names[-1], values[-1]))


if __name__ == "__main__":
    main()
