"""The reference's hierarchical Darknet on synthetic clips: train_yolov3.py --new_model --hier 3,3,1,1,1 --h_join_type max
builds a YOLOV3TB over HDarknet (wrappers.py:40-44, h_darknet.py:103-188): a clip of T = 9 frames goes through the stem
frame by frame, consecutive triples of frames are max-pooled in front of each of the first two stride-2 convs, and from
there on the net is the single-frame one on the clips.  The max has no parameters, so a single-frame model's file is a valid
start.  A few augmented training steps (YOLO3VideoTrainTransform with k = T: one draw per clip, one launch per batch) from
such a file, then a validation pass with detect_yolo3.py's surface.

--join conv trains the reference's learned join instead (--h_join_type conv: a per-channel 3-tap filter over each triple,
BatchNorm, LeakyReLU; videoyolo_amd.YOLOV3HierConv).  The joins have parameters of their own, which the single-frame file
does not hold: it loads with allow_missing=True and the joins keep their start — here a mean, every weight 1/3, because the
reference's own start, all zeros, makes every joined plane a constant until the first updates have moved the weights.

    python examples/train_hier.py [--join max|conv] [--size 416] [--clips 4] [--hier 3,3,1,1,1] [--steps 5] [--src 240x320]
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
    ap.add_argument("--clips", type=int, default=4)
    ap.add_argument("--hier", default="3,3,1,1,1")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--src", default="240x320", help="height x width of the synthetic source frames")
    ap.add_argument("--join", choices=("max", "conv"), default="max", help="how a triple of frames is joined (h_join_type)")
    args = ap.parse_args()

    import random
    import torch
    import videoyolo_amd as vy
    from videoyolo_amd import autograd, metrics, targets
    from videoyolo_amd.transforms import YOLO3VideoTrainTransform

    dev = torch.device("cuda", 0)
    classes = ["c%d" % i for i in range(20)]
    hier = [int(v) for v in args.hier.split(",")]
    sh, sw = [int(v) for v in args.src.split("x")]

    # start from a single-frame model's file: the keys are the same, the pools add none
    single = vy.yolo3_darknet53(classes, pretrained_base=False)
    single.initialize(init="synthetic", seed=233)
    path = os.path.join(tempfile.mkdtemp(prefix="hier_"), "single.params")
    single.save_parameters(path)
    if args.join == "conv":
        net = vy.YOLOV3HierConv(classes, hierarchical=hier)
        net.initialize()                                                                 # the joins: zeros, as the reference
        for name, p in net.collect_params(r"hjoin\.\d\.0\.weight").items():             # ... moved to a mean start
            p.set_data(np.full(p.shape, 1.0 / 3.0, np.float32))
        net.load_parameters(path, ctx=dev, allow_missing=True)
    else:
        net = vy.yolo3_darknet53(classes, pretrained_base=False, new_model=True, hierarchical=hier, h_join_type="max")
        net.load_parameters(path, ctx=dev)
    t = net.frames
    print("hierarchical %s%s: clips of %d frames" % (net.hierarchical, " (conv join)" if args.join == "conv" else "", t))

    n = 2 * args.clips
    rng = np.random.default_rng(1)
    videos = [rng.integers(0, 256, (t, sh, sw, 3), dtype=np.uint8) for _ in range(n)]     # decoded clips
    labels = []
    for i in range(n):                                                                   # one label set per clip
        x0, y0 = rng.uniform(0, sw * 0.5, 3), rng.uniform(0, sh * 0.5, 3)
        w, h = rng.uniform(sw * 0.2, sw * 0.45, 3), rng.uniform(sh * 0.2, sh * 0.45, 3)
        labels.append(np.stack([x0, y0, x0 + w, y0 + h, rng.integers(0, len(classes), 3)], 1).astype(np.float32))

    for p in net.collect_params(".*beta|.*gamma|.*bias").values():                       # --no_wd
        p.wd_mult = 0.0
    trainer = vy.Trainer(net.collect_params(), "sgd", {"learning_rate": 1e-3, "wd": 5e-4, "momentum": 0.9})
    transform = YOLO3VideoTrainTransform(t, args.size, args.size, net, rng=(random.Random(3), np.random.RandomState(3)))
    for step in range(args.steps):
        ids = [(step * args.clips + i) % n for i in range(args.clips)]
        x, gt, *fixed = transform.batch([videos[i] for i in ids], [labels[i] for i in ids], device=dev)
        with autograd.record():
            obj, ctr, scl, cls = net(x, gt, *fixed)
            autograd.backward([obj + ctr + scl + cls])
        trainer.step(args.clips)
        print("step %d  obj %.3f  center %.3f  scale %.3f  cls %.3f" % (
            step, obj.mean().item(), ctr.mean().item(), scl.mean().item(), cls.mean().item()))

    # validation: resized, normalised clips through the inference branch, one detection set per clip
    metric = metrics.VOCMApMetric(iou_thresh=0.5, class_names=classes)
    net.set_nms(nms_thresh=0.45, nms_topk=400)
    val = rng.standard_normal((n, t, 3, args.size, args.size)).astype(np.float32)
    gt_boxes, gt_ids = targets.synthetic_gt(n, args.size, len(classes), m=4, seed=7)
    for s in range(0, n, args.clips):
        ids = list(range(s, min(s + args.clips, n)))
        det_ids, scores, bboxes = [a.cpu().numpy() for a in net(val[ids])]
        metric.update(np.clip(bboxes, 0, args.size), det_ids, scores, gt_boxes[ids], gt_ids[ids])
    names, values = metric.get()
    print("%s = %.4f (synthetic weights against random boxes: a plumbing check, not a score)" % (names[-1], values[-1]))


if __name__ == "__main__":
    main()
