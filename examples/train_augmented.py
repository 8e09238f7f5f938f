"""Training on augmented clips: the reference's train_dataset.transform(YOLO3VideoTrainTransform(k, w, h, net))
(train_yolov3.py:241-267) on synthetic uint8 videos of differing sizes with moving boxes.  Each batch is drawn on the
host (colour distortion, expansion, constrained crop, random interpolation, flip — the reference's draws in the
reference's order), its frames are transformed by ONE HIP launch and its targets by one more, and the result goes
straight into the training call: a k-frame window net first, then a single-frame net.

    python examples/train_augmented.py [--size 416] [--clips 8] [--k 3] [--steps 4] [--seed 233]
"""
import argparse
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic_video(rng, frames, h, w, boxes):
    """frames x (h, w, 3) uint8: a textured background and `boxes` bright rectangles drifting a few pixels per frame.
    Returns the video and, per frame, its (boxes, 5) label [x1, y1, x2, y2, class]."""
    y, x = np.mgrid[0:h, 0:w]
    back = 110 + 60 * np.sin(x / 9.0)[..., None] * np.cos(y / 7.0)[..., None] * np.array([1.0, 0.6, -0.8])
    video = np.empty((frames, h, w, 3), np.uint8)
    labels = np.zeros((frames, boxes, 5), np.float32)
    pos = rng.uniform([0, 0], [w * 0.6, h * 0.6], (boxes, 2))
    size = rng.uniform([w * 0.15, h * 0.15], [w * 0.4, h * 0.4], (boxes, 2))
    vel = rng.uniform(-3, 3, (boxes, 2))
    cls = rng.integers(0, 20, boxes)
    colour = rng.integers(0, 256, (boxes, 3))
    for t in range(frames):
        img = back + rng.normal(0, 12, (h, w, 3))
        p = np.clip(pos + t * vel, 0, [w - 1, h - 1] - size)
        for i in range(boxes):
            x1, y1 = p[i]
            x2, y2 = p[i] + size[i]
            img[int(y1):int(y2), int(x1):int(x2)] = colour[i]
            labels[t, i] = (x1, y1, x2, y2, cls[i])
        video[t] = np.clip(img, 0, 255).astype(np.uint8)
    return video, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--seed", type=int, default=233)
    args = ap.parse_args()

    import torch
    import videoyolo_amd as vy
    from videoyolo_amd import autograd
    from videoyolo_amd.transforms import YOLO3VideoTrainTransform

    dev = torch.device("cuda", 0)
    classes = ["c%d" % i for i in range(20)]
    rng = np.random.default_rng(args.seed)
    sizes = [(240, 320), (180, 320), (288, 352), (360, 270)]
    videos = [synthetic_video(rng, args.k + args.steps, *sizes[i % len(sizes)], boxes=1 + i % 3) for i in range(args.clips)]
    # the reference seeds the two global generators its transform draws from (train_yolov3.py:135)
    random.seed(args.seed)
    np.random.seed(args.seed)

    single = vy.yolo3_darknet53(classes, pretrained_base=False)
    single.initialize(init="synthetic", seed=233)
    params = {p.name: p.data() for p in single.collect_params().values()}
    for k in (args.k, 1):
        if k > 1:
            net = vy.yolo3_darknet53(classes, pretrained_base=False, k=k, k_join_type="max", k_join_pos="early")
        else:
            net = vy.yolo3_darknet53(classes, pretrained_base=False)
        net.set_parameters(params)
        net.collect_params().reset_ctx(dev)
        trainer = vy.Trainer(net.collect_params(), "sgd", {"learning_rate": 1e-3, "wd": 5e-4, "momentum": 0.9})
        transform = YOLO3VideoTrainTransform(k, args.size, args.size, net)
        print("k = %d: %d clips per step from sources %s" % (k, args.clips, sorted({v.shape[1:3] for v, _ in videos})))
        for step in range(args.steps):
            # a clip is k consecutive frames; its label is its last frame's (datasets/imgnetvid.py:190-224)
            srcs = [v[step:step + k] for v, _ in videos]
            labels = [lab[step + k - 1] for _, lab in videos]
            x, gt_boxes, *fixed = transform.batch(srcs, labels, device=dev)
            with autograd.record():
                obj, ctr, scl, cls = net(x, gt_boxes, *fixed)
                autograd.backward([obj + ctr + scl + cls])
            trainer.step(args.clips)
            vals = [t.mean().item() for t in (obj, ctr, scl, cls)]
            assert all(np.isfinite(v) for v in vals), vals
            print("  step %d  x %s  boxes %d  obj %.3f  center %.3f  scale %.3f  cls %.3f" % (
                step, tuple(x.shape), int((gt_boxes[..., 0] >= 0).sum().item()), *vals))
    print("trained on augmented clips: one transform launch and one target launch per batch")


if __name__ == "__main__":
    main()
