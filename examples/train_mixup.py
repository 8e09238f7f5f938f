"""Training with mixup: the reference's epoch loop (train_yolov3.py:227-229, 571-581) — the training set wrapped in
MixupDetection, ``set_mixup(np.random.beta, 1.5, 1.5)`` at the start of an epoch and ``set_mixup(None)`` for the last
``--no-mixup-epochs`` — on synthetic uint8 videos of differing sizes.  A mixed sample reaches the transform as a MixedClip:
two clips and a ratio, NOT blended.  YOLO3VideoTrainTransform.batch packs both sources once and the ONE transform launch
of the batch blends every pixel it reads (vy_train_transform_mix); the label's last column weighs the objectness loss.

Before training, each net's first batch is made twice under the same seeds — from the MixedClips, and from the clips
MixedClip.numpy() materialises on the host as gluoncv does — and the two must be identical, images and targets.

    python examples/train_mixup.py [--size 96] [--clips 4] [--k 3] [--epochs 3] [--no-mixup-epochs 1] [--seed 233]
"""
import argparse
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from train_augmented import synthetic_video  # noqa: E402  (examples/train_augmented.py)


class ClipDataset(object):
    """dataset[i] = (the first k frames of video i, (N, 5) label of the clip's last frame) (datasets/imgnetvid.py:190-224);
    a single image, (h, w, 3), for k = 1."""

    def __init__(self, videos, k):
        self._videos, self._k = videos, k

    def __len__(self):
        return len(self._videos)

    def __getitem__(self, i):
        video, labels = self._videos[i]
        clip = video[:self._k]
        return (clip[0] if self._k == 1 else clip), labels[self._k - 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--clips", type=int, default=4)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--no-mixup-epochs", type=int, default=1)
    ap.add_argument("--seed", type=int, default=233)
    args = ap.parse_args()

    import torch
    import videoyolo_amd as vy
    from videoyolo_amd import MixedClip, MixupDetection, autograd
    from videoyolo_amd.transforms import YOLO3VideoTrainTransform

    dev = torch.device("cuda", 0)
    classes = ["c%d" % i for i in range(20)]
    rng = np.random.default_rng(args.seed)
    sizes = [(120, 160), (90, 160), (144, 176), (180, 135)]
    videos = [synthetic_video(rng, args.k, *sizes[i % len(sizes)], boxes=1 + i % 3) for i in range(args.clips)]

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
        train_dataset = MixupDetection(ClipDataset(videos, k))                      # train_yolov3.py:228-229
        transform = YOLO3VideoTrainTransform(k, args.size, args.size, net, mixup=True)

        def batch(materialise=False):
            samples = [train_dataset[i] for i in range(len(train_dataset))]
            srcs = [s.numpy() if materialise and isinstance(s, MixedClip) else s for s, _ in samples]
            mixed = sum(isinstance(s, MixedClip) for s, _ in samples)
            return transform.batch(srcs, [label for _, label in samples], device=dev), mixed

        # the device blend is the host blend: one batch both ways under the same seeds
        train_dataset.set_mixup(np.random.beta, 1.5, 1.5)
        both = []
        for materialise in (False, True):
            random.seed(args.seed)          # the reference seeds the two global generators its transform and
            np.random.seed(args.seed)       # gluoncv's wrapper draw from (train_yolov3.py:135)
            both.append(batch(materialise))
        assert both[0][1] == args.clips, "beta(1.5, 1.5) < 1: every sample is mixed"
        for u, v in zip(both[0][0], both[1][0]):
            assert torch.equal(u, v), "the launch's blend differs from MixedClip.numpy()'s"
        print("k = %d: %d clips per step from sources %s; the mix launch equals the host blend, bit for bit" % (
            k, args.clips, sorted({v.shape[1:3] for v, _ in videos})))

        for epoch in range(args.epochs):
            if epoch >= args.epochs - args.no_mixup_epochs:                          # train_yolov3.py:571-581
                train_dataset.set_mixup(None)
            else:
                train_dataset.set_mixup(np.random.beta, 1.5, 1.5)
            (x, gt_boxes, *fixed), mixed = batch()
            with autograd.record():
                obj, ctr, scl, cls = net(x, gt_boxes, *fixed)
                autograd.backward([obj + ctr + scl + cls])
            trainer.step(args.clips)
            vals = [t.mean().item() for t in (obj, ctr, scl, cls)]
            assert all(np.isfinite(v) for v in vals), vals
            ratios = fixed[0][fixed[0] > 0]
            assert mixed or bool((ratios == 1).all()), "without mixup every objectness target is 1"
            print("  epoch %d  mixed %d/%d  x %s  boxes %d  obj %.3f  center %.3f  scale %.3f  cls %.3f" % (
                epoch, mixed, args.clips, tuple(x.shape), int((gt_boxes[..., 0] >= 0).sum().item()), *vals))
    print("trained with mixup: two clips blended inside the one transform launch of each batch")


if __name__ == "__main__":
    main()
