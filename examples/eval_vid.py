"""Scoring a detected video with the ImageNet-VID motion / area mAP, as the reference's detect driver does for its main
dataset (detect_yolo3.py:181-195 builds VIDDetectionMetric, :659-695 feeds it batch by batch and prints get()).

A synthetic video with moving boxes, a stand-in dataset that has the four attributes the metric reads (sample ids, labels,
class names and a motion IoU per ground truth), a window net that detects the whole video, and the metric updated with the
device tensors the net returns: the rows are matched on the device (vy_vid_match) and only get() copies them.  The same
rows go through the host path too, and the two must give the same AP table.  The net's parameters are synthetic, so the
scores say nothing about the detector; the point is the plumbing.

    python examples/eval_vid.py [--frames 48] [--size 224] [--k 3]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _iou(a, b):
    iw = min(a[2], b[2]) - max(a[0], b[0]) + 1
    ih = min(a[3], b[3]) - max(a[1], b[1]) + 1
    if iw <= 0 or ih <= 0:
        return 0.0
    return iw * ih / ((a[2] - a[0] + 1) * (a[3] - a[1] + 1) + (b[2] - b[0] + 1) * (b[3] - b[1] + 1) - iw * ih)


class MovingBoxes(object):
    """A stand-in for the ImageNet-VID validation set: `n_obj` boxes of fixed size and class, each drifting at its own
    speed.  A ground truth's motion IoU is the mean IoU of its box with the same object's box up to 10 frames either side
    (the definition ImageNet-VID's motion evaluation uses), so slow objects land in the [0.9, 1] range and fast ones
    below 0.7."""

    def __init__(self, n_frames, size, classes, n_obj=4, seed=5):
        rng = np.random.default_rng(seed)
        self.classes = self.wn_classes = list(classes)
        wh = rng.integers(size // 8, size // 2, (n_obj, 2))
        xy0 = rng.integers(0, size // 2, (n_obj, 2))
        speed = np.array([0.2, 1.0, 3.0, 6.0])[:n_obj, None] * rng.choice([-1, 1], (n_obj, 2))
        cls = rng.integers(0, len(classes), n_obj)
        track = np.zeros((n_frames, n_obj, 5))
        for t in range(n_frames):
            xy = np.mod(np.round(xy0 + speed * t), size - wh)
            track[t] = np.concatenate([xy, xy + wh - 1, cls[:, None]], 1)
        self._labels = {t: track[t, :1 + t % n_obj] for t in range(n_frames)}     # 1..n_obj objects are annotated
        self.motion_ious = {}
        for t in range(n_frames):
            near = [u for u in range(max(0, t - 10), min(n_frames, t + 11)) if u != t]
            self.motion_ious[str(t)] = [float(np.mean([_iou(track[t, o], track[u, o]) for u in near]))
                                        for o in range(len(self._labels[t]))]
        self.size, self.n_frames = size, n_frames

    def get_sample_ids(self):
        return list(range(self.n_frames))

    def get_label(self, i):
        return self._labels[i]

    def frames(self, seed=3):
        """(T, 3, size, size) float32: noise with every annotated box brightened."""
        rng = np.random.default_rng(seed)
        x = rng.standard_normal((self.n_frames, 3, self.size, self.size)).astype(np.float32)
        for t in range(self.n_frames):
            for b in self._labels[t]:
                x[t, :, int(b[1]):int(b[3]) + 1, int(b[0]):int(b[2]) + 1] += 1.5
        return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--k", type=int, default=3)
    args = ap.parse_args()

    import torch
    import videoyolo_amd as vy

    dev = torch.device("cuda", 0)
    classes = ["c%d" % i for i in range(30)]
    dataset = MovingBoxes(args.frames, args.size, classes)
    net = vy.yolo3_darknet53(classes, pretrained_base=False, k=args.k, k_join_type="max", k_join_pos="early")
    net.initialize(init="synthetic", seed=233, obj_bias=-2.0)
    net.collect_params().reset_ctx(dev)
    net.set_nms(0.45, 400, 100)

    frames = torch.from_numpy(dataset.frames()).to(dev)
    ids, scores, bboxes = net.detect_video(frames)                 # (T, 100, 1), (T, 100, 1), (T, 100, 4), on the device

    metric = vy.VIDDetectionMetric(dataset)
    metric.update(bboxes, ids, scores, sid=range(args.frames))     # matched on the device, nothing copied
    names, values = metric.get()                                   # one copy, then AP on the host

    host = vy.VIDDetectionMetric(dataset)
    host.update(bboxes.cpu().numpy(), ids.cpu().numpy(), scores.cpu().numpy(), sid=range(args.frames))
    host.get()
    assert np.array_equal(metric.ap, host.ap), "device and host paths differ"

    print(names[0] + values[0])
    kept = len(metric.matches()[0])
    print("%d frames, %d rows kept of %d, AP table %s: device path equals host path" % (
        args.frames, kept, ids.shape[0] * ids.shape[1], metric.ap.shape))


if __name__ == "__main__":
    main()
