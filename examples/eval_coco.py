"""Scoring detections with the COCO metric, the second metric the reference's detect driver builds by default on every
dataset (detect_yolo3.py:53, :185; metrics/mscoco.py).

A synthetic dataset object with the attributes the metric reads (sample ids, class names, image sizes and a COCO-style
ground-truth file written by build_coco_json), a single-frame net that detects batches of noise frames with the annotated
boxes brightened, and the metric updated with the device tensors the net returns: the rows are matched on the device
(vy_coco_match) and only get() copies them.  The same rows go through the host path too, and the two must give the same
results.  The net's parameters are synthetic, so the scores say nothing about the detector; the point is the plumbing.

    python examples/eval_coco.py [--images 24] [--size 160] [--batch 8]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class Boxes(object):
    """A stand-in for a detection dataset: `n` images of `size` x `size` shown to the net at that size, each annotated with
    0..3 boxes; every image's own size is 1.5x that, so the metric's data_shape scaling does something."""

    def __init__(self, n, size, classes, seed=5):
        rng = np.random.default_rng(seed)
        self.classes = list(classes)
        self.sample_ids = [10 * i + 3 for i in range(n)]
        self.size = size
        self._boxes = {}
        anns = []
        for k, i in enumerate(self.sample_ids):
            m = k % 4
            xy = rng.integers(0, size // 2, (m, 2))
            wh = rng.integers(size // 8, size // 2, (m, 2))
            self._boxes[i] = np.concatenate([xy, wh], 1)
            for b in self._boxes[i]:
                x, y, w, h = (1.5 * b).tolist()
                anns.append({'id': len(anns), 'image_id': i, 'category_id': int(rng.integers(0, len(classes))),
                             'bbox': [x, y, w, h], 'area': w * h, 'iscrowd': int(rng.random() < 0.1)})
        self._data = {'images': [{'id': i, 'width': int(1.5 * size), 'height': int(1.5 * size)} for i in self.sample_ids],
                      'annotations': anns, 'categories': [{'id': c, 'name': n} for c, n in enumerate(classes)]}

    def image_size(self, i):
        return int(1.5 * self.size), int(1.5 * self.size)

    def build_coco_json(self):
        fd, path = tempfile.mkstemp(suffix='.json')
        with os.fdopen(fd, 'w') as f:
            json.dump(self._data, f)
        return path

    def frames(self, ids, seed=3):
        rng = np.random.default_rng(seed + ids[0])
        x = rng.standard_normal((len(ids), 3, self.size, self.size)).astype(np.float32)
        for k, i in enumerate(ids):
            for bx, by, bw, bh in self._boxes[i]:
                x[k, :, by:by + bh, bx:bx + bw] += 1.5
        return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=24)
    ap.add_argument("--size", type=int, default=160)
    ap.add_argument("--batch", type=int, default=8)
    args = ap.parse_args()

    import torch
    import videoyolo_amd as vy

    dev = torch.device("cuda", 0)
    classes = ["c%d" % i for i in range(20)]
    dataset = Boxes(args.images, args.size, classes)
    net = vy.yolo3_darknet53(classes, pretrained_base=False)
    net.initialize(init="synthetic", seed=233, obj_bias=-2.0)
    net.collect_params().reset_ctx(dev)
    net.set_nms(0.45, 400, 100)

    shape = (args.size, args.size)
    metric = vy.COCODetectionMetric(dataset, data_shape=shape)
    host = vy.COCODetectionMetric(dataset, data_shape=shape)
    ids_sorted = sorted(dataset.sample_ids)
    for lo in range(0, args.images, args.batch):
        frames = torch.from_numpy(dataset.frames(ids_sorted[lo:lo + args.batch])).to(dev)
        ids, scores, bboxes = net(frames)                          # (B, 100, 1), (B, 100, 1), (B, 100, 4), on the device
        metric.update(bboxes, ids, scores)                         # matched on the device, nothing copied
        host.update(bboxes.cpu().numpy(), ids.cpu().numpy(), scores.cpu().numpy())
    names, values = metric.get()                                   # one copy, then the accumulation on the host
    assert (names, values) == host.get(), "device and host paths differ"
    assert np.array_equal(metric.precision, host.precision) and np.array_equal(metric.recall, host.recall)
    assert np.array_equal(metric.stats, host.stats)

    print(names[0] + values[0])
    print(names[-1] + values[-1])
    print("%d images in %d launches: device path equals host path" % (args.images, metric.device_updates))


if __name__ == "__main__":
    main()
