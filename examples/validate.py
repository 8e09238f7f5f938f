"""The reference's validation loop (train_yolov3.py:434-490, validate(): what training runs after every epoch) on this
package, with synthetic frames: set_nms -> net(x) -> clip the boxes to the frame -> VOCMApMetric.update -> get().

The frames are noise with brightened rectangles planted in them, and the labels are those rectangles, (B, M, 6) rows
[x1, y1, x2, y2, class, difficult] padded with -1 as the reference's batchify pads them.  update() takes the device
tensors the net returns and the labels on the device: the rows are matched there (vy_voc_match), nothing is copied and
nothing waits until get().  The same rows then go through the host path (numpy), and the two must give the same result.
The net's parameters are synthetic, so the score says nothing about the detector; the point is the plumbing.

    python examples/validate.py [--size 416] [--batch 8] [--batches 4]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CLASSES = ["aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable",
           "dog", "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor"]


def planted_batch(rng, batch, size, max_gt=6):
    """(batch, 3, size, size) float32 frames and (batch, max_gt, 6) float32 labels, -1 rows where an image has fewer."""
    x = rng.standard_normal((batch, 3, size, size)).astype(np.float32)
    label = np.full((batch, max_gt, 6), -1, np.float32)
    for i in range(batch):
        n = int(rng.integers(1, max_gt + 1))
        wh = rng.integers(size // 8, size // 2, (n, 2))
        xy = rng.integers(0, size - wh)
        label[i, :n, :2], label[i, :n, 2:4] = xy, xy + wh
        label[i, :n, 4] = rng.integers(0, len(CLASSES), n)
        label[i, :n, 5] = rng.random(n) < 0.2
        for b in label[i, :n]:
            x[i, :, int(b[1]):int(b[3]), int(b[0]):int(b[2])] += 1.5
    return x, label


def validate(net, batches, metric, size, on_device):
    """train_yolov3.py:434-490 for one pass over `batches`: [(frames, labels)] device tensors."""
    metric.reset()
    net.set_nms(nms_thresh=0.45, nms_topk=400)                                  # :441
    for x, label in batches:
        ids, scores, bboxes = net(x)                                            # :452
        bboxes = bboxes.clamp(0, size)                                          # :457 clip to the image
        args = [bboxes, ids, scores, label[:, :, :4], label[:, :, 4:5], label[:, :, 5:6]]      # :459-461
        if not on_device:
            args = [a.cpu().numpy() for a in args]
        metric.update(*args)                                                    # :464
    return metric.get()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--batches", type=int, default=4)
    args = ap.parse_args()

    import torch
    import videoyolo_amd as vy

    dev = torch.device("cuda", 0)
    net = vy.yolo3_darknet53(CLASSES, pretrained_base=False)
    net.initialize(init="synthetic", seed=233, obj_bias=-2.0)
    net.collect_params().reset_ctx(dev)
    rng = np.random.default_rng(11)
    batches = [tuple(torch.from_numpy(a).to(dev) for a in planted_batch(rng, args.batch, args.size))
               for _ in range(args.batches)]

    metric = vy.metrics.VOCMApMetric(iou_thresh=0.5, class_names=CLASSES)
    names, values = validate(net, batches, metric, args.size, on_device=True)
    assert metric.device_updates == args.batches, "the device path was not taken"
    host_metric = vy.metrics.VOCMApMetric(iou_thresh=0.5, class_names=CLASSES)
    host_names, host_values = validate(net, batches, host_metric, args.size, on_device=False)
    assert host_metric.device_updates == 0
    same = names == host_names and all(a == b or (a != a and b != b) for a, b in zip(values, host_values))
    assert same, "device and host paths differ: %s / %s" % (values, host_values)

    scored = sum(len(v) for v in metric._scores.values())
    hits = sum(int(f == 1) for v in metric._flags.values() for f in v)
    print("%d frames of %d x %d in %d batches: %d detections scored against %d ground truths, %d true positives" % (
        args.batch * args.batches, args.size, args.size, args.batches, scored, sum(metric._n_pos.values()), hits))
    print("%s = %.4f; matched on the device in %d launches: device path equals host path" % (
        names[-1], values[-1], metric.device_updates))


if __name__ == "__main__":
    main()
