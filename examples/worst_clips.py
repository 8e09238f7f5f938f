"""The reference's per-frame metric and worst-clip ranking (detect_yolo3.py --per_frame_metric: add_metrics_to_predictions,
:451-534, and the summary.txt that --worst_video_path ranks clips by) on this package, with synthetic videos.

Every video goes through a window net's detect_video; every batch of its frames goes, as the device tensors the net
returned, into a FrameMApMetric (one mean AP per frame: vy_voc_match and vy_voc_frame_ap, nothing copied, nothing waits)
and into a VOCMApMetric (the data set's mAP) side by side.  The ground truths are made from the net's own boxes, shifted
more from video to video, so the videos rank.  get() copies the frame scores once; they are checked against the host's
frame_map_host, the ranking is printed worst first, and the first frame's 8-column lines are shown.
The net's parameters are synthetic, so the scores say nothing about the detector; the point is the plumbing.

    python examples/worst_clips.py [--videos 3] [--frames 12] [--size 128] [--k 3] [--batch 4]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))



def synthetic_video(n, h, w, seed):
    """uint8 HWC frames: a drifting noise field with a moving bright box."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 255, (h, w, 3), dtype=np.uint8)
    out = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        f = np.roll(base, 3 * i, axis=1).copy()
        x0 = (17 * i) % max(1, w - 30)
        f[h // 3:h // 3 + 24, x0:x0 + 30] = 255 - f[h // 3:h // 3 + 24, x0:x0 + 30] // 4
        out[i] = f
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=3)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    args = ap.parse_args()

    import torch
    import torch.nn.functional as F
    import videoyolo_amd as vy
    from videoyolo_amd.metrics import frame_map_host, frame_metric_lines

    dev = torch.device("cuda", 0)
    classes = ["c%d" % i for i in range(20)]
    net = vy.yolo3_darknet53(classes, pretrained_base=False, k=args.k, k_join_type="max", k_join_pos="early")
    net.initialize(init="synthetic", seed=233, obj_bias=-2.0)
    net.collect_params().reset_ctx(dev)
    net.set_nms(nms_thresh=0.45, nms_topk=400, post_nms=100)

    frame_metric = vy.FrameMApMetric(iou_thresh=0.5, class_names=classes)
    set_metric = vy.metrics.VOCMApMetric(iou_thresh=0.5, class_names=classes)
    fed, updates = [], 0
    for v in range(args.videos):
        raw = synthetic_video(args.frames, 90, 120, seed=3 + v)
        x = torch.from_numpy(raw).to(dev).permute(0, 3, 1, 2).float() / 255.0
        x = F.interpolate(x, size=(args.size, args.size), mode="bilinear", align_corners=False).contiguous()
        ids, scores, bboxes = net.detect_video(x, frames_per_step=args.batch)
        bboxes = bboxes.clamp(0, args.size)
        # ground truths: every other one of the frame's first 12 boxes, moved by 2 + 3 v pixels; the second is difficult
        gt_boxes = bboxes[:, 0:12:2].clone() + float(2 + 3 * v)
        gt_ids = ids[:, 0:12:2].clone()
        gt_diff = torch.zeros_like(gt_ids)
        gt_diff[:, 1] = 1
        for lo in range(0, args.frames, args.batch):
            batch = [t[lo:lo + args.batch] for t in (bboxes, ids, scores, gt_boxes, gt_ids, gt_diff)]
            frame_metric.update(*batch, keys=[("video%d" % v, lo + i) for i in range(len(batch[0]))])
            set_metric.update(*batch)
            fed.append(batch)
            updates += 1
    assert frame_metric.device_updates == updates == set_metric.device_updates, "the device path was not taken"

    keys, got = frame_metric.get()
    want = np.concatenate([frame_map_host(*[t.cpu().numpy() for t in batch]) for batch in fed])
    assert len(keys) == args.videos * args.frames == len(got)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "device and host disagree on the frames without a score"
    bound = 2.0 * (100 + 6 + 2) * 2.0 ** -53
    worst_diff = float(np.nanmax(np.abs(got - want))) if not np.isnan(want).all() else 0.0
    assert worst_diff <= bound, "device and host frame scores differ by %g" % worst_diff

    print("%d videos of %d frames at %d x %d, k = %d: %d frames scored on the device in %d launches, %d without a score" % (
        args.videos, args.frames, args.size, args.size, args.k, len(keys) - len(frame_metric.unscored), updates,
        len(frame_metric.unscored)))
    print("videos, worst first (mean of the frames' mAP, frames):")
    for video, mean, frames in frame_metric.by_video():
        print("  %s\t%.4f\t%d" % (video, mean, frames))
    print("frames, worst first:")
    for key, score in frame_metric.worst(5):
        print("  %s frame %d\t%.4f" % (key[0], key[1], score))
    first = fed[0]
    rows = [(first[1][0, j, 0].item(), first[2][0, j, 0].item()) + tuple((first[0][0, j] / args.size).tolist())
            for j in range(first[1].shape[1]) if first[1][0, j, 0].item() >= 0][:3]
    for line in frame_metric_lines("video0/000000.JPEG", rows, got[0]):
        print("  " + line.rstrip())
    print("%s over all frames = %.4f; device frame scores equal the host's (worst difference %.3g, bound %.3g)" % (
        set_metric.get()[0][-1], set_metric.get()[1][-1], worst_diff, bound))


if __name__ == "__main__":
    main()
