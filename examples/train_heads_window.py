"""Temporal training with a frozen backbone on synthetic frames, without paying for the backbone more than once: the
reference's --features_dir --window k workflow (extract_base_features.py:120-160 once, then train_yolov3.py on windows of the
stored routes, datasets/imgnetvid.py:146-174).  A single-frame net extracts the three routes of every frame of a video,
in chunks; the bank stays in device memory; the heads train on windows around random centre frames and validate on every
frame of the video, the clips of detect_yolo3.py --window k,step.  The script asserts that those detections are, bit for
bit, what the full window net gives for the frames.

    python examples/train_heads_window.py [--size 416] [--batch 16] [--frames 48] [--k 3] [--step 1] [--steps 10]
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
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--join", default="max", choices=["max", "mean"])
    ap.add_argument("--step", type=int, default=1, help="frames between the frames of a window")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=16, help="frames per backbone call while extracting")
    args = ap.parse_args()

    import torch
    import videoyolo_amd as vy
    from videoyolo_amd import autograd, metrics, targets

    dev = torch.device("cuda", 0)
    classes = ["c%d" % i for i in range(20)]
    rng = np.random.default_rng(1)
    video = rng.standard_normal((args.frames, 3, args.size, args.size)).astype(np.float32)
    gt_boxes, gt_ids = targets.synthetic_gt(args.frames, args.size, len(classes), m=4, seed=7)

    # ---- 1. the backbone once per frame, in chunks; the three banks stay on the device
    backbone = vy.yolo3_darknet53(classes, pretrained_base=False)
    backbone.initialize(init="synthetic", seed=233)
    backbone.collect_params().reset_ctx(dev)
    chunks = [backbone.extract_features(video[s:s + args.chunk]) for s in range(0, args.frames, args.chunk)]
    f1, f2, f3 = (torch.cat([c[i] for c in chunks], 0) for i in range(3))
    del chunks
    print("extracted %d frames x 3 routes: %.1f MB on the device" % (
        args.frames, sum(f.numel() for f in (f1, f2, f3)) * 4 / 1e6))

    # ---- 2. the heads alone, on windows of the stored routes
    net = vy.yolo3_no_backbone(classes, k=args.k, k_join_type=args.join, k_join_pos="early")
    model_file = os.path.join(tempfile.mkdtemp(prefix="heads_window_"), "full.params")
    backbone.save_parameters(model_file)
    net.load_parameters(model_file, ignore_extra=True)
    net.collect_params().reset_ctx(dev)
    for p in net.collect_params(".*beta|.*gamma|.*bias").values():                 # --no_wd
        p.wd_mult = 0.0
    trainer = vy.Trainer(net.collect_params(), "sgd", {"learning_rate": 1e-3, "wd": 5e-4, "momentum": 0.9})
    gen = targets.YOLOV3PrefetchTargetGenerator(len(classes))
    windows = vy.window_indices(args.frames, args.k, args.step)                     # row i: the window around frame i
    for step in range(args.steps):
        centres = rng.integers(0, args.frames, args.batch)
        fixed = gen(args.size, args.size, gt_boxes[centres], gt_ids[centres], device=dev)
        with autograd.record():
            obj, ctr, scl, cls = net.from_bank(f1, f2, f3, windows[centres], torch.as_tensor(gt_boxes[centres]).to(dev), *fixed)
            autograd.backward([obj + ctr + scl + cls])
        trainer.step(args.batch)
        print("step %d  obj %.3f  center %.3f  scale %.3f  cls %.3f" % (
            step, obj.mean().item(), ctr.mean().item(), scl.mean().item(), cls.mean().item()))

    # ---- 3. validation: every frame of the stored video
    net.set_nms(nms_thresh=0.45, nms_topk=400)
    got = net.detect_video_features(f1, f2, f3, step=args.step, clips_per_step=args.batch, return_index=True)
    metric = metrics.VOCMApMetric(iou_thresh=0.5, class_names=classes)
    det_ids, scores, bboxes = [t.cpu().numpy() for t in got[:3]]
    metric.update(np.clip(bboxes, 0, args.size), det_ids, scores, gt_boxes, gt_ids)
    names, values = metric.get()
    print("%s = %.4f (synthetic weights against random boxes: a plumbing check, not a score)" % (names[-1], values[-1]))

    # ---- 4. the same detections from the frames: the full window net with the trained heads and the same backbone
    heads_file = os.path.join(os.path.dirname(model_file), "heads.params")
    net.save_parameters(heads_file)
    full = vy.yolo3_darknet53(classes, pretrained_base=False, k=args.k, k_join_type=args.join, k_join_pos="early")
    full.load_parameters(model_file)               # a single-frame file: the backbone (and the untrained heads)
    full.load_parameters(heads_file, allow_missing=True)
    full.collect_params().reset_ctx(dev)
    full.set_nms(nms_thresh=0.45, nms_topk=400)
    want = full.detect_video(video, step=args.step, frames_per_step=args.batch, return_index=True)
    for name, g, w in zip(("ids", "scores", "bboxes", "keep_idx"), got, want):
        assert g.shape == w.shape and torch.equal(g.view(torch.int32), w.view(torch.int32)), name
    print("%d frames, k = %d, step = %d: the stored routes and the frames detect the same, bit for bit" % (
        args.frames, args.k, args.step))


if __name__ == "__main__":
    main()
