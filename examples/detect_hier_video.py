"""The reference's windowed detect loop with a hierarchical net, on a synthetic video: detect_yolo3.py --window T,step takes
one T-frame clip per frame (datasets/imgnetvid.py:480-506: centred on the frame, `step` apart, clamped at the ends of the
video), T = 3^n for a net that pools n times inside its backbone.  Consecutive clips share almost all of their frames, so
videoyolo_amd.hier_detect_video(net, frames) runs the stem and every group of cells once per frame position (the joins as dilated triples) instead of
once per clip; the clip path — net(clips) on the materialised clips — runs next to it, and the two outputs must be equal.

    python examples/detect_hier_video.py [--frames 64] [--size 416] [--hierarchical 3,3,1,1,1] [--join max|conv] [--step 1]
                                         [--frames-per-step 16]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from detect_video import synthetic_video  # noqa: E402  (the sibling example's drifting gradient with a moving box)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--hierarchical", default="3,3,1,1,1")
    ap.add_argument("--join", default="max", choices=("max", "conv"))
    ap.add_argument("--step", type=int, default=1)
    ap.add_argument("--frames-per-step", type=int, default=16)
    args = ap.parse_args()
    hier = [int(v) for v in args.hierarchical.split(",")]

    import torch
    import torch.nn.functional as F
    import videoyolo_amd as vy

    dev = torch.device("cuda", 0)
    classes = ["c%d" % i for i in range(20)]
    if args.join == "conv":
        net = vy.YOLOV3HierConv(classes, hierarchical=hier)
    else:
        net = vy.yolo3_darknet53(classes, pretrained_base=False, new_model=True, hierarchical=hier, h_join_type="max")
    net.initialize(init="synthetic", seed=233)
    net.collect_params().reset_ctx(dev)
    net.set_nms(nms_thresh=0.45, nms_topk=400)

    raw = synthetic_video(args.frames, 360, 480)
    mean = torch.tensor([0.485, 0.456, 0.406], device=dev).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], device=dev).view(1, 3, 1, 1)

    def transform(chunk):  # resize + ToTensor + normalize, as the reference's validation transform
        x = torch.from_numpy(chunk).to(dev).permute(0, 3, 1, 2).float() / 255.0
        x = F.interpolate(x, size=(args.size, args.size), mode="bilinear", align_corners=False)
        return ((x - mean) / std).contiguous()

    def post(outs):  # boxes back to the source frame, a line per detection
        ids, scores, bboxes = [t.cpu().numpy() for t in outs[:3]]
        sx, sy = raw.shape[2] / args.size, raw.shape[1] / args.size
        lines = []
        for i in range(len(ids)):
            for j in np.nonzero(ids[i, :, 0] >= 0)[0]:
                b = bboxes[i, j] * (sx, sy, sx, sy)
                lines.append("%d %s %.4f %.1f %.1f %.1f %.1f" % (i, classes[int(ids[i, j, 0])], scores[i, j, 0], *b))
        return lines

    frames = transform(raw)  # every source frame is resized once, in either path
    fps = {}
    # ---- the video path: each level once per frame position
    for rep in range(2):  # the first pass warms up (plan, workspace); the second is timed
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        video = vy.hier_detect_video(net, frames, step=args.step, frames_per_step=args.frames_per_step, return_index=True)
        torch.cuda.synchronize()
        fps["video"] = args.frames / (time.perf_counter() - t0)

    # ---- the clip path: the same clips, materialised, frames_per_step of them per call
    idx = torch.from_numpy(vy.window_indices(args.frames, net.frames, args.step)).to(dev)
    for rep in range(2):
        outs = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(0, args.frames, args.frames_per_step):
            outs.append(net(frames[idx[s:s + args.frames_per_step]], return_index=True))
        torch.cuda.synchronize()
        fps["clip"] = args.frames / (time.perf_counter() - t0)
    clip = [torch.cat(ts, 0) for ts in zip(*outs)]

    for name, a, b in zip(("ids", "scores", "bboxes", "keep_idx"), video, clip):
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    lines = post(video)
    assert lines == post(clip)
    for l in lines[:5]:
        print(l)
    print("%d frames, hierarchical %s (T = %d), step = %d, %s join: %d prediction lines, video path equals clip path bit for "
          "bit" % (args.frames, hier, net.frames, args.step, args.join, len(lines)))
    print("video path %.1f frames/s   clip path %.1f frames/s   (%d frames per call, %d frames of context on either side)" % (
        fps["video"], fps["clip"], args.frames_per_step, args.step * (net.frames - 1) // 2))


if __name__ == "__main__":
    main()
