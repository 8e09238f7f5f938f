"""The reference's windowed detect loop on a synthetic video: detect_yolo3.py --window k,step takes one k-frame clip per
frame (datasets/imgnetvid.py:480-506: centred on the frame, `step` apart, clamped at the ends of the video), resizes it,
runs the net and post-processes the boxes.  Here the frames are resized and pushed through a VideoSession, which runs
Darknet-53 once per frame and pools every clip out of a ring of per-frame routes; the clip path — net(clips) on the
materialised clips, every frame through the backbone k times — runs next to it, and the two outputs must be equal.

    python examples/detect_video.py [--frames 64] [--size 416] [--k 3] [--step 1] [--join max] [--frames-per-step 16]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic_video(n, h, w, seed=3):
    """uint8 HWC frames: a drifting gradient with a moving bright box."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 255, (h, w, 3), dtype=np.uint8)
    out = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        f = np.roll(base, 3 * i, axis=1).copy()
        x0 = (17 * i) % max(1, w - 80)
        f[h // 3:h // 3 + 60, x0:x0 + 80] = 255 - f[h // 3:h // 3 + 60, x0:x0 + 80] // 4
        out[i] = f
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--step", type=int, default=1)
    ap.add_argument("--join", default="max", choices=("max", "mean"))
    ap.add_argument("--frames-per-step", type=int, default=16)
    args = ap.parse_args()

    import torch
    import torch.nn.functional as F
    import videoyolo_amd as vy

    dev = torch.device("cuda", 0)
    classes = ["c%d" % i for i in range(20)]
    net = vy.yolo3_darknet53(classes, pretrained_base=False, k=args.k, k_join_type=args.join, k_join_pos="early")
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

    def post(outs, n0):  # boxes back to the source frame, a line per detection
        ids, scores, bboxes = [t.cpu().numpy() for t in outs[:3]]
        sx, sy = raw.shape[2] / args.size, raw.shape[1] / args.size
        lines = []
        for i in range(len(ids)):
            for j in np.nonzero(ids[i, :, 0] >= 0)[0]:
                b = bboxes[i, j] * (sx, sy, sx, sy)
                lines.append("%d %s %.4f %.1f %.1f %.1f %.1f" % (n0 + i, classes[int(ids[i, j, 0])], scores[i, j, 0], *b))
        return lines

    fps = {}
    # ---- the video path: push frames as they arrive, detections come back one look-ahead later
    session = net.video(frames_per_step=args.frames_per_step, step=args.step)
    outs, lines = [], []
    for rep in range(2):  # the first pass warms up (plan, workspace); the second is timed
        outs, lines, n0 = [], [], 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(0, args.frames, args.frames_per_step):
            got = session.push(transform(raw[s:s + args.frames_per_step]), return_index=True)
            outs.append(got)
            lines += post(got, n0)
            n0 += got[0].shape[0]
        got = session.flush(return_index=True)
        outs.append(got)
        lines += post(got, n0)
        torch.cuda.synchronize()
        fps["video"] = args.frames / (time.perf_counter() - t0)
    video = [torch.cat(ts, 0) for ts in zip(*outs)]

    # ---- the clip path: the same clips, materialised
    idx = vy.window_indices(args.frames, args.k, args.step)
    for rep in range(2):
        outs, clip_lines = [], []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in range(0, args.frames, args.frames_per_step):
            rows = idx[s:s + args.frames_per_step]
            lo, hi = int(rows.min()), int(rows.max()) + 1
            x = transform(raw[lo:hi])  # each source frame is resized once per batch of clips
            got = net(x[torch.from_numpy(rows - lo).to(dev)], return_index=True)
            outs.append(got)
            clip_lines += post(got, s)
        torch.cuda.synchronize()
        fps["clip"] = args.frames / (time.perf_counter() - t0)
    clip = [torch.cat(ts, 0) for ts in zip(*outs)]

    for name, a, b in zip(("ids", "scores", "bboxes", "keep_idx"), video, clip):
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    assert lines == clip_lines
    for l in lines[:5]:
        print(l)
    print("%d frames, k = %d, step = %d, %s join: %d prediction lines, video path equals clip path bit for bit" % (
        args.frames, args.k, args.step, args.join, len(lines)))
    print("video path %.1f frames/s   clip path %.1f frames/s   (ring of %d slots, %d frames per backbone call)" % (
        fps["video"], fps["clip"], session.ring, session.frames_per_step))


if __name__ == "__main__":
    main()
