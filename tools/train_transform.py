"""Cost of the training transform (csrc/augment.hip) next to the training step it feeds: ms per batch of 16 samples from
720p sources to 416 x 416 for each of the five interpolations, at k = 1 (single-frame net) and k = 3 (window net), timed
with device events after a warm-up, ALTERNATING with the training step of the same net in the same process (so both see
the same clocks), in a fresh child process.  The descriptor is the costliest plain draw: the whole 720p frame as the crop
(every source byte is read), all four colour ops, flipped.  A second descriptor crops a 4x-expanded canvas (mostly fill;
the largest shrink factors).  Bytes moved per launch: the sources once plus the output.  t.batch's wall time from host
numpy sources (draws, packing, the copy to the device, both launches) is printed for information.

With --stats the same child runs a second time under `rocprofv3 --kernel-trace --stats` and the kernel's own mean time
is added.  The table goes to --out (default profiles/train_transform.txt).

With --mixup the whole-frame draw is also timed through vy_train_transform_mix, every sample mixed with a
second source of the same size (each tap reads twice the source bytes: the costliest mix), in the same rounds as the plain
launches; and from host numpy sources, alternating, the wall time of the mixed path (pack both sources, one copy, the mix
launch) next to the path it replaces (MixedClip.numpy() on the host, pack, one copy, the plain launch).

    python tools/train_transform.py [--stats] [--mixup] [--size 416] [--batch 16] [--src 720x1280] [--rounds 3] [--out PATH]
"""
import argparse
import json
import os
import sys
import time

import _measure
from _measure import ROOT

sys.path.insert(0, ROOT)
CHILD_TIMEOUT_S = 600  # either child: the measurement, or the same under rocprofv3
INTERP = ["nearest", "linear", "cubic", "area", "lanczos4"]


def measure(args):
    import ctypes
    import numpy as np
    import torch
    import videoyolo_amd as vy
    from videoyolo_amd import _lib, autograd, targets
    from videoyolo_amd.transforms import YOLO3VideoTrainTransform

    dev = torch.device("cuda", 0)
    lib = _lib.load()
    classes = ["c%d" % i for i in range(20)]
    b, s = args.batch, args.size
    sh, sw = [int(v) for v in args.src.split("x")]
    base = vy.yolo3_darknet53(classes, pretrained_base=False)
    base.initialize(init="synthetic", seed=233)
    params = {p.name: p.data() for p in base.collect_params().values()}
    f32 = np.float32
    hue = np.eye(3, dtype=f32) * f32(0.9) + f32(0.03)
    ops = [(_lib.VY_AUG_BRIGHTNESS, f32(12.5), f32(0)), (_lib.VY_AUG_CONTRAST, f32(1.2), f32(0)),
           (_lib.VY_AUG_SATURATION, f32(0.8), f32(0.2)), (_lib.VY_AUG_HUE, f32(0), f32(0))]
    draws = {
        "whole frame": dict(src=(sh, sw), expand=None, crop=(0, 0, sw, sh), flip=True, ops=ops, hue=hue),
        "expanded x4": dict(src=(sh, sw), expand=(sw, sh, 4 * sw, 4 * sh), crop=(sw // 2, sh // 2, 3 * sw, 3 * sh), flip=True,
                            ops=ops, hue=hue),
    }
    out = {"device": torch.cuda.get_device_name(0), "batch": b, "size": s, "src": [sh, sw], "rounds": args.rounds, "k": {}}
    for k in (1, 3):
        if k == 1:
            net = vy.yolo3_darknet53(classes, pretrained_base=False)
        else:
            net = vy.yolo3_darknet53(classes, pretrained_base=False, k=k, k_join_type="max", k_join_pos="early")
        net.set_parameters(params)
        net.collect_params().reset_ctx(dev)
        tr = vy.Trainer(net.collect_params(), "sgd", {"learning_rate": 1e-4, "wd": 5e-4, "momentum": 0.9})
        gt_boxes, gt_ids = targets.synthetic_gt(b, s, len(classes), m=8, seed=1)
        gt = torch.as_tensor(gt_boxes).to(dev)
        fixed = targets.YOLOV3PrefetchTargetGenerator(len(classes))(s, s, gt_boxes, gt_ids, device=dev)
        t = YOLO3VideoTrainTransform(k, s, s, net)
        frame_bytes = sh * sw * 3
        src = torch.randint(0, 256, (b * k * frame_bytes,), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(dev)
        x = torch.empty((b, k, 3, s, s) if k > 1 else (b, 3, s, s), dtype=torch.float32, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        three = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

        def launch(descs):
            _lib.check(lib.vy_train_transform(ctypes.c_void_p(src.data_ptr()), descs, b, k, ctypes.c_void_p(x.data_ptr()), s, s,
                                              three(t._fill), three(t._mean), three(t._std), stream))

        def step():
            with autograd.record():
                l = net(x, gt, *fixed)
                autograd.backward([l[0] + l[1] + l[2] + l[3]])
            tr.step(b)

        timed = lambda fn, n: _measure.timed(torch, fn, n)  # noqa: E731

        descs = {}
        for name, d in draws.items():
            for interp in range(5):
                a = dict(d, interp=interp)
                descs[name, interp] = (_lib.TrainAug * b)(*[t.descriptor(a, i * k * frame_bytes) for i in range(b)])
        if args.mixup:
            from videoyolo_amd.transforms import MixedClip
            # the first sources again, then as many second sources; sample i is mixed with sample b + i
            src_mix = torch.cat([src, torch.randint(0, 256, (b * k * frame_bytes,), dtype=torch.uint8,
                                                    generator=torch.Generator().manual_seed(1)).to(dev)])
            mix_one = _lib.TrainMix * b
            mixes = mix_one(*[_lib.TrainMix((b + i) * k * frame_bytes, sh, sw, sh, sw, float(np.float32(0.37)), float(np.float32(1.0 - 0.37)))
                              for i in range(b)])

            def launch_mix(descs):
                _lib.check(lib.vy_train_transform_mix(ctypes.c_void_p(src_mix.data_ptr()), descs, mixes, b, k,
                                                      ctypes.c_void_p(x.data_ptr()), s, s, three(t._fill), three(t._mean),
                                                      three(t._std), stream))
            for interp in range(5):
                launch_mix(descs["whole frame", interp])
            ms_mix = {interp: [] for interp in range(5)}
        launch(descs["whole frame", 1])  # a real input for the step
        for _ in range(args.warmup):
            step()
        for key in descs:
            launch(descs[key])
        torch.cuda.synchronize()
        ms = {key: [] for key in descs}
        step_ms = []
        for _ in range(args.rounds):
            for key in descs:
                ms[key].append(timed(lambda: launch(descs[key]), args.launches))
                if args.mixup and key[0] == "whole frame":
                    ms_mix[key[1]].append(timed(lambda: launch_mix(descs[key]), args.launches))
            step_ms.append(timed(step, args.steps))
        med = lambda v: float(np.median(v))  # noqa: E731
        # t.batch end to end from host numpy sources (information only: the copy of the sources dominates)
        host = [np.random.default_rng(i).integers(0, 256, (k, sh, sw, 3), dtype=np.uint8) for i in range(b)]
        labels = [np.array([[100, 100, 600, 500, 3]], np.float32) for _ in range(b)]
        t.batch(host, labels, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            t.batch(host, labels, device=dev)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / 3 * 1e3
        out["k"][str(k)] = {
            "step_ms": round(med(step_ms), 3), "step_ms_rounds": [round(v, 3) for v in step_ms],
            "bytes_per_launch": b * k * frame_bytes + b * k * 3 * s * s * 4,
            "transform_ms": {"%s/%s" % (n, INTERP[i]): round(med(v), 4) for (n, i), v in ms.items()},
            "batch_wall_ms_from_host": round(wall, 2)}
        if args.mixup:
            host2 = [np.random.default_rng(100 + i).integers(0, 256, (k, sh, sw, 3), dtype=np.uint8) for i in range(b)]
            whole = [dict(draws["whole frame"], interp=1)] * b

            def wall_ms(make):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                t.transform_frames(make(), whole, device=dev)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3
            in_launch = lambda: [MixedClip(u, v, 0.37) for u, v in zip(host, host2)]  # noqa: E731
            on_host = lambda: [MixedClip(u, v, 0.37).numpy() for u, v in zip(host, host2)]  # noqa: E731
            wall_ms(in_launch), wall_ms(on_host)
            walls = {"in_launch": [], "on_host": []}
            for _ in range(3):  # alternating
                walls["in_launch"].append(wall_ms(in_launch))
                walls["on_host"].append(wall_ms(on_host))
            out["k"][str(k)]["mixup"] = {
                "bytes_per_launch": 2 * b * k * frame_bytes + b * k * 3 * s * s * 4,
                "transform_ms": {INTERP[i]: round(med(v), 4) for i, v in ms_mix.items()},
                "plain_ms_rounds": {INTERP[i]: [round(u, 4) for u in ms["whole frame", i]] for i in range(5)},
                "mix_ms_rounds": {INTERP[i]: [round(u, 4) for u in v] for i, v in ms_mix.items()},
                "wall_ms_in_launch": [round(v, 1) for v in walls["in_launch"]],
                "wall_ms_blend_on_host": [round(v, 1) for v in walls["on_host"]]}
        del net, tr
    return out


def kernel_stats(argv):
    rows = _measure.kernel_rows(__file__, ["--child", "--rounds", "1", "--launches", "3", "--steps", "1", "--warmup", "1"] + argv,
                                CHILD_TIMEOUT_S, "train_transform_")
    if isinstance(rows, dict):
        return rows
    found = {}
    for r in rows:
        if "train_transform_kernel" in r["name"]:  # the mix instantiation carries its argument struct's name
            found.setdefault("mix" if "MixArgs" in r["name"] else "plain", _measure.stats_of(r))
    if "plain" not in found:
        return {"error": "no train_transform_kernel row in the kernel statistics"}
    return dict(found["plain"], mix=found["mix"]) if "mix" in found else found["plain"]


def table(res, stats):
    lines = ["Training transform next to the training step: %s, batch %d, %dx%d sources -> %d x %d, median of %d rounds" % (
        res["device"], res["batch"], res["src"][0], res["src"][1], res["size"], res["size"], res["rounds"]),
        "(device events; transform launches and training steps alternate in one process; tools/train_transform.py)", ""]
    for k, r in res["k"].items():
        lines.append("k = %s   training step %.3f ms (rounds %s)   %.1f MB moved per launch (sources once + output)" % (
            k, r["step_ms"], r["step_ms_rounds"], r["bytes_per_launch"] / 1e6))
        lines.append("  %-28s %10s %12s %10s" % ("draw / interp", "ms/batch", "% of step", "GB/s"))
        for name, ms in r["transform_ms"].items():
            lines.append("  %-28s %10.4f %11.2f%% %10.0f" % (name, ms, 100 * ms / r["step_ms"], r["bytes_per_launch"] / ms / 1e6))
        worst = max(r["transform_ms"].values())
        lines.append("  slowest: %.2f%% of the step (bar: 2%%) -> %s" % (100 * worst / r["step_ms"],
                                                                        "within" if worst <= 0.02 * r["step_ms"] else "MISSED"))
        lines.append("  t.batch from host numpy sources, wall: %.1f ms (draws, packing, host-to-device copy, both launches)" % (
            r["batch_wall_ms_from_host"]))
        if "mixup" in r:
            m = r["mixup"]
            lines.append("  mixup, whole frame, every sample mixed with a second %dx%d source: %.1f MB moved per launch" % (
                res["src"][0], res["src"][1], m["bytes_per_launch"] / 1e6))
            lines.append("  %-28s %10s %12s %10s   %s" % ("mix launch / interp", "ms/batch", "x plain", "GB/s", "rounds: plain | mix"))
            for name, ms in m["transform_ms"].items():
                plain = r["transform_ms"]["whole frame/" + name]
                lines.append("  %-28s %10.4f %12.2f %10.0f   %s | %s" % (name, ms, ms / plain, m["bytes_per_launch"] / ms / 1e6,
                                                                         m["plain_ms_rounds"][name], m["mix_ms_rounds"][name]))
            lines.append("  from host numpy sources, linear, wall ms: both sources packed + mix launch %s; MixedClip.numpy() on the "
                         "host + plain launch %s" % (m["wall_ms_in_launch"], m["wall_ms_blend_on_host"]))
        lines.append("")
    if stats is not None:
        lines.append("rocprofv3 --kernel-trace --stats, train_transform_kernel over both k, both draws and all interps: %s" %
                     json.dumps(stats))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--src", default="720x1280")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stats", action="store_true")
    ap.add_argument("--mixup", action="store_true", help="also time vy_train_transform_mix and the host blend it replaces")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_transform.txt"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args)))
        return
    argv = ["--size", str(args.size), "--batch", str(args.batch), "--src", args.src] + (["--mixup"] if args.mixup else [])
    res = _measure.run_child(__file__, ["--child", "--rounds", str(args.rounds), "--launches", str(args.launches), "--steps",
                                        str(args.steps), "--warmup", str(args.warmup)] + argv, CHILD_TIMEOUT_S)
    text = table(res, kernel_stats(argv) if args.stats else None)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
