"""What the measuring tools share: device-event timing, the fresh child process every measurement runs in, the same child
under `rocprofv3 --kernel-trace --stats`, and (the three metric tools) the detect net and the loop that alternates a
metric's update() with detect steps.  Every child has a time limit: a hung one ends the tool, not the machine's queue."""
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(torch, fn, n):
    """ms per call of fn over n calls, by device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def run_child(script, argv, timeout_s):
    """`python script argv` in a fresh process: the JSON of its last stdout line.  A failed or hung child ends the tool."""
    try:
        p = subprocess.run([sys.executable, os.path.abspath(script)] + argv, cwd=ROOT, stdout=subprocess.PIPE,
                           universal_newlines=True, timeout=timeout_s)
    except subprocess.TimeoutExpired:
        sys.exit("the measurement did not finish within %d s" % timeout_s)
    if p.returncode != 0:
        sys.exit(p.returncode)
    return json.loads(p.stdout.strip().splitlines()[-1])


def kernel_rows(script, child_argv, timeout_s, prefix):
    """`python script child_argv` under rocprofv3 --kernel-trace --stats (no counters in that run; output in a temporary
    directory named after prefix): the rows of its kernel statistics as dicts (name, calls, mean_us, min_us, max_us and the
    unrounded mean_ns), or a dict with "error" that says what went wrong."""
    out = tempfile.mkdtemp(prefix=prefix)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "run", "--", sys.executable,
           os.path.abspath(script)] + child_argv
    try:
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True,
                           timeout=timeout_s)
    except subprocess.TimeoutExpired:
        return {"error": "rocprofv3 run did not finish within %d s" % timeout_s}
    if p.returncode != 0:
        return {"error": "rocprofv3 run failed (%d)" % p.returncode, "tail": p.stdout[-1500:]}
    paths = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if not paths:
        return {"error": "no kernel_stats.csv under %s" % out,
                "files": sorted(glob.glob(os.path.join(out, "**", "*"), recursive=True))[:20]}
    rows = []
    for path in paths:
        with open(path) as f:
            for r in csv.DictReader(f):
                us = lambda key: round(float(r.get(key, 0)) / 1e3, 2)  # noqa: E731
                rows.append({"name": r.get("Name") or r.get("KernelName") or "", "calls": int(r["Calls"]),
                             "mean_us": us("AverageNs"), "min_us": us("MinNs"), "max_us": us("MaxNs"),
                             "mean_ns": float(r["AverageNs"])})
    return rows


def stats_of(row, keys=("calls", "mean_us", "min_us", "max_us")):
    return {k: row[k] for k in keys}


# ------------------------------------------------------------------------------------------------- the three metric tools
def detect_net(vy, classes, dev):
    """The single-frame net whose detect step a metric's update() is held against: synthetic weights, the validation NMS."""
    net = vy.yolo3_darknet53(classes, pretrained_base=False)
    net.initialize(init="synthetic", seed=233, obj_bias=-2.0)
    net.collect_params().reset_ctx(dev)
    net.set_nms(0.45, 400, 100)
    return net


def update_and_detect(torch, update, net, dev, batch, sizes, args):
    """args.rounds rounds of args.updates update() calls, then args.steps detect steps of `batch` frames at every size, in
    this process (same clocks).  Returns the update's ms per call round by round, {size: the detect step's ms round by
    round}, and the host's side of one update() call in ms."""
    x = {s: torch.randn((batch, 3, s, s), device=dev) for s in sizes}
    for s in sizes:
        for _ in range(2):
            net(x[s])
    torch.cuda.synchronize()
    upd_ms, det_ms = [], {s: [] for s in sizes}
    for _ in range(args.rounds):
        upd_ms.append(timed(torch, update, args.updates))
        for s in sizes:
            det_ms[s].append(timed(torch, lambda: net(x[s]), args.steps))
    t0 = time.perf_counter()
    for _ in range(args.updates):
        update()
    call_ms = (time.perf_counter() - t0) / args.updates * 1e3      # the host's side of a call: nothing waits for the device
    torch.cuda.synchronize()
    return upd_ms, det_ms, call_ms
