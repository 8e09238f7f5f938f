"""-m gpu: examples/train_hier.py --join conv runs end to end at a small size — a single-frame model's file into a
[3,3,1,1,1] net with the learned join (allow_missing: the joins keep their mean start), augmented training steps on 9-frame
clips, a validation pass — and the loss is finite and changes from step to step."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_train_hier_example_with_the_conv_join():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "examples/train_hier.py", "--join", "conv", "--size", "96", "--clips", "2", "--steps", "3",
                        "--src", "72x96"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, universal_newlines=True)
    assert p.returncode == 0, p.stdout[-3000:]
    out = p.stdout
    assert "(conv join): clips of 9 frames" in out and "mAP" in out
    steps = [l for l in out.splitlines() if l.startswith("step ")]
    assert len(steps) == 3
    rows = [[float(l.split(key)[1].split()[0]) for key in ("obj", "center", "scale", "cls")] for l in steps]
    assert all(v == v and abs(v) != float("inf") and v >= 0 for r in rows for v in r), rows
    assert all(r[0] > 0 for r in rows) and len({tuple(r) for r in rows}) == 3, rows  # finite, and it changes
