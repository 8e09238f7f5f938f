"""-m gpu: examples/train_augmented.py runs end to end at 64 x 64 — synthetic uint8 videos of differing sizes through
YOLO3VideoTrainTransform.batch into training steps of a k = 3 window net and of a single-frame net, through the public
surface only; the script itself asserts that every loss is finite."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_train_augmented_example():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "examples/train_augmented.py", "--size", "64", "--clips", "3", "--k", "3", "--steps",
                        "2"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600,
                       universal_newlines=True)
    assert p.returncode == 0, p.stdout[-3000:]
    assert "k = 3: 3 clips per step" in p.stdout and "k = 1: 3 clips per step" in p.stdout
    assert "x (3, 3, 3, 64, 64)" in p.stdout and "x (3, 3, 64, 64)" in p.stdout
    assert p.stdout.count("  step ") == 4 and "trained on augmented clips" in p.stdout
