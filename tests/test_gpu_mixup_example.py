"""-m gpu: examples/train_mixup.py runs end to end at 64 x 64 — MixupDetection round synthetic uint8 videos of differing
sizes, mixup on with beta(1.5, 1.5) and off for the last epoch, into training steps of a k = 3 window net and of a
single-frame net, through the public surface only; the script itself asserts that the mix launch's batch equals the
batch made from MixedClip.numpy()-materialised clips under the same seeds, and that every loss is finite."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_train_mixup_example():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "examples/train_mixup.py", "--size", "64", "--clips", "3", "--k", "3", "--epochs", "2",
                        "--no-mixup-epochs", "1"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=600, universal_newlines=True)
    assert p.returncode == 0, p.stdout[-3000:]
    assert "k = 3: 3 clips per step" in p.stdout and "k = 1: 3 clips per step" in p.stdout
    assert p.stdout.count("equals the host blend, bit for bit") == 2
    assert "x (3, 3, 3, 64, 64)" in p.stdout and "x (3, 3, 64, 64)" in p.stdout
    assert p.stdout.count("mixed 3/3") == 2 and p.stdout.count("mixed 0/3") == 2
    assert p.stdout.count("  epoch ") == 4 and "trained with mixup" in p.stdout
