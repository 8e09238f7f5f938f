"""-m gpu: examples/validate.py runs end to end — the reference's validate() loop (train_yolov3.py:434-490) on synthetic
frames through the public surface only, the VOC metric fed with device tensors; the script itself asserts that the device
path ran and equals the host path."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_validate_example():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "examples/validate.py", "--size", "96", "--batch", "3", "--batches", "2"], cwd=ROOT,
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, universal_newlines=True)
    assert p.returncode == 0, p.stdout[-3000:]
    assert "6 frames of 96 x 96 in 2 batches" in p.stdout and "mAP = " in p.stdout
    assert "in 2 launches: device path equals host path" in p.stdout
