"""-m gpu: examples/eval_coco.py runs end to end at a small size — a synthetic dataset scored with the COCO metric through
the device path and the host path; the script itself asserts that both give the same results."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_eval_coco_example():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "examples/eval_coco.py", "--images", "6", "--size", "64", "--batch", "4"], cwd=ROOT,
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, universal_newlines=True)
    assert p.returncode == 0, p.stdout[-3000:]
    assert "Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ]" in p.stdout
    assert "6 images in 2 launches: device path equals host path" in p.stdout
