"""-m gpu: examples/detect_hier_video.py runs end to end — the reference's windowed detect loop (detect_yolo3.py --window
T,step) with a hierarchical net on a synthetic video through the public surface only; the script itself asserts that
hier_detect_video and the clip path return the same bits."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("join", ["max", "conv"])
def test_detect_hier_video_example(join):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "examples/detect_hier_video.py", "--frames", "10", "--size", "256", "--join", join,
                        "--frames-per-step", "4"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=600, universal_newlines=True)
    assert p.returncode == 0, p.stdout[-3000:]
    assert "10 frames, hierarchical [3, 3, 1, 1, 1] (T = 9)" in p.stdout and "bit for bit" in p.stdout
    assert "video path" in p.stdout and "clip path" in p.stdout and "frames/s" in p.stdout
