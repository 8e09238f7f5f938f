"""-m gpu: examples/worst_clips.py runs end to end at its smallest setting — synthetic videos through a window net's
detect_video, every batch into a FrameMApMetric and a VOCMApMetric as device tensors; the script itself asserts that the
device path ran and that the frame scores equal frame_map_host's."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_worst_clips_example():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, "examples/worst_clips.py", "--videos", "2", "--frames", "4", "--size", "64", "--k", "3",
                        "--batch", "2"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600,
                       universal_newlines=True)
    assert p.returncode == 0, p.stdout[-3000:]
    assert "2 videos of 4 frames at 64 x 64, k = 3: " in p.stdout and "on the device in 4 launches" in p.stdout
    assert "videos, worst first" in p.stdout and "video0/000000.JPEG," in p.stdout
    assert "device frame scores equal the host's" in p.stdout
