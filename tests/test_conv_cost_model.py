"""-m "not gpu": the conv launch decision (vy_conv_plan of videoyolo_amd/csrc/conv_launch.h, the function every conv launch
goes through, over the cost models of conv_cost_model.h) compiled with g++: the (kernel, block tile, schedule) decisions for BASELINE's conv shapes as they were measured and adopted on
the MI355X (profiles/r03_layers_608_b64.txt, r03_train416_b16_layers.txt), and the model's structural properties."""
import os
import subprocess

from videoyolo_amd.build import HIPCC

HERE = os.path.dirname(os.path.abspath(__file__))

# M N K -> tile of the exact kernel | conv mode split_bf16x3: the kernel the launch goes to (round 4;
# profiles/r04_layers_608_b64_split.txt, tools/probe/run_split_batch_sweep.sh, run_split_ksplit_sweep.sh):
# 608x608 batch 64, then 416x416 batch 16 (training forward shapes), then batch 1; third column: 3x3 cells the Winograd
# F(2, 3) instance takes instead (conv_wino.hip, vy_predict_wino; fitted on tools/layer_profile.py sweeps).
# Last column: LDS stages and schedule of the exact form, as the training labels print them (s4: four stages; sk: stream-K;
# ks<S>: split-K; ck<S>: S runs of K with parked chains; plain: none of these).
# After "-- 128 CUs": the exact kernel's tiles on a device of 128 CUs (the models count rounds in the device's CU count;
# the split / Winograd choices are refused there: vy_model_fitted, checked by the program itself)
EXPECTED = """\
5914624 64 288 -> 128x64   | split 256x64   | plain
5914624 32 64 -> 128x32   | plain
1478656 128 576 -> 128x128   | split 128x128   | wino   | plain
1478656 64 128 -> 128x64   | split 128x64   | plain
369664 256 1152 -> 128x128   | split 128x128   | wino   | plain
369664 128 256 -> 128x128   | split 128x128   | plain
92416 512 2304 -> 128x128sk   | split 128x128   | wino   | sk
92416 256 512 -> 128x128   | split 128x128   | plain
23104 1024 4608 -> 128x128sk   | split 128x128   | wino   | ck4sk
23104 512 1024 -> 128x128   | split 128x128   | plain
23104 75 1024 -> 64x64   | plain
43264 256 1152 -> 128x128sk   | split 128x128   | -   | sk
10816 512 2304 -> 128x64sk   | split 128x128 k2   | -   | sk
2704 1024 4608 -> 64x64sk   | split 128x64 k2   | -   | ck4sk
2704 512 1024 -> 64x64   | split 128x128 k5   | s4
43264 128 256 -> 128x64   | split 128x64   | plain
5776 256 1152 -> 64x64   | split 128x128 k5   | -   | s4
361 1024 4608 -> 64x64   | split 128x128 k10   | -   | s4ks4
-- 128 CUs
5914624 64 288 -> 128x64   | plain
5914624 32 64 -> 128x32   | plain
1478656 128 576 -> 128x128   | plain
1478656 64 128 -> 128x64   | plain
369664 256 1152 -> 128x128   | plain
369664 128 256 -> 128x128   | plain
92416 512 2304 -> 128x128   | plain
92416 256 512 -> 128x64   | plain
23104 1024 4608 -> 128x64   | ck4
23104 512 1024 -> 128x128   | plain
23104 75 1024 -> 128x64   | plain
43264 256 1152 -> 128x64   | plain
10816 512 2304 -> 64x64   | plain
2704 1024 4608 -> 128x64   | ck4
2704 512 1024 -> 64x64   | s4
43264 128 256 -> 128x128   | plain
5776 256 1152 -> 64x64   | s4
361 1024 4608 -> 64x64   | s4ck4
"""


def test_tile_and_stream_k_decisions(tmp_path):
    exe = str(tmp_path / "conv_cost_model_check")
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "include")  # (ConvArgs: kernels.h)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-isystem", rocm_include, "-o", exe,
                    os.path.join(HERE, "conv_cost_model_check.cpp")], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=60)
    assert p.returncode == 0, p.stderr
    assert p.stdout == EXPECTED, p.stdout
