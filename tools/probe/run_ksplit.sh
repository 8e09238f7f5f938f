#!/bin/bash
# A/B of the split-K execution form of the pinned run order (VY_CONV_KSPLIT, conv_igemm.hip).  The summation order cuts
# long K into runs (include/vy_math.h); a launch whose tiles leave at least half of the CUs empty either runs each run of a
# tile in a workgroup of its own, the last one adding the others' sums in run order (VY_CONV_KSPLIT=1, the default), or
# runs the runs in turn in one workgroup with the finished chains parked in scratch (VY_CONV_KSPLIT=0).  Both forms give
# the same bits: this prices only the execution form, one frame at 608 / 416 (latency and per-launch tables).
# (Not the round-6 experiment that priced independent chains before the order was pinned: profiles/r06_ksplit_probe.txt.)
R=$(cd "$(dirname "$0")/../.." && pwd)
OUT=${OUT:-/tmp}
cd /tmp; export TMPDIR=/tmp
for size in 608 416; do
  for ks in 0 1; do
    echo "== size $size VY_CONV_KSPLIT=$ks"
    VY_CONV_KSPLIT=$ks python3 $R/tools/small_batch_latency.py --size $size --batches 1,2,4 2>/dev/null
    VY_CONV_KSPLIT=$ks python3 $R/tools/small_batch_latency.py --size $size --batches 1 --graph 2>/dev/null | sed 's/^/graph /'
    VY_CONV_KSPLIT=$ks python3 $R/tools/layer_profile.py --size $size --batch 1 --out $OUT/ks${ks}_layers_${size}_b1.txt > /dev/null 2>&1
  done
done
