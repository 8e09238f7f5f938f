// conv_launch.h — what a conv launch is, decided once.  vy_conv_plan turns a launch's ConvArgs into a VyConvPlan: which of the
// three kernels serves it (exact fp32 conv_igemm.hip, split-fp32 conv_split.hip, Winograd conv_wino.hip; none: the launch is
// refused), on which block tile, with how many LDS stages and on which schedule.  The launchers execute that value
// (vy_launch_conv), the profile and the training step print it (vy_conv_plan_label), the training step reads its
// statistics rows from it — nobody asks a second time.  Host-only, plain C++: tests/conv_cost_model_check.cpp calls the
// same function under g++.  Every comparison between kernels and every scratch / overflow guard of a launch lives here.
#pragma once

#include <algorithm>
#include <cstdio>

#include "kernels.h"
#include "../../include/vy_math.h"
#include "conv_cost_model.h"

#ifndef VY_SPLIT_M16  // the split kernel's MFMA shape (split_device.h)
#define VY_SPLIT_M16 0
#endif

enum VyKernelId { VY_KERNEL_NONE = 0, VY_KERNEL_EXACT, VY_KERNEL_SPLIT, VY_KERNEL_WINO };

struct VyConvPlan {
  int kernel;        // VyKernelId; none: the launch is refused (hipErrorInvalidValue)
  int bm, bn, ns;    // block tile; LDS stages of the exact instance (2 / 4)
  int sk, ks, ck;    // exact: stream-K; split-K workgroups per tile; the runs of K one workgroup takes in turn with parked
                     // chains (0: K is one run, or the launch is split-K)
  int split_ks;      // split kernel: k-slices (1: none)
  long long grid;    // workgroups of the (first) launch
  int k_chunk;       // exact: k-steps per run (ConvArgs::k_chunk of the launch; 0: one run)
  int stat_rows;     // rows of per-tile statistics the launch writes when a.stats is set
};

// resident blocks per CU of the five exact instances (their stream-K build), forward and data gradient
enum { VY_EXACT_128x128 = 0, VY_EXACT_128x64, VY_EXACT_128x32, VY_EXACT_64x64, VY_EXACT_64x64_S4, VY_EXACT_INSTANCES };
struct VyConvResidency {
  int fwd[VY_EXACT_INSTANCES], dgrad[VY_EXACT_INSTANCES];
};

// ---- what each kernel can serve
inline bool vy_conv_split_supported(const ConvArgs& a) {  // N % 64 == 0, Kc % 32 == 0, an epilogue the kernel has
  if (!a.w_split) return false;
  if (a.stats && VY_SPLIT_M16) return false;
  if (a.Kc % 32 != 0 || a.N % 64 != 0 || a.ntaps < 1 || a.ntaps > 9) return false;
  return vy_conv_epilogue_supported(a);
}
inline bool vy_conv_wino_supported(const ConvArgs& a) {
  if (!a.w_wino || a.ntaps != 9 || a.a_s != 1 || a.ups != 1 || a.o_s != 1 || a.dgrad || a.stats) return false;
  if (!a.scale || !a.shift || !a.leaky) return false;  // the conv + BN + leaky cell (+ residual)
  if (a.Kc % 32 != 0 || a.N % 128 != 0 || a.LW < 2) return false;
  for (int t = 0; t < 9; ++t)
    if (a.tap_dy[t] != t / 3 - 1 || a.tap_dx[t] != t % 3 - 1 || a.tap_w[t] != t) return false;
  return true;
}
// pixel pairs per block of a Winograd launch (probe builds: VY_WINO_BM=128)
inline int vy_conv_wino_bm(const ConvArgs& a) {
#ifdef VY_WINO_BM128
  if (vy_args_knobs(a).wino_bm == 128) return 128;
#endif
  return 64;
}
// k-slices the split kernel's slab scratch holds, 64 at most
inline int vy_conv_split_max_ksplit(const ConvArgs& a) {
  if (!a.splitk_slabs || a.stats) return 1;  // (the per-tile statistics need whole sums)
  return (int)std::min<long long>(std::max<long long>(1, (long long)(a.splitk_bytes / ((unsigned long long)a.M * a.N * 4ull))), 64);
}
// ck_scratch bytes a conv of M x N outputs summed in `runs` runs may need (any tile)
inline size_t vy_conv_chunk_scratch_bytes(long long M, int N, int runs) {
  const long long m = (M + 127) / 128 * 128, n = ((long long)N + 127) / 128 * 128;
  return runs > 1 ? (size_t)((runs - 1) * m * n * 4) : 0;
}

// Data gradients are never stream-K by the model (in the training step the weight-gradient stream runs beside them and
// its blocks already fill the CUs a partly filled round leaves idle; measured, stream-K there only moves the idle time);
// VY_CONV_SK_SLOTS (tests) forces it on them too
inline bool vy_conv_sk_allowed(const ConvArgs& a) {
  const VyKnobs& k = vy_args_knobs(a);
  return k.conv_sk && a.sk_partials && a.sk_flags && (!a.dgrad || k.conv_sk_slots > 0);
}

// ---- the exact kernel's form on block tile bm x bn: stages, runs of K, schedule.  false: refused
inline bool vy_conv_plan_exact(const ConvArgs& a, const VyConvResidency& res, int bm, int bn, VyConvPlan* p) {
  const VyKnobs& knobs = vy_args_knobs(a);
  const int cus = vy_args_cus(a);
  int inst = bn == 32 ? VY_EXACT_128x32 : bm == 128 && bn == 64 ? VY_EXACT_128x64 : bm == 64 ? VY_EXACT_64x64 : VY_EXACT_128x128;
  if (inst == VY_EXACT_64x64) {
    // few blocks (at most two per CU) and a k-loop long enough to fill it: the four-stage pipeline
    const long long nb = (long long)((a.M + 63) / 64) * ((a.N + 63) / 64);
    if (nb <= 512 && a.ntaps * (a.Kc >> 5) >= 8) inst = VY_EXACT_64x64_S4;
  }
  static const int kTile[VY_EXACT_INSTANCES][2] = {{128, 128}, {128, 64}, {128, 32}, {64, 64}, {64, 64}};
  const int BM = kTile[inst][0], BN = kTile[inst][1];
  const int tiles_m = (a.M + BM - 1) / BM, tiles_n = (a.N + BN - 1) / BN;
  const long long tiles = (long long)tiles_m * tiles_n;
  p->kernel = VY_KERNEL_EXACT;
  p->bm = BM;
  p->bn = BN;
  p->ns = inst == VY_EXACT_64x64_S4 ? 4 : 2;
  p->grid = tiles_m * tiles_n;
  p->stat_rows = tiles_m;
  if (!vy_conv_epilogue_supported(a)) return false;
  // the runs of the pinned summation order (forward launches only; gradients are not held to the oracle's bits)
  const int T_runs = a.ntaps * (a.Kc >> 5);
  const int ksplit_S = a.dgrad ? 1 : vy_conv_runs(a.ntaps, a.Kc >> 5);
  if (ksplit_S > 1) {
    p->k_chunk = T_runs / ksplit_S;
    p->ck = ksplit_S;
    // a workgroup that runs more than one run of a tile parks the finished runs' sum in the tile's scratch
    if (!a.ck_scratch || (ksplit_S - 1) * tiles * BM * BN * 4ll > (long long)a.ck_bytes) return false;
  }
  // Stream-K when the cost model says it pays (vy_predict_launch): the launches whose last round of the CUs is poorly
  // filled.  ON by default for forward launches since the hand-off is write-through and the schedule keeps a plain
  // launch's locality (profiles/r03_negative_results.txt section 2 has the two builds that lost and why): 608x608
  // batch 64 +0.7 %, 416x416 +0.6 %, the training forward -0.3 ms; VY_CONV_SK=0 restores plain launches.
  if (!vy_conv_sk_allowed(a)) return true;
  const int res_f = res.fwd[inst], res_d = res.dgrad[inst];
  const int sk_slots = knobs.conv_sk_slots;
  // blocks per CU: as many as fit, but never so many that a share is shorter than one tile (a share is at most
  // [head][whole tiles][tail]).  344 tiles (the 13x13 maps at batch 16): ONE block per CU with 1.34 tiles each, where
  // the plain launch leaves 88 CUs with two tiles and 168 with one
  const long long per_cu = std::min<long long>(a.dgrad ? res_d : res_f, tiles / cus);
  const long long G = sk_slots > 0 ? sk_slots : (long long)cus * per_cu;
  // Split-K: a launch whose K is summed in S > 1 runs (the pinned order, vy_math.h) and whose tiles leave at least half
  // of the CUs empty goes out as tiles x S workgroups, one run each; the last run's workgroup adds the others' sums in
  // run order (conv_tile, ks_reduce) — the same arithmetic as one workgroup running the runs one after the other.
  // Measured (profiles/r06_ksplit_probe.txt, one frame): 13x13 / 19x19 3x3 cells on 512 channels 75 -> 33 / 47 us; a
  // launch of 184 tiles cut in two lost 4 %: hence tiles <= CUs / 2.  VY_CONV_KSPLIT=0: never.
  if (ksplit_S > 1) {
    const long long cap = (long long)cus * res_f;
    if (knobs.conv_ksplit && sk_slots == 0 && 2 * tiles <= cus && tiles * ksplit_S <= cap && tiles * ksplit_S * BM * BN * 4ll <= (long long)a.sk_bytes &&
        tiles * ksplit_S <= a.sk_nflags) {
      p->ks = ksplit_S;
      p->ck = 0;  // one workgroup per run: nothing is parked
      p->grid = tiles * ksplit_S;
      return true;
    }
  }
  bool pays = false;
  if (const VyTileModel* tm = vy_tile_model(BM, BN))
    vy_predict_launch(a.M, a.N, (double)a.ntaps * a.Kc, *tm, VySkPolicy{true, knobs.conv_sk_gain, knobs.conv_sk_cost}, &pays, cus);
  if (G > 0 && tiles > G && tiles * (G + 8) < (1ll << 31) && 2 * (G / 8 + 1) * (long long)(a.ntaps * (a.Kc >> 5)) < (1ll << 31) &&
      (sk_slots > 0 || pays) && G * BM * BN * 4ll <= (long long)a.sk_bytes && G <= a.sk_nflags) {
    p->sk = 1;
    p->grid = G;
  }
  return true;
}

// The plan of a launch.  Order of preference: Winograd, split, exact.  Each of the other two kernels has to be supported
// (weight images included) and predicted faster than what it replaces by 3 % (conv_cost_model.h; both comparisons were
// fitted on 256 CUs and are refused elsewhere: vy_model_fitted) —
//   split    against the exact kernel's model: small launches (a single frame's deep layers) stay on the exact kernel,
//            which has the small tiles and stream-K.  VY_SPLIT_ALWAYS=1 (tests): every supported launch, however small
//   Winograd against the better of the other two: at 608x608 every supported cell from batch 8 on, the 152x152 / 76x76 ones
//            from batch 2, none of a single frame's (the split kernel's k-split covers those).  VY_SPLIT_WINO=0: never,
//            =2: wherever supported (tests)
// Each model is evaluated at most once; with neither set of weight images (the default conv mode) only the exact tile choice runs.
inline VyConvPlan vy_conv_plan(const ConvArgs& a, const VyConvResidency& res) {
  VyConvPlan p = {};
  p.split_ks = 1;
  const VyKnobs& knobs = vy_args_knobs(a);
  const int cus = vy_args_cus(a);
  const double K = (double)a.ntaps * a.Kc;
  const bool split_ok = a.w_split && vy_conv_split_supported(a), wino_ok = a.w_wino && vy_conv_wino_supported(a);
  const bool wino_model = wino_ok && knobs.split_wino == 1 && vy_model_fitted(cus);
  const bool split_model = split_ok && !knobs.split_always && vy_model_fitted(cus);
  // the exact kernel's own tile and predicted time (0: N <= 32, its own tile, no model — never handed on)
  int bm = 0, bn = 0;
  double t_exact = 0.0;
  if (wino_model || split_model || !knobs.conv_force_bm) {
    bool sk_unused;
    t_exact = vy_select_tile(a.M, a.N, K, VySkPolicy{vy_conv_sk_allowed(a), knobs.conv_sk_gain, knobs.conv_sk_cost}, &bm, &bn, &sk_unused, cus);
  }
  // the split kernel's tile and k-split: the cost model's choice among 128x128, 128x64 and, for the 64-channel layers,
  // 256x64; k-split > 1 only where the slabs fit the scratch the net provides
  const int max_ks = split_ok ? vy_conv_split_max_ksplit(a) : 1;
  int sbm = 0, sbn = 0, sks = 1;
  const double t_split = split_ok ? vy_predict_split(a.M, a.N, K, max_ks, &sbm, &sbn, &sks, cus) : 0.0;

  bool wino = wino_ok && knobs.split_wino == 2;
  if (wino_model) {
    const long long pairs = (long long)a.B * a.LH * ((a.LW + 1) / 2);
    wino = vy_predict_wino(pairs, a.N, a.Kc, cus) < 0.97 * (split_ok ? std::min(t_exact, t_split) : t_exact);
  }
  if (wino) {
    p.kernel = VY_KERNEL_WINO;
    p.bm = vy_conv_wino_bm(a);
    p.bn = 128;
    const long long pairs = (long long)a.B * a.LH * ((a.LW + 1) / 2);
    p.grid = ((pairs + p.bm - 1) / p.bm) * (a.N / 128);
    return p;
  }
  if (split_ok && (knobs.split_always || (split_model && t_split < 0.97 * t_exact))) {
    // VY_SPLIT_FORCE (tests: the forms no small shape reaches): the named tile where the launch's channels divide by it;
    // the named k-split as far as the slabs' scratch, the per-tile statistics (whole sums) and the k-steps allow
    // NOTE: this reaches forms the cost model never picks — 256x64 on layers of 128 channels and more (the model keeps the
    // 256-row tile for the 64-channel layers) and k-slices down to ONE k-step (the model wants steps / S >= 6; T = 1 is
    // served by the k-loop's tail, and the clamp below keeps T >= 1).  The kernel is correct on them, and the per-cell tests
    // that run under this knob certify them too; the census ties plans to walked forms only as (tile, k1 | k>1).
    if (knobs.split_force_bm && a.N % knobs.split_force_bn == 0) {
      sbm = knobs.split_force_bm;
      sbn = knobs.split_force_bn;
    }
    if (knobs.split_force_ks)
      sks = (int)std::max<long long>(1, std::min<long long>({(long long)knobs.split_force_ks, (long long)max_ks, (long long)a.ntaps * (a.Kc >> 4)}));
    p.kernel = VY_KERNEL_SPLIT;
    p.bm = sbm;
    p.bn = sbn;
    p.split_ks = sks;
    p.stat_rows = (a.M + sbm - 1) / sbm;
    p.grid = (long long)p.stat_rows * (a.N / sbn) * sks;
    return p;
  }
  // the exact tile: conv_cost_model.h, or the tile VY_CONV_FORCE names (tools/train_layers.sh, tools/probe/run_model_sweep.sh)
  if (knobs.conv_force_bm) {
    bm = knobs.conv_force_bm;
    bn = knobs.conv_force_bn;
  }
  if (!vy_conv_plan_exact(a, res, bm, bn, &p)) p.kernel = VY_KERNEL_NONE;
  return p;
}

// ---- the label of a plan.  Profile style (the label column of vy_net_profile, after "<cell>|"):
//   "<BM>x<BN>[sk | ks<S>]"   "split<BM>x<BN>[k<S>]"   "wino<BM>x<BN>"
// training style (the "# via" lines of VY_TRAIN_LABELS):
//   "exact <BM>x<BN>[s4][sk | ks<S> | ck<S> | ck<S>sk]"   "split <BM>x<BN> k<S>"
enum { VY_LABEL_PROFILE = 0, VY_LABEL_TRAIN = 1 };
inline void vy_conv_plan_label(const VyConvPlan& p, int style, char* buf, size_t n) {
  char sched[24] = "";
  if (p.kernel == VY_KERNEL_WINO) {
    snprintf(buf, n, "wino%dx%d", p.bm, p.bn);
  } else if (p.kernel == VY_KERNEL_SPLIT) {
    if (style == VY_LABEL_TRAIN) snprintf(buf, n, "split %dx%d k%d", p.bm, p.bn, p.split_ks);
    else if (p.split_ks > 1) snprintf(buf, n, "split%dx%dk%d", p.bm, p.bn, p.split_ks);
    else snprintf(buf, n, "split%dx%d", p.bm, p.bn);
  } else if (style == VY_LABEL_TRAIN) {
    if (p.ks) snprintf(sched, sizeof sched, "ks%d", p.ks);
    else if (p.ck) snprintf(sched, sizeof sched, "ck%d%s", p.ck, p.sk ? "sk" : "");
    else if (p.sk) snprintf(sched, sizeof sched, "sk");
    snprintf(buf, n, "exact %dx%d%s%s", p.bm, p.bn, p.ns == 4 ? "s4" : "", sched);
  } else {
    if (p.ks) snprintf(sched, sizeof sched, "ks%d", p.ks);
    else if (p.sk) snprintf(sched, sizeof sched, "sk");
    snprintf(buf, n, "%dx%d%s", p.bm, p.bn, sched);
  }
}

// ---- executing a plan.  `p` is vy_conv_plan's value for these very arguments: the launchers check the arguments' shape and
// fill the fields the kernels read (fd_lw / fd_lh / pk_* / k_chunk); they decide nothing
const VyConvResidency& vy_conv_residency();  // of the current device (conv_igemm.hip: the occupancy query, once per process; 1 where it fails)
VyConvPlan vy_conv_plan(const ConvArgs& a);   // ... the plan with that table
hipError_t vy_launch_conv_igemm(const ConvArgs& a, const VyConvPlan& p, hipStream_t s);
hipError_t vy_launch_conv_split(const ConvArgs& a, const VyConvPlan& p, hipStream_t s);
hipError_t vy_launch_conv_wino(const ConvArgs& a, const VyConvPlan& p, hipStream_t s);
inline hipError_t vy_launch_conv(const ConvArgs& a, const VyConvPlan& p, hipStream_t s) {
  switch (p.kernel) {
    case VY_KERNEL_EXACT: return vy_launch_conv_igemm(a, p, s);
    case VY_KERNEL_SPLIT: return vy_launch_conv_split(a, p, s);
    case VY_KERNEL_WINO: return vy_launch_conv_wino(a, p, s);
    default: return hipErrorInvalidValue;
  }
}
