// knobs.h — the library's launch switches.  A net reads them from the environment once, at vy_net_create
// (vy_knobs_read: the only reader of the environment in the library), and keeps its values for its life; launch code
// reads them from the net (vy_net::knobs, ConvArgs::knobs).  The member initialisers are the compiled-in policy.
// None is needed in production: they exist for the GPU tests and for A/B measurements.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <string>

struct VyKnobs {
  // stream-K and split-K of the exact conv kernel (conv_igemm.hip)
  int conv_sk = 1;             // VY_CONV_SK=0: plain launches only
  int conv_sk_slots = 0;       // VY_CONV_SK_SLOTS=n (tests): EVERY launch of more than n tiles on n blocks, data gradients too
  double conv_sk_gain = 0.03;  // VY_CONV_SK_GAIN: stream-K when it saves at least this fraction of the plain launch ...
  double conv_sk_cost = 7.5;   // VY_CONV_SK_COST: ... after this hand-off cost (us)
  int conv_ksplit = 1;         // VY_CONV_KSPLIT=0: a launch whose K is summed in runs never goes out as split-K
  int conv_force_bm = 0, conv_force_bn = 0;  // VY_CONV_FORCE=128x64: every exact launch on that block tile (0: the model's)
  // split-fp32 conv modes (conv_split.hip, conv_wino.hip, wgrad_split.hip, train.hip)
  int split_always = 0;  // VY_SPLIT_ALWAYS=1 (tests): every supported launch to the split kernel, however small
  int split_wino = 1;    // VY_SPLIT_WINO: 1 where the cost models say Winograd wins, 0 never, 2 (tests) wherever supported
  int split_train = 1;   // VY_SPLIT_TRAIN: 0 none, 1 forward + data gradients, 2 forward only, 3 data gradients only
  int split_wgrad = 1;   // VY_SPLIT_WGRAD=0: the weight gradients stay exact
  // VY_SPLIT_FORCE=256x64k4 (tests): every conv_split_kernel launch on that block tile and / or k-split (0: the model's)
  int split_force_bm = 0, split_force_bn = 0, split_force_ks = 0;
  // training step (train.hip)
  int train_side_stream = 1;  // VY_TRAIN_SIDE_STREAM=0: weight gradients on the main stream
  std::string train_labels;   // VY_TRAIN_LABELS=<path>: the first training step's launch labels go there (empty: none)
  // hier-video plans (hier.hip)
  int hier_chain = 1;  // VY_HIER_CHAIN=0 (A/B, tests): the dilated joins as three reads per frame, not as chain walks
  // planners (net_internal.h, train.hip, detect.hip)
  int plan_guard = 0;  // VY_PLAN_GUARD=<bytes> (tests): unused bytes behind every carve; 0 or a multiple of 256 up to 1 MiB
  // measurement builds only (read under -DVY_TRAIN_ABL_BUILD / -DVY_WINO_BM128; the defaults elsewhere)
  int train_abl = 0, train_abl_after = 3;  // VY_TRAIN_ABL, VY_TRAIN_ABL_AFTER
  int wino_bm = 64;                        // VY_WINO_BM=128
};

// the compiled-in policy: for a ConvArgs that did not come from a net (a probe's hand-made one)
inline const VyKnobs& vy_knobs_default() {
  static const VyKnobs k;
  return k;
}

inline VyKnobs vy_knobs_read() {
  VyKnobs k;
  auto geti = [](const char* name, int& v) {
    if (const char* s = getenv(name)) v = atoi(s);
  };
  auto getd = [](const char* name, double& v) {
    if (const char* s = getenv(name)) v = atof(s);
  };
  geti("VY_CONV_SK", k.conv_sk);
  geti("VY_CONV_SK_SLOTS", k.conv_sk_slots);
  getd("VY_CONV_SK_GAIN", k.conv_sk_gain);
  getd("VY_CONV_SK_COST", k.conv_sk_cost);
  geti("VY_CONV_KSPLIT", k.conv_ksplit);
  if (const char* s = getenv("VY_CONV_FORCE")) {  // the tiles conv_igemm instantiates only
    int bm = 0, bn = 0;
    if (sscanf(s, "%dx%d", &bm, &bn) == 2 &&
        ((bm == 128 && (bn == 32 || bn == 64 || bn == 128)) || (bm == 64 && bn == 64))) {
      k.conv_force_bm = bm;
      k.conv_force_bn = bn;
    }
  }
  geti("VY_SPLIT_ALWAYS", k.split_always);
  geti("VY_SPLIT_WINO", k.split_wino);
  geti("VY_SPLIT_TRAIN", k.split_train);
  geti("VY_SPLIT_WGRAD", k.split_wgrad);
  if (const char* s = getenv("VY_SPLIT_FORCE")) {  // "<BM>x<BN>", "<BM>x<BN>k<S>" or "k<S>"; the tiles conv_split instantiates only
    int bm = 0, bn = 0, ks = 0;
    const int n = sscanf(s, "%dx%dk%d", &bm, &bn, &ks);
    if (n >= 2 && ((bm == 128 && (bn == 64 || bn == 128)) || (bm == 256 && bn == 64))) {
      k.split_force_bm = bm;
      k.split_force_bn = bn;
      if (n == 3 && ks >= 1 && ks <= 64) k.split_force_ks = ks;
    } else if (sscanf(s, "k%d", &ks) == 1 && ks >= 1 && ks <= 64) {
      k.split_force_ks = ks;
    }
  }
  geti("VY_TRAIN_SIDE_STREAM", k.train_side_stream);
  if (const char* s = getenv("VY_TRAIN_LABELS")) k.train_labels = s;
  geti("VY_HIER_CHAIN", k.hier_chain);
  geti("VY_PLAN_GUARD", k.plan_guard);
  if (k.plan_guard < 0 || k.plan_guard % 256 || k.plan_guard > (1 << 20)) k.plan_guard = 0;
#ifdef VY_TRAIN_ABL_BUILD
  geti("VY_TRAIN_ABL", k.train_abl);
  geti("VY_TRAIN_ABL_AFTER", k.train_abl_after);
  if (k.train_abl)
    fprintf(stderr, "libvyolo (VY_TRAIN_ABL_BUILD): VY_TRAIN_ABL=%d — training launches are being SKIPPED, gradients are garbage\n",
            k.train_abl);
#endif
#ifdef VY_WINO_BM128
  if (const char* s = getenv("VY_WINO_BM"))
    if (atoi(s) == 128) k.wino_bm = 128;
#endif
  return k;
}
