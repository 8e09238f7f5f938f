// Host-side check of the conv launch decision (g++, CPU test suite): videoyolo_amd/csrc/conv_launch.h's vy_conv_plan — the
// function every launch goes through — on a ConvArgs per conv shape of BASELINE.json's workloads, as measured and adopted on
// the MI355X, and the structural properties of the cost models behind it (conv_cost_model.h).  A change of a constant
// that moves one of these decisions has to be re-measured, not slipped in.
// Output: one line per shape "M N K -> BMxBN[sk]   [| split ... | exact]   [| wino | -]   | <stages and schedule of the exact
// form: [s4][sk | ks<S> | ck<S>[sk]], or plain>"; exit code 1 on a violated property.
#include <cstdio>
#include <cstring>

#include "../videoyolo_amd/csrc/conv_launch.h"

int vy_cu_count() { return VY_MODEL_CUS; }  // (every ConvArgs below names its CUs)

// resident blocks per CU of the exact instances (128x128, 128x64, 128x32, 64x64, 64x64 with four stages), as the
// occupancy query answers on the MI355X
static const VyConvResidency kRes = {{2, 3, 3, 4, 2}, {2, 3, 3, 4, 2}};

struct Shape {
  int B, H;  // H x H output pixels per frame
  int N;
  double K;  // 3x3 taps where K is a multiple of 288, else 1x1
};

static float dummy[4];  // addresses only: nothing here runs a launch

// the conv + BN + leaky cell of shape s on a net's scratch; sk: with the stream-K scratch
static ConvArgs cell(const Shape& s, int cus, bool sk, const VyKnobs* knobs) {
  ConvArgs a;
  memset(&a, 0, sizeof a);
  a.in = a.w = a.scale = a.shift = dummy;
  a.out = dummy;
  a.B = s.B, a.LH = a.LW = s.H, a.M = s.B * s.H * s.H;
  a.ntaps = (long long)s.K % 288 == 0 ? 9 : 1;
  a.Kc = (int)(s.K / a.ntaps);
  for (int t = 0; t < a.ntaps; ++t) {
    a.tap_dy[t] = (signed char)(a.ntaps == 9 ? t / 3 - 1 : 0);
    a.tap_dx[t] = (signed char)(a.ntaps == 9 ? t % 3 - 1 : 0);
    a.tap_w[t] = (unsigned char)t;
  }
  a.w_taps = a.ntaps, a.w_cin = a.Kc, a.w_cout = a.N = s.N;
  a.a_s = a.o_s = a.ups = 1;
  a.leaky = 1;
  a.knobs = knobs;
  a.cus = cus;
  a.ck_scratch = dummy;
  a.ck_bytes = vy_conv_chunk_scratch_bytes(a.M, a.N, 4);
  if (sk) {
    a.sk_partials = dummy;
    a.sk_flags = reinterpret_cast<unsigned*>(dummy);
    a.sk_bytes = VY_SK_PARTIAL_BYTES;
    a.sk_nflags = VY_SK_FLAGS;
  }
  return a;
}
// ... with the split kernel's weight images and slab scratch for 64 k-slices (the models' own choice, whatever a net's
// scratch would hold), and the Winograd image sets
static ConvArgs with_images(ConvArgs a, bool wino) {
  a.w_split = dummy;
  a.splitk_slabs = dummy;
  a.splitk_bytes = 64ull * a.M * a.N * 4ull;
  if (wino) a.w_wino = dummy;
  return a;
}
// stages and schedule of an exact plan: the training label without kernel and tile
static const char* schedule(const VyConvPlan& p, char* buf, size_t n) {
  char t[64], tile[32];
  vy_conv_plan_label(p, VY_LABEL_TRAIN, t, sizeof t);
  const size_t skip = (size_t)snprintf(tile, sizeof tile, "exact %dx%d", p.bm, p.bn);
  snprintf(buf, n, "%s", strlen(t) > skip ? t + skip : "plain");
  return buf;
}

int main() {
  const VySkPolicy on = {true, 0.03, 7.5}, off = {false, 0.03, 7.5};
  const VyKnobs knobs;
  // 608x608 batch 64 (configs[1]), 416x416 batch 16 forward (configs[2]), 608x608 batch 1
  const Shape shapes[] = {
      {64, 304, 64, 288},  {64, 304, 32, 64},   {64, 152, 128, 576}, {64, 152, 64, 128}, {64, 76, 256, 1152}, {64, 76, 128, 256},
      {64, 38, 512, 2304}, {64, 38, 256, 512},  {64, 19, 1024, 4608}, {64, 19, 512, 1024}, {64, 19, 75, 1024}, {16, 52, 256, 1152},
      {16, 26, 512, 2304}, {16, 13, 1024, 4608}, {16, 13, 512, 1024}, {16, 52, 128, 256},  {1, 76, 256, 1152}, {1, 19, 1024, 4608},
  };
  char sched[32];
  for (const Shape& s : shapes) {
    const ConvArgs a = cell(s, 256, true, &knobs);
    const long long M = a.M;
    const VyConvPlan p = vy_conv_plan(a, kRes);
    if (p.kernel != VY_KERNEL_EXACT) return fprintf(stderr, "a launch without weight images must go to the exact kernel\n"), 1;
    const int bm = p.bm, bn = p.bn;
    const bool sk = p.sk;
    int bm0 = 0, bn0 = 0, bmm = 0, bnm = 0;
    bool sk0 = true, skm = false;
    const double t = vy_select_tile(M, s.N, s.K, on, &bmm, &bnm, &skm);
    const double t0 = vy_select_tile(M, s.N, s.K, off, &bm0, &bn0, &sk0);
    if (bmm != bm || bnm != bn || skm != sk) return fprintf(stderr, "the plan's tile / stream-K is not the tile model's\n"), 1;
    printf("%lld %d %.0f -> %dx%d%s", M, s.N, s.K, bm, bn, sk ? "sk" : "");
    // conv mode VY_CONV_SPLIT_BF16X3: which kernel the launch goes to with the split kernel's images, and that kernel's
    // tile / k-split
    if (s.N % 64 == 0) {
      const VyConvPlan ps = vy_conv_plan(with_images(a, false), kRes);
      int b1, b2, k1, sbm = 0, sbn = 0, sks = 0;
      const double ts = vy_predict_split(M, s.N, s.K, 64, &sbm, &sbn, &sks);
      if (ps.kernel == VY_KERNEL_SPLIT) printf("   | split %dx%d%s%.0d", ps.bm, ps.bn, ps.split_ks > 1 ? " k" : "", ps.split_ks > 1 ? ps.split_ks : 0);
      else if (ps.kernel == VY_KERNEL_EXACT) printf("   | exact");
      else return fprintf(stderr, "split images: neither split nor exact\n"), 1;
      if (ps.kernel == VY_KERNEL_SPLIT && (ps.bm != sbm || ps.bn != sbn || ps.split_ks != sks))
        return fprintf(stderr, "the plan's split tile / k-split is not the split model's\n"), 1;
      if (sks < 1 || (sks > 1 && (s.K / 16) / sks < 6)) return fprintf(stderr, "k-split with slices shorter than 6 k-steps\n"), 1;
      if (vy_predict_split(M, s.N, s.K, 1, &b1, &b2, &k1) < ts - 1e-9 || k1 != 1)
        return fprintf(stderr, "allowing k-split made the split prediction worse\n"), 1;
    }
    // ... and whether its 3x3 stride-1 cell goes to the Winograd F(2, 3) instance instead, given those images too
    if (s.N % 128 == 0 && (long long)s.K % 288 == 0) {
      const VyConvPlan pw = vy_conv_plan(with_images(a, true), kRes);
      if (pw.kernel == VY_KERNEL_NONE) return fprintf(stderr, "Winograd images: refused\n"), 1;
      printf(pw.kernel == VY_KERNEL_WINO ? "   | wino" : "   | -");
    }
    printf("   | %s\n", schedule(p, sched, sizeof sched));
    if (sk0) return fprintf(stderr, "stream-K chosen although not allowed\n"), 1;
    if (t > t0 * (1.0 + 1e-12)) return fprintf(stderr, "allowing stream-K made the prediction worse\n"), 1;
    if (s.N <= 32 && !(bm == 128 && bn == 32 && !sk)) return fprintf(stderr, "N <= 32 must use the 128x32 tile\n"), 1;
    if (s.N > 32 && !vy_tile_model(bm, bn)) return fprintf(stderr, "tile without a model\n"), 1;
    if (sk) {  // a stream-K launch has more tiles than blocks, and its predicted saving clears the threshold
      const VyTileModel* m = vy_tile_model(bm, bn);
      const long long tiles = ((M + bm - 1) / bm) * ((s.N + bn - 1) / bn);
      const long long per_cu = tiles / 256 < m->resident ? tiles / 256 : m->resident;
      bool dummy;
      const double plain = vy_predict_launch(M, s.N, s.K, *m, off, &dummy);
      if (per_cu < 1 || tiles <= 256 * per_cu) return fprintf(stderr, "stream-K launch without a cut tile\n"), 1;
      if (plain - t < 0.03 * plain - 1e-9) return fprintf(stderr, "stream-K below its threshold\n"), 1;
      if (p.grid != 256 * per_cu) return fprintf(stderr, "stream-K launch not on the blocks the chip holds\n"), 1;
    }
  }
  // ---- another chip: the models count their rounds in the device's CU count, and every choice
  // BETWEEN kernels is refused where the constants were not fitted.  128 CUs = the MI355X in DPX mode.
  if (!vy_model_fitted(256) || vy_model_fitted(128) || vy_model_fitted(64) || vy_model_fitted(304))
    return fprintf(stderr, "vy_model_fitted must hold for 256 CUs only\n"), 1;
  printf("-- 128 CUs\n");
  for (const Shape& s : shapes) {
    const ConvArgs a = cell(s, 128, false, &knobs);
    const long long M = a.M;
    const VyConvPlan p = vy_conv_plan(a, kRes), pi = vy_conv_plan(with_images(a, true), kRes);
    const int bm = p.bm, bn = p.bn;
    int b2 = 0, n2 = 0, bmm = 0, bnm = 0;
    bool sk = false, sk2 = false;
    const double t128 = vy_select_tile(M, s.N, s.K, off, &bmm, &bnm, &sk, 128);
    const double t256 = vy_select_tile(M, s.N, s.K, off, &b2, &n2, &sk2, 256);
    if (bmm != bm || bnm != bn || p.sk) return fprintf(stderr, "the plan's tile is not the tile model's\n"), 1;
    if (pi.kernel != VY_KERNEL_EXACT || pi.bm != bm || pi.bn != bn) return fprintf(stderr, "a choice between kernels on an unfitted chip\n"), 1;
    printf("%lld %d %.0f -> %dx%d   | %s\n", M, s.N, s.K, bm, bn, schedule(p, sched, sizeof sched));
    if (s.N > 32 && t128 < t256 * (1.0 - 1e-12)) return fprintf(stderr, "half the CUs predicted faster\n"), 1;
    // a launch that fills 256 CUs for many rounds takes twice as long on 128
    const long long tiles = ((M + bm - 1) / bm) * ((s.N + bn - 1) / bn);
    if (s.N > 32 && tiles >= 64 * 256 && bm == b2 && bn == n2 && (t128 < 1.9 * t256 || t128 > 2.1 * t256))
      return fprintf(stderr, "a long launch must scale with the CU count (%.1f vs %.1f)\n", t128, t256), 1;
    if (s.N % 64 == 0) {
      int sbm, sbn, sks;
      const double a = vy_predict_split(M, s.N, s.K, 64, &sbm, &sbn, &sks, 128), b = vy_predict_split(M, s.N, s.K, 64, &sbm, &sbn, &sks, 256);
      if (a < b * (1.0 - 1e-12)) return fprintf(stderr, "split model: half the CUs predicted faster\n"), 1;
    }
    if (s.N % 128 == 0 && (long long)s.K % 288 == 0 &&
        vy_predict_wino(M / 2, s.N, (int)(s.K / 9), 128) < vy_predict_wino(M / 2, s.N, (int)(s.K / 9), 256) * (1.0 - 1e-12))
      return fprintf(stderr, "Winograd model: half the CUs predicted faster\n"), 1;
  }
  return 0;
}
