// train.hip — host side of the training step: plans the extra planes (raw conv outputs z / their
// gradients dz, gradient planes g), builds the forward-train and backward launch sequences from the
// same conv list the inference path uses, and implements the training C-ABI of include/vyolo.h.
//
// Forward (recording), per `_conv2d` cell (layers.py:63-70 under autograd.record()):
//   conv (raw, + per-tile channel sums) -> reduce partials -> [SyncBN all-reduce] -> finalize
//   (mean/var -> scale/shift, running stats) -> apply (BN affine + leaky [+ residual] [x2 replicate])
// then the prediction convs, then the fused target-merge + loss + d(loss)/d(pred) kernel.
// Backward, cells in reverse order:
//   BN/leaky backward reduce -> [all-reduce] -> finalize (dgamma, dbeta, coefficients) -> apply (dz
//   overwrites z) -> wgrad (split-K slabs + ordered reduce) -> dgrad into the input's gradient plane
//   (overwrite, or accumulate when the plane already holds another consumer's contribution, plus
//   the skip connection's gradient as an addend).
// plan_train computes one TrainPlan (regions, a TrainCell per conv, tables); the passes are sequences of per-cell steps that
// read it; the six step entries share the run_entry frame of the inference entries.
#include <cstdlib>

#include "net_internal.h"

namespace {

// One conv at the planned shape.  Its geometry is derived in plan_train and nowhere else: the pixel tables, both passes, the
// taps and vy_net_train_conv_plan read it (training sizes are multiples of 32: it agrees with the planes' ceil(input / div))
struct TrainCell {
  int B = 0, Ho = 0, Wo = 0;  // frames the conv runs on (a window net's backbone: b * k) and its output size
  long long M = 0;            // B * Ho * Wo output pixels
  int z_cs = 0;               // BatchNorm cells: channel stride of the raw-output plane z (0: none) ...
  size_t z_off = 0;           // ... its float offset in the z region
  size_t save_off = 0;        // ... and the float offset of the saved [mean | invstd] rows in the save region
  int splits = 1, k_per_split = 32;  // weight-gradient split-K
  size_t tab_off = 0;         // byte offset of its weight-gradient pixel table in the workspace
  // conv mode VY_CONV_SPLIT_BF16X3_TRAIN: byte offset of its weights' DATA-GRADIENT tile images ([k = cout][n = cin]
  // operand; conv_split.hip) in the region at TrainPlan::dsplit_off, -1: none.  The forward images are the NetPlan's.
  long long dsplit = -1;
  // the split-fp32 routing, decided once from (conv mode, VY_SPLIT_TRAIN): does the forward launch of this cell carry its
  // split images, does its data gradient (the cost model has the last word)
  bool fwd_split = false, dgrad_split = false;
  int bucket = 0;             // gradient bucket: 0 heads, 1 stages.2, 2 stages.1, 3 stages.0
};

// One conv join of a hierarchical net at the planned shape (vy_net::HierPool with VY_HJOIN_CONV): the geometry of its pooled
// plane, and its z plane, saved statistics and partial rows — regions like a cell's
struct TrainJoin {
  int B = 0, H = 0, W = 0;  // pooled frames (b * fm) and their size
  long long M = 0;          // B * H * W pooled positions: the BatchNorm's count
  size_t z_off = 0;         // float offset of its z plane (B, H + 2, W + 2, C) in the z region
  size_t save_off = 0;      // float offset of its saved [mean | invstd] rows in the save region
  int blocks = 0;           // blocks = partial rows of its training launches (vy_hier_join_blocks)
};

struct TrainPlan {
  int B = 0, H = 0, W = 0;
  // vy_net::commits when vy_net_bind_train committed the inference plan these regions lie behind — 0: none; any later
  // commit (vy_net_bind_workspace, vy_net_bind_video) lays the workspace out anew and voids this plan (bound_train)
  unsigned behind = 0;
  // regions: byte offsets in the workspace, behind the inference plan
  size_t dsplit_off = 0, g_off = 0, z_off = 0, save_off = 0, coef_off = 0, sums_off = 0, slice_off = 0, part_off = 0;
  size_t slab_off = 0, loss_part_off = 0, loss_off = 0, zero_off = 0, sdesc_off = 0, seg_off = 0, chunk_off = 0, total = 0;
  std::vector<TrainCell> cells;  // per conv
  std::vector<TrainJoin> joins;  // per conv join of a hierarchical net (none otherwise)
  // all image sets (forward + data gradient) for the one-launch rebuild
  std::vector<SplitDesc> sdesc;
  long long sdesc_total = 0;
  std::vector<SgdSeg> segs;
  std::vector<int32_t> chunk_seg;
  // gradient buckets (contiguous parameter ranges, by TrainCell::bucket): first element, length (0: no such bucket)
  int64_t bucket_lo[4] = {0, 0, 0, 0}, bucket_len[4] = {0, 0, 0, 0};
  // the conv joins' parameters lie behind the heads': a second range of the stages.0 bucket (0: no conv join)
  int64_t join_lo = 0, join_len = 0;
};

struct BwdDgrad {
  ConvArgs a[4];
  int n = 0;
};

}  // namespace

// what outlives a plan: buffers, options, callbacks, the side stream — and the committed plan with its upload flags
struct VyTrain {
  TrainPlan plan;
  bool sdesc_uploaded = false, tabs_built = false, seg_uploaded = false;
  float* grads = nullptr;
  float* mom = nullptr;
  float ignore_iou = 0.7f;
  int label_smooth = 0;
  std::vector<float> lr_mult, wd_mult;
  std::vector<int> enabled;
  // SyncBN
  int world = 1;
  vy_allreduce_cb ar_cb = nullptr;
  void* ar_user = nullptr;
  vy_grad_bucket_cb gb_cb = nullptr;
  void* gb_user = nullptr;
  bool forward_done = false;
  int M = 0;
  // weight gradients run on a side stream, concurrently with the dgrad / BatchNorm chain
  hipStream_t side = nullptr;
  hipEvent_t ev_main = nullptr, ev_side = nullptr;
  ~VyTrain() {
    if (ev_main) (void)hipEventDestroy(ev_main);
    if (ev_side) (void)hipEventDestroy(ev_side);
    if (side) (void)hipStreamDestroy(side);
  }
};

void vy_train_free(vy_net* net) {
  delete net->train;
  net->train = nullptr;
}

namespace {

// Profiling aid (tools/train_layers.py): with VY_TRAIN_LABELS=<path> the first training step appends one line per
// matrix-core launch — kind (fwd / wgrad / dgrad), cell name, FLOPs, GEMM dims — so that a rocprofv3 kernel trace
// can be joined with the layers by launch order within each kernel class.  Once per path: the first step of the first
// net that names a path fills it (`done`); a later net that names another path (the GPU tests: one file per case) gets
// its own first step.
struct LabelLog {
  FILE* f = nullptr;
  std::string path, done;  // the file being written; the last one finished
  void note(const vy_net* net, const char* kind, const std::string& name, double M, double N, double K) {
    const std::string& want = net->knobs.train_labels;
    if (want.empty() || want == done) return;
    if (!f && (f = fopen(want.c_str(), "w"))) path = want;
    if (f) fprintf(f, "%s %s %.0f %.0f %.0f %.0f\n", kind, name.c_str(), 2.0 * M * N * K, M, N, K);
  }
  // which kernel the preceding line went to, and in which form (tests assert that the launches they mean to cover really
  // ran; tools/train_layers.py skips '#' lines):
  //   "# via split 128x128 k2"          fwd / dgrad on the split-fp32 kernel
  //   "# via exact 128x64sk"            fwd / dgrad on the exact kernel: tile, stages and schedule (vy_conv_plan_label)
  //   "# via wgrad_kernel<32,64> splits 14 reduce wide<8> stream side"   wgrad: the kernel instance, its slabs, their
  //                                     reduce (plain / wide<8> / wide<32>) and the stream both went to (side / main)
  void via(const char* text) {
    if (f) fprintf(f, "# via %s\n", text);
  }
  void via_wgrad(const char* kernel, int splits, bool side) {
    if (!f) return;
    const int g = vy_slab_reduce_groups(splits);
    char t[112];
    snprintf(t, sizeof t, "%s splits %d reduce %s stream %s", kernel, splits, g == 32 ? "wide<32>" : g == 8 ? "wide<8>" : "plain",
             side ? "side" : "main");
    via(t);
  }
  void close_step() {
    if (!f) return;
    fclose(f);
    f = nullptr;
    done = path;
  }
};
LabelLog g_labels;

// Measurement aid (tools/ab_bn_bounds.sh): VY_TRAIN_ABL skips BatchNorm launches of the training step to BOUND what
// fusing them into the neighbouring conv launches could return — bit 1: bn_bwd_reduce (+ its finalize), 2: the forward
// bn_apply, 4: bn_bwd_apply; and, to see which stream of the backward pass holds the step, 8: no weight-gradient
// kernels, 16: no data-gradient kernels, 32: no weight-gradient kernels for the early cells (N <= 128, K <= 576); 64 / 128: the
// finalize launch between the backward / forward statistics reduce and its apply pass (tools/ab_bn_finalize.sh).  The step then
// computes garbage; nothing else reads this.
// Compiled in ONLY with -DVY_TRAIN_ABL_BUILD (the A/B scripts build their own library): the shipped library never reads
// the variable, so a leftover VY_TRAIN_ABL in somebody's environment cannot silently turn a training run into garbage.
#ifdef VY_TRAIN_ABL_BUILD
// bits 64 / 128 (a finalize launch skipped: its outputs keep the previous step's values) only after VY_TRAIN_ABL_AFTER recorded
// forwards (default 3), so that the planes never hold the all-zero data of a net whose statistics were never finalized
static int g_abl_forwards = 0;
static int train_abl(const vy_net* net) {
  const int v = net->knobs.train_abl;
  return g_abl_forwards > net->knobs.train_abl_after ? v : (v & ~(64 | 128));
}
#else
static constexpr int train_abl(const vy_net*) { return 0; }
#endif

constexpr int kBwdChunk = 64;  // pixels per partial-sum block of the bias-gradient reductions (and the scratch bound)

// the per-parameter options a net starts with
void default_options(const vy_net& net, VyTrain* t) {
  t->lr_mult.assign(net.params.size(), 1.0f);
  t->wd_mult.assign(net.params.size(), 1.0f);
  t->enabled.resize(net.params.size());
  for (size_t i = 0; i < net.params.size(); ++i) t->enabled[i] = net.params[i].info.trainable;
}

VyTrain* get_train(vy_net* net) {
  if (!net->train) default_options(*net, net->train = new VyTrain());
  return net->train;
}

// Split-K of a weight gradient over its M pixels.  A block runs k_per_split / 32 k-steps (+ ~3 k-steps worth of prologue
// and slab store); the chip holds `held` blocks at a time (2 per CU: 512 on the MI355X), so the launch costs about
// ceil(tiles * splits / held) * (k_per_split / 32 + 3).  Round 1 took the smallest split count with >= 1024
// blocks, which for the three big 3x3 groups lands just past a multiple of 512 (18 x 57 = 1026,
// 72 x 15 = 1080, 288 x 4 = 1152 blocks): a last round of a few blocks with the chip idle around them.  Now the
// cheapest (splits, k_per_split) under that model is taken; a split is >= 256 pixels.
void wgrad_split_k(long long M, long long tiles, long long held, int* splits, int* k_per_split) {
  const long long whole = ((M + 31) / 32) * 32;
  long long best_k = whole, best_sp = 1;
  double best_cost = 1e300;
  for (long long k = 256; k <= whole && M >= 256; k += 32) {
    const long long sp_k = (M + k - 1) / k;
    const long long rounds = (tiles * sp_k + held - 1) / held;
    const double cost = (double)rounds * ((double)k / 32.0 + 3.0);
    if (cost < best_cost) {
      best_cost = cost;
      best_k = k;
      best_sp = sp_k;
    }
  }
  *splits = (int)best_sp;
  *k_per_split = (int)best_k;
}

// The training regions behind the inference plan `fwd` (of the same shape, every plane kept: backward reads them all), and
// everything the step derives from the shape.  Reads the per-parameter options of `opt`; writes nothing.
// regions (tests: vy_net_plan_region): every carve is appended to it, in offset order
TrainPlan plan_train(const vy_net& net, const VyTrain& opt, const NetPlan& fwd, int b, int h, int w,
                     std::vector<PlanRegion>* regions = nullptr) {
  TrainPlan p;
  p.B = b;
  p.H = h;
  p.W = w;
  // carves 256-byte aligned regions off the workspace, in call order, each followed by the guard gap of the inference plan
  // (VY_PLAN_GUARD; 0 outside the tests); no bytes, no carve
  struct {
    size_t off, guard;
    std::vector<PlanRegion>* regions;
    size_t take(size_t bytes, const char* kind, const std::string& what = std::string()) {
      if (!bytes) return off;
      if (regions) regions->push_back({what.empty() ? std::string(kind) : kind + (":" + what), off, bytes});
      return std::exchange(off, off + vy_net::al(bytes) + guard);
    }
  } ws{vy_net::al(fwd.total), (size_t)fwd.guard, regions};
  const size_t gap_fl = ws.guard / sizeof(float);  // the gap behind a gradient or z plane, in floats
  const size_t n = net.convs.size();
  p.cells.resize(n);
  // split-fp32 training mode: the data gradients whose N (= cin) the split kernel has a tile for get their own weight
  // images — whenever VY_SPLIT_TRAIN != 0, the forward-only mode 2 included, which does not launch with them
  const int st = net.knobs.split_train;  // 0 none, 1 both, 2 forward only, 3 dgrad only
  const bool images = net.conv_mode == VY_CONV_SPLIT_BF16X3_TRAIN && st != 0;
  p.dsplit_off = ws.off;
  for (size_t i = 0; i < n; ++i) {
    const ConvT& c = net.convs[i];
    TrainCell& cell = p.cells[i];
    const int div_in = c.is_stem ? 1 : net.planes[c.in_plane].div;
    cell.B = b * net.planes[c.out_plane].fm;
    cell.Ho = h / div_in / c.stride;
    cell.Wo = w / div_in / c.stride;
    cell.M = (long long)cell.B * cell.Ho * cell.Wo;
    cell.bucket = c.name.rfind("stages.2", 0) == 0 ? 1 : c.name.rfind("stages.1", 0) == 0 ? 2 : c.name.rfind("stages.0", 0) == 0 ? 3 : 0;
    cell.fwd_split = images && st != 3 && net.split_eligible(c);
    if (images && !c.is_stem && c.cin % 64 == 0) {
      cell.dsplit = (long long)(ws.take(vy_split_weight_dgrad_bytes(c.cout, c.k * c.k, c.cin), "dgrad_image", c.name) - p.dsplit_off);
      cell.dgrad_split = st != 2;
    }
  }
  // gradient planes mirror the activation planes (of a plan that keeps them all: fwd.planes[i].off, gaps included)
  p.g_off = ws.off;
  for (size_t i = 0; i < net.planes.size(); ++i) {
    const PlaneT& pl = net.planes[i];
    ws.take((size_t)b * pl.fm * (h / pl.div + 2) * (w / pl.div + 2) * pl.C * sizeof(float), "grad", regions ? net.plane_name((int)i) : std::string());
  }
  // z planes and saved statistics: one per BN conv; the partial-sum and slab scratch: the largest any conv needs
  size_t zfl = 0, sfl = 0, part = 0, slab = 0;
  std::vector<size_t> z_used(n, 0);  // bytes of each z plane
  for (size_t i = 0; i < n; ++i) {
    const ConvT& c = net.convs[i];
    TrainCell& cell = p.cells[i];
    const long long M = cell.M;
    const size_t chunks = (size_t)((M + kBwdChunk - 1) / kBwdChunk);
    if (c.p_gamma >= 0) {
      cell.z_cs = c.cout;
      cell.z_off = zfl;
      z_used[i] = (size_t)cell.B * (cell.Ho + 2) * (cell.Wo + 2) * c.cout * sizeof(float);
      zfl += vy_net::al(z_used[i]) / sizeof(float) + gap_fl;
      cell.save_off = sfl;
      sfl += 2 * (size_t)((c.cout + 63) & ~63);
      // partials: forward stats, backward sums
      const size_t tiles_m = (size_t)((M + 31) / 32);  // per-tile statistics rows, sized for 32-row tiles (every tile has more)
      size_t pf = 2 * (c.is_stem ? (size_t)vy_stem_blocks(cell.B, h, w) * 64 : tiles_m * 2 * c.cout);  // doubles
      pf = std::max(pf, chunks * 2 * c.cout);
      // bn_bwd_reduce chunks by image rows, not by 64 pixels: ceil(B*Ho / rows_per_chunk) partial rows of 2*C
      // floats — more than the pixel-chunk bound on maps narrower than 64 pixels (W = 32 training shapes)
      const int rpc = vy_bn_bwd_rows_per_chunk(cell.B, cell.Ho, c.cout);
      pf = std::max(pf, (size_t)(((long long)cell.B * cell.Ho + rpc - 1) / rpc) * 2 * c.cout);
      if (c.is_stem) pf = std::max(pf, (size_t)vy_stem_wgrad_blocks(cell.B, h, w) * 864);
      part = std::max(part, pf);
    } else {
      part = std::max(part, chunks * c.cout);
    }
    if (!c.is_stem) {
      const int Ntot = c.k * c.k * c.cin;
      const int rows = vy_wgrad_tile_rows(c.cout, c.k, c.cin);
      const int tiles = ((c.cout + rows - 1) / rows) * ((Ntot + 127) / 128);
      wgrad_split_k(M, tiles, 2ll * net.resolve_cus(), &cell.splits, &cell.k_per_split);
      slab = std::max(slab, (size_t)cell.splits * c.cout * Ntot);
    }
  }
  // the conv joins of a hierarchical net, behind the cells: z of the pooled plane's geometry (border included), saved
  // statistics, and the partial rows of their three passes — statistics [blocks][2][C] and weight gradient [blocks][C][3] in
  // double, bn_bwd_reduce's [chunks][2][C] floats
  std::vector<size_t> jz_used;
  for (const vy_net::HierPool& hp : net.hpools) {
    if (hp.join != VY_HJOIN_CONV) continue;
    const PlaneT& dp = net.planes[hp.dst];
    TrainJoin j;
    j.B = b * dp.fm;
    j.H = h / dp.div;
    j.W = w / dp.div;
    j.M = (long long)j.B * j.H * j.W;
    j.blocks = (int)vy_hier_join_blocks(j.B, j.H, j.W, hp.C);
    j.z_off = zfl;
    jz_used.push_back((size_t)j.B * (j.H + 2) * (j.W + 2) * hp.C * sizeof(float));
    zfl += vy_net::al(jz_used.back()) / sizeof(float) + gap_fl;
    j.save_off = sfl;
    sfl += 2 * (size_t)((hp.C + 63) & ~63);
    const int rpc = vy_bn_bwd_rows_per_chunk(j.B, j.H, hp.C);
    part = std::max(part, 2 * (size_t)j.blocks * 3 * hp.C);  // (doubles: 3 columns per channel cover the forward's 2)
    part = std::max(part, (size_t)(((long long)j.B * j.H + rpc - 1) / rpc) * 2 * hp.C);
    p.joins.push_back(j);
  }
  p.z_off = ws.off;
  for (size_t i = 0; i < n; ++i) ws.take(z_used[i], "z", net.convs[i].name);  // (cell.z_off: the same walk, above)
  for (size_t i = 0; i < jz_used.size(); ++i) ws.take(jz_used[i], "z", net.join_name((int)i));
  p.save_off = ws.take(sfl * sizeof(float), "train.save");
  p.coef_off = ws.take(3 * 1024 * sizeof(float), "train.coef");
  p.sums_off = ws.take(2 * 2 * 1024 * sizeof(double), "train.sums");  // [global | local] x [2][C]
  p.slice_off = ws.take((size_t)VY_REDUCE_SLICES * 2 * 1024 * sizeof(double), "train.slices");  // slice sums of long per-tile statistics lists
  p.part_off = ws.take(part * sizeof(float), "train.part");
  p.slab_off = ws.take(slab * sizeof(float), "train.slab");
  int N = 0;
  for (int i = 0; i < 3; ++i) {
    const int dv = net.planes[net.head_plane[i]].div;
    N += 3 * (h / dv) * (w / dv);
  }
  p.loss_part_off = ws.take((size_t)vy_loss_blocks_per_image(N) * b * 4 * sizeof(float), "train.loss_part");
  p.loss_off = ws.take((size_t)4 * b * sizeof(float), "train.loss");
  p.zero_off = ws.take(1024, "train.zero");
  // SGD segment tables
  for (size_t i = 0; i < net.params.size(); ++i) {
    const vy_param_info& pi = net.params[i].info;
    if (!pi.trainable) continue;
    const int32_t si = (int32_t)p.segs.size();
    p.segs.push_back(SgdSeg{pi.offset, pi.size, opt.lr_mult[i], opt.wd_mult[i], opt.enabled[i] ? 1 : 0, 0});
    const int nch = (int)((pi.size + VY_SGD_CHUNK - 1) / VY_SGD_CHUNK);
    for (int c = 0; c < nch; ++c) {
      p.chunk_seg.push_back(si);
      p.chunk_seg.push_back(c);
    }
  }
  // weight-gradient pixel tables (wgrad.hip): 8 bytes per output pixel of every conv but the stem
  for (size_t i = 0; i < n; ++i)
    if (!net.convs[i].is_stem) p.cells[i].tab_off = ws.take(vy_wgrad_table_entries(p.cells[i].M) * 8, "wgrad_table", net.convs[i].name);
  p.sdesc_off = ws.take(sizeof(SplitDesc) * 2 * n, "train.sdesc");
  p.seg_off = ws.take(p.segs.size() * sizeof(SgdSeg), "train.seg");
  p.chunk_off = ws.take(p.chunk_seg.size() * sizeof(int32_t), "train.chunk");
  p.total = ws.off;
  // the image sets and the gradient buckets' parameter ranges
  int64_t lo[4] = {INT64_MAX, INT64_MAX, INT64_MAX, INT64_MAX}, hi[4] = {0, 0, 0, 0};
  for (size_t i = 0; i < n; ++i) {
    const ConvT& c = net.convs[i];
    const TrainCell& cell = p.cells[i];
    const long long w_off = net.params[c.p_weight].info.offset;
    if (fwd.convs[i].split_off >= 0) {
      p.sdesc.push_back(SplitDesc{p.sdesc_total, w_off, (long long)(fwd.wsplit_off + fwd.convs[i].split_off), c.cout, c.k * c.k, c.cin, 0});
      p.sdesc_total += (long long)c.cout * c.k * c.k * c.cin / 8;
    }
    if (cell.dsplit >= 0) {
      p.sdesc.push_back(SplitDesc{p.sdesc_total, w_off, (long long)(p.dsplit_off + cell.dsplit), c.cout, c.k * c.k, c.cin, 1});
      p.sdesc_total += (long long)((c.cout + 31) & ~31) * c.k * c.k * c.cin / 8;
    }
    for (int pidx : {c.p_weight, c.p_gamma, c.p_beta, c.p_bias}) {
      if (pidx < 0) continue;
      const vy_param_info& pi = net.params[pidx].info;
      lo[cell.bucket] = std::min(lo[cell.bucket], pi.offset);
      hi[cell.bucket] = std::max(hi[cell.bucket], pi.offset + ((pi.size + 63) & ~(int64_t)63));
    }
  }
  if (!p.joins.empty()) {  // (appended in order: the first join's weight ... the last join's running_var)
    const vy_param_info &first = net.params[net.hpools.front().p_weight].info, &last = net.params[net.hpools.back().p_var].info;
    p.join_lo = first.offset;
    p.join_len = last.offset + ((last.size + 63) & ~(int64_t)63) - first.offset;
  }
  for (int k = 0; k < 4; ++k)
    if (hi[k] > lo[k]) {
      p.bucket_lo[k] = lo[k];
      p.bucket_len[k] = hi[k] - lo[k];
    }
  return p;
}

// BatchNorm state of one cell: parameters, folded affine, the statistics saved for backward
struct BnViews {
  float *gamma, *beta, *running_mean, *running_var, *scale, *shift, *save_mean, *save_invstd;
};

struct TrainCtx {
  vy_net* net;
  VyTrain* t;
  const TrainPlan& p;
  hipStream_t s;
  TrainCtx(vy_net* n, void* stream) : net(n), t(n->train), p(n->train->plan), s(static_cast<hipStream_t>(stream)) {}
  template <typename T>
  T* at(size_t off) const { return reinterpret_cast<T*>(net->dev_ws + off); }
  const TrainCell& cell(int ci) const { return p.cells[ci]; }
  float* gplanes() const { return at<float>(p.g_off); }
  float* gplane(int i) const { return gplanes() + net->cur.planes[i].off; }
  float* zplane(int ci) const { return at<float>(p.z_off) + p.cells[ci].z_off; }
  float* coef() const { return at<float>(p.coef_off); }
  double* sums_global() const { return at<double>(p.sums_off); }
  double* sums_local() const { return sums_global() + 2 * 1024; }
  double* slice_sums() const { return at<double>(p.slice_off); }
  float* partials() const { return at<float>(p.part_off); }
  float* slabs() const { return at<float>(p.slab_off); }
  float* param(int pidx) const { return net->dev_params + net->params[pidx].info.offset; }
  float* grad_of(int pidx) const { return t->grads + net->params[pidx].info.offset; }
  // conv join i: its plan record, z plane and BatchNorm state
  const TrainJoin& join(int i) const { return p.joins[i]; }
  float* join_z(int i) const { return at<float>(p.z_off) + p.joins[i].z_off; }
  BnViews join_bn(int i) const {
    const vy_net::HierPool& hp = net->hpools[i];
    float* save = at<float>(p.save_off) + p.joins[i].save_off;
    return {param(hp.p_gamma), param(hp.p_beta), param(hp.p_mean), param(hp.p_var), net->dev_params + hp.scale_off,
            net->dev_params + hp.shift_off, save, save + ((hp.C + 63) & ~63)};
  }
  BnViews bn_views(int ci) const {
    const ConvT& cv = net->convs[ci];
    float* save = at<float>(p.save_off) + p.cells[ci].save_off;
    return {param(cv.p_gamma), param(cv.p_beta), param(cv.p_mean), param(cv.p_var), net->dev_params + cv.scale_off,
            net->dev_params + cv.shift_off, save, save + ((cv.cout + 63) & ~63)};
  }
};

NoHook plain;  // the shared vy_net steps of the forward run without a hook

// SyncBatchNorm statistics are exchanged when there is more than one rank — or when a callback was installed for ONE rank
// (videoyolo_amd.parallel with VY_FORCE_COLLECTIVES=1: the all-reduce over one rank is the identity; it exists so that the
// whole exchange path, RCCL included, can be executed on a one-GPU box)
static bool sync_exchange(const VyTrain* t) { return t->world > 1 || (t->world == 1 && t->ar_cb != nullptr); }

// The statistics hand-off of a BatchNorm cell, forward and backward alike: from the partial rows a pass left to the sums the
// normalisation uses.  Ranks exchange statistics only for the SyncBatchNorm layers: `reduce_to_local` launches the ordered
// reduce of the partial rows into sums_local(), the all-reduce gives *use = the global sums and *count samples over all
// ranks, and the caller finalizes from them.  Everywhere else *use stays null: the ordered reduce of the partial rows and
// the finalize are ONE launch, the caller's.
template <typename Reduce>
int combine_sums(const TrainCtx& c, const ConvT& cv, int n_cols, Reduce&& reduce_to_local, double* count, const double** use) {
  *use = nullptr;
  if (!(sync_exchange(c.t) && is_sync_layer(cv))) return 0;
  HIP_TRY(reduce_to_local());
  if (!c.t->ar_cb) return fail(VY_ERR_STATE, "SyncBN world > 1 without an all-reduce callback");
  HIP_TRY(hipMemcpyAsync(c.sums_global(), c.sums_local(), sizeof(double) * n_cols, hipMemcpyDeviceToDevice, c.s));
  if (int rc = c.t->ar_cb(c.t->ar_user, c.sums_global(), n_cols)) return fail(VY_ERR_STATE, "all-reduce callback failed (%d)", rc);
  *count *= c.t->world;
  *use = c.sums_global();
  return 0;
}

// conv mode VY_CONV_SPLIT_BF16X3 in training: both sets of weight images follow the parameters (rebuilt after every
// optimizer step: 0.6 GB of traffic, ~0.3 ms, beside a 26 ms step)
int refresh_split_images(const TrainCtx& c) {
  vy_net* net = c.net;
  if (net->conv_mode != VY_CONV_SPLIT_BF16X3_TRAIN || !(net->split_dirty || net->dsplit_dirty) || c.p.sdesc.empty()) return 0;
  SplitDesc* d = c.at<SplitDesc>(c.p.sdesc_off);
  if (!c.t->sdesc_uploaded) {
    HIP_TRY(hipMemcpyAsync(d, c.p.sdesc.data(), sizeof(SplitDesc) * c.p.sdesc.size(), hipMemcpyHostToDevice, c.s));
    HIP_TRY(hipStreamSynchronize(c.s));  // pageable host vector; once per plan
    c.t->sdesc_uploaded = true;
  }
  // one launch for every image set of the net (per-conv launches: 140 kernel boundaries per step)
  HIP_TRY(vy_launch_split_weights_batch(net->dev_params, net->dev_ws, d, (int)c.p.sdesc.size(), c.p.sdesc_total, c.s));
  net->split_dirty = net->dsplit_dirty = false;
  return 0;
}

// the conv launch of the training passes, by its plan (conv_launch.h): the split-fp32 kernel where the launch has its weight
// images (a.w_split: see TrainCell::fwd_split / dgrad_split) and the cost model predicts a gain; the exact kernel otherwise.
// Never the Winograd kernel: it serves the conv + BN + leaky cell only, and no training launch is one — the recorded forward
// carries a.stats, a data gradient a.dgrad, a prediction conv no scale (vy_conv_wino_supported refuses each)
static int launch_conv(const ConvArgs& a, const VyConvPlan& plan, hipStream_t s) {
  if (g_labels.f) {
    char t[64];
    vy_conv_plan_label(plan, VY_LABEL_TRAIN, t, sizeof t);
    g_labels.via(t);
  }
  HIP_TRY(vy_launch_conv(a, plan, s));
  return 0;
}

// ---- forward: the steps of one cell
// prediction conv: bias, no BatchNorm, straight into its plane
int pred_conv(const TrainCtx& c, int ci) {
  const ConvT& cv = c.net->convs[ci];
  const ConvArgs a = c.net->conv_args(ci);
  g_labels.note(c.net, "fwd", cv.name, a.M, a.N, (double)a.ntaps * a.Kc);
  return launch_conv(a, vy_conv_plan(a), c.s);  // (no weight images for a conv without BatchNorm: the exact kernel)
}

// the raw conv of a BatchNorm cell (the stem: from the image batch x) into its z plane, with the per-tile channel sums
// in partials(); *n_part: their rows
int raw_conv(const TrainCtx& c, int ci, const float* x, int* n_part) {
  vy_net* net = c.net;
  const ConvT& cv = net->convs[ci];
  const TrainCell& cell = c.cell(ci);
  if (cv.is_stem) {
    StemArgs a = net->stem_args(cv, x);
    a.scale = a.shift = nullptr;
    a.out = c.zplane(ci);
    a.out_cs = cell.z_cs;
    a.out_co = 0;
    HIP_TRY(vy_launch_stem_raw(a, reinterpret_cast<double*>(c.partials()), c.s));
    *n_part = vy_stem_blocks(a.B, a.H, a.W);
    return 0;
  }
  ConvArgs a = net->conv_args(ci);
  a.scale = a.shift = a.res = nullptr;
  a.leaky = 0;
  a.out = c.zplane(ci);
  a.o_Hp = cell.Ho + 2;
  a.o_Wp = cell.Wo + 2;
  a.o_cs = cell.z_cs;
  a.o_co = 0;
  a.o_s = 1;
  a.ups = 1;
  a.stats = reinterpret_cast<double*>(c.partials());
  if (!cell.fwd_split) a.w_split = nullptr;
  g_labels.note(net, "fwd", cv.name, a.M, a.N, (double)a.ntaps * a.Kc);
  const VyConvPlan plan = vy_conv_plan(a);
  VY_TRY(launch_conv(a, plan, c.s));
  *n_part = plan.stat_rows;  // the per-tile statistics rows follow the tile that ran
  return 0;
}

// the finalize of a train-mode BatchNorm over `count` samples, a cell's or a conv join's (sums: null — the partial rows)
BnFinalizeArgs finalize_args(const vy_net* net, const BnViews& bn, int C, double count) {
  BnFinalizeArgs f;
  f.sums = nullptr;
  f.count = count;
  f.gamma = bn.gamma;
  f.beta = bn.beta;
  f.running_mean = bn.running_mean;
  f.running_var = bn.running_var;
  f.scale = bn.scale;
  f.shift = bn.shift;
  f.save_mean = bn.save_mean;
  f.save_invstd = bn.save_invstd;
  f.C = C;
  f.eps = 1e-5f;
  f.momentum = 0.9f;  // layers.py:68 (and :57, the join's)
  f.var_unbiased = net->sem.bn_running_var_unbiased;  // vy_net_set_semantics: read at every launch
  return f;
}

// statistics -> scale / shift, running and saved statistics; then the apply pass from z into the cell's output view
int bn_forward(const TrainCtx& c, int ci, int n_part) {
  vy_net* net = c.net;
  const ConvT& cv = net->convs[ci];
  const TrainCell& cell = c.cell(ci);
  const BnViews bn = c.bn_views(ci);
  const int C = cv.cout;
  const double* parts = reinterpret_cast<const double*>(c.partials());
  BnFinalizeArgs f = finalize_args(net, bn, C, (double)cell.M);
  VY_TRY(combine_sums(c, cv, 2 * C, [&] { return vy_launch_reduce_partials_f64(parts, n_part, 2 * C, c.sums_local(), c.s); },
                      &f.count, &f.sums));
  if (f.sums)
    HIP_TRY(vy_launch_bn_finalize(f, c.s));
  else if (!(train_abl(net) & 128))  // (128: the finalize launch of the forward statistics skipped)
    HIP_TRY(vy_launch_bn_reduce_finalize(parts, n_part, f, c.slice_sums(), c.s));
  BnApplyArgs ap;
  memset(&ap, 0, sizeof ap);
  ap.z = c.zplane(ci);
  ap.scale = bn.scale;
  ap.shift = bn.shift;
  ap.out = net->plane_ptr(cv.out_plane);
  ap.B = cell.B;
  ap.H = cell.Ho;
  ap.W = cell.Wo;
  ap.C = C;
  ap.o_Hp = cell.Ho * cv.ups + 2;
  ap.o_Wp = cell.Wo * cv.ups + 2;
  ap.o_cs = net->planes[cv.out_plane].C;
  ap.o_co = cv.out_co;
  ap.ups = cv.ups;
  if (cv.res_plane >= 0) {
    ap.res = net->plane_ptr(cv.res_plane);
    ap.r_cs = net->planes[cv.res_plane].C;
    ap.r_co = cv.res_co;
  }
  if (!(train_abl(net) & 2)) HIP_TRY(vy_launch_bn_apply(ap, c.s));
  return 0;
}

// the cells [first, last) in recording mode; x: the image batch the stem reads
int train_cells(const TrainCtx& c, int first, int last, const float* x) {
  for (int ci = first; ci < last; ++ci) {
    if (c.net->convs[ci].p_gamma < 0) {
      VY_TRY(pred_conv(c, ci));
      continue;
    }
    int n_part = 0;
    VY_TRY(raw_conv(c, ci, x, &n_part));
    VY_TRY(bn_forward(c, ci, n_part));
  }
  return 0;
}

// join `i` of a hierarchical net in recording mode.  The max is the inference launch.  The conv join: z and its per-block
// statistics rows, then the finalize and the apply pass every cell uses, into the pooled plane's channels — its BatchNorm is
// never a synchronised one (`_conv1d` is called without norm_layer), so the ranks exchange nothing here
int train_join(const TrainCtx& c, int i) {
  vy_net* net = c.net;
  const vy_net::HierPool& hp = net->hpools[i];
  if (hp.join != VY_HJOIN_CONV) return net->hier_pool(i, c.s, plain);
  const TrainJoin& jn = c.join(i);
  const BnViews bn = c.join_bn(i);
  HierJoinArgs j = net->join_args(hp, nullptr);
  j.z = c.join_z(i);
  j.partials = reinterpret_cast<double*>(c.partials());
  HIP_TRY(vy_launch_hier_join_raw(j, c.s));
  const BnFinalizeArgs f = finalize_args(net, bn, hp.C, (double)jn.M);
  HIP_TRY(vy_launch_bn_reduce_finalize(j.partials, jn.blocks, f, c.slice_sums(), c.s));
  BnApplyArgs ap;
  memset(&ap, 0, sizeof ap);
  ap.z = j.z;
  ap.scale = bn.scale;
  ap.shift = bn.shift;
  ap.out = net->plane_ptr(hp.dst);
  ap.B = jn.B;
  ap.H = jn.H;
  ap.W = jn.W;
  ap.C = hp.C;
  ap.o_Hp = jn.H + 2;
  ap.o_Wp = jn.W + 2;
  ap.o_cs = net->planes[hp.dst].C;
  ap.o_co = hp.dst_co;
  ap.ups = 1;
  HIP_TRY(vy_launch_bn_apply(ap, c.s));
  return 0;
}

// routes (heads-only nets): the three route tensors, imported into their planes in front of the first conv; bank (windowed
// heads-only nets): each clip's frames of the bank, pooled into the same planes
int forward_train(const TrainCtx& c, const float* x, const float* const* routes, const BankRef* bank = nullptr) {
  vy_net* net = c.net;
  VY_TRY(refresh_split_images(c));
  if (routes) VY_TRY(net->route_import(routes, c.s, plain));
  if (bank) VY_TRY(net->import_pool(*bank, c.s, plain));
  int first = 0;
  for (int i = 0; i < (int)net->hpools.size(); ++i) {  // a hierarchical net: the pool in front of the conv that reads it
    VY_TRY(train_cells(c, first, net->hpools[i].conv, x));
    VY_TRY(train_join(c, i));
    first = net->hpools[i].conv;
  }
  VY_TRY(train_cells(c, first, net->n_backbone, x));
  if (net->clip_net()) VY_TRY(net->window_pool(c.s, plain));  // the stages are done: pool the routes
  return train_cells(c, net->n_backbone, (int)net->convs.size(), nullptr);
}

// ---- backward
// dz of a cell, final on the main stream: a plane (B, Ho + 2, Wo + 2, cs) of the cell's geometry
struct DzView {
  const float* p;
  int cs;
};

// what the cells of one backward pass share
struct BwdState {
  // which channel ranges of each gradient plane already hold a contribution
  std::vector<std::vector<std::pair<int, int>>> touched;
  // pending skip-connection gradients: block input plane view -> gradient view of the block output
  struct Skip {
    int plane, co;  // input view of the block (where the addend must land)
    int src_plane, src_co;
  };
  std::vector<Skip> skips;
  int covered(int plane, int lo, int hi) const {  // 1 accumulate, 0 overwrite, -1 partial overlap
    for (auto& r : touched[plane])
      if (lo < r.second && r.first < hi) return (r.first <= lo && hi <= r.second) ? 1 : -1;
    return 0;
  }
  void whole(const vy_net* net, int plane) { touched[plane].push_back({0, net->planes[plane].C}); }
};

// prediction conv: dz = d(loss)/d(pred) as written by the loss kernel; its column sums are the bias gradient
int bias_grad(const TrainCtx& c, int ci, DzView* dz) {
  const ConvT& cv = c.net->convs[ci];
  const TrainCell& cell = c.cell(ci);
  const int cs = c.net->planes[cv.out_plane].C;
  *dz = {c.gplane(cv.out_plane), cs};
  const int chunks = vy_colsum_chunks(cell.B, cell.Ho, cell.Wo, kBwdChunk);
  HIP_TRY(vy_launch_colsum(dz->p, cell.B, cell.Ho, cell.Wo, cs, 0, cv.cout, kBwdChunk, c.partials(), c.s));
  HIP_TRY(vy_launch_reduce_partials(c.partials(), chunks, cv.cout, c.sums_local(), c.s));
  HIP_TRY(vy_launch_f64_to_f32(c.sums_local(), c.grad_of(cv.p_bias), cv.cout, c.s));
  return 0;
}

// BatchNorm + leaky backward: reduce -> dgamma, dbeta, coefficients -> apply (dz overwrites z)
int bn_backward(const TrainCtx& c, int ci, BwdState& st, DzView* dz) {
  vy_net* net = c.net;
  const ConvT& cv = net->convs[ci];
  const TrainCell& cell = c.cell(ci);
  const BnViews bn = c.bn_views(ci);
  if (st.covered(cv.out_plane, cv.out_co, cv.out_co + cv.cout) != 1)
    return fail(VY_ERR_STATE, "internal: gradient of '%s' output was never produced", cv.name.c_str());
  BnBwdArgs bb;
  memset(&bb, 0, sizeof bb);
  bb.g = c.gplane(cv.out_plane);
  bb.z = c.zplane(ci);
  bb.scale = bn.scale;
  bb.shift = bn.shift;
  bb.save_mean = bn.save_mean;
  bb.save_invstd = bn.save_invstd;
  bb.coef = c.coef();
  bb.partials = c.partials();
  bb.B = cell.B;
  bb.H = cell.Ho;
  bb.W = cell.Wo;
  bb.C = cv.cout;
  bb.g_Hp = cell.Ho * cv.ups + 2;
  bb.g_Wp = cell.Wo * cv.ups + 2;
  bb.g_cs = net->planes[cv.out_plane].C;
  bb.g_co = cv.out_co;
  bb.ups = cv.ups;
  bb.chunk = vy_bn_bwd_rows_per_chunk(cell.B, cell.Ho, cv.cout);
  if (!(train_abl(net) & 1)) HIP_TRY(vy_launch_bn_bwd_reduce(bb, c.s));
  BnBwdFinalizeArgs f;
  memset(&f, 0, sizeof f);
  f.count = (double)cell.M;
  VY_TRY(combine_sums(c, cv, 2 * cv.cout,
                      [&] { return vy_launch_reduce_partials(c.partials(), vy_bn_bwd_chunks(bb), 2 * cv.cout, c.sums_local(), c.s); },
                      &f.count, &f.sums));
  f.local_sums = c.sums_local();
  f.gamma = bn.gamma;
  f.save_invstd = bn.save_invstd;
  f.dgamma = c.grad_of(cv.p_gamma);
  f.dbeta = c.grad_of(cv.p_beta);
  f.coef = c.coef();
  f.C = cv.cout;
  if (f.sums)
    HIP_TRY(vy_launch_bn_bwd_finalize(f, c.s));
  else if (!(train_abl(net) & (1 | 64)))  // (64: the finalize launch alone skipped)
    HIP_TRY(vy_launch_bn_bwd_reduce_finalize(c.partials(), vy_bn_bwd_chunks(bb), f, c.s));
  if (!(train_abl(net) & 4)) HIP_TRY(vy_launch_bn_bwd_apply(bb, c.s));
  *dz = {c.zplane(ci), cell.z_cs};
  if (cv.res_plane >= 0) st.skips.push_back({cv.res_plane, cv.res_co, cv.out_plane, cv.out_co});
  return 0;
}

// split-K slabs + ordered slab reduce into the weight's gradient, on stream ws
int launch_wgrad(const TrainCtx& c, int ci, DzView dz, hipStream_t ws) {
  vy_net* net = c.net;
  const ConvT& cv = net->convs[ci];
  const TrainCell& cell = c.cell(ci);
  const PlaneAt ip = net->plane(cv.in_plane);
  WgradArgs w;
  memset(&w, 0, sizeof w);
  w.dz = dz.p;
  w.a = net->plane_ptr(cv.in_plane);
  w.slabs = c.slabs();
  w.zero = c.at<const float>(c.p.zero_off);
  w.B = cell.B;
  w.Ho = cell.Ho;
  w.Wo = cell.Wo;
  w.M = (int)cell.M;
  w.z_cs = dz.cs;
  w.Cout = cv.cout;
  w.a_Hp = ip.H + 2;
  w.a_Wp = ip.W + 2;
  w.a_cs = ip.C;
  w.a_co = cv.in_co;
  w.stride = cv.stride;
  w.k = cv.k;
  w.Cin = cv.cin;
  w.splits = cell.splits;
  w.k_per_split = cell.k_per_split;
  w.tab = c.at<const uint2>(cell.tab_off);
  g_labels.note(net, "wgrad", cv.name, w.M, w.Cout, (double)cv.k * cv.k * cv.cin);
  // conv mode VY_CONV_SPLIT_BF16X3_TRAIN: the split-fp32 weight-gradient kernel where it has the tile (Cout % 128 == 0)
  if ((train_abl(net) & 8) || ((train_abl(net) & 32) && (long long)cv.k * cv.k * cv.cin <= 576 && cv.cout <= 128)) {
    // (bound measurements: no weight-gradient kernel at all / none for the early cells — N <= 128, K <= 576: stages.0.1 ... 0.5 —
    // whose output tile is mostly padding: what would a perfect kernel for them return to the step?)
  } else if (net->knobs.split_wgrad && net->conv_mode == VY_CONV_SPLIT_BF16X3_TRAIN && vy_wgrad_split_supported(w)) {
    g_labels.via_wgrad("wgrad_split_kernel", w.splits, ws != c.s);
    HIP_TRY(vy_launch_wgrad_split(w, ws));
  } else {
    g_labels.via_wgrad(vy_wgrad_tile_rows(w.Cout, w.k, w.Cin) == 64 ? "wgrad_kernel<32,64>" : "wgrad_kernel<32,128>", w.splits, ws != c.s);
    HIP_TRY(vy_launch_wgrad(w, ws));
  }
  HIP_TRY(vy_launch_slab_reduce(c.slabs(), w.splits, (long long)cv.cout * cv.k * cv.k * cv.cin, c.grad_of(cv.p_weight), ws));
  return 0;
}

// the weight gradient of a cell from its final dz: the stem's from the image batch x, every other conv's through the slabs
int weight_grad(const TrainCtx& c, int ci, DzView dz, const float* x) {
  const ConvT& cv = c.net->convs[ci];
  if (cv.is_stem) {
    StemWgradArgs sw;
    sw.x = x;
    sw.dz = dz.p;
    sw.partials = c.partials();
    sw.B = c.cell(ci).B;
    sw.H = c.p.H;
    sw.W = c.p.W;
    HIP_TRY(vy_launch_stem_wgrad(sw, c.s));
    HIP_TRY(vy_launch_reduce_partials(c.partials(), vy_stem_wgrad_blocks(sw.B, sw.H, sw.W), 864, c.sums_local(), c.s));
    HIP_TRY(vy_launch_f64_to_f32(c.sums_local(), c.grad_of(cv.p_weight), 864, c.s));
    return 0;
  }
  // dz is final on the main stream: the weight gradient (its own scratch: the slabs) goes to the side
  // stream and overlaps with this layer's dgrad and the next layers' BatchNorm kernels
  if (!c.t->side) return launch_wgrad(c, ci, dz, c.s);
  HIP_TRY(hipEventRecord(c.t->ev_main, c.s));
  HIP_TRY(hipStreamWaitEvent(c.t->side, c.t->ev_main, 0));
  return launch_wgrad(c, ci, dz, c.t->side);
}

// dgrad launches of conv ci: gradient w.r.t. its input view, from the dz view
BwdDgrad make_dgrad(const TrainCtx& c, int ci, DzView dz, const float* addend, int add_cs, int add_co) {
  vy_net* net = c.net;
  const ConvT& cv = net->convs[ci];
  const TrainCell& cell = c.cell(ci);
  BwdDgrad out;
  const PlaneAt ip = net->plane(cv.in_plane);
  ConvArgs a;
  memset(&a, 0, sizeof a);  // (ntaps = 0: counted below)
  a.in = dz.p;
  a.w = c.param(cv.p_weight);
  a.out = c.gplane(cv.in_plane);
  a.res = addend;
  a.r_cs = add_cs;
  a.r_co = add_co;
  a.B = cell.B;
  a.a_Hp = cell.Ho + 2;
  a.a_Wp = cell.Wo + 2;
  a.a_cs = dz.cs;
  a.a_co = 0;
  a.a_s = 1;
  a.a_oy = a.a_ox = 1;
  a.Kc = (cv.cout + 31) & ~31;
  a.w_taps = cv.k * cv.k;
  a.w_cin = cv.cin;
  a.w_cout = cv.cout;
  a.N = cv.cin;
  a.o_Hp = ip.H + 2;
  a.o_Wp = ip.W + 2;
  a.o_cs = ip.C;
  a.o_co = cv.in_co;
  a.ups = 1;
  a.dgrad = 1;
  // split-fp32 conv mode: this conv's data-gradient weight images and the split-K scratch (the stream-K region)
  net->launch_env(a, /*k_runs=*/false, /*splitk=*/cell.dgrad_split);
  if (cell.dgrad_split) a.w_split = net->dev_ws + c.p.dsplit_off + cell.dsplit;
  // Input pixel (s y' + py, s x' + px) of a stride-s conv (pad k / 2) receives the taps with (py + pad - kh), (px + pad - kw)
  // multiples of s: one launch at stride 1, one per parity class (py, px) at stride 2
  const int sd = cv.stride, pad = cv.k / 2;
  for (int py = 0; py < sd; ++py)
    for (int px = 0; px < sd; ++px) {
      ConvArgs& q = out.a[out.n++] = a;
      q.LH = cell.Ho;
      q.LW = cell.Wo;
      q.M = (int)cell.M;
      q.o_s = sd;
      q.o_oy = 1 + py;
      q.o_ox = 1 + px;
      for (int kh = 0; kh < cv.k; ++kh) {
        if ((py + pad - kh) % sd) continue;
        for (int kw = 0; kw < cv.k; ++kw) {
          if ((px + pad - kw) % sd) continue;
          q.tap_dy[q.ntaps] = (signed char)((py + pad - kh) / sd);
          q.tap_dx[q.ntaps] = (signed char)((px + pad - kw) / sd);
          q.tap_w[q.ntaps] = (unsigned char)(kh * cv.k + kw);
          ++q.ntaps;
        }
      }
    }
  return out;
}

// Data gradient into the input view.  A heads-only net computes none into its imported routes: yolo_blocks.0.body.0
// (input: the stride-32 route) gets no data gradient at all, yolo_blocks.1/2.body.0 only the one of the upsampled
// transition channels [0, co) in front of the route in their concat plane (a narrower N: every output is the same
// fp32 chain whatever the tile, so these channels are bit-identical to the full net's)
int data_grad(const TrainCtx& c, int ci, DzView dz, BwdState& st) {
  vy_net* net = c.net;
  const ConvT& cv = net->convs[ci];
  const int lo = cv.in_co;
  int hi = cv.in_co + cv.cin;
  if (net->heads_only)
    for (const auto& r : net->routes)
      if (r.plane == cv.in_plane && r.co < hi) hi = std::max(lo, r.co);
  if (hi == lo) return 0;
  const int cov = st.covered(cv.in_plane, lo, hi);
  if (cov < 0) return fail(VY_ERR_STATE, "internal: partial gradient overlap at '%s'", cv.name.c_str());
  const float* addend = nullptr;
  int add_cs = 0, add_co = 0;
  int skip_i = -1;
  for (size_t k = 0; k < st.skips.size(); ++k)
    if (st.skips[k].plane == cv.in_plane && st.skips[k].co == cv.in_co) skip_i = (int)k;
  if (skip_i >= 0) {
    if (cov == 1) return fail(VY_ERR_STATE, "internal: skip + accumulate at '%s'", cv.name.c_str());
    addend = c.gplane(st.skips[skip_i].src_plane);
    add_cs = net->planes[st.skips[skip_i].src_plane].C;
    add_co = st.skips[skip_i].src_co;
    st.skips.erase(st.skips.begin() + skip_i);
  } else if (cov == 1) {
    addend = c.gplane(cv.in_plane);
    add_cs = net->planes[cv.in_plane].C;
    add_co = cv.in_co;
  }
  BwdDgrad dg = make_dgrad(c, ci, dz, addend, add_cs, add_co);
  for (int k = 0; k < dg.n; ++k) {
    ConvArgs& a = dg.a[k];
    if (hi - lo != cv.cin) {
      a.N = hi - lo;
      a.w_split = nullptr;  // (the split kernel's data-gradient images are tiled for the whole cin)
    }
    g_labels.note(net, "dgrad", cv.name, a.M, a.N, (double)a.ntaps * a.Kc);
    if (train_abl(net) & 16) continue;  // (bound measurement: no data-gradient kernel)
    VY_TRY(launch_conv(a, vy_conv_plan(a), c.s));
  }
  if (cov == 0) st.touched[cv.in_plane].push_back({lo, hi});
  return 0;
}

// The backward of conv join `i`, from the complete gradient of its pooled plane (the caller has checked that): the
// BatchNorm + leaky backward of every cell on the join's z plane (dz overwrites z; dgamma, dbeta), then hier_join_bwd — the
// three frames' gradients WRITTEN into the pre-pool gradient plane, and dw through its per-block rows and the ordered
// column sum, in double, rounded to fp32 once.  All on the main stream: partials() and sums_local() are its scratch
int join_backward(const TrainCtx& c, int i) {
  vy_net* net = c.net;
  const vy_net::HierPool& hp = net->hpools[i];
  const TrainJoin& jn = c.join(i);
  const BnViews bn = c.join_bn(i);
  BnBwdArgs bb;
  memset(&bb, 0, sizeof bb);
  bb.g = c.gplane(hp.dst);
  bb.z = c.join_z(i);
  bb.scale = bn.scale;
  bb.shift = bn.shift;
  bb.save_mean = bn.save_mean;
  bb.save_invstd = bn.save_invstd;
  bb.coef = c.coef();
  bb.partials = c.partials();
  bb.B = jn.B;
  bb.H = jn.H;
  bb.W = jn.W;
  bb.C = hp.C;
  bb.g_Hp = jn.H + 2;
  bb.g_Wp = jn.W + 2;
  bb.g_cs = net->planes[hp.dst].C;
  bb.g_co = hp.dst_co;
  bb.ups = 1;
  bb.chunk = vy_bn_bwd_rows_per_chunk(jn.B, jn.H, hp.C);
  HIP_TRY(vy_launch_bn_bwd_reduce(bb, c.s));
  BnBwdFinalizeArgs f;
  memset(&f, 0, sizeof f);
  f.count = (double)jn.M;
  f.local_sums = c.sums_local();
  f.gamma = bn.gamma;
  f.save_invstd = bn.save_invstd;
  f.dgamma = c.grad_of(hp.p_gamma);
  f.dbeta = c.grad_of(hp.p_beta);
  f.coef = c.coef();
  f.C = hp.C;
  HIP_TRY(vy_launch_bn_bwd_reduce_finalize(c.partials(), vy_bn_bwd_chunks(bb), f, c.s));
  HIP_TRY(vy_launch_bn_bwd_apply(bb, c.s));
  HierJoinArgs j = net->join_args(hp, c.gplanes());
  j.z = bb.z;
  j.partials = reinterpret_cast<double*>(c.partials());
  HIP_TRY(vy_launch_hier_join_bwd(j, c.s));
  HIP_TRY(vy_launch_reduce_partials_f64(j.partials, jn.blocks, 3 * hp.C, c.sums_local(), c.s));
  HIP_TRY(vy_launch_f64_to_f32(c.sums_local(), c.grad_of(hp.p_weight), 3 * hp.C, c.s));
  return 0;
}

// the main stream waits for the weight gradients launched so far
int join_side(const TrainCtx& c) {
  if (!c.t->side) return 0;
  HIP_TRY(hipEventRecord(c.t->ev_side, c.t->side));
  HIP_TRY(hipStreamWaitEvent(c.s, c.t->ev_side, 0));
  return 0;
}

// gradient bucket bk is complete: heads | stages.2 | stages.1 | stages.0 (TrainPlan::bucket_lo / bucket_len)
int emit_bucket(const TrainCtx& c, int bk) {
  if (!c.t->gb_cb) return 0;
  VY_TRY(join_side(c));  // the bucket's weight gradients must be final
  if (c.p.bucket_len[bk] == 0) return 0;
  if (int rc = c.t->gb_cb(c.t->gb_user, c.p.bucket_lo[bk], c.p.bucket_len[bk]))
    return fail(VY_ERR_STATE, "gradient bucket callback failed (%d)", rc);
  if (bk == 3 && c.p.join_len)  // the conv joins of a hierarchical net: stages.0's, in a range of their own behind the heads
    if (int rc = c.t->gb_cb(c.t->gb_user, c.p.join_lo, c.p.join_len))
      return fail(VY_ERR_STATE, "gradient bucket callback failed (%d)", rc);
  return 0;
}

// the cells [first, last) in reverse order; a bucket closes behind its first cell
int backward_cells(const TrainCtx& c, BwdState& st, int first, int last, const float* x) {
  for (int ci = last - 1; ci >= first; --ci) {
    const ConvT& cv = c.net->convs[ci];
    DzView dz;
    if (cv.p_gamma < 0)
      VY_TRY(bias_grad(c, ci, &dz));
    else
      VY_TRY(bn_backward(c, ci, st, &dz));
    VY_TRY(weight_grad(c, ci, dz, x));
    if (!cv.is_stem) VY_TRY(data_grad(c, ci, dz, st));  // (no gradient w.r.t. the image)
    for (const vy_net::HierPool& hp : c.net->hpools) {
      if (hp.conv != ci) continue;
      // a hierarchical net: this conv read a pooled plane, whose gradient is final now (route 0 of a four-pool net: the
      // stride-8 head's contribution and this conv's, summed by data_grad).  hier_pool_bwd writes the pre-pool plane's
      // gradient, which the producer in front reads as its output gradient
      if (st.covered(hp.dst, hp.dst_co, hp.dst_co + hp.C) != 1)
        return fail(VY_ERR_STATE, "internal: gradient of the pooled plane in front of '%s' was never produced", cv.name.c_str());
      if (hp.join == VY_HJOIN_CONV)
        VY_TRY(join_backward(c, (int)(&hp - c.net->hpools.data())));
      else
        HIP_TRY(vy_launch_hier_pool_bwd(c.net->hier_args(hp, c.gplanes()), c.s));
      st.touched[hp.src].push_back({0, hp.C});
    }
    if (ci == 0 || c.cell(ci - 1).bucket != c.cell(ci).bucket) VY_TRY(emit_bucket(c, c.cell(ci).bucket));
  }
  return 0;
}

// the weight-gradient pixel tables depend on the planned shape only: built once after vy_net_bind_train
int build_wgrad_tables(const TrainCtx& c) {
  vy_net* net = c.net;
  for (size_t ci = 0; ci < net->convs.size(); ++ci) {
    const ConvT& cv = net->convs[ci];
    const TrainCell& cell = c.cell((int)ci);
    if (cv.is_stem) continue;
    const PlaneAt ip = net->plane(cv.in_plane);
    const int z_cs = cv.p_gamma >= 0 ? cell.z_cs : net->planes[cv.out_plane].C;
    if (cell.M >= (1ll << 31) - 64) return fail(VY_ERR_UNSUPPORTED, "'%s': 2^31 output pixels or more in one batch", cv.name.c_str());
    // (offsets are relative to each split's first pixel: planes of 4 GiB and more are fine — 608x608 past batch 84)
    HIP_TRY(vy_launch_wgrad_table(net->dev_ws + cell.tab_off, (int)cell.M, (int)vy_wgrad_table_entries(cell.M), cell.Ho, cell.Wo,
                                  z_cs, ip.H + 2, ip.W + 2, ip.C, cv.stride, cell.B, cell.k_per_split, c.s));
  }
  c.t->tabs_built = true;
  return 0;
}

int backward_train(const TrainCtx& c, const float* x) {
  vy_net* net = c.net;
  if (!c.t->tabs_built) VY_TRY(build_wgrad_tables(c));
  BwdState st;
  st.touched.resize(net->planes.size());
  // the prediction planes' gradients were written by the loss kernel
  for (int i = 0; i < 3; ++i) st.whole(net, net->head_plane[i]);
  VY_TRY(backward_cells(c, st, net->n_backbone, (int)net->convs.size(), x));
  if (net->clip_net()) {
    // the heads are done: the pooled routes' gradients (cat2 / cat1 route channels, the pooled stride-32 plane) are
    // final.  window_pool_bwd writes the per-frame route planes' gradients; stages.1.0 / stages.2.0 accumulate onto them
    HIP_TRY(vy_launch_window_pool_bwd(net->pool_args(c.gplanes()), c.s));
    for (int i = 0; i < 3; ++i) st.whole(net, net->frame_routes[i]);
  }
  VY_TRY(backward_cells(c, st, 0, net->n_backbone, x));
  VY_TRY(join_side(c));
  if (!st.skips.empty()) return fail(VY_ERR_STATE, "internal: unresolved skip gradient");
  g_labels.close_step();
  return 0;
}

// VY_ERR_STATE unless vy_net_bind_train bound the gradient buffers — and, same_shape: no inference plan was committed
// since, so its regions still lie behind the plan in force (the step entries; `hint` completes the message)
int bound_train(const vy_net* net, bool same_shape, const char* hint) {
  const VyTrain* t = net->train;
  if (!t || !t->grads || (same_shape && t->plan.behind != net->commits))
    return fail(VY_ERR_STATE, "training workspace not bound%s", hint);
  return 0;
}

// the recorded forward, then the fused target-merge + loss + d(loss)/d(pred) kernel
struct LossInputs {
  const float *gt_boxes, *obj_t, *centers_t, *scales_t, *weights_t, *clas_t;
  int32_t M;
  float* losses;
  bool ok() const { return obj_t && centers_t && scales_t && weights_t && clas_t && losses && (M <= 0 || gt_boxes); }
};
int train_forward(vy_net* net, const float* x, const float* const* routes, const LossInputs& in, hipStream_t s,
                  const BankRef* bank = nullptr) {
  VY_TRY(bound_train(net, true, " (vy_net_bind_train)"));
  TrainCtx c(net, s);
  VY_TRY(forward_train(c, x, routes, bank));
  const DetArgs d = net->det_args();
  LossArgs la;
  memset(&la, 0, sizeof la);
  int N = 0;
  for (int i = 0; i < 3; ++i) {
    la.head[i] = d.head[i];
    la.dpred[i] = c.gplane(net->head_plane[i]);
    N += 3 * d.head[i].H * d.head[i].W;
  }
  la.gt_boxes = in.gt_boxes;
  la.obj_t = in.obj_t;
  la.centers_t = in.centers_t;
  la.scales_t = in.scales_t;
  la.weights_t = in.weights_t;
  la.clas_t = in.clas_t;
  la.partials = c.at<float>(c.p.loss_part_off);
  la.B = net->cur.B;
  la.C = net->num_class;
  la.M = in.M;
  la.N = N;
  la.ignore_iou_thresh = c.t->ignore_iou;
  la.label_smooth = c.t->label_smooth;
  HIP_TRY(vy_launch_loss(la, c.s));
  HIP_TRY(vy_launch_loss_reduce(la.partials, vy_loss_blocks_per_image(N), net->cur.B, in.losses, c.s));
  c.t->forward_done = true;
  c.t->M = in.M;
  return 0;
}

// the training-mode forward without a recording: the raw predictions
struct RawOutputs {
  float *box_preds, *centers, *scales, *objness, *class_pred;
  bool ok() const { return box_preds && centers && scales && objness && class_pred; }
};
int train_mode_forward(vy_net* net, const float* x, const float* const* routes, const RawOutputs& out, hipStream_t s,
                       const BankRef* bank = nullptr) {
  VY_TRY(bound_train(net, true, " (vy_net_bind_train)"));
  TrainCtx c(net, s);
  VY_TRY(forward_train(c, x, routes, bank));
  c.t->forward_done = false;  // nothing was recorded: no backward may follow
  const DetArgs d = net->det_args();
  RawPredArgs ra;
  memset(&ra, 0, sizeof ra);
  int N = 0;
  for (int i = 0; i < 3; ++i) {
    ra.head[i] = d.head[i];
    N += 3 * d.head[i].H * d.head[i].W;
  }
  ra.box = out.box_preds;
  ra.centers = out.centers;
  ra.scales = out.scales;
  ra.objness = out.objness;
  ra.class_pred = out.class_pred;
  ra.B = net->cur.B;
  ra.C = net->num_class;
  ra.N = N;
  HIP_TRY(vy_launch_raw_preds(ra, c.s));
  return 0;
}

int train_backward(vy_net* net, const float* x, hipStream_t s) {
  VyTrain* t = net->train;
  if (!t || !t->forward_done) return fail(VY_ERR_STATE, "vy_net_train_backward without a recorded forward");
  t->forward_done = false;
  VY_TRY(bound_train(net, true, " (vy_net_bind_train)"));  // (a bind since the forward: its recording is gone)
  return backward_train(TrainCtx(net, s), x);
}

}  // namespace

extern "C" {

// Training keeps the reference scripts' shapes: multiples of 32 (train_yolov3.py resizes to --data-shape, gluoncv's
// random shapes step by 32).  Inference takes any size (cropped upsample).
static int check_train_shape(int32_t height, int32_t width) {
  if (height % 32 || width % 32)
    return fail(VY_ERR_UNSUPPORTED, "training input %dx%d: height and width must be multiples of 32", height, width);
  return 0;
}

size_t vy_net_train_workspace_bytes(const vy_net* net, int32_t batch, int32_t height, int32_t width) {
  if (!net) return 0;
  if (check_train_shape(height, width)) return 0;
  if (vy_check_shape(batch, height, width)) return 0;
  const NetPlan fwd = net->plan(batch, height, width, /*keep_all=*/true);
  if (net->train) return plan_train(*net, *net->train, fwd, batch, height, width).total;
  VyTrain fresh;  // (a query allocates nothing on the net)
  default_options(*net, &fresh);
  return plan_train(*net, fresh, fwd, batch, height, width).total;
}

// Plans anew at every call, as the sizing queries do, and keeps nothing
int vy_net_plan_region(const vy_net* net, int32_t plan, int32_t batch, int32_t height, int32_t width, int32_t frames,
                       int32_t ring, int32_t index, vy_plan_region* out) {
  if (!net || !out || index < 0) return fail(VY_ERR_INVALID, "vy_net_plan_region: bad argument");
  std::vector<PlanRegion> regions;
  size_t total = 0;
  if (plan == VY_PLAN_CLIP) {
    if (!vy_net_workspace_bytes(net, batch, height, width)) return VY_ERR_INVALID;
    total = net->plan(batch, height, width, net->keep_activations, 0, 0, &regions).total;
  } else if (plan == VY_PLAN_VIDEO) {
    if (!vy_net_video_workspace_bytes(net, frames, batch, ring, height, width)) return VY_ERR_INVALID;
    total = net->plan(batch, height, width, net->keep_activations, frames, ring, &regions).total;
  } else if (plan == VY_PLAN_HIER_VIDEO) {  // batch: the centres, frames: the step
    if (!vy_net_hier_video_workspace_bytes(net, batch, frames, height, width)) return VY_ERR_INVALID;
    total = net->plan(batch, height, width, net->keep_activations, 0, 0, &regions, frames).total;
  } else if (plan == VY_PLAN_TRAIN) {
    if (!vy_net_train_workspace_bytes(net, batch, height, width)) return VY_ERR_INVALID;
    const NetPlan fwd = net->plan(batch, height, width, /*keep_all=*/true, 0, 0, &regions);
    VyTrain fresh;
    if (!net->train) default_options(*net, &fresh);
    total = plan_train(*net, net->train ? *net->train : fresh, fwd, batch, height, width, &regions).total;
  } else {
    return fail(VY_ERR_INVALID, "vy_net_plan_region: plan %d", plan);
  }
  if ((size_t)index >= regions.size()) return VY_ERR_RANGE;  // (the end of the list: not worth an error text)
  const PlanRegion& r = regions[index];
  memset(out, 0, sizeof *out);
  snprintf(out->name, sizeof out->name, "%s", r.name.c_str());
  out->offset = r.off;
  out->bytes = r.used;
  out->span = ((size_t)index + 1 < regions.size() ? regions[index + 1].off : total) - r.off;
  return 0;
}

int vy_net_bind_train(vy_net* net, void* dev_ws, size_t bytes, int32_t batch, int32_t height, int32_t width,
                      void* dev_grads, void* dev_momentum, void* stream) {
  if (!net || !dev_ws || !dev_grads || !dev_momentum) return fail(VY_ERR_INVALID, "null argument");
  if (int rc = check_train_shape(height, width)) return rc;
  if (vy_check_shape(batch, height, width)) return VY_ERR_INVALID;
  if (int rc = net->bind_cus(dev_ws)) return rc;
  VyTrain* t = get_train(net);
  NetPlan fwd = net->plan(batch, height, width, /*keep_all=*/true);
  TrainPlan plan = plan_train(*net, *t, fwd, batch, height, width);
  const size_t need = plan.total;
  if (bytes < need) return fail(VY_ERR_INVALID, "training workspace too small: %zu < %zu bytes", bytes, need);
  t->plan = std::move(plan);
  t->sdesc_uploaded = t->tabs_built = t->seg_uploaded = false;  // (the workspace is zeroed below)
  t->grads = static_cast<float*>(dev_grads);
  t->mom = static_cast<float*>(dev_momentum);
  t->forward_done = false;
  VY_TRY(net->commit_bind(std::move(fwd), dev_ws, bytes, need, static_cast<hipStream_t>(stream)));
  t->plan.behind = net->commits;
  if (net->knobs.train_side_stream && !t->side) {
    // (The weight-gradient stream at the LOWEST queue priority was measured: +0.4 % on top of the raised issue priority of the
    // BatchNorm passes in a fresh process — and the whole training step 1.55x SLOWER, forward included, in a process that had
    // run the host-fed inference legs before (other streams alive: profiles/r06_ab_bn_prio.txt).  Default priority it stays.)
    HIP_TRY(hipStreamCreateWithFlags(&t->side, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&t->ev_main, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&t->ev_side, hipEventDisableTiming));
  }
  return 0;
}

int vy_net_set_train_options(vy_net* net, float ignore_iou_thresh, int32_t label_smooth) {
  if (!net) return fail(VY_ERR_INVALID, "net is null");
  VyTrain* t = get_train(net);
  t->ignore_iou = ignore_iou_thresh;
  t->label_smooth = label_smooth ? 1 : 0;
  return 0;
}

// ---- the six step entries: the kind check, then the frame of the inference entries (run_entry) around the pass
int vy_net_train_forward(vy_net* net, const float* x, const float* gt_boxes, int32_t M, const float* obj_t,
                         const float* centers_t, const float* scales_t, const float* weights_t,
                         const float* clas_t, float* losses, void* stream) {
  VY_TRY(vy_serves(net, "vy_net_train_forward", VY_FULL | VY_WINDOW | VY_HIER));
#ifdef VY_TRAIN_ABL_BUILD
  ++g_abl_forwards;
#endif
  const LossInputs in{gt_boxes, obj_t, centers_t, scales_t, weights_t, clas_t, M, losses};
  return run_entry(net, x && in.ok(), nullptr, stream, [&](hipStream_t s) { return train_forward(net, x, nullptr, in, s); });
}

int vy_net_train_forward_routes(vy_net* net, const float* f0, const float* f1, const float* f2, const float* gt_boxes,
                                int32_t M, const float* obj_t, const float* centers_t, const float* scales_t,
                                const float* weights_t, const float* clas_t, float* losses, void* stream) {
  VY_TRY(vy_serves(net, "vy_net_train_forward_routes", VY_HEADS));
  const float* const routes[3] = {f0, f1, f2};
  const LossInputs in{gt_boxes, obj_t, centers_t, scales_t, weights_t, clas_t, M, losses};
  return run_entry(net, f0 && f1 && f2 && in.ok(), nullptr, stream,
                   [&](hipStream_t s) { return train_forward(net, nullptr, routes, in, s); });
}

int vy_net_train_mode_forward(vy_net* net, const float* x, float* box_preds, float* centers, float* scales,
                              float* objness, float* class_pred, void* stream) {
  VY_TRY(vy_serves(net, "vy_net_train_mode_forward", VY_FULL | VY_WINDOW | VY_HIER));
  const RawOutputs out{box_preds, centers, scales, objness, class_pred};
  return run_entry(net, x && out.ok(), nullptr, stream, [&](hipStream_t s) { return train_mode_forward(net, x, nullptr, out, s); });
}

int vy_net_train_mode_forward_routes(vy_net* net, const float* f0, const float* f1, const float* f2, float* box_preds,
                                     float* centers, float* scales, float* objness, float* class_pred, void* stream) {
  VY_TRY(vy_serves(net, "vy_net_train_mode_forward_routes", VY_HEADS));
  const float* const routes[3] = {f0, f1, f2};
  const RawOutputs out{box_preds, centers, scales, objness, class_pred};
  return run_entry(net, f0 && f1 && f2 && out.ok(), nullptr, stream,
                   [&](hipStream_t s) { return train_mode_forward(net, nullptr, routes, out, s); });
}

int vy_net_train_forward_bank(vy_net* net, const float* f0, const float* f1, const float* f2, int32_t n_frames,
                              const int32_t* table, const float* gt_boxes, int32_t M, const float* obj_t,
                              const float* centers_t, const float* scales_t, const float* weights_t, const float* clas_t,
                              float* losses, void* stream) {
  VY_TRY(vy_serves(net, "vy_net_train_forward_bank", VY_HEADS_WINDOW));
  const BankRef bank{{f0, f1, f2}, n_frames, table};
  const LossInputs in{gt_boxes, obj_t, centers_t, scales_t, weights_t, clas_t, M, losses};
  return run_entry(net, bank.ok() && in.ok(), nullptr, stream, [&](hipStream_t s) {
    VY_TRY(vy_check_bank(net, "vy_net_train_forward_bank", bank));
    return train_forward(net, nullptr, nullptr, in, s, &bank);
  });
}

int vy_net_train_mode_forward_bank(vy_net* net, const float* f0, const float* f1, const float* f2, int32_t n_frames,
                                   const int32_t* table, float* box_preds, float* centers, float* scales, float* objness,
                                   float* class_pred, void* stream) {
  VY_TRY(vy_serves(net, "vy_net_train_mode_forward_bank", VY_HEADS_WINDOW));
  const BankRef bank{{f0, f1, f2}, n_frames, table};
  const RawOutputs out{box_preds, centers, scales, objness, class_pred};
  return run_entry(net, bank.ok() && out.ok(), nullptr, stream, [&](hipStream_t s) {
    VY_TRY(vy_check_bank(net, "vy_net_train_mode_forward_bank", bank));
    return train_mode_forward(net, nullptr, nullptr, out, s, &bank);
  });
}

int vy_net_train_backward(vy_net* net, const float* x, void* stream) {
  VY_TRY(vy_serves(net, "vy_net_train_backward", VY_FULL | VY_WINDOW | VY_HIER));
  return run_entry(net, x != nullptr, nullptr, stream, [&](hipStream_t s) { return train_backward(net, x, s); });
}

int vy_net_train_backward_routes(vy_net* net, const float* f0, const float* f1, const float* f2, void* stream) {
  // (nothing is read from the routes: see data_grad — so a windowed heads-only net, whose forward read a bank, is served
  // too, and may pass NULL)
  VY_TRY(vy_serves(net, "vy_net_train_backward_routes", VY_HEADS | VY_HEADS_WINDOW));
  return run_entry(net, net->kind() == VY_HEADS_WINDOW || (f0 && f1 && f2), nullptr, stream,
                   [&](hipStream_t s) { return train_backward(net, nullptr, s); });
}

int vy_net_param_set_opt(vy_net* net, int32_t i, float lr_mult, float wd_mult, int32_t enabled) {
  if (!net || i < 0 || i >= (int32_t)net->params.size()) return fail(VY_ERR_INVALID, "bad argument");
  VyTrain* t = get_train(net);
  t->lr_mult[i] = lr_mult;
  t->wd_mult[i] = wd_mult;
  t->enabled[i] = enabled ? 1 : 0;
  // refresh the segment table in place if it is already planned (a segment per trainable parameter, in order)
  int si = 0;
  for (int p = 0; p < i; ++p) si += net->params[p].info.trainable ? 1 : 0;
  if (!net->params[i].info.trainable || si >= (int)t->plan.segs.size()) return 0;
  SgdSeg& sg = t->plan.segs[si];
  const int en = enabled ? 1 : 0;
  if (sg.lr_mult != lr_mult || sg.wd_mult != wd_mult || sg.enabled != en) {  // re-upload only on a change
    sg.lr_mult = lr_mult;
    sg.wd_mult = wd_mult;
    sg.enabled = en;
    t->seg_uploaded = false;
  }
  return 0;
}

int vy_net_sgd_step(vy_net* net, float lr, float momentum, float wd, float rescale_grad, void* stream) {
  if (!net) return fail(VY_ERR_INVALID, "net is null");
  VY_TRY(net->check_ready());
  VY_TRY(bound_train(net, false, " (vy_net_bind_train)"));
  TrainCtx c(net, stream);
  SgdSeg* segs = c.at<SgdSeg>(c.p.seg_off);
  int32_t* chunks = c.at<int32_t>(c.p.chunk_off);
  if (!c.t->seg_uploaded) {
    HIP_TRY(hipMemcpyAsync(segs, c.p.segs.data(), c.p.segs.size() * sizeof(SgdSeg), hipMemcpyHostToDevice, c.s));
    HIP_TRY(hipMemcpyAsync(chunks, c.p.chunk_seg.data(), c.p.chunk_seg.size() * sizeof(int32_t), hipMemcpyHostToDevice, c.s));
    HIP_TRY(hipStreamSynchronize(c.s));  // pageable host vectors; only when the table changed
    c.t->seg_uploaded = true;
  }
  HIP_TRY(vy_launch_sgd(net->dev_params, c.t->grads, c.t->mom, segs, chunks, (int)(c.p.chunk_seg.size() / 2), lr, momentum,
                        wd, rescale_grad, c.s));
  net->split_dirty = net->dsplit_dirty = net->wino_dirty = true;  // conv mode VY_CONV_SPLIT_BF16X3: the weight images are stale now
  return 0;
}

int vy_net_grad_get(vy_net* net, int32_t i, float* host_dst, void* stream) {
  if (!net || !host_dst || i < 0 || i >= (int32_t)net->params.size()) return fail(VY_ERR_INVALID, "bad argument");
  VY_TRY(bound_train(net, false, ""));
  const vy_param_info& pi = net->params[i].info;
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::vector<float> tmp((size_t)pi.size);
  HIP_TRY(hipMemcpyAsync(tmp.data(), net->train->grads + pi.offset, sizeof(float) * pi.size, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (pi.ndim == 4) {
    unpack_oihw(tmp.data(), host_dst, pi.shape[0], pi.shape[1], pi.shape[2]);
  } else {
    memcpy(host_dst, tmp.data(), sizeof(float) * pi.size);
  }
  return 0;
}

int vy_net_read_grad_activation(vy_net* net, const char* name, float* dst_dev, void* stream) {
  if (!net || !name || !dst_dev) return fail(VY_ERR_INVALID, "bad argument");
  VY_TRY(net->check_ready());
  VY_TRY(bound_train(net, false, ""));
  TrainCtx c(net, stream);
  TapRef t;
  VY_TRY(vy_resolve_tap(net, name, &t));
  HIP_TRY(vy_tap_to_nchw(net, t, c.gplanes(), dst_dev, c.s));
  return 0;
}

int vy_net_read_train_tap(vy_net* net, const char* name, int32_t which, float* dst_dev, int32_t* dims, void* stream) {
  if (!net || !name) return fail(VY_ERR_INVALID, "bad argument");
  VY_TRY(net->check_ready());
  VY_TRY(bound_train(net, false, ""));
  TrainCtx c(net, stream);
  TapRef t;
  VY_TRY(vy_resolve_tap(net, name, &t));
  if (t.hpool >= 0) {  // a pooled plane: its gradient, or the pre-pool plane it was made of
    const vy_net::HierPool& hp = net->hpools[t.hpool];
    if (hp.join == VY_HJOIN_CONV && (which == VY_TAP_Z || which == VY_TAP_BN)) {  // a conv join: z / dz and BatchNorm, as a cell's
      const TrainJoin& jn = c.join(t.hpool);
      const bool z = which == VY_TAP_Z;
      const int32_t d[4] = {z ? jn.B : 4, hp.C, z ? jn.H + 2 : 1, z ? jn.W + 2 : 1};
      if (dims) memcpy(dims, d, sizeof d);
      if (!dst_dev) return 0;
      if (z) {
        HIP_TRY(vy_launch_padded_plane_to_nchw(c.join_z(t.hpool), d[0], d[2], d[3], hp.C, 0, hp.C, dst_dev, c.s));
        return 0;
      }
      const BnViews v = c.join_bn(t.hpool);
      const float* rows[4] = {v.save_mean, v.save_invstd, v.scale, v.shift};
      for (int r = 0; r < 4; ++r)
        HIP_TRY(hipMemcpyAsync(dst_dev + (size_t)r * hp.C, rows[r], sizeof(float) * hp.C, hipMemcpyDeviceToDevice, c.s));
      return 0;
    }
    if (which != VY_TAP_GRAD_PADDED && which != VY_TAP_INPUT_PADDED)
      return fail(VY_ERR_INVALID, "'%s' has the taps VY_TAP_GRAD_PADDED and VY_TAP_INPUT_PADDED only", name);
    const bool grad = which == VY_TAP_GRAD_PADDED;
    const int pl = grad ? hp.dst : hp.src;
    const PlaneAt p = net->plane(pl);
    const int32_t d[4] = {net->plane_batch(pl), hp.C, p.H + 2, p.W + 2};
    if (dims) memcpy(dims, d, sizeof d);
    if (dst_dev)
      HIP_TRY(vy_launch_padded_plane_to_nchw(grad ? c.gplane(pl) : net->plane_ptr(pl), d[0], d[2], d[3], p.C, grad ? hp.dst_co : 0,
                                             hp.C, dst_dev, c.s));
    return 0;
  }
  if (t.conv < 0) return fail(VY_ERR_INVALID, "no cell named '%s'", name);  // (a pooled route: vy_net_read_grad_activation reads it)
  const int ci = t.conv;
  const ConvT& cv = net->convs[ci];
  const TrainCell& cell = c.cell(ci);
  const bool bn = cv.p_gamma >= 0;
  int32_t d[4] = {net->conv_batch(cv), cv.cout, 0, 0};
  const float* src = nullptr;
  int cs = 0, co = 0;
  switch (which) {
    case VY_TAP_Z:
      if (!bn) return fail(VY_ERR_INVALID, "'%s' has no z plane", name);
      src = c.zplane(ci);
      d[2] = cell.Ho + 2;
      d[3] = cell.Wo + 2;
      cs = cell.z_cs;
      break;
    case VY_TAP_BN:
      if (!bn) return fail(VY_ERR_INVALID, "'%s' has no BatchNorm", name);
      d[0] = 4;
      d[2] = d[3] = 1;
      break;
    case VY_TAP_GRAD_PADDED: {
      const PlaneAt p = net->plane(cv.out_plane);
      src = c.gplane(cv.out_plane);
      d[2] = p.H + 2;
      d[3] = p.W + 2;
      cs = p.C;
      co = cv.out_co;
      break;
    }
    case VY_TAP_INPUT_PADDED: {
      if (cv.is_stem) return fail(VY_ERR_INVALID, "the stem reads the image, not a plane");
      const PlaneAt p = net->plane(cv.in_plane);
      src = net->plane_ptr(cv.in_plane);
      d[1] = cv.cin;
      d[2] = p.H + 2;
      d[3] = p.W + 2;
      cs = p.C;
      co = cv.in_co;
      break;
    }
    default:
      return fail(VY_ERR_INVALID, "unknown tap %d", which);
  }
  if (dims) memcpy(dims, d, sizeof d);
  if (!dst_dev) return 0;
  if (which == VY_TAP_BN) {
    const BnViews v = c.bn_views(ci);
    const float* rows[4] = {v.save_mean, v.save_invstd, v.scale, v.shift};
    for (int r = 0; r < 4; ++r)
      HIP_TRY(hipMemcpyAsync(dst_dev + (size_t)r * cv.cout, rows[r], sizeof(float) * cv.cout, hipMemcpyDeviceToDevice, c.s));
    return 0;
  }
  HIP_TRY(vy_launch_padded_plane_to_nchw(src, d[0], d[2], d[3], cs, co, d[1], dst_dev, c.s));
  return 0;
}

int vy_net_train_conv_plan(const vy_net* net, int32_t i, int32_t* wgrad_splits, int32_t* wgrad_k_per_split,
                           int32_t* bn_bwd_rows_per_chunk) {
  if (!net || i < 0 || i >= (int32_t)net->convs.size()) return fail(VY_ERR_INVALID, "bad argument");
  const VyTrain* t = net->train;
  if (!t || t->plan.cells.size() != net->convs.size()) return fail(VY_ERR_STATE, "no training plan");
  const ConvT& cv = net->convs[i];
  const TrainCell& cell = t->plan.cells[i];
  // (stem_wgrad_kernel: one fp32 accumulator per wave over 512 pixels, the four waves of a block added in fp32, the
  // blocks in double)
  if (wgrad_splits) *wgrad_splits = cv.is_stem ? 4 : cell.splits;
  if (wgrad_k_per_split) *wgrad_k_per_split = cv.is_stem ? 512 : cell.k_per_split;
  if (bn_bwd_rows_per_chunk) *bn_bwd_rows_per_chunk = cv.p_gamma >= 0 ? vy_bn_bwd_rows_per_chunk(cell.B, cell.Ho, cv.cout) : 0;
  return 0;
}

int vy_net_set_sync_bn(vy_net* net, int32_t world, vy_allreduce_cb cb, void* user) {
  if (!net || world < 1) return fail(VY_ERR_INVALID, "bad argument");
  if (world > 1 && !cb) return fail(VY_ERR_INVALID, "world > 1 needs an all-reduce callback");
  VyTrain* t = get_train(net);
  t->world = world;
  t->ar_cb = cb;
  t->ar_user = user;
  return 0;
}

int vy_net_set_grad_bucket_cb(vy_net* net, vy_grad_bucket_cb cb, void* user) {
  if (!net) return fail(VY_ERR_INVALID, "net is null");
  VyTrain* t = get_train(net);
  t->gb_cb = cb;
  t->gb_user = user;
  return 0;
}

}  // extern "C"
