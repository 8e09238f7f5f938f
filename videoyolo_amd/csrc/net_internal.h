// net_internal.h — the vy_net object shared by net.hip (graph, planner, inference C-ABI) and
// train.hip (training planner and C-ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "vy_support.h"
#include "kernels.h"
#include "conv_launch.h"
#include "../../include/vy_math.h"

// VY_ERR_INVALID unless (batch, h, w) is a shape the planner takes (defined in net.hip)
int vy_check_shape(int32_t batch, int32_t h, int32_t w);

// The kind of a net (vy_net::kind), one bit each so that an entry point states the kinds it serves as a set (vy_serves)
enum VyKind : unsigned {
  VY_FULL = 1,           // vy_net_create: single frames
  VY_HEADS = 2,          // vy_net_create_heads: the heads on the three routes of single frames
  VY_WINDOW = 4,         // vy_net_create_window: clips of k frames, the routes pooled over each clip
  VY_HEADS_WINDOW = 8,   // vy_net_create_heads_window: the heads on windows of a bank of per-frame routes
  VY_HIER = 16,          // vy_net_create_hier: clips of 3^n frames pooled by threes inside the backbone
};
// OIHW (reference) <-> O,kh,kw,I (device): the host copy of a conv weight or of its gradient
inline void pack_oihw(const float* src, float* dst, int O, int I, int k) {
  for (int o = 0; o < O; ++o)
    for (int i = 0; i < I; ++i)
      for (int t = 0; t < k * k; ++t) dst[((size_t)o * k * k + t) * I + i] = src[((size_t)o * I + i) * k * k + t];
}
inline void unpack_oihw(const float* src, float* dst, int O, int I, int k) {
  for (int o = 0; o < O; ++o)
    for (int i = 0; i < I; ++i)
      for (int t = 0; t < k * k; ++t) dst[((size_t)o * I + i) * k * k + t] = src[((size_t)o * k * k + t) * I + i];
}

// the inputs of a *_bank entry: three banks of per-frame routes (n_frames, C, h, w) and the (B, k) table of frames
struct BankRef {
  const float* f[3];
  int32_t n_frames;
  const int32_t* table;
  bool ok() const { return f[0] && f[1] && f[2] && table; }
};

// hook before, launch, hook after
#define HOOKED(hook, name, fl, by, launch) \
  do {                                     \
    hook(name, fl, by, true);              \
    HIP_TRY(launch);                       \
    hook(name, fl, by, false);             \
  } while (0)

// the hook of a plain forward (vy_net::kLabels)
struct NoHook {
  void operator()(const char*, double, double, bool) const {}
};

struct ParamT {
  vy_param_info info;
};

struct PlaneT {
  int C = 0;    // channel stride
  int div = 1;  // spatial = input / div
  // frames per batch entry: k for the stem and stage planes of a window net (B*k frames); 3^(pools still ahead) for the
  // backbone planes of a hierarchical net; 1 otherwise
  int fm = 1;
};

struct ConvT {
  std::string name;      // structural prefix of the cell, e.g. "stages.0.2.body.1"
  int in_plane, in_co, cin;
  int out_plane, out_co, cout;
  int k, stride, leaky, ups;
  int res_plane, res_co;          // -1: none
  int p_weight;                   // param indices
  int p_gamma, p_beta, p_mean, p_var;  // -1 for the prediction convs
  int p_bias;                     // -1 for cells
  int64_t scale_off, shift_off;   // folded BN scratch (element offsets), -1 if none
  int is_stem;
};

// Where one shape puts the graph in the workspace: everything a bind decides.  vy_net::plan computes one from the graph and
// the settings and writes nothing; a bind commits it by assignment (vy_net::cur, commit_bind)
struct NetPlan {
  int B = 0, H = 0, W = 0;
  // a video plan (vy_net_bind_video): the stem and stage planes hold video_F single frames, the planes from the
  // pooled routes on hold B clips, and behind the planes lies a ring of video_R slots of per-frame routes (video.hip).
  // 0: the clip plan — binding either way switches the net over
  int video_F = 0, video_R = 0;
  // a hier-video plan (vy_net_bind_hier_video): B counts the centres of a chunk, hier_step is the step between
  // the frames of a clip, and a backbone plane holds the frame positions its level needs for them (vy_net::frames_of) —
  // the joins run dilated (hier.hip).  0: any other plan
  int hier_step = 0;
  size_t fold_desc_off = 0, det_scratch_off = 0;  // byte offsets in the workspace
  size_t sk_off = 0, sk_slabs_off = 0;  // stream-K scratch of the conv launches (conv_igemm.hip): the flags, the slabs
  int guard = 0;  // unused bytes behind every carve (VY_PLAN_GUARD; 0 outside the tests)
  size_t ck_off = 0, ck_bytes = 0;  // running-sum scratch of the convs whose K is summed in runs (conv_igemm.hip)
  size_t wsplit_off = 0, planes_off = 0;
  size_t ring_off = 0;             // the ring of a video plan
  long long ring_slot_floats = 0;  // floats per slot
  size_t total = 0;                // bytes of the workspace the plan needs
  bool planes_shared = false;      // the plan recycles planes (read_activation is then meaningless)
  struct Plane {
    int H = 0, W = 0;
    size_t off = 0;  // float offset in the plane region
  };
  // conv mode VY_CONV_SPLIT_BF16X3: byte offsets in the region at wsplit_off of the bf16 weight images (-1: exact kernel)
  // and of the Winograd-transformed image sets (conv_wino.hip: 3x3 stride-1 cells with cout % 128 == 0; -1: none)
  struct Conv {
    int64_t split_off = -1, wino_off = -1;
  };
  std::vector<Plane> planes;  // per plane of the graph
  std::vector<Conv> convs;    // per conv
};

// One carve of a plan, for the tests' region table (vy_net_plan_region): its name, its byte offset in the workspace and the
// bytes the kernels are meant to use of it — the rounding to 256 and the guard gap follow
struct PlanRegion {
  std::string name;
  size_t off, used;
};

// a plane of the graph where the committed plan put it (vy_net::plane)
struct PlaneAt {
  int C, H, W;
  size_t off;
};

// the cells Darknet3D builds with the norm_layer passed to yolo3_darknet53 — the stem and the five stride-2 convs
// (three_darknet.py:163-181); every other BatchNorm of the model is a plain per-device one: the residual blocks hard-wire
// BatchNorm (darknet.py:89-91) and wrappers.py:101-103 does not hand norm_layer to YOLOV3T, so the heads default to it
inline bool is_sync_layer(const ConvT& c) {
  return c.p_gamma >= 0 && c.name.rfind("stages.", 0) == 0 && c.name.find(".body.") == std::string::npos;
}

static const int kAnchors[3][6] = {{10, 13, 16, 30, 33, 23}, {30, 61, 62, 45, 59, 119}, {116, 90, 156, 198, 373, 326}};
static const int kStrides[3] = {8, 16, 32};  // wrappers.py:80-84

struct VyTrain;
void vy_train_free(struct vy_net* net);

struct vy_net {
  int num_class = 0;
  float nms_thresh = 0.45f;  // YOLOV3T.__init__ defaults, yolo3.py:959-963
  int nms_topk = 400, post_nms = 100;
  // vy_net_set_semantics: the recalled box_nms / BatchNorm choices of this net, all 0 by default.  Not part of any plan:
  // det_args() and bn_forward (train.hip) read them at every launch, so they survive every bind
  vy_semantics sem = {};
  std::vector<ParamT> params;
  std::vector<PlaneT> planes;
  std::vector<ConvT> convs;
  int n_backbone = 0;  // convs [0, n_backbone) are the stem and the stages, [n_backbone, size) the heads (0: heads-only net)
  int head_plane[3] = {-1, -1, -1};  // prediction conv outputs, order stride 32,16,8
  int64_t param_elems = 0;           // tensors + scratch
  int64_t tensor_elems = 0;
  std::vector<FoldDesc> folds;
  // the graph above is written by build() alone.  Bound state:
  float* dev_params = nullptr;
  unsigned char* dev_ws = nullptr;
  size_t ws_bytes = 0;
  NetPlan cur;           // the committed plan (commit_bind): what every launch reads
  unsigned commits = 0;  // plans committed so far: a training plan is valid while the one it was carved behind is the last
  bool fold_uploaded = false;
  bool fold_in_stem = false;  // set by prepare(): this sequence's stem launch carries the BatchNorm fold
  bool keep_activations = false;  // vy_net_set_keep_activations: inference planes are not recycled (parity taps)
  // vy_net_set_conv_mode: VY_CONV_SPLIT_BF16X3 sends the inference launches conv_split.hip can serve through the bf16
  // matrix core (bf16 x 3, six products, fp32 accumulate); their pre-split weight images live in the workspace and are
  // rebuilt by the next forward whenever the parameters may have changed (split_dirty)
  // stream-K bookkeeping: sk_ok = the device's workgroup placement was verified at bind time (vy_sk_verify_topology);
  // sk_dirty = an entry point of this handle returned an error after it may have launched stream-K kernels: the hand-off
  // flags are cleared by their consumers, so an aborted sequence can leave one up — the next forward / step zeroes them
  bool sk_ok = false;
  bool sk_dirty = false;
  int conv_mode = 0;
  bool split_dirty = true;    // the forward weight images are stale
  bool dsplit_dirty = true;   // the data-gradient weight images (training plans; train.hip) are stale
  // the Winograd image sets (conv_wino.hip) are stale.  Their own flag: a training plan holds them too (model.py reuses it
  // for inference at the same size) but train.hip's refresh_split_images rebuilds only the forward and data-gradient sets —
  // only prepare() below, which does rebuild them, may clear it
  bool wino_dirty = true;
  // the launch switches (knobs.h), read from the environment once, by vy_net_create: every launch of this net reads them
  // here (ConvArgs::knobs), so a switch set or changed later affects only nets created after it
  VyKnobs knobs;
  // CUs of THIS net's device: resolved once, by the first sizing / bind call, from the calling thread's current device —
  // and checked at every bind against the device that owns the workspace (bind_cus below), so that a C-ABI caller whose
  // current device differs between vy_net_*workspace_bytes and vy_net_bind_* gets an error instead of a plan sized for
  // one chip and bound on another.  Every cost-model choice reads this through ConvArgs::cus.
  mutable int cus = 0;
  int resolve_cus() const {
    if (!cus) cus = vy_cu_count();
    return cus;
  }
  int bind_cus(const void* ws) const {
    const int sized = resolve_cus();
    const int owner = vy_cu_count_of_ptr(ws);
    if (owner && owner != sized)
      return fail(VY_ERR_STATE,
                  "the workspace lives on a device with %d CUs but this net sized its plan for %d (the calling thread's current "
                  "device at the first vy_net_*workspace_bytes call): size and bind with the same current device", owner, sized);
    return 0;
  }
  struct VyTrain* train = nullptr;  // training planner state, owned by train.hip
  // vy_net_create_heads: the graph starts at the three route tensors (YOLOV3_noback, yolo3.py:1686-1920) — no stem, no
  // stages; the routes are imported into the planes the backbone's last blocks write in a full net
  bool heads_only = false;
  // the route slices, order stride 8, 16, 32 (features[:15], [15:24], [24:]): plane, first channel, channels
  struct RouteSlot {
    int plane = -1, co = 0, C = 0;
  } routes[3];
  // vy_net_create_window: a k-frame clip net (YOLOV3T, early join).  The stem and stages run on B*k frames; the three
  // route cells write per-frame planes of their own (frame_routes, order stride 8, 16, 32), which window_pool
  // (temporal.hip) pools over each clip into `routes` — the slices the heads read — once, after the last stage cell
  int window_k = 0;  // 0: not a window net
  int window_join = 0;
  // vy_net_create_heads_window: heads_only with window_k set.  The plan is the heads-only net's, number for number: there
  // is no backbone to run on B*k frames and no per-frame plane; route_import_pool (routes.hip) pools each clip's k frames
  // out of the caller's bank of stored routes on the way into the planes route_import fills.  Everything that concerns
  // the B*k-frame backbone of a window net keys on clip_net()
  bool clip_net() const { return window_k && !heads_only; }
  int frame_routes[3] = {-1, -1, -1};
  // vy_net_create_hier: a hierarchical net (HDarknet, h_join_type 'max'; hier.hip).  A clip of 3^hier_n frames goes through
  // the stem per frame; in front of each of the first hier_n stride-2 convs the frames are max-pooled by threes into a
  // plane of a third of the frames, which that conv reads.  From the last pool on it is the single-frame net on B clips.
  // The conv list and the parameter table are the single-frame net's; only planes and their fm differ
  int hier_n = 0;  // pools, 1..4; 0: not a hierarchical net
  // vy_net_create_hier_join: how the triples are joined, VY_HJOIN_MAX or VY_HJOIN_CONV (h_join_type 'conv': `_conv1d`,
  // layers.py:50-60 — a depthwise 3-tap filter over the frames, BatchNorm, LeakyReLU).  The conv join has parameters of its
  // own, "hjoin.<i>.0.weight" (C, 3) and the four BatchNorm tensors "hjoin.<i>.1.*", appended BEHIND the single-frame net's
  // table, which stays a prefix of this one; the conv list is still the single-frame net's: a join is not a ConvT
  int hier_join = VY_HJOIN_MAX;
  struct HierPool {
    int src, dst, dst_co, C;  // pre-pool plane (its C channels at 0) -> channels [dst_co, dst_co + C) of the pooled plane
    int conv;                 // the stride-2 conv that reads the pooled plane: the pool runs in front of it
    int join = VY_HJOIN_MAX;  // the net's hier_join
    // VY_HJOIN_CONV: parameter indices and the folded-BatchNorm scratch (element offsets), as a ConvT's
    int p_weight = -1, p_gamma = -1, p_beta = -1, p_mean = -1, p_var = -1;
    int64_t scale_off = -1, shift_off = -1;
  };
  std::vector<HierPool> hpools;
  int hier_frames() const {
    int f = 1;
    for (int i = 0; i < hier_n; ++i) f *= 3;
    return f;
  }
  // what the three fields above make of this net: the one place that says so (build() and the planner read the fields)
  VyKind kind() const {
    if (heads_only) return window_k ? VY_HEADS_WINDOW : VY_HEADS;
    return window_k ? VY_WINDOW : hier_n ? VY_HIER : VY_FULL;
  }
  // one pool launch, forward (grads == nullptr) or backward (grads: the training gradient planes)
  HierPoolArgs hier_args(const HierPool& hp, float* grads) const {
    HierPoolArgs a;
    memset(&a, 0, sizeof a);
    const PlaneAt sp = plane(hp.src), dp = plane(hp.dst);
    a.src = plane_ptr(hp.src);
    a.dst = plane_ptr(hp.dst);
    if (grads) {
      a.gsrc = grads + sp.off;
      a.gdst = grads + dp.off;
    }
    a.frames = plane_batch(hp.dst);
    if (cur.hier_step) {  // pool i joins positions d = step * 3^i apart: h_(i+1) - h_i
      a.dil = cur.hier_step;
      for (const HierPool* q = hpools.data(); q != &hp; ++q) a.dil *= 3;
    }
    a.H = dp.H;
    a.W = dp.W;
    a.C = hp.C;
    a.s_cs = sp.C;
    a.d_cs = dp.C;
    a.d_co = hp.dst_co;
    return a;
  }
  // one launch of a conv join: inference (grads == nullptr; z and partials stay null) or a training launch, whose z plane and
  // partial rows train.hip adds
  HierJoinArgs join_args(const HierPool& hp, float* grads) const {
    HierJoinArgs j;
    memset(&j, 0, sizeof j);
    j.g = hier_args(hp, grads);
    j.w = dev_params + params[hp.p_weight].info.offset;
    j.scale = dev_params + hp.scale_off;
    j.shift = dev_params + hp.shift_off;
    return j;
  }

  // frames a stem / stage plane holds for `b` clips: b * fm of the clip plan; `frames` of a window net's video plan; of a
  // hier-video plan with step `hstep` (b centres) the positions of the plane's level L, T / fm = 3^L:
  // b + 2 (h_n - h_L) = b + hstep (T - T / fm) with h_L = hstep (3^L - 1) / 2 — b from the last pool on
  int frames_of(const PlaneT& p, int b, int frames, int hstep) const {
    if (hstep) return b + hstep * (hier_frames() - hier_frames() / p.fm);
    return frames && p.fm > 1 ? frames : b * p.fm;
  }
  // frames of the batch a plane holds / a conv runs on (its output plane's: a window net's backbone cells B*k)
  int plane_batch(int p) const { return frames_of(planes[p], cur.B, cur.video_F, cur.hier_step); }
  int conv_batch(const ConvT& c) const { return plane_batch(c.out_plane); }
  PlaneAt plane(int i) const { return {planes[i].C, cur.planes[i].H, cur.planes[i].W, cur.planes[i].off}; }
  // the pooling launch of a window net, forward (grads == nullptr) or backward (grads: the training gradient planes,
  // same offsets as the activation planes)
  WindowPoolArgs pool_args(float* grads) const {
    WindowPoolArgs a;
    memset(&a, 0, sizeof a);
    a.n = 3;
    a.B = cur.B;
    a.k = window_k;
    a.join = window_join;
    for (int i = 0; i < 3; ++i) {
      const PlaneAt fp = plane(frame_routes[i]);
      const PlaneAt dp = plane(routes[i].plane);
      PoolRoute& r = a.r[i];
      r.src = plane_ptr(frame_routes[i]);
      r.dst = plane_ptr(routes[i].plane);
      if (grads) {
        r.gsrc = grads + fp.off;
        r.gdst = grads + dp.off;
      }
      r.H = dp.H;
      r.W = dp.W;
      r.C = routes[i].C;
      r.s_cs = fp.C;
      r.d_cs = dp.C;
      r.d_co = routes[i].co;
    }
    return a;
  }

  // floats of one ring slot at input size (h, w): the three routes, tight, rounded to 256 B
  long long slot_floats(int h, int w) const {
    long long fl = 0;
    for (int i = 0; i < 3; ++i) {
      const int d = planes[routes[i].plane].div;
      fl += (long long)((h + d - 1) / d) * ((w + d - 1) / d) * routes[i].C;
    }
    return (fl + 63) & ~63ll;
  }
  // the three routes of a video plan's launches (video.hip): per-frame planes, ring, pooled planes
  void ring_routes(RingRoute* rr) const {
    float* ring = reinterpret_cast<float*>(dev_ws + cur.ring_off);
    for (int i = 0; i < 3; ++i) {
      const PlaneAt fp = plane(frame_routes[i]);
      const PlaneAt dp = plane(routes[i].plane);
      RingRoute& r = rr[i];
      r.plane = plane_ptr(frame_routes[i]);
      r.ring = ring;
      r.dst = plane_ptr(routes[i].plane);
      r.H = dp.H;
      r.W = dp.W;
      r.C = routes[i].C;
      r.s_cs = fp.C;
      r.d_cs = dp.C;
      r.d_co = routes[i].co;
      ring += (long long)r.H * r.W * r.C;
    }
  }

  int add_param(const std::string& name, int kind, int ndim, const int* shape, int trainable, int backbone) {
    ParamT p;
    memset(&p.info, 0, sizeof p.info);
    snprintf(p.info.name, sizeof p.info.name, "%s", name.c_str());
    p.info.kind = kind;
    p.info.ndim = ndim;
    int64_t sz = 1;
    for (int i = 0; i < ndim; ++i) {
      p.info.shape[i] = shape[i];
      sz *= shape[i];
    }
    p.info.size = sz;
    p.info.offset = param_elems;
    p.info.trainable = trainable;
    p.info.backbone = backbone;
    param_elems += (sz + 63) & ~(int64_t)63;  // 256-B aligned tensors
    params.push_back(p);
    return (int)params.size() - 1;
  }

  int add_plane(int C, int div, int fm = 1) {
    PlaneT p;
    p.C = C;
    p.div = div;
    p.fm = fm;
    planes.push_back(p);
    return (int)planes.size() - 1;
  }

  // `_conv2d` cell (layers.py:63-70) or a bare prediction conv (yolo3.py:62) when bn == false
  int add_conv(const std::string& name, int in_plane, int in_co, int cin, int out_plane, int out_co, int cout,
               int k, int stride, bool bn, int backbone, int res_plane = -1, int res_co = 0, int ups = 1) {
    ConvT c;
    c.name = name;
    c.in_plane = in_plane;
    c.in_co = in_co;
    c.cin = cin;
    c.out_plane = out_plane;
    c.out_co = out_co;
    c.cout = cout;
    c.k = k;
    c.stride = stride;
    c.leaky = bn ? 1 : 0;
    c.ups = ups;
    c.res_plane = res_plane;
    c.res_co = res_co;
    c.is_stem = (cin == 3);
    c.p_gamma = c.p_beta = c.p_mean = c.p_var = c.p_bias = -1;
    c.scale_off = c.shift_off = -1;
    const int wshape[4] = {cout, cin, k, k};
    const int cshape[1] = {cout};
    if (bn) {
      c.p_weight = add_param(name + ".0.weight", VY_P_WEIGHT, 4, wshape, 1, backbone);
      c.p_gamma = add_param(name + ".1.gamma", VY_P_GAMMA, 1, cshape, 1, backbone);
      c.p_beta = add_param(name + ".1.beta", VY_P_BETA, 1, cshape, 1, backbone);
      c.p_mean = add_param(name + ".1.running_mean", VY_P_RUNNING_MEAN, 1, cshape, 0, backbone);
      c.p_var = add_param(name + ".1.running_var", VY_P_RUNNING_VAR, 1, cshape, 0, backbone);
    } else {
      c.p_weight = add_param(name + ".weight", VY_P_WEIGHT, 4, wshape, 1, backbone);
      c.p_bias = add_param(name + ".bias", VY_P_BIAS, 1, cshape, 1, backbone);
    }
    convs.push_back(c);
    return (int)convs.size() - 1;
  }

  void build() {
    char nm[128];
    const int layers[5] = {1, 2, 8, 8, 4};
    const int chans[6] = {32, 64, 128, 256, 512, 1024};
    const int C = num_class;
    const int npred = 3 * (5 + C);
    // concat planes of the two shallower heads: [upsampled transition | backbone route]
    const int cat1 = add_plane(256 + 512, 16);  // yolo3.py:1177 at stride 16
    const int cat2 = add_plane(128 + 256, 8);   // ... at stride 8
    // ---- Darknet-53 features (three_darknet.py:162-195), named by stage slice (wrappers.py:58)
    int feat = 0;  // index into features[]
    auto feat_name = [&](int f) {
      int si = f < 15 ? 0 : (f < 24 ? 1 : 2);
      int j = f - (si == 0 ? 0 : (si == 1 ? 15 : 24));
      snprintf(nm, sizeof nm, "stages.%d.%d", si, j);
      return std::string(nm);
    };
    routes[0] = {cat2, 128, 256};
    routes[1] = {cat1, 256, 512};
    int bfm = clip_net() ? window_k : hier_frames();  // frames per batch entry of the backbone planes (falls at a hier pool)
    int cur = add_plane(heads_only ? 1024 : 32, heads_only ? 32 : 1, bfm), cur_co = 0;
    if (!heads_only) add_conv(feat_name(feat++), -1, 0, 3, cur, 0, 32, 3, 1, true, 1);
    int div = 1;
    for (int st = 0; st < 5 && !heads_only; ++st) {
      const int ch = chans[st + 1];
      if (st < hier_n) {  // pool point: the frames of `cur` by threes into a plane that this stage's stride-2 conv reads
        bfm /= 3;
        HierPool hp;
        hp.src = cur;
        hp.C = chans[st];
        hp.conv = (int)convs.size();
        hp.join = hier_join;
        if (st == 3) {  // the fourth pooled plane is route 0: straight into the place a single-frame backbone writes it
          hp.dst = cat2;
          hp.dst_co = 128;
        } else {
          hp.dst = add_plane(chans[st], div, bfm);
          hp.dst_co = 0;
        }
        hpools.push_back(hp);
        cur = hp.dst;
        cur_co = hp.dst_co;
      }
      div *= 2;
      int nxt = add_plane(ch, div, bfm);
      add_conv(feat_name(feat++), cur, cur_co, chans[st], nxt, 0, ch, 3, 2, true, 1);
      cur = nxt;
      cur_co = 0;
      for (int bi = 0; bi < layers[st]; ++bi) {
        const std::string pre = feat_name(feat++);
        const int mid = add_plane(ch / 2, div, bfm);
        add_conv(pre + ".body.0", cur, cur_co, ch, mid, 0, ch / 2, 1, 1, true, 1);
        // the last block of stages 0 and 1 (features[14], features[23]) writes the route straight
        // into its concat plane (a window net: into a per-frame route plane, pooled into the concat plane later)
        int outp, outco = 0;
        if (clip_net() && (feat - 1 == 14 || feat - 1 == 23)) {
          outp = add_plane(ch, div, bfm);
          frame_routes[feat - 1 == 14 ? 0 : 1] = outp;
        } else if (feat - 1 == 14 && hier_n < 4) {  // (four pools: route 0 is pooled into cat2 out of a plane of its own)
          outp = cat2;
          outco = 128;
        } else if (feat - 1 == 23) {
          outp = cat1;
          outco = 256;
        } else {
          outp = add_plane(ch, div, bfm);
        }
        add_conv(pre + ".body.1", mid, 0, ch / 2, outp, outco, ch, 3, 1, true, 1, cur, cur_co);
        cur = outp;
        cur_co = outco;
      }
    }
    if (clip_net()) {  // the heads read the pooled stride-32 route
      frame_routes[2] = cur;
      cur = add_plane(1024, 32);
      cur_co = 0;
    }
    routes[2] = {cur, cur_co, 1024};
    // ---- heads, deep -> shallow (yolo3.py:1013-1054, 1126-1177)
    const int hch[3] = {512, 256, 128};
    const int hdiv[3] = {32, 16, 8};
    int x = cur, x_co = cur_co, x_c = 1024;
    for (int i = 0; i < 3; ++i) {
      const int ch = hch[i], dv = hdiv[i];
      for (int j = 0; j < 5; ++j) {
        snprintf(nm, sizeof nm, "yolo_blocks.%d.body.%d", i, j);
        const int oc = (j % 2 == 0) ? ch : ch * 2;
        const int op = add_plane(oc, dv);
        add_conv(nm, x, x_co, x_c, op, 0, oc, (j % 2 == 0) ? 1 : 3, 1, true, 0);
        x = op;
        x_co = 0;
        x_c = oc;
      }
      const int route = x;
      snprintf(nm, sizeof nm, "yolo_blocks.%d.tip", i);
      const int tip = add_plane(ch * 2, dv);
      add_conv(nm, route, 0, ch, tip, 0, ch * 2, 3, 1, true, 0);
      snprintf(nm, sizeof nm, "yolo_outputs.%d.prediction", i);
      // channel stride padded to 32 so the plane can be the A operand of the prediction conv's dgrad
      head_plane[i] = add_plane((npred + 31) & ~31, dv);
      add_conv(nm, tip, 0, ch * 2, head_plane[i], 0, npred, 1, 1, false, 0);
      if (i == 2) break;
      // transition 1x1 (c -> c/2) stored x2-replicated into channels [0, c/2) of the concat plane
      snprintf(nm, sizeof nm, "transitions.%d", i);
      const int cat = (i == 0) ? cat1 : cat2;
      add_conv(nm, route, 0, ch, cat, 0, ch / 2, 1, 1, true, 0, -1, 0, 2);
      x = cat;
      x_co = 0;
      x_c = planes[cat].C;
    }
    while (n_backbone < (int)convs.size() && params[convs[n_backbone].p_weight].info.backbone) ++n_backbone;
    // the conv joins' tensors, behind the last single-frame parameter: a `_conv2d` cell's five, part of the backbone
    // (wrappers.py:50-52 freezes d_model whole).  Library shape (C, 3): the reference's (C, 1, 3, 1, 1)
    for (size_t i = 0; i < hpools.size(); ++i) {
      HierPool& hp = hpools[i];
      if (hp.join != VY_HJOIN_CONV) continue;
      const std::string pre = "hjoin." + std::to_string(i);
      const int wshape[2] = {hp.C, 3}, cshape[1] = {hp.C};
      hp.p_weight = add_param(pre + ".0.weight", VY_P_WEIGHT, 2, wshape, 1, 1);
      hp.p_gamma = add_param(pre + ".1.gamma", VY_P_GAMMA, 1, cshape, 1, 1);
      hp.p_beta = add_param(pre + ".1.beta", VY_P_BETA, 1, cshape, 1, 1);
      hp.p_mean = add_param(pre + ".1.running_mean", VY_P_RUNNING_MEAN, 1, cshape, 0, 1);
      hp.p_var = add_param(pre + ".1.running_var", VY_P_RUNNING_VAR, 1, cshape, 0, 1);
    }
    tensor_elems = param_elems;
    // folded-BN scratch behind the tensors
    for (auto& c : convs) {
      if (c.p_gamma < 0) continue;
      c.scale_off = param_elems;
      param_elems += (c.cout + 63) & ~63;
      c.shift_off = param_elems;
      param_elems += (c.cout + 63) & ~63;
      FoldDesc f;
      f.gamma = params[c.p_gamma].info.offset;
      f.beta = params[c.p_beta].info.offset;
      f.mean = params[c.p_mean].info.offset;
      f.var = params[c.p_var].info.offset;
      f.scale = c.scale_off;
      f.shift = c.shift_off;
      f.C = c.cout;
      f.pad = 0;
      folds.push_back(f);
    }
    for (HierPool& hp : hpools) {  // ... and the joins' BatchNorms behind the cells' (folds[0] stays the stem's)
      if (hp.join != VY_HJOIN_CONV) continue;
      hp.scale_off = param_elems;
      param_elems += (hp.C + 63) & ~63;
      hp.shift_off = param_elems;
      param_elems += (hp.C + 63) & ~63;
      FoldDesc f;
      f.gamma = params[hp.p_gamma].info.offset;
      f.beta = params[hp.p_beta].info.offset;
      f.mean = params[hp.p_mean].info.offset;
      f.var = params[hp.p_var].info.offset;
      f.scale = hp.scale_off;
      f.shift = hp.shift_off;
      f.C = hp.C;
      f.pad = 0;
      folds.push_back(f);
    }
  }

  // ---- planning
  static size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

  // which inference launches the split-fp32 kernel takes in conv mode VY_CONV_SPLIT_BF16X3: every conv+BN+leaky cell
  // whose tile geometry it has (cout a multiple of 64, cin of 32) — the 3x3 cells (1.4-1.5x the exact kernel at
  // 608x608 batch 64; the two 64-channel ones 1.15x) and the 1x1 cells (1.13x at K = 128 ... 1.5x at K = 1024).
  // The stem (Cin = 3), the 64 -> 32 bottleneck and the prediction convs (75 channels) stay on the exact kernel.
  bool split_eligible(const ConvT& c) const {
    if (conv_mode == VY_CONV_EXACT_FP32 || c.is_stem || c.p_gamma < 0) return false;
    return c.cout % 64 == 0 && c.cin % 32 == 0;
  }

  // Plane -> storage slot.  keep_all (training, or vy_net_set_keep_activations): every plane has its own storage — the
  // backward pass (and the parity taps) read them all.  Otherwise planes are recycled by liveness: a plane may take over
  // the storage of an earlier plane of the SAME geometry (channel stride and resolution: the zero borders coincide and
  // stay zero, the interior is fully overwritten by the producing conv) once every reader of that plane has been
  // launched — strictly before the new plane's first writer, because a conv reads its input / addend while it writes.
  // In a residual stage that is two alternating block-output planes and one bottleneck plane instead of 2 x blocks.
  std::vector<int> plane_slots(bool keep_all) const {
    const int np = (int)planes.size();
    std::vector<int> slot(np);
    for (int i = 0; i < np; ++i) slot[i] = i;
    if (keep_all) return slot;
    const int kLive = 1 << 30;
    std::vector<int> def(np, kLive), last(np, -1);
    for (int ci = 0; ci < (int)convs.size(); ++ci) {
      const ConvT& c = convs[ci];
      if (c.out_plane >= 0 && ci < def[c.out_plane]) def[c.out_plane] = ci;
      if (c.in_plane >= 0 && ci > last[c.in_plane]) last[c.in_plane] = ci;
      if (c.res_plane >= 0 && ci > last[c.res_plane]) last[c.res_plane] = ci;
    }
    for (int i = 0; i < 3; ++i) last[head_plane[i]] = kLive;  // read by decode + NMS (and vy_net_read_head) afterwards
    if (heads_only || window_k)  // the routes are imported / pooled outside the conv list: those planes own their storage
      for (int i = 0; i < 3; ++i) def[routes[i].plane] = -1;
    if (clip_net())  // ... and window_pool reads the per-frame routes after the last stage cell
      for (int i = 0; i < 3; ++i) last[frame_routes[i]] = kLive;
    for (const HierPool& hp : hpools) {  // a pool runs in front of its conv: it writes dst, and src stays live up to it
      def[hp.dst] = std::min(def[hp.dst], hp.conv);
      last[hp.src] = std::max(last[hp.src], hp.conv);
    }
    std::vector<int> order(np);
    for (int i = 0; i < np; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return def[a] < def[b]; });
    std::vector<int> free_at(np, -1);  // per slot (= index of the plane that owns the storage): last reader so far
    std::vector<int> owners;
    for (int p : order) {
      int take = -1;
      // a prediction plane never takes over a freed plane: its conv writes npred of the C (padded) channels and the
      // padding must stay the zeros of the bind-time memset (80 classes: 255 -> 256 channels, the geometry of the
      // stage-1 bottleneck planes)
      const bool is_head = p == head_plane[0] || p == head_plane[1] || p == head_plane[2];
      for (int o : owners)
        if (!is_head && planes[o].C == planes[p].C && planes[o].div == planes[p].div && planes[o].fm == planes[p].fm &&
            free_at[o] < def[p]) {
          take = o;
          break;
        }
      if (take < 0) {
        take = p;
        owners.push_back(p);
      }
      slot[p] = take;
      free_at[take] = last[p];
    }
    return slot;
  }

  // what join `i` of a hierarchical net is called: as a tap, a launch label and in the region table
  std::string join_name(int i) const { return (hier_join == VY_HJOIN_CONV ? "hjoin." : "hpool.") + std::to_string(i); }

  // what a plane is called in the region table: the first cell that writes it, else the pool of a hierarchical net that
  // does, else the route that is imported / pooled into it
  std::string plane_name(int p) const {
    for (const ConvT& c : convs)
      if (c.out_plane == p) return c.name;
    for (size_t i = 0; i < hpools.size(); ++i)
      if (hpools[i].dst == p) return join_name((int)i);
    for (int i = 0; i < 3; ++i)
      if (routes[i].plane == p) return "route." + std::to_string(i);
    return "plane." + std::to_string(p);
  }

  // frames / ring: a video plan (vy_net_bind_video) — `frames` single frames in the stem and stage planes instead of b*k,
  // b clips from the pooled routes on, and `ring` route slots behind the planes; 0, 0: the clip plan.
  // hstep: a hier-video plan (vy_net_bind_hier_video) — b centres, every backbone plane at its level's count (frames_of).
  // regions (tests: vy_net_plan_region): every carve is appended to it, in offset order
  NetPlan plan(int b, int h, int w, bool keep_all, int frames = 0, int ring = 0, std::vector<PlanRegion>* regions = nullptr,
               int hstep = 0) const {
    NetPlan p;
    p.B = b;
    p.hier_step = hstep;
    p.H = h;
    p.W = w;
    p.planes_shared = !keep_all;
    p.guard = knobs.plan_guard;
    size_t off = 0;
    // one carve: `bytes` at the running offset, rounded up to 256, then the guard gap; no bytes, no carve
    auto take = [&](size_t bytes, const char* kind, const std::string& what = std::string()) {
      const size_t at = off;
      if (!bytes) return at;
      if (regions) regions->push_back({what.empty() ? std::string(kind) : kind + (":" + what), at, bytes});
      off += al(bytes) + (size_t)p.guard;
      return at;
    };
    p.fold_desc_off = take(sizeof(FoldDesc) * folds.size(), "fold");
    p.det_scratch_off = off;
    int n_items = 0;
    // a plane's spatial size = ceil(input / div): every stride-2 3x3 pad-1 conv maps n rows to ceil(n / 2), and the
    // x2 upsample is cropped to the route it is concatenated with (slice_like, yolo3.py:1177) — inputs need not be
    // multiples of 32
    auto cdiv = [](int a, int d) { return (a + d - 1) / d; };
    for (int i = 0; i < 3; ++i) n_items += 3 * cdiv(h, planes[head_plane[i]].div) * cdiv(w, planes[head_plane[i]].div);
    {  // the detection scratch carves its five sub-regions itself (detect.hip)
      static const char* const kDet[5] = {"det.state", "det.hist", "det.entries", "det.list", "det.score"};
      size_t d_off[5], d_used[5];
      const size_t det_bytes = vy_det_scratch_layout(b, n_items, num_class, p.guard, d_off, d_used);
      for (int i = 0; i < 5 && regions; ++i) regions->push_back({kDet[i], off + d_off[i], d_used[i]});
      off += det_bytes;
    }
    p.sk_off = take((size_t)VY_SK_FLAGS * sizeof(unsigned), "sk.flags");
    p.sk_slabs_off = take(VY_SK_PARTIAL_BYTES, "sk.slabs");
    // parked chains of the convs whose K is summed in runs (vy_conv_k_chunks; conv_igemm.hip `boundary`): runs - 1 tile-shaped
    // slabs per output tile of the conv that needs most
    for (const ConvT& c : convs) {
      const int runs = c.is_stem ? 1 : vy_conv_runs(c.k * c.k, (c.cin + 31) >> 5);
      if (runs < 2) continue;
      const PlaneT& op = planes[c.out_plane];
      const long long Mo = (long long)frames_of(op, b, frames, hstep) * cdiv(h, op.div) * cdiv(w, op.div);
      p.ck_bytes = std::max(p.ck_bytes, vy_conv_chunk_scratch_bytes(Mo, c.cout, runs));
    }
    p.ck_off = take(p.ck_bytes, "ck");
    p.wsplit_off = off;  // split-fp32 weight images (conv mode VY_CONV_SPLIT_BF16X3 only)
    p.convs.resize(convs.size());
    for (size_t i = 0; i < convs.size(); ++i) {
      const ConvT& c = convs[i];
      if (!split_eligible(c)) continue;
      p.convs[i].split_off = (int64_t)(take(vy_split_weight_bytes(c.cout, c.k * c.k, c.cin), "wsplit", c.name) - p.wsplit_off);
      if (c.k == 3 && c.stride == 1 && c.ups == 1 && c.cout % 128 == 0)
        p.convs[i].wino_off = (int64_t)(take(vy_wino_weight_bytes(c.cout, c.cin), "wino", c.name) - p.wsplit_off);
    }
    p.planes_off = off;
    const std::vector<int> slot = plane_slots(keep_all);
    p.planes.resize(planes.size());
    for (size_t i = 0; i < planes.size(); ++i) {
      const PlaneT& g = planes[i];
      NetPlan::Plane& q = p.planes[i];
      q.H = cdiv(h, g.div);
      q.W = cdiv(w, g.div);
      if ((size_t)slot[i] == i)  // owns its storage
        q.off = (take((size_t)frames_of(g, b, frames, hstep) * (q.H + 2) * (q.W + 2) * g.C * sizeof(float), "plane",
                      regions ? plane_name((int)i) : std::string()) - p.planes_off) / sizeof(float);
    }
    for (size_t i = 0; i < planes.size(); ++i) p.planes[i].off = p.planes[slot[i]].off;  // (an owner may come later)
    p.ring_off = off;
    if (ring > 0) {
      p.video_F = frames;
      p.video_R = ring;
      p.ring_slot_floats = slot_floats(h, w);
      take((size_t)ring * p.ring_slot_floats * sizeof(float), "ring");
    }
    p.total = off;
    return p;
  }

  float* plane_ptr(int i) const { return reinterpret_cast<float*>(dev_ws + cur.planes_off) + cur.planes[i].off; }

  // video_ok: the entry also serves a net bound for video (the video entries, the taps); every other entry runs the clip plan
  int check_ready(bool video_ok = false) const {
    if (!dev_params) return fail(VY_ERR_STATE, "parameters not bound (vy_net_bind_params)");
    if (!dev_ws) return fail(VY_ERR_STATE, "workspace not bound (vy_net_bind_workspace)");
    if ((cur.video_F || cur.hier_step) && !video_ok)
      return fail(VY_ERR_STATE, "the net is bound for video (%s): bind a clip plan again with "
                  "vy_net_bind_workspace / vy_net_bind_train", cur.hier_step ? "vy_net_bind_hier_video" : "vy_net_bind_video");
    return 0;
  }

  // forward launch of conv `ci`: reads plane views, writes `out_plane_ptr` (the activation plane, or
  // the raw-conv "z" plane in training)
  ConvArgs conv_args(int ci) const {
    ConvArgs a;
    memset(&a, 0, sizeof a);
    const ConvT& c = convs[ci];
    const PlaneAt ip = plane(c.in_plane);
    const PlaneAt op = plane(c.out_plane);
    a.in = plane_ptr(c.in_plane);
    a.w = dev_params + params[c.p_weight].info.offset;
    if (c.p_gamma >= 0) {
      a.scale = dev_params + c.scale_off;
      a.shift = dev_params + c.shift_off;
    } else {
      a.scale = nullptr;
      a.shift = dev_params + params[c.p_bias].info.offset;
    }
    a.res = c.res_plane >= 0 ? plane_ptr(c.res_plane) : nullptr;
    a.out = plane_ptr(c.out_plane);
    a.stats = nullptr;
    const int Ho = (ip.H + c.stride - 1) / c.stride, Wo = (ip.W + c.stride - 1) / c.stride;
    const int Bf = conv_batch(c);
    a.B = Bf;
    a.LH = Ho;
    a.LW = Wo;
    a.M = Bf * Ho * Wo;
    a.a_Hp = ip.H + 2;
    a.a_Wp = ip.W + 2;
    a.a_cs = ip.C;
    a.a_co = c.in_co;
    a.a_s = c.stride;
    a.a_oy = a.a_ox = 1;
    a.Kc = c.cin;
    a.ntaps = c.k * c.k;
    for (int t = 0; t < a.ntaps; ++t) {
      a.tap_dy[t] = (signed char)(c.k == 3 ? t / 3 - 1 : 0);
      a.tap_dx[t] = (signed char)(c.k == 3 ? t % 3 - 1 : 0);
      a.tap_w[t] = (unsigned char)t;
    }
    a.w_taps = c.k * c.k;
    a.w_cin = c.cin;
    a.w_cout = c.cout;
    a.N = c.cout;
    a.o_Hp = op.H + 2;  // ups == 2: the route's size, which may be one short of 2 x (Ho, Wo) — the store crops
    a.o_Wp = op.W + 2;
    a.o_cs = op.C;
    a.o_co = c.out_co;
    a.o_s = c.ups;
    a.o_oy = a.o_ox = 1;
    a.ups = c.ups;
    if (c.res_plane >= 0) {
      a.r_cs = planes[c.res_plane].C;
      a.r_co = c.res_co;
    }
    a.leaky = c.leaky;
    a.dgrad = 0;
    const NetPlan::Conv& im = cur.convs[ci];
    a.w_split = im.split_off >= 0 ? dev_ws + cur.wsplit_off + im.split_off : nullptr;
    a.w_wino = im.wino_off >= 0 ? dev_ws + cur.wsplit_off + im.wino_off : nullptr;
    launch_env(a, /*k_runs=*/true, /*splitk=*/true);
    return a;
  }

  // the stem launch of conv `c` on the image batch `x`: the folded BatchNorm affine into the activation plane (run_cells adds
  // the fold that may ride in it; the training forward turns it into the raw launch that writes z)
  StemArgs stem_args(const ConvT& c, const float* x) const {
    StemArgs a;
    a.x = x;
    a.w = dev_params + params[c.p_weight].info.offset;
    a.scale = dev_params + c.scale_off;
    a.shift = dev_params + c.shift_off;
    a.out = plane_ptr(c.out_plane);
    a.B = conv_batch(c);
    a.H = cur.H;
    a.W = cur.W;
    a.Cout = c.cout;
    a.out_cs = planes[c.out_plane].C;
    a.out_co = c.out_co;
    a.cus = cus;
    return a;
  }

  // `plan` comes into force in the workspace `ws`, of whose `bytes` it (and what a training plan carved behind it) uses
  // `need`: every image set is stale, the fold table gone; zero the bytes in use (all stream-K flags down) and probe the
  // device's workgroup placement.  A training plan carved behind an earlier commit is void from here on (bound_train)
  int commit_bind(NetPlan&& plan, void* ws, size_t bytes, size_t need, hipStream_t s) {
    cur = std::move(plan);
    ++commits;
    dev_ws = static_cast<unsigned char*>(ws);
    ws_bytes = bytes;
    split_dirty = dsplit_dirty = wino_dirty = true;
    fold_uploaded = false;
    HIP_TRY(hipMemsetAsync(ws, 0, need, s));
    sk_dirty = false;
    sk_ok = vy_sk_verify_topology(reinterpret_cast<unsigned*>(dev_ws + cur.sk_off), s) != 0;
    return 0;
  }
  // a setting the plan depends on changed: the workspace has to be sized and bound again
  void unbind() {
    dev_ws = nullptr;
    ws_bytes = 0;
  }

  int sk_begin(hipStream_t s) {
    if (sk_dirty && dev_ws) {
      HIP_TRY(hipMemsetAsync(dev_ws + cur.sk_off, 0, (size_t)VY_SK_FLAGS * sizeof(unsigned), s));
      sk_dirty = false;
    }
    return 0;
  }
  int sk_end(int rc) {
    if (rc != 0) sk_dirty = true;
    return rc;
  }

  // The launch environment of a conv launch, forward or data gradient: the net's switches and CU count (the cost models read
  // them) and the scratch it may use — k_runs: the parked chains of a K summed in runs; splitk: the split-fp32 kernel's
  // split-K slabs (in the stream-K region); and the stream-K scratch of this net's workspace (zeroed at bind time: all flags
  // down), left null — plain launches only — unless the device's workgroup placement was verified
  void launch_env(ConvArgs& a, bool k_runs, bool splitk) const {
    a.knobs = &knobs;
    a.cus = cus;
    float* const sk_slabs = reinterpret_cast<float*>(dev_ws + cur.sk_slabs_off);
    if (k_runs) {
      a.ck_scratch = cur.ck_bytes ? reinterpret_cast<float*>(dev_ws + cur.ck_off) : nullptr;
      a.ck_bytes = cur.ck_bytes;
    }
    if (splitk) {
      a.splitk_slabs = sk_slabs;
      a.splitk_bytes = VY_SK_PARTIAL_BYTES;
    }
    if (!sk_ok) return;
    a.sk_flags = reinterpret_cast<unsigned*>(dev_ws + cur.sk_off);
    a.sk_partials = sk_slabs;
    a.sk_bytes = VY_SK_PARTIAL_BYTES;
    a.sk_nflags = VY_SK_FLAGS;
  }

  // the three route slices of the bound plan and the caller's dense NCHW tensors (routes.hip)
  RouteArgs route_args(const float* const* nchw) const {
    RouteArgs r;
    memset(&r, 0, sizeof r);
    r.n = 3;
    r.B = cur.B;
    for (int i = 0; i < 3; ++i) {
      const PlaneAt p = plane(routes[i].plane);
      r.r[i].plane = plane_ptr(routes[i].plane);
      r.r[i].nchw = const_cast<float*>(nchw[i]);
      r.r[i].H = p.H;
      r.r[i].W = p.W;
      r.r[i].C = routes[i].C;
      r.r[i].cs = p.C;
      r.r[i].co = routes[i].co;
    }
    return r;
  }

  DetArgs det_args() const {
    DetArgs d;
    memset(&d, 0, sizeof d);
    int base = 0;
    for (int i = 0; i < 3; ++i) {
      const PlaneAt p = plane(head_plane[i]);
      HeadView& hv = d.head[i];
      hv.pred = plane_ptr(head_plane[i]);
      hv.H = p.H;
      hv.W = p.W;
      hv.cs = p.C;
      hv.co = 0;
      hv.stride = (float)kStrides[2 - i];  // anchors/strides used in reverse order, yolo3.py:1013
      for (int a = 0; a < 3; ++a) {
        hv.aw[a] = (float)kAnchors[2 - i][2 * a];
        hv.ah[a] = (float)kAnchors[2 - i][2 * a + 1];
      }
      hv.cand_base = base;
      base += num_class * p.H * p.W * 3;
    }
    d.B = cur.B;
    d.C = num_class;
    d.n_cand = base;
    d.valid_thresh = 0.01f;  // yolo3.py:1199
    d.nms_thresh = nms_thresh;
    d.topk = nms_topk;
    d.post_nms = post_nms;
    d.valid_ge = sem.nms_valid_ge;
    d.overlap_ge = sem.nms_overlap_ge;
    d.tie_desc = sem.nms_tie_descending;
    d.topk_after = sem.nms_topk_after;
    d.iou_plus1 = sem.nms_iou_plus_one;
    d.guard = cur.guard;
    return d;
  }

  // ---- the steps of an inference launch sequence; the entry points of net.hip put them together.  `hook` is called around
  // every launch (vy_net_profile_infer: an event on either side); NoHook = the plain path, which builds no label
  template <typename Hook>
  static constexpr bool kLabels = !std::is_same<Hook, NoHook>::value;

  // In front of the first cell: the one-time fold-table upload, the BatchNorm fold, the weight images of the split modes.
  // stem_runs: the sequence launches the stem, which then carries the fold if it can (run_cells reads fold_in_stem)
  template <typename Hook>
  int prepare(hipStream_t s, Hook& hook, bool stem_runs) {
    FoldDesc* fd = reinterpret_cast<FoldDesc*>(dev_ws + cur.fold_desc_off);
    if (!fold_uploaded) {
      HIP_TRY(hipMemcpyAsync(fd, folds.data(), sizeof(FoldDesc) * folds.size(), hipMemcpyHostToDevice, s));
      HIP_TRY(hipStreamSynchronize(s));  // `folds` is pageable host memory; one-time
      fold_uploaded = true;
    }
    // The fold runs EVERY forward (the caller owns the parameter buffer and may have written to it) — inside the stem launch
    // when that has a block per layer (StemArgs), in a launch of its own otherwise
    fold_in_stem = stem_runs && !convs.empty() && convs[0].is_stem && convs[0].scale_off == folds[0].scale &&
                   vy_stem_can_fold(conv_batch(convs[0]), cur.H, cur.W, (int)folds.size(), cus);
    if (!fold_in_stem) HOOKED(hook, "bn_fold", 0.0, 0.0, vy_launch_bn_fold(dev_params, fd, (int)folds.size(), 1024, 1e-5f, s));
    if (conv_mode != VY_CONV_EXACT_FP32 && (split_dirty || wino_dirty)) {  // once per parameter change, not per forward
      hook("split_weights", 0.0, 0.0, true);
      unsigned char* const images = dev_ws + cur.wsplit_off;
      for (size_t i = 0; i < convs.size(); ++i)
        if (const ConvT& c = convs[i]; split_dirty && cur.convs[i].split_off >= 0)
          HIP_TRY(vy_launch_split_weights(dev_params + params[c.p_weight].info.offset, images + cur.convs[i].split_off, c.cout,
                                          c.k * c.k, c.cin, s));
      for (size_t i = 0; i < convs.size(); ++i)
        if (const ConvT& c = convs[i]; wino_dirty && cur.convs[i].wino_off >= 0)
          HIP_TRY(vy_launch_wino_weights(dev_params + params[c.p_weight].info.offset, images + cur.convs[i].wino_off, c.cout,
                                         c.cin, s));
      hook("split_weights", 0.0, 0.0, false);
      split_dirty = wino_dirty = false;
    }
    return 0;
  }

  // the cells [first, last) of the conv list; x: the image batch the stem reads (unused unless the span holds it)
  template <typename Hook>
  int run_cells(int first, int last, const float* x, hipStream_t s, Hook& hook) {
    for (int ci = first; ci < last; ++ci) {
      const ConvT& c = convs[ci];
      if (c.is_stem) {
        StemArgs a = stem_args(c, x);
        const int Bs = a.B;
        if (fold_in_stem) {
          a.fold_params = dev_params;
          a.fold_descs = reinterpret_cast<FoldDesc*>(dev_ws + cur.fold_desc_off);
          a.fold_n = (int)folds.size();
          a.fold_stem = 0;
          a.fold_eps = 1e-5f;
        }
        const double fl = kLabels<Hook> ? 2.0 * Bs * a.H * a.W * 27.0 * c.cout : 0.0;
        const double by = kLabels<Hook> ? 4.0 * Bs * a.H * a.W * (3.0 + c.cout) : 0.0;
        HOOKED(hook, c.name.c_str(), fl, by, vy_launch_stem(a, s));
        continue;
      }
      const ConvArgs a = conv_args(ci);
      const VyConvPlan plan = vy_conv_plan(a);
      if (!kLabels<Hook>) {  // plain forward: no label (batch-1 latency path)
        HIP_TRY(vy_launch_conv(a, plan, s));
        continue;
      }
      const double fl = 2.0 * a.M * (double)a.N * a.ntaps * a.Kc;
      const double by = 4.0 * ((double)a.B * (a.a_Hp - 2) * (a.a_Wp - 2) * a.Kc + (double)a.M * a.N * a.ups * a.ups +
                               (double)a.N * a.ntaps * a.Kc + (a.res ? (double)a.M * a.N : 0.0));
      char form[32], nm[96];
      vy_conv_plan_label(plan, VY_LABEL_PROFILE, form, sizeof form);
      snprintf(nm, sizeof nm, "%s|%s", c.name.c_str(), form);
      HOOKED(hook, nm, fl, by, vy_launch_conv(a, plan, s));
    }
    return 0;
  }

  // heads-only nets: the caller's three route tensors into the planes the first head cells read
  template <typename Hook>
  int route_import(const float* const* nchw, hipStream_t s, Hook& hook) {
    HOOKED(hook, "route_import", 0.0, 0.0, vy_launch_route_import(route_args(nchw), s));
    return 0;
  }
  // windowed heads-only nets (the caller has checked the table): each clip's k frames of the bank, pooled, into the same planes
  template <typename Hook>
  int import_pool(const BankRef& bank, hipStream_t s, Hook& hook) {
    RoutePoolArgs ra;
    memset(&ra, 0, sizeof ra);
    const RouteArgs r = route_args(bank.f);
    double floats = 0;
    for (int i = 0; i < 3; ++i) {
      ra.r[i] = r.r[i];
      floats += (double)r.r[i].C * r.r[i].H * r.r[i].W;
    }
    ra.n = 3;
    ra.B = cur.B;
    ra.k = window_k;
    ra.join = window_join;
    ra.T = bank.n_frames;
    memcpy(ra.table, bank.table, sizeof(int32_t) * cur.B * window_k);
    HOOKED(hook, "route_import_pool", 0.0, 4.0 * (window_k + 1) * cur.B * floats, vy_launch_route_import_pool(ra, s));
    return 0;
  }
  // full nets, after the last stage cell: the three routes out to the caller's tensors
  template <typename Hook>
  int route_export(const float* const* nchw, hipStream_t s, Hook& hook) {
    HOOKED(hook, "route_export", 0.0, 0.0, vy_launch_route_export(route_args(nchw), s));
    return 0;
  }
  // window nets, clip plan: the stages are done, pool the per-frame routes of each clip
  template <typename Hook>
  int window_pool(hipStream_t s, Hook& hook) {
    HOOKED(hook, "window_pool", 0.0, 0.0, vy_launch_window_pool(pool_args(nullptr), s));
    return 0;
  }
  // hierarchical nets: join `i` — the max, or the conv join with its folded BatchNorm — in front of the conv that reads the
  // pooled plane
  template <typename Hook>
  int hier_pool(int i, hipStream_t s, Hook& hook) {
    const HierPoolArgs a = hier_args(hpools[i], nullptr);
    // three reads, one write, either join; a dilated join (a hier-video plan): its algorithmic bytes — the source plane's
    // frames + 2 dil frames once, the destination once
    const double by = 4.0 * (a.dil ? 2.0 * (a.frames + a.dil) : 4.0 * a.frames) * a.H * a.W * a.C;
    char nm[16];
    if (hpools[i].join == VY_HJOIN_CONV) {
      snprintf(nm, sizeof nm, "hjoin.%d", i);
      const HierJoinArgs j = join_args(hpools[i], nullptr);
      HOOKED(hook, nm, 6.0 * a.frames * a.H * a.W * a.C, by,
             a.dil ? vy_launch_hier_join_dilated(j, knobs.hier_chain, s) : vy_launch_hier_join(j, s));
      return 0;
    }
    snprintf(nm, sizeof nm, "hpool.%d", i);
    HOOKED(hook, nm, 0.0, by, a.dil ? vy_launch_hier_pool_dilated(a, knobs.hier_chain, s) : vy_launch_hier_pool(a, s));
    return 0;
  }
  // the backbone: the stem and stage cells, with the pools of a hierarchical net between the groups they separate
  template <typename Hook>
  int run_backbone(const float* x, hipStream_t s, Hook& hook) {
    int first = 0;
    for (int i = 0; i < (int)hpools.size(); ++i) {
      VY_TRY(run_cells(first, hpools[i].conv, x, s, hook));
      VY_TRY(hier_pool(i, s, hook));
      first = hpools[i].conv;
    }
    return run_cells(first, n_backbone, x, s, hook);
  }
  // video plans (the caller has checked the tables): pool the B clips of `table` out of the ring ...
  template <typename Hook>
  int ring_pool(const int32_t* table, hipStream_t s, Hook& hook) {
    RingPoolArgs ra;
    memset(&ra, 0, sizeof ra);
    ring_routes(ra.r);
    ra.n = 3;
    ra.B = cur.B;
    ra.k = window_k;
    ra.join = window_join;
    ra.R = cur.video_R;
    ra.slot_stride = cur.ring_slot_floats;
    memcpy(ra.table, table, sizeof(int32_t) * cur.B * window_k);
    HOOKED(hook, "ring_pool", 0.0, 4.0 * (window_k + 1) * cur.B * cur.ring_slot_floats, vy_launch_ring_pool(ra, s));
    return 0;
  }
  // ... and store the routes of the video_F frames the stages just ran on in the slots `slots`
  template <typename Hook>
  int ring_push(const int32_t* slots, hipStream_t s, Hook& hook) {
    RingPushArgs ra;
    memset(&ra, 0, sizeof ra);
    ring_routes(ra.r);
    ra.n = 3;
    ra.F = cur.video_F;
    ra.R = cur.video_R;
    ra.slot_stride = cur.ring_slot_floats;
    memcpy(ra.slot, slots, sizeof(int32_t) * cur.video_F);
    HOOKED(hook, "ring_push", 0.0, 8.0 * cur.video_F * cur.ring_slot_floats, vy_launch_ring_push(ra, s));
    return 0;
  }

  // decode + NMS of the three prediction planes into the caller's outputs
  template <typename Hook>
  int detect_tail(float* ids, float* scores, float* bboxes, int32_t* keep_idx, hipStream_t s, Hook& hook) {
    const DetArgs d = det_args();
    double dby = 0;
    for (int i = 0; i < 3; ++i) dby += 4.0 * d.B * d.head[i].H * d.head[i].W * d.head[i].cs;
    const bool nms_on = nms_thresh > 0.f && nms_thresh < 1.f;  // yolo3.py:1197; off: the outputs are (B, N*C, .), the detection tensor itself
    HOOKED(hook, "decode_nms", 0.0, dby,
           nms_on ? vy_launch_detect(d, dev_ws + cur.det_scratch_off, ids, scores, bboxes, keep_idx, s)
                  : vy_launch_raw_detections(d, ids, scores, bboxes, keep_idx, s));
    return 0;
  }
};

// ---- the first line of every entry point that serves some kinds of net and not others: `kinds` is the set it serves.
// VY_ERR_STATE for a net of another kind (VY_ERR_INVALID for none), before any argument is looked at
inline int vy_serves(const vy_net* net, const char* entry, unsigned kinds) {
  static const struct {
    const char *name, *is;
  } k[5] = {{"full", "a full net (vy_net_create), which the entry points that take an image batch serve"},
            {"heads-only", "a heads-only net (vy_net_create_heads), which the *_routes entry points serve"},
            {"window", "a window net (vy_net_create_window), which vy_net_forward_infer, vy_net_train_*forward / _backward and "
                       "vy_net_video_* serve"},
            {"windowed heads-only", "a windowed heads-only net (vy_net_create_heads_window), which the *_bank entry points and "
                                    "vy_net_train_backward_routes serve"},
            {"hierarchical", "a hierarchical net (vy_net_create_hier), which vy_net_forward_infer, vy_net_profile_infer, "
                             "vy_net_train_*forward / _backward and vy_net_hier_video_* serve"}};
  if (!net) return fail(VY_ERR_INVALID, "%s: net is null", entry);
  const unsigned kind = net->kind();
  if (kind & kinds) return 0;
  std::string served;
  const char* is = "";
  for (int i = 0; i < 5; ++i) {
    if (kinds & (1u << i)) served += (served.empty() ? "" : " / ") + std::string(k[i].name);
    if (kind == (1u << i)) is = k[i].is;
  }
  return fail(VY_ERR_STATE, "%s serves a %s net: this is %s", entry, served.c_str(), is);
}

// ---- the frame of every entry point that launches a sequence of steps, inference (net.hip) and training (train.hip)
// The frame's checks, before anything is launched: arguments, bound, and for a video entry (named) bound for video
inline int entry_ready(vy_net* net, bool args_ok, const char* video_entry) {
  int rc = 0;
  if (!net || !args_ok) rc = fail(VY_ERR_INVALID, "null argument");
  if (rc == 0) rc = net->check_ready(video_entry != nullptr);
  if (rc == 0 && video_entry && !(net->hier_n ? net->cur.hier_step : net->cur.video_F))
    rc = fail(VY_ERR_STATE, "%s: the net is not bound for video (%s)", video_entry,
              net->hier_n ? "vy_net_bind_hier_video" : "vy_net_bind_video");
  if (rc && net) net->sk_dirty = true;  // (any error return: see vy_net::sk_dirty)
  return rc;
}
// ... then the stream-K flags zeroed if an earlier call left them dirty, and `run(stream)`: the launches
template <typename Run>
int run_entry(vy_net* net, bool args_ok, const char* video_entry, void* stream, Run&& run) {
  VY_TRY(entry_ready(net, args_ok, video_entry));
  hipStream_t s = static_cast<hipStream_t>(stream);
  int rc = net->sk_begin(s);
  if (rc == 0) rc = run(s);
  return net->sk_end(rc);
}

// VY_ERR_INVALID unless the bank and the table of a *_bank entry fit the bound plan: B * k table entries (they travel in the
// kernel arguments), each a frame of the bank.  Before anything is launched
inline int vy_check_bank(const vy_net* net, const char* entry, const BankRef& bank) {
  const long long n = (long long)net->cur.B * net->window_k;
  if (n > VY_ROUTE_TABLE_MAX)
    return fail(VY_ERR_INVALID, "%s: clips * k = %d x %d exceeds %d table entries (they travel in the kernel arguments)", entry,
                net->cur.B, net->window_k, VY_ROUTE_TABLE_MAX);
  if (bank.n_frames < 1) return fail(VY_ERR_INVALID, "%s: a bank of %d frames", entry, bank.n_frames);
  for (int i = 0; i < (int)n; ++i)
    if (bank.table[i] < 0 || bank.table[i] >= bank.n_frames)
      return fail(VY_ERR_INVALID, "%s: entry %d of the table is %d, outside [0, %d)", entry, i, bank.table[i], bank.n_frames);
  return 0;
}

// ---- what a tap name means, for every entry that takes one (vy_net_tap_frames, vy_net_read_activation; train.hip:
// vy_net_read_grad_activation, vy_net_read_train_tap): channels [co, co + C) of `plane`.  A cell's name is its output
// (conv: its index); "hpool.<i>" the plane pool i of a hierarchical net writes (hpool: i) — "hjoin.<i>" on a net with the
// conv join, which has no "hpool.*" as a max net has no "hjoin.*"; "pool.<i>" pooled route i of either window kind.  The frames the tap holds are the plane's, whatever it names: planes[plane].fm per batch entry,
// plane_batch(plane) in the bound plan
struct TapRef {
  int plane, co, C;
  int conv, hpool;  // -1: not a cell / not a pooled plane of a hierarchical net (either join: vy_net::hier_join says which)
};
// VY_ERR_INVALID if the net has no such tap
inline int vy_resolve_tap(const vy_net* net, const char* name, TapRef* t) {
  auto index = [name](const char* prefix, int n) {  // name = prefix + one digit below n: the digit, else -1
    const size_t len = strlen(prefix);
    return strncmp(name, prefix, len) == 0 && name[len] >= '0' && name[len] < '0' + n && !name[len + 1] ? name[len] - '0' : -1;
  };
  if (const int i = index(net->hier_join == VY_HJOIN_CONV ? "hjoin." : "hpool.", net->hier_n); i >= 0) {
    const vy_net::HierPool& hp = net->hpools[i];
    *t = {hp.dst, hp.dst_co, hp.C, -1, i};
    return 0;
  }
  if (const int i = index("pool.", net->window_k ? 3 : 0); i >= 0) {
    *t = {net->routes[i].plane, net->routes[i].co, net->routes[i].C, -1, -1};
    return 0;
  }
  for (int ci = 0; ci < (int)net->convs.size(); ++ci)
    if (const ConvT& cv = net->convs[ci]; cv.name == name) {
      *t = {cv.out_plane, cv.out_co, cv.cout, ci, -1};
      return 0;
    }
  return fail(VY_ERR_INVALID, "no cell named '%s'", name);
}
// the tap, out of the activation planes or (`grads`: their base, same offsets) the gradient planes, as dense NCHW
inline hipError_t vy_tap_to_nchw(const vy_net* net, const TapRef& t, float* grads, float* dst_dev, hipStream_t s) {
  const PlaneAt p = net->plane(t.plane);
  return vy_launch_plane_to_nchw(grads ? grads + p.off : net->plane_ptr(t.plane), net->plane_batch(t.plane), p.H, p.W, p.C,
                                 t.co, t.C, dst_dev, s);
}
