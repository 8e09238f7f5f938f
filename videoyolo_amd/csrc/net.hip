// net.hip — host side of libvyolo.so: the yolo3_darknet53 graph, parameter table, activation
// planner and the C-ABI of include/vyolo.h.
//
// The graph is the reference's (paths relative to /root/reference):
//   Darknet-53 stages       models/definitions/darknet/three_darknet.py:162-195, 252-258
//                           sliced features[:15] / [15:24] / [24:]  (yolo/wrappers.py:58)
//   detection blocks/heads  models/definitions/yolo/yolo3.py:218-263, 1013-1054
//   forward order           models/definitions/yolo/yolo3.py:1105-1206
// but it is executed as a flat list of fused launches over zero-bordered NHWC planes (kernels.h):
// conv+BN+leaky(+residual) is one kernel, upsample+concat costs nothing (the transition conv
// stores x2-replicated straight into the channel range [0,c) of the concat plane, whose range
// [c, ..) the backbone stage wrote in place), decode+NMS never materialises (B, N*C, 6).
#include "net_internal.h"

static thread_local std::string g_err;

#undef fail
int vy_fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
#define fail vy_fail

int vy_check_shape(int32_t batch, int32_t h, int32_t w) {
  if (batch < 1) return fail(VY_ERR_INVALID, "batch %d < 1", batch);
  if (h < 32 || w < 32 || h > 4096 || w > 4096)
    return fail(VY_ERR_INVALID, "input %dx%d: height and width must lie in [32, 4096]", h, w);
  return 0;
}

// the constructors: the checks they share, and the net itself (k = 0: not a window net)
static int check_create(int32_t num_class, vy_net** out) {
  if (!out) return fail(VY_ERR_INVALID, "out is null");
  if (num_class < 1 || num_class > 1000) return fail(VY_ERR_INVALID, "num_class %d out of range", num_class);
  return 0;
}
static vy_net* create(int32_t num_class, bool heads_only, int32_t k, int32_t join, int32_t hier_n = 0,
                      int32_t hier_join = VY_HJOIN_MAX) {
  vy_net* n = new vy_net();
  n->hier_n = hier_n;
  n->hier_join = hier_join;
  n->num_class = num_class;
  n->knobs = vy_knobs_read();
  n->heads_only = heads_only;
  n->window_k = k;
  n->window_join = join;
  n->build();
  return n;
}

// ---- the inference entries: each is the sequence of vy_net steps it documents in vyolo.h, inside one shared frame
static NoHook plain;  // of every entry but vy_net_profile_infer, which has its own
// (run_entry / entry_ready: net_internal.h, shared with the training entries)

// vy_net_forward_infer and vy_net_profile_infer: stem and stages, the pooling of a window net, heads, detection tail
template <typename Hook>
static int infer_sequence(vy_net* net, const float* x, float* ids, float* scores, float* bboxes, int32_t* keep_idx,
                          hipStream_t s, Hook& hook) {
  VY_TRY(net->prepare(s, hook, true));
  VY_TRY(net->run_backbone(x, s, hook));
  if (net->clip_net()) VY_TRY(net->window_pool(s, hook));
  VY_TRY(net->run_cells(net->n_backbone, (int)net->convs.size(), nullptr, s, hook));
  return net->detect_tail(ids, scores, bboxes, keep_idx, s, hook);
}

// ------------------------------------------------------------------------------------------ C ABI
extern "C" {

const char* vy_last_error(void) { return g_err.c_str(); }
const char* vy_version(void) { return "vyolo 1 gfx950"; }

int vy_net_create(int32_t num_class, vy_net** out) {
  VY_TRY(check_create(num_class, out));
  *out = create(num_class, false, 0, 0);
  return 0;
}

int vy_net_create_heads(int32_t num_class, vy_net** out) {
  VY_TRY(check_create(num_class, out));
  *out = create(num_class, true, 0, 0);
  return 0;
}

int vy_net_create_window(int32_t num_class, int32_t k, int32_t join, vy_net** out) {
  VY_TRY(check_create(num_class, out));
  if (k < 2 || k > 64) return fail(VY_ERR_INVALID, "window k = %d: a window net has 2 ... 64 frames (k = 1: vy_net_create)", k);
  if (join != VY_JOIN_MAX && join != VY_JOIN_MEAN)
    return fail(VY_ERR_INVALID, "join %d: VY_JOIN_MAX (%d) or VY_JOIN_MEAN (%d)", join, VY_JOIN_MAX, VY_JOIN_MEAN);
  *out = create(num_class, false, k, join);
  return 0;
}

int vy_net_create_heads_window(int32_t num_class, int32_t k, int32_t join, vy_net** out) {
  VY_TRY(check_create(num_class, out));
  if (k < 2 || k > 64)
    return fail(VY_ERR_INVALID, "window k = %d: a windowed heads net has 2 ... 64 frames (k = 1: vy_net_create_heads)", k);
  if (join != VY_JOIN_MAX && join != VY_JOIN_MEAN)
    return fail(VY_ERR_INVALID, "join %d: VY_JOIN_MAX (%d) or VY_JOIN_MEAN (%d)", join, VY_JOIN_MAX, VY_JOIN_MEAN);
  *out = create(num_class, true, k, join);
  return 0;
}

int vy_net_window(const vy_net* net, int32_t* k, int32_t* join) {
  if (!net) return fail(VY_ERR_INVALID, "net is null");
  if (k) *k = net->window_k;
  if (join) *join = net->window_k ? net->window_join : 0;
  return 0;
}

int vy_net_create_hier_join(int32_t num_class, int32_t n_pools, int32_t join, vy_net** out) {
  VY_TRY(check_create(num_class, out));
  if (n_pools < 1 || n_pools > 4)
    return fail(VY_ERR_INVALID, "n_pools = %d: a hierarchical net pools 1 ... 4 times (0: vy_net_create)", n_pools);
  if (join != VY_HJOIN_MAX && join != VY_HJOIN_CONV)
    return fail(VY_ERR_INVALID, "join %d: VY_HJOIN_MAX (%d) or VY_HJOIN_CONV (%d)", join, VY_HJOIN_MAX, VY_HJOIN_CONV);
  *out = create(num_class, false, 0, 0, n_pools, join);
  return 0;
}

int vy_net_create_hier(int32_t num_class, int32_t n_pools, vy_net** out) {
  return vy_net_create_hier_join(num_class, n_pools, VY_HJOIN_MAX, out);
}

int vy_net_hier(const vy_net* net, int32_t* n_pools, int32_t* frames) {
  if (!net) return fail(VY_ERR_INVALID, "net is null");
  if (n_pools) *n_pools = net->hier_n;
  if (frames) *frames = net->hier_frames();
  return 0;
}

int vy_net_tap_frames(const vy_net* net, const char* name, int32_t* frames) {
  if (!net || !name || !frames) return fail(VY_ERR_INVALID, "null argument");
  TapRef t;
  VY_TRY(vy_resolve_tap(net, name, &t));
  *frames = net->planes[t.plane].fm;  // (a pooled route's plane: 1)
  return 0;
}

void vy_net_destroy(vy_net* net) {
  if (!net) return;
  vy_train_free(net);
  delete net;
}

int vy_net_set_nms(vy_net* net, float nms_thresh, int32_t nms_topk, int32_t post_nms) {
  if (!net) return fail(VY_ERR_INVALID, "net is null");
  net->nms_thresh = nms_thresh;
  net->nms_topk = nms_topk;
  net->post_nms = post_nms;
  return 0;
}

int vy_net_set_semantics(vy_net* net, const vy_semantics* s) {
  if (!net || !s) return fail(VY_ERR_INVALID, "null argument");
  const int32_t f[6] = {s->nms_valid_ge,   s->nms_overlap_ge,   s->nms_tie_descending,
                        s->nms_topk_after, s->nms_iou_plus_one, s->bn_running_var_unbiased};
  for (int i = 0; i < 6; ++i)
    if (f[i] != 0 && f[i] != 1) return fail(VY_ERR_INVALID, "vy_semantics: field %d is %d, expected 0 or 1", i, f[i]);
  for (int i = 0; i < 10; ++i)
    if (s->reserved[i] != 0) return fail(VY_ERR_INVALID, "vy_semantics: reserved[%d] is %d, must be 0", i, s->reserved[i]);
  net->sem = *s;
  return 0;
}

int vy_net_get_semantics(const vy_net* net, vy_semantics* out) {
  if (!net || !out) return fail(VY_ERR_INVALID, "null argument");
  *out = net->sem;
  return 0;
}

int32_t vy_net_num_params(const vy_net* net) { return net ? (int32_t)net->params.size() : 0; }

int vy_net_param_info(const vy_net* net, int32_t i, vy_param_info* out) {
  if (!net || !out || i < 0 || i >= (int32_t)net->params.size()) return fail(VY_ERR_INVALID, "bad param index %d", i);
  *out = net->params[i].info;
  return 0;
}

int32_t vy_net_num_convs(const vy_net* net) { return net ? (int32_t)net->convs.size() : 0; }

int vy_net_conv_info(const vy_net* net, int32_t i, vy_conv_info* out) {
  if (!net || !out || i < 0 || i >= (int32_t)net->convs.size()) return fail(VY_ERR_INVALID, "bad conv index %d", i);
  const ConvT& c = net->convs[i];
  memset(out, 0, sizeof *out);
  snprintf(out->name, sizeof out->name, "%s", c.name.c_str());
  out->cin = c.cin;
  out->cout = c.cout;
  out->kernel = c.k;
  out->stride = c.stride;
  out->pad = c.k / 2;
  out->has_bn = c.p_gamma >= 0;
  out->sync_bn = is_sync_layer(c);
  out->residual = c.res_plane >= 0;
  out->upsample = c.ups;
  out->concat_offset = c.out_co;
  out->out_channels_total = net->planes[c.out_plane].C;
  return 0;
}

size_t vy_net_param_bytes(const vy_net* net) { return net ? (size_t)net->param_elems * sizeof(float) : 0; }

int vy_net_bind_params(vy_net* net, void* dev_params) {
  if (!net || !dev_params) return fail(VY_ERR_INVALID, "null argument");
  net->dev_params = static_cast<float*>(dev_params);
  net->split_dirty = net->dsplit_dirty = net->wino_dirty = true;
  return 0;
}

int vy_net_param_set(vy_net* net, int32_t i, const float* host_src, void* stream) {
  if (!net || !host_src || i < 0 || i >= (int32_t)net->params.size()) return fail(VY_ERR_INVALID, "bad argument");
  if (!net->dev_params) return fail(VY_ERR_STATE, "parameters not bound");
  const vy_param_info& pi = net->params[i].info;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* dst = net->dev_params + pi.offset;
  net->split_dirty = net->dsplit_dirty = net->wino_dirty = true;
  if (pi.ndim == 4) {
    std::vector<float> tmp((size_t)pi.size);
    pack_oihw(host_src, tmp.data(), pi.shape[0], pi.shape[1], pi.shape[2]);
    HIP_TRY(hipMemcpyAsync(dst, tmp.data(), sizeof(float) * pi.size, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
  } else {
    HIP_TRY(hipMemcpyAsync(dst, host_src, sizeof(float) * pi.size, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  return 0;
}

int vy_net_param_get(vy_net* net, int32_t i, float* host_dst, void* stream) {
  if (!net || !host_dst || i < 0 || i >= (int32_t)net->params.size()) return fail(VY_ERR_INVALID, "bad argument");
  if (!net->dev_params) return fail(VY_ERR_STATE, "parameters not bound");
  const vy_param_info& pi = net->params[i].info;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const float* src = net->dev_params + pi.offset;
  if (pi.ndim == 4) {
    std::vector<float> tmp((size_t)pi.size);
    HIP_TRY(hipMemcpyAsync(tmp.data(), src, sizeof(float) * pi.size, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    unpack_oihw(tmp.data(), host_dst, pi.shape[0], pi.shape[1], pi.shape[2]);
  } else {
    HIP_TRY(hipMemcpyAsync(host_dst, src, sizeof(float) * pi.size, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  return 0;
}

size_t vy_net_workspace_bytes(const vy_net* net, int32_t batch, int32_t height, int32_t width) {
  if (!net || vy_check_shape(batch, height, width)) return 0;
  net->resolve_cus();
  return net->plan(batch, height, width, net->keep_activations).total;
}

// plan, check the caller's workspace against the plan, commit it and take the workspace.  frames, ring, hstep: vy_net::plan
static int bind_plan(vy_net* net, void* dev_ws, size_t bytes, int b, int h, int w, int frames, int ring, const char* what,
                     void* stream, int hstep = 0) {
  VY_TRY(net->bind_cus(dev_ws));
  NetPlan plan = net->plan(b, h, w, net->keep_activations, frames, ring, nullptr, hstep);
  const size_t need = plan.total;
  if (bytes < need) return fail(VY_ERR_INVALID, "%sworkspace too small: %zu < %zu bytes", what, bytes, need);
  return net->commit_bind(std::move(plan), dev_ws, bytes, need, static_cast<hipStream_t>(stream));
}

int vy_net_bind_workspace(vy_net* net, void* dev_ws, size_t bytes, int32_t batch, int32_t height, int32_t width,
                          void* stream) {
  if (!net || !dev_ws) return fail(VY_ERR_INVALID, "null argument");
  VY_TRY(vy_check_shape(batch, height, width));
  return bind_plan(net, dev_ws, bytes, batch, height, width, 0, 0, "", stream);
}

int vy_net_set_keep_activations(vy_net* net, int32_t keep) {
  if (!net) return fail(VY_ERR_INVALID, "net is null");
  if ((keep != 0) != net->keep_activations) {
    net->keep_activations = keep != 0;
    net->unbind();
  }
  return 0;
}

int vy_net_set_conv_mode(vy_net* net, int32_t mode) {
  if (!net) return fail(VY_ERR_INVALID, "net is null");
  if (mode < VY_CONV_EXACT_FP32 || mode > VY_CONV_SPLIT_BF16X3_TRAIN) return fail(VY_ERR_INVALID, "conv mode %d", mode);
  if (const VyKind kind = net->kind(); (kind == VY_WINDOW || kind == VY_HIER) && mode != VY_CONV_EXACT_FP32)
    return fail(VY_ERR_UNSUPPORTED, "conv mode %d: a %s net runs the exact fp32 kernels only", mode,
                kind == VY_WINDOW ? "window" : "hierarchical");
  if (mode != net->conv_mode) {
    net->conv_mode = mode;
    net->unbind();  // (the weight images live in the workspace)
  }
  return 0;
}

int32_t vy_net_get_conv_mode(const vy_net* net) { return net ? net->conv_mode : 0; }

int vy_net_streamk_state(const vy_net* net, int32_t* enabled, size_t* flags_offset, int32_t* n_flags) {
  if (!net) return fail(VY_ERR_INVALID, "net is null");
  if (!net->dev_ws) return fail(VY_ERR_STATE, "workspace not bound");
  if (enabled) *enabled = net->sk_ok ? 1 : 0;
  if (flags_offset) *flags_offset = net->cur.sk_off;
  if (n_flags) *n_flags = VY_SK_FLAGS;
  return 0;
}

int vy_net_invalidate_split_weights(vy_net* net) {
  if (!net) return fail(VY_ERR_INVALID, "net is null");
  net->split_dirty = net->dsplit_dirty = net->wino_dirty = true;
  return 0;
}

int32_t vy_net_num_anchors(const vy_net* net) {
  if (!net || !net->dev_ws) return 0;
  int n = 0;
  for (int i = 0; i < 3; ++i) n += 3 * net->plane(net->head_plane[i]).H * net->plane(net->head_plane[i]).W;
  return n;
}

int vy_net_forward_infer(vy_net* net, const float* x, float* ids, float* scores, float* bboxes, int32_t* keep_idx,
                         void* stream) {
  VY_TRY(vy_serves(net, "vy_net_forward_infer", VY_FULL | VY_WINDOW | VY_HIER));
  return run_entry(net, x && ids && scores && bboxes, nullptr, stream, [&](hipStream_t s) {
    return infer_sequence(net, x, ids, scores, bboxes, keep_idx, s, plain);
  });
}

int vy_net_forward_features(vy_net* net, const float* x, float* f0, float* f1, float* f2, void* stream) {
  VY_TRY(vy_serves(net, "vy_net_forward_features", VY_FULL));
  return run_entry(net, x && f0 && f1 && f2, nullptr, stream, [&](hipStream_t s) {
    const float* const out[3] = {f0, f1, f2};
    VY_TRY(net->prepare(s, plain, true));
    VY_TRY(net->run_cells(0, net->n_backbone, x, s, plain));
    return net->route_export(out, s, plain);
  });
}

int vy_net_forward_infer_routes(vy_net* net, const float* f0, const float* f1, const float* f2, float* ids, float* scores,
                                float* bboxes, int32_t* keep_idx, void* stream) {
  VY_TRY(vy_serves(net, "vy_net_forward_infer_routes", VY_HEADS));
  return run_entry(net, f0 && f1 && f2 && ids && scores && bboxes, nullptr, stream, [&](hipStream_t s) {
    const float* const in[3] = {f0, f1, f2};
    VY_TRY(net->prepare(s, plain, false));
    VY_TRY(net->route_import(in, s, plain));
    VY_TRY(net->run_cells(0, (int)net->convs.size(), nullptr, s, plain));
    return net->detect_tail(ids, scores, bboxes, keep_idx, s, plain);
  });
}

int vy_net_forward_infer_bank(vy_net* net, const float* f0, const float* f1, const float* f2, int32_t n_frames,
                              const int32_t* table, float* ids, float* scores, float* bboxes, int32_t* keep_idx,
                              void* stream) {
  VY_TRY(vy_serves(net, "vy_net_forward_infer_bank", VY_HEADS_WINDOW));
  const BankRef bank{{f0, f1, f2}, n_frames, table};
  return run_entry(net, bank.ok() && ids && scores && bboxes, nullptr, stream, [&](hipStream_t s) {
    VY_TRY(vy_check_bank(net, "vy_net_forward_infer_bank", bank));
    VY_TRY(net->prepare(s, plain, false));
    VY_TRY(net->import_pool(bank, s, plain));
    VY_TRY(net->run_cells(0, (int)net->convs.size(), nullptr, s, plain));
    return net->detect_tail(ids, scores, bboxes, keep_idx, s, plain);
  });
}

// ---- video plans
static int check_video_shape(const vy_net* net, int32_t frames, int32_t clips, int32_t ring, int32_t h, int32_t w) {
  if (frames < 1 || clips < 1 || ring < 1)
    return fail(VY_ERR_INVALID, "video plan: frames %d, clips %d, ring %d must all be >= 1", frames, clips, ring);
  if (frames > VY_VIDEO_TABLE_MAX || (long long)clips * net->window_k > VY_VIDEO_TABLE_MAX)
    return fail(VY_ERR_INVALID, "video plan: frames %d and clips * k = %d x %d must not exceed %d table entries (they travel "
                "in the kernel arguments)", frames, clips, net->window_k, VY_VIDEO_TABLE_MAX);
  if (net->conv_mode != VY_CONV_EXACT_FP32) return fail(VY_ERR_UNSUPPORTED, "a video plan runs the exact fp32 kernels only");
  return vy_check_shape(clips, h, w);
}

size_t vy_net_video_workspace_bytes(const vy_net* net, int32_t frames, int32_t clips, int32_t ring, int32_t height,
                                    int32_t width) {
  if (vy_serves(net, "vy_net_video_workspace_bytes", VY_WINDOW) || check_video_shape(net, frames, clips, ring, height, width)) return 0;
  net->resolve_cus();
  return net->plan(clips, height, width, net->keep_activations, frames, ring).total;
}

int vy_net_bind_video(vy_net* net, void* dev_ws, size_t bytes, int32_t frames, int32_t clips, int32_t ring, int32_t height,
                      int32_t width, void* stream) {
  VY_TRY(vy_serves(net, "vy_net_bind_video", VY_WINDOW));
  if (!dev_ws) return fail(VY_ERR_INVALID, "null argument");
  VY_TRY(check_video_shape(net, frames, clips, ring, height, width));
  return bind_plan(net, dev_ws, bytes, clips, height, width, frames, ring, "video ", stream);
}

// VY_ERR_INVALID unless the `n` entries of a video entry's slot table lie in [lo, ring)
static int check_slots(const vy_net* net, const char* entry, const int32_t* table, int n, int lo) {
  for (int i = 0; i < n; ++i)
    if (table[i] < lo || table[i] >= net->cur.video_R)
      return fail(VY_ERR_INVALID, "%s: entry %d of the slot table is %d, outside [%d, %d)", entry, i, table[i], lo, net->cur.video_R);
  return 0;
}

int vy_net_video_push(vy_net* net, const float* x, const int32_t* slots, void* stream) {
  VY_TRY(vy_serves(net, "vy_net_video_push", VY_WINDOW));
  return run_entry(net, x && slots, "vy_net_video_push", stream, [&](hipStream_t s) {
    VY_TRY(check_slots(net, "vy_net_video_push", slots, net->cur.video_F, -1));
    VY_TRY(net->prepare(s, plain, true));
    VY_TRY(net->run_cells(0, net->n_backbone, x, s, plain));
    return net->ring_push(slots, s, plain);
  });
}

int vy_net_video_detect(vy_net* net, const int32_t* table, float* ids, float* scores, float* bboxes, int32_t* keep_idx,
                        void* stream) {
  VY_TRY(vy_serves(net, "vy_net_video_detect", VY_WINDOW));
  return run_entry(net, table && ids && scores && bboxes, "vy_net_video_detect", stream, [&](hipStream_t s) {
    VY_TRY(check_slots(net, "vy_net_video_detect", table, net->cur.B * net->window_k, 0));
    VY_TRY(net->prepare(s, plain, false));
    VY_TRY(net->ring_pool(table, s, plain));
    VY_TRY(net->run_cells(net->n_backbone, (int)net->convs.size(), nullptr, s, plain));
    return net->detect_tail(ids, scores, bboxes, keep_idx, s, plain);
  });
}

int vy_net_video_read_slot(vy_net* net, int32_t slot, float* f0, float* f1, float* f2, void* stream) {
  VY_TRY(vy_serves(net, "vy_net_video_read_slot", VY_WINDOW));
  VY_TRY(entry_ready(net, f0 && f1 && f2, "vy_net_video_read_slot"));
  if (slot < 0 || slot >= net->cur.video_R) return fail(VY_ERR_INVALID, "slot %d outside [0, %d)", slot, net->cur.video_R);
  RingRoute rr[3];
  net->ring_routes(rr);
  float* const out[3] = {f0, f1, f2};
  for (int i = 0; i < 3; ++i)
    HIP_TRY(vy_launch_ring_read(rr[i].ring + slot * net->cur.ring_slot_floats, rr[i].H, rr[i].W, rr[i].C, out[i],
                                static_cast<hipStream_t>(stream)));
  return 0;
}

// ---- hier-video plans
static int check_hier_video_shape(int32_t centres, int32_t step, int32_t h, int32_t w) {
  if (centres < 1 || centres > VY_VIDEO_TABLE_MAX || step < 1 || step > VY_HIER_VIDEO_STEP_MAX)
    return fail(VY_ERR_INVALID, "hier-video plan: centres %d must lie in [1, %d] and step %d in [1, %d]", centres,
                VY_VIDEO_TABLE_MAX, step, VY_HIER_VIDEO_STEP_MAX);
  return vy_check_shape(centres, h, w);
}

int vy_net_hier_video_frames(const vy_net* net, int32_t centres, int32_t step, int32_t* frames_in) {
  VY_TRY(vy_serves(net, "vy_net_hier_video_frames", VY_HIER));
  if (!frames_in) return fail(VY_ERR_INVALID, "null argument");
  VY_TRY(check_hier_video_shape(centres, step, 32, 32));
  *frames_in = centres + step * (net->hier_frames() - 1);
  return 0;
}

size_t vy_net_hier_video_workspace_bytes(const vy_net* net, int32_t centres, int32_t step, int32_t height, int32_t width) {
  if (vy_serves(net, "vy_net_hier_video_workspace_bytes", VY_HIER) || check_hier_video_shape(centres, step, height, width)) return 0;
  net->resolve_cus();
  return net->plan(centres, height, width, net->keep_activations, 0, 0, nullptr, step).total;
}

int vy_net_bind_hier_video(vy_net* net, void* dev_ws, size_t bytes, int32_t centres, int32_t step, int32_t height,
                           int32_t width, void* stream) {
  VY_TRY(vy_serves(net, "vy_net_bind_hier_video", VY_HIER));
  if (!dev_ws) return fail(VY_ERR_INVALID, "null argument");
  VY_TRY(check_hier_video_shape(centres, step, height, width));
  return bind_plan(net, dev_ws, bytes, centres, height, width, 0, 0, "hier-video ", stream, step);
}

int vy_net_hier_video_detect(vy_net* net, const float* x, float* ids, float* scores, float* bboxes, int32_t* keep_idx,
                             void* stream) {
  VY_TRY(vy_serves(net, "vy_net_hier_video_detect", VY_HIER));
  return run_entry(net, x && ids && scores && bboxes, "vy_net_hier_video_detect", stream, [&](hipStream_t s) {
    return infer_sequence(net, x, ids, scores, bboxes, keep_idx, s, plain);  // (the joins of this plan run dilated)
  });
}

int vy_net_read_head(vy_net* net, int32_t i, float* dst_dev, void* stream) {
  if (!net || !dst_dev || i < 0 || i > 2) return fail(VY_ERR_INVALID, "bad argument");
  if (int rc = net->check_ready(true)) return rc;
  const PlaneAt p = net->plane(net->head_plane[i]);
  HIP_TRY(vy_launch_plane_to_nchw(net->plane_ptr(net->head_plane[i]), net->cur.B, p.H, p.W, p.C, 0,
                                  3 * (5 + net->num_class), dst_dev, static_cast<hipStream_t>(stream)));
  return 0;
}

int vy_net_detect_heads(vy_net* net, const float* head0, const float* head1, const float* head2, float* ids, float* scores,
                        float* bboxes, int32_t* keep_idx, void* stream) {
  if (!net || !head0 || !head1 || !head2 || !ids || !scores || !bboxes) return fail(VY_ERR_INVALID, "null argument");
  if (int rc = net->check_ready()) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const float* src[3] = {head0, head1, head2};
  for (int i = 0; i < 3; ++i) {
    const PlaneAt p = net->plane(net->head_plane[i]);
    HIP_TRY(vy_launch_nchw_to_plane(src[i], net->cur.B, p.H, p.W, p.C, 0, 3 * (5 + net->num_class),
                                    net->plane_ptr(net->head_plane[i]), s));
  }
  return net->detect_tail(ids, scores, bboxes, keep_idx, s, plain);
}

int vy_net_read_activation(vy_net* net, const char* name, float* dst_dev, int32_t* c, int32_t* h, int32_t* w,
                           void* stream) {
  if (!net || !name) return fail(VY_ERR_INVALID, "bad argument");
  if (int rc = net->check_ready(true)) return rc;
  if (dst_dev && net->cur.planes_shared)
    return fail(VY_ERR_STATE, "activation planes are recycled in this plan: call vy_net_set_keep_activations(net, 1) "
                "before sizing / binding the workspace to read intermediate activations");
  TapRef t;
  VY_TRY(vy_resolve_tap(net, name, &t));
  if (c) *c = t.C;
  if (h) *h = net->plane(t.plane).H;
  if (w) *w = net->plane(t.plane).W;
  if (dst_dev) HIP_TRY(vy_tap_to_nchw(net, t, nullptr, dst_dev, static_cast<hipStream_t>(stream)));
  return 0;
}

int vy_net_profile_infer(vy_net* net, const float* x, float* ids, float* scores, float* bboxes,
                         vy_launch_stat* stats, int32_t* n, void* stream) {
  VY_TRY(vy_serves(net, "vy_net_profile_infer", VY_FULL | VY_HIER));
  if (!stats || !n) return fail(VY_ERR_INVALID, "null argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int cap = *n;
  std::vector<hipEvent_t> ev0, ev1;
  std::vector<vy_launch_stat> rec;
  bool bad = false;
  auto hook = [&](const char* name, double fl, double by, bool before) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) {
      bad = true;
      return;
    }
    (void)hipEventRecord(e, s);
    if (before) {
      vy_launch_stat st;
      memset(&st, 0, sizeof st);
      snprintf(st.name, sizeof st.name, "%s", name);
      st.flops = fl;
      st.bytes = by;
      rec.push_back(st);
      ev0.push_back(e);
    } else {
      ev1.push_back(e);
    }
  };
  // (a hierarchical net bound for video: the launches of a vy_net_hier_video_detect call on x)
  int rc = run_entry(net, true, net->cur.hier_step ? "vy_net_profile_infer" : nullptr, stream,
                     [&](hipStream_t) { return infer_sequence(net, x, ids, scores, bboxes, nullptr, s, hook); });
  if (rc == 0) {
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) rc = fail(VY_ERR_HIP, "sync: %s", hipGetErrorString(e));
  }
  int cnt = 0;
  for (size_t i = 0; i < ev1.size() && i < ev0.size(); ++i) {
    if (rc == 0) (void)hipEventElapsedTime(&rec[i].ms, ev0[i], ev1[i]);
    if ((int)i < cap) stats[i] = rec[i], cnt = (int)i + 1;
  }
  for (auto e : ev0) (void)hipEventDestroy(e);
  for (auto e : ev1) (void)hipEventDestroy(e);
  *n = cnt;
  if (bad && rc == 0) rc = fail(VY_ERR_HIP, "hipEventCreate failed");
  return rc;
}

int vy_stream_create(void** stream) {
  if (!stream) return fail(VY_ERR_INVALID, "null argument");
  hipStream_t s = nullptr;
  hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
  if (e != hipSuccess) return fail(VY_ERR_HIP, "hipStreamCreateWithFlags: %s", hipGetErrorString(e));
  *stream = s;
  return 0;
}

int vy_stream_destroy(void* stream) {
  if (!stream) return 0;
  hipError_t e = hipStreamDestroy(static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(VY_ERR_HIP, "hipStreamDestroy: %s", hipGetErrorString(e));
  return 0;
}

}  // extern "C"
