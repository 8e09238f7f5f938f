/*
 * vyolo.h — C-ABI of libvyolo.so, the MI355X-native yolo3_darknet53 hot path.
 *
 * The reference has no FFI: its "operator API" for this path is the duck-typed surface of the
 * Gluon HybridBlock that models/definitions/yolo/wrappers.py:9-110 (yolo3_darknet53) returns,
 * as driven by train_yolov3.py and detect_yolo3.py.  Each entry point below names the reference
 * call it stands in for (paths relative to /root/reference).  The Python class that presents
 * the Gluon surface over these entry points is videoyolo_amd/model.py; INTEGRATION.md shows the
 * ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C types only; every function returns 0 on success or a negative vy_status and
 *     leaves a message for vy_last_error() (thread-local).
 *   - the library never allocates or frees device memory and never synchronises the device
 *     inside a forward/step call: the caller owns three device buffers per net
 *     (parameters, workspace, and — for training — gradients/momentum), sized by the vy_*_bytes
 *     queries, and passes the HIP stream to launch on (hipStream_t as void*; NULL = default).
 *   - one vy_net per device / rank / stream; a net holds no global state.
 *   - tensors at the boundary use the reference's layouts: images NCHW fp32, conv weights OIHW,
 *     detections (ids (B,post_nms,1), scores (B,post_nms,1), bboxes (B,post_nms,4)) fp32 with
 *     -1 filler, exactly what YOLOV3T.hybrid_forward returns (yolo3.py:1203-1206).
 */
#ifndef VYOLO_H
#define VYOLO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vy_net vy_net;

enum vy_status {
  VY_OK = 0,
  VY_ERR_INVALID = -1,      /* bad argument / unsupported configuration */
  VY_ERR_STATE = -2,        /* call order: buffers not bound, not planned, ... */
  VY_ERR_HIP = -3,          /* a HIP runtime call or kernel launch failed */
  VY_ERR_UNSUPPORTED = -4,  /* reference feature outside the hot path (temporal variants ...) */
  VY_ERR_RANGE = -5         /* an index past the end of a list (vy_net_plan_region); leaves no error text */
};

enum vy_param_kind {
  VY_P_WEIGHT = 0, VY_P_GAMMA = 1, VY_P_BETA = 2, VY_P_RUNNING_MEAN = 3, VY_P_RUNNING_VAR = 4,
  VY_P_BIAS = 5
};

/* One row of collect_params() (train_yolov3.py:494-497, wrappers.py:55-57). */
typedef struct vy_param_info {
  char name[96];        /* gluon structural name, e.g. "stages.0.2.body.1.0.weight" */
  int32_t kind;         /* vy_param_kind */
  int32_t ndim;         /* 4 for conv weights (O,I,kh,kw), else 1 */
  int32_t shape[4];     /* reference shape */
  int64_t size;         /* element count */
  int64_t offset;       /* element offset of this tensor inside the device parameter buffer
                           (device layout: conv weights are stored O,kh,kw,I) */
  int32_t trainable;    /* 0 for running_mean / running_var */
  int32_t backbone;     /* 1 if the tensor belongs to the Darknet-53 stages (freeze_base) */
} vy_param_info;

/* Last error message of the calling thread ("" if none). */
const char* vy_last_error(void);

/* Library build id ("vyolo <n> gfx950"). */
const char* vy_version(void);

/* yolo3_darknet53(classes, ...) at k=1 — wrappers.py:9-12,54-58,80-84,101-103 and
 * YOLOV3T.__init__ yolo3.py:959-1054.  num_class = len(classes). */
int vy_net_create(int32_t num_class, vy_net** out);
/* yolo3_no_backbone(classes) — wrappers.py:133-161, YOLOV3_noback yolo3.py:1686-1920 (train_yolov3.py:335-343 with
 * --features_dir): the same heads, entered at the three Darknet-53 route tensors.  Its parameter table is the full net's
 * head rows (yolo_blocks.*, transitions.*, yolo_outputs.*) with the same names and shapes, in the same order.  Sizing,
 * binding, parameters, gradients, SGD, NMS, training options, taps and vy_net_train_conv_plan work as on a full net;
 * (batch, height, width) stay the size of the image the routes came from.  Its forward / training entries are the
 * *_routes ones below: an entry that takes an image batch fails on it with VY_ERR_STATE (and a *_routes entry on a full
 * net), doing nothing. */
int vy_net_create_heads(int32_t num_class, vy_net** out);
/* yolo3_darknet53(classes, k=k, k_join_type=..., k_join_pos='early') — YOLOV3T yolo3.py:1016-1121 with early join: a
 * k-frame clip net.  The backbone runs on batch * k frames (TimeDistributed: frame t of clip b is frame b * k + t, so
 * x is (batch, k, 3, h, w)); each of its three routes is pooled over the clip's k frames (TemporalPooling 'direct',
 * layers.py:193-204) as soon as its stage ends, and the ordinary heads run on the batch clips.  k >= 2 (k = 1 is
 * vy_net_create); join VY_JOIN_MAX or VY_JOIN_MEAN; anything else is VY_ERR_INVALID.  The parameter table is
 * vy_net_create's, name for name and offset for offset.  `batch` counts clips in sizing, binding and every entry.
 * vy_net_forward_infer and the training entries work on it; vy_net_forward_features, vy_net_profile_infer and the
 * *_routes entries fail with VY_ERR_STATE, the split conv modes with VY_ERR_UNSUPPORTED.  Taps: vy_net_read_activation
 * and vy_net_read_grad_activation take "pool.0" .. "pool.2" (strides 8, 16, 32: the pooled route, (batch, C, h, w)); a
 * backbone cell's tap gives its batch * k frames. */
#define VY_JOIN_MAX 0
#define VY_JOIN_MEAN 1
int vy_net_create_window(int32_t num_class, int32_t k, int32_t join, vy_net** out);
/* yolo3_no_backbone(classes, k=k, k_join_type=..., k_join_pos='early') — the head half of vy_net_create_window, for
 * train_yolov3.py --features_dir --window k (datasets/imgnetvid.py:146-174 stacks the k frames' saved routes): a heads-only
 * net whose routes are pooled over a window of k stored per-frame routes on the way in.  k >= 2, join VY_JOIN_MAX or
 * VY_JOIN_MEAN; anything else is VY_ERR_INVALID.  The parameter table, conv list, plan, vy_net_workspace_bytes,
 * vy_net_train_workspace_bytes and vy_net_train_conv_plan are vy_net_create_heads', number for number: no per-frame plane
 * exists.  `batch` counts clips.  Its forward entries are the *_bank ones below; vy_net_train_backward_routes serves it
 * (route arguments ignored, NULL allowed).  Image entries, the other *_routes entries and the video entries fail on it
 * with VY_ERR_STATE, doing nothing — as the *_bank entries do on every other kind of net.  Conv modes as on a heads-only
 * net.  Taps: "pool.0" .. "pool.2" as on a window net. */
int vy_net_create_heads_window(int32_t num_class, int32_t k, int32_t join, vy_net** out);
/* k and join of a window net (of either kind); k = 0 for any other net. */
int vy_net_window(const vy_net* net, int32_t* k, int32_t* join);
/* yolo3_darknet53(classes, new_model=True, hierarchical=[3,..,1], h_join_type='max') — HDarknet, h_darknet.py:103-188: a
 * detector over clips of T = 3^n_pools frames that pools INSIDE the backbone.  x is (batch, T, 3, h, w), frame t of clip b
 * is frame b * T + t.  The stem runs per frame; in front of each of the first n_pools stride-2 convs (after features[0],
 * [1:3], [3:6], [6:15]) consecutive triples of frames are reduced with an element-wise max (hier.hip: strict > in frame
 * order; backward writes the full gradient to every tied frame), so the cells between pool i - 1 and pool i run on
 * batch * 3^(n_pools - i) frames and everything behind the last pool on the batch clips, as a single-frame net would.
 * n_pools 1 .. 4, anything else VY_ERR_INVALID.  With four pools the fourth pooled plane is route 0 itself.  The max has
 * no parameters: the parameter table and the conv list are vy_net_create's, name for name, offset for offset and in the
 * same order.  `batch` counts clips in sizing, binding and every entry.  vy_net_forward_infer, vy_net_profile_infer
 * (launches "hpool.<i>") and the training entries work on it; vy_net_forward_features, the *_routes / *_bank entries and
 * the video entries fail with VY_ERR_STATE, the split conv modes with VY_ERR_UNSUPPORTED.  Taps: vy_net_read_activation,
 * vy_net_read_grad_activation and vy_net_read_train_tap (VY_TAP_GRAD_PADDED: the pooled plane's gradient,
 * VY_TAP_INPUT_PADDED: the pre-pool plane) take "hpool.0" .. "hpool.<n_pools - 1>"; every tap has batch *
 * vy_net_tap_frames frames. */
int vy_net_create_hier(int32_t num_class, int32_t n_pools, vy_net** out);
/* The hierarchical net with the join named: VY_HJOIN_MAX is vy_net_create_hier, table for table; VY_HJOIN_CONV is
 * h_join_type='conv' (`_conv1d`, layers.py:50-60; h_darknet.py:97-101, 116-119): in place of the max, per channel
 *   z[n, c, y, x] = fmaf(w[c][2], x[3n + 2], fmaf(w[c][1], x[3n + 1], w[c][0] * x[3n]))     (first product rounded alone)
 * then BatchNorm(eps 1e-5, momentum 0.9; train mode: statistics over the batch * frames * h * w pooled positions, never a
 * synchronised one) and LeakyReLU(0.1).  Any other join, n_pools outside 1 .. 4: VY_ERR_INVALID.  Join i (C = 32, 64, 128,
 * 256) has five parameters, appended BEHIND vy_net_create's table, which is a prefix of this one name for name and offset
 * for offset: "hjoin.<i>.0.weight" of shape (C, 3) (the reference's (C, 1, 3, 1, 1)) and "hjoin.<i>.1.gamma" / ".beta" /
 * ".running_mean" / ".running_var" (C,), all with backbone = 1 and the trainable flags of a cell's five.  The conv list is
 * vy_net_create's: a join is not a conv.  Entries, refusals and conv modes are vy_net_create_hier's; the launches of
 * vy_net_profile_infer and the taps are "hjoin.<i>" instead of "hpool.<i>" (each name is VY_ERR_INVALID on the other
 * net): vy_net_read_activation the pooled plane, vy_net_read_grad_activation its gradient, vy_net_read_train_tap all four
 * taps with a cell's meaning (VY_TAP_Z: the join's z, dz after the backward; VY_TAP_INPUT_PADDED: the pre-pool plane).
 * Training: one rank, exact conv mode; the join's gradients travel with the gradient bucket of stages.0. */
#define VY_HJOIN_MAX 0
#define VY_HJOIN_CONV 1
int vy_net_create_hier_join(int32_t num_class, int32_t n_pools, int32_t join, vy_net** out);
/* pools and frames per clip (3^n_pools) of a hierarchical net; 0 and 1 for any other net. */
int vy_net_hier(const vy_net* net, int32_t* n_pools, int32_t* frames);
/* frames per batch entry of the tap `name` (a cell, "pool.<i>", "hpool.<i>" or "hjoin.<i>") of any net: its leading dimension in a plan
 * bound for `batch` is batch * frames (a video plan aside).  VY_ERR_INVALID: no such tap. */
int vy_net_tap_frames(const vy_net* net, const char* name, int32_t* frames);
void vy_net_destroy(vy_net* net);

/* net.set_nms(nms_thresh, nms_topk, post_nms) — yolo3.py:1208-1228.
 *   nms_topk in [1, VY_MAX_TOPK]   the nms_topk best valid candidates go through NMS (the scripts use 400)
 *   nms_topk <= 0                  "-1 to disable": EVERY valid candidate goes through NMS (consumed in
 *                                  score order in chunks of VY_MAX_TOPK until the output rows are filled)
 *   nms_topk > VY_MAX_TOPK         the same chunked kernel, stopped after nms_topk candidates
 *   post_nms > 0                   the outputs have post_nms rows (any value; > VY_MAX_TOPK with a chunked nms_topk: the
 *                                  kept rows are read back from the output instead of living in LDS)
 *   post_nms <= 0                  no slice (yolo3.py:1201-1202): nms_topk rows, or — nms_topk <= 0 too — all N*C rows
 *                                  of box_nms's un-sliced output (vy_net_num_anchors * num_class; quadratic in the worst
 *                                  case, like the reference's loop)
 *   nms_thresh outside (0, 1)      no NMS at all: see vy_net_forward_infer */
#define VY_MAX_TOPK 1024
int vy_net_set_nms(vy_net* net, float nms_thresh, int32_t nms_topk, int32_t post_nms);

/* The choices of contrib.box_nms and BatchNorm that this library restates from memory of mxnet's source
 * ([UPSTREAM-RECALLED]), each switchable per net so that a deployment can be set to what its mxnet
 * does (tests/golden/RUNBOOK.md: one kit case per choice).  All 0 = what the library has always computed.
 * Every entry that ends in the detection tail (vy_net_forward_infer, *_routes, *_bank, vy_net_video_detect,
 * vy_net_detect_heads, vy_net_profile_infer) honours the five nms_* fields from its next call on; every recorded training
 * forward honours bn_running_var_unbiased.  The setting needs no bound plan and survives every bind.  A launch sequence
 * captured into a HIP graph holds the setting it was captured with.
 * box_nms's treatment of rows with id -1 ("background") has no flag: ids on this path are 0 .. C-1 (yolo3.py:194), no such
 * row reaches the operator. */
typedef struct vy_semantics {
  int32_t nms_valid_ge;          /* 0: score >  valid_thresh (default)   1: >=                              */
  int32_t nms_overlap_ge;        /* 0: iou   >  overlap_thresh (default) 1: >=                              */
  int32_t nms_tie_descending;    /* 0: equal scores in ascending candidate row (default)  1: descending     */
  int32_t nms_topk_after;        /* 0: top-k cut before suppression (default)  1: after, survivors refill   */
  int32_t nms_iou_plus_one;      /* 0: corner IoU without +1 (default)  1: +1 on widths and heights         */
  int32_t bn_running_var_unbiased; /* 0: biased batch variance into running_var (default)  1: x n/(n-1)     */
  int32_t reserved[10];          /* must be 0 */
} vy_semantics;
/* VY_ERR_INVALID, changing nothing: a null pointer, a field outside {0, 1}, a non-zero reserved word.
 * nms_topk_after: every valid candidate goes through suppression (the chunked kernel of nms_topk <= 0), the survivors are
 * cut at nms_topk, then the post_nms slice follows; the output row count is that of vy_net_set_nms, rows past the cut are
 * -1 filler. */
int vy_net_set_semantics(vy_net* net, const vy_semantics* s);
int vy_net_get_semantics(const vy_net* net, vy_semantics* out);

/* collect_params(): number of tensors, and row i. */
int32_t vy_net_num_params(const vy_net* net);
int vy_net_param_info(const vy_net* net, int32_t i, vy_param_info* out);

/* The graph the planner executes, one row per convolution in EXECUTION order (host-only; no device needed): what
 * `net.summary(x)` (train_yolov3.py:758) prints per layer, and what tests/test_graph_structure.py compares with the
 * structure the reference's own constructors build (wrappers.py:54-58,80-103; three_darknet.py:162-195;
 * yolo3.py:218-263,1013-1054; layers.py:63-70) — tests/golden/graph_structure.json. */
typedef struct vy_conv_info {
  char name[96];        /* structural prefix of the cell ("stages.0.2.body.1"; the Conv2D itself is "<name>.0") or of the
                           prediction conv ("yolo_outputs.0.prediction") */
  int32_t cin, cout, kernel, stride, pad;
  int32_t has_bn;       /* 1: Conv2D(use_bias=False) -> norm_layer -> LeakyReLU(0.1) (layers.py:63-70); 0: bias, no activation */
  int32_t sync_bn;      /* 1: the cell is built with the norm_layer passed to yolo3_darknet53 (SyncBatchNorm exchanges its
                           statistics there); 0: hard-wired / defaulted BatchNorm (darknet.py:89-91, wrappers.py:101-103) */
  int32_t residual;     /* 1: the block's input is added to this cell's output (darknet.py:40) */
  int32_t upsample;     /* 2: the output is stored x2-replicated and cropped into the concat plane (layers.py:11-20,
                           yolo3.py:1167-1177); 1 otherwise */
  int32_t concat_offset;/* first channel of this conv's output inside its output plane (concat fusion: the upsampled
                           transition comes FIRST, the backbone route after it) */
  int32_t out_channels_total; /* channels of that output plane */
} vy_conv_info;
int32_t vy_net_num_convs(const vy_net* net);
int vy_net_conv_info(const vy_net* net, int32_t i, vy_conv_info* out);

/* Bytes of the device parameter buffer (all tensors + folded-BN scratch). */
size_t vy_net_param_bytes(const vy_net* net);
/* Bind the caller-owned device parameter buffer (net.collect_params().reset_ctx(ctx),
 * detect_yolo3.py:199). */
int vy_net_bind_params(vy_net* net, void* dev_params);

/* net.load_parameters / save_parameters go through these per-tensor copies (train_yolov3.py:
 * 293-303,323-327): host data in the REFERENCE layout; the library converts OIHW <-> device
 * layout.  Both enqueue on `stream` and return after the copy has completed. */
int vy_net_param_set(vy_net* net, int32_t i, const float* host_src, void* stream);
int vy_net_param_get(vy_net* net, int32_t i, float* host_dst, void* stream);

/* Shape planning.  Workspace bytes needed for inference on (batch, 3, height, width) input;
 * height and width in [32, 4096] (alloc_size = (128,128), yolo3.py:67-74).  They need not be multiples of 32:
 * like the reference, every stride-2 conv yields ceil(n / 2) rows and the x2 upsample is cropped to the route it is
 * concatenated with (slice_like, yolo3.py:1177), so the heads have ceil(h / 32), ceil(h / 16), ceil(h / 8) rows. */
size_t vy_net_workspace_bytes(const vy_net* net, int32_t batch, int32_t height, int32_t width);
/* Bind a caller-owned device workspace of at least that size and plan for that shape.  Zeroes the
 * workspace (asynchronously, on `stream`): the padded activation planes rely on zero borders.  A refused bind changes
 * nothing.  The bind lays the workspace out anew, so it ends a training plan (vy_net_bind_train) even at the same
 * shape: the training step entries return VY_ERR_STATE until vy_net_bind_train is called again. */
int vy_net_bind_workspace(vy_net* net, void* dev_ws, size_t bytes, int32_t batch, int32_t height,
                          int32_t width, void* stream);

/* Inference activation planes are recycled by liveness (a residual stage needs two alternating block-output planes
 * and one bottleneck plane, not two per block: 608x608 batch 64 plans ~3x less workspace) — the intermediate
 * activations of a finished forward are then gone, like the intermediates of the reference's hybridized graph.
 * keep != 0 gives every cell its own plane so that vy_net_read_activation works (parity taps).  Changes the plan:
 * call before vy_net_workspace_bytes / vy_net_bind_workspace (a bound workspace is unbound by a change).  Training
 * plans always keep every plane (backward reads them). */
int vy_net_set_keep_activations(vy_net* net, int32_t keep);

/* Arithmetic of the inference convolutions (Conv2D inside `_conv2d`, models/definitions/layers.py:63-70; SURVEY 7
 * hard-part (iii) admits "split-fp32").  No counterpart in the reference: mxnet picks its conv algorithm itself.
 *   VY_CONV_EXACT_FP32     default, the parity path: every output one fp32 fma chain on v_mfma_f32_32x32x2_f32,
 *                          bit-identical to oracle/ 
 *   VY_CONV_SPLIT_BF16X3   opt-in, INFERENCE: every conv+BN+leaky cell with cout % 64 == 0 whose launch is large enough
 *                          (per-launch cost model) runs on the bf16 matrix core — every fp32 operand cut exactly into
 *                          three bf16 numbers, six partial products per multiply, fp32 accumulation
 *                          (csrc/conv_split.hip); its long-K 3x3 stride-1 cells in big launches run the same
 *                          arithmetic as a 1-D Winograd F(2, 3) (csrc/conv_wino.hip: a third fewer multiplications).
 *                          NOT bit-equal to the exact path (tolerances: tests/test_gpu_split.py), 1.5x the frames/s at
 *                          608x608 batch 64.  Planes, stem, prediction convs, decode and NMS are shared with the exact
 *                          path.  Training runs the exact kernels.
 *   VY_CONV_SPLIT_BF16X3_TRAIN   as above, and TRAINING too: the recorded forward, the data gradients (conv_split.hip)
 *                          and the weight gradients of every conv with cout % 128 == 0 (wgrad_split.hip) on the bf16
 *                          matrix core; 1.15x the training frames/s at 416x416 batch 16.  Losses within 1e-4 of the exact
 *                          path; gradients as far from it as a one-ulp change of the input moves the exact path's own
 *                          (tests/test_gpu_split.py).
 * Changes the plan (the pre-split weight images live in the workspace): call before vy_net_workspace_bytes /
 * vy_net_bind_workspace; a bound workspace is unbound by a change. */
enum vy_conv_mode { VY_CONV_EXACT_FP32 = 0, VY_CONV_SPLIT_BF16X3 = 1, VY_CONV_SPLIT_BF16X3_TRAIN = 2 };
int vy_net_set_conv_mode(vy_net* net, int32_t mode);
int32_t vy_net_get_conv_mode(const vy_net* net);
/* The weight images of VY_CONV_SPLIT_BF16X3 are rebuilt by the next inference forward after any parameter write the
 * library performs itself (vy_net_bind_params, vy_net_param_set, vy_net_sgd_step, vy_net_bind_workspace).  A caller
 * that writes the device parameter buffer directly (the Trainer's broadcast from rank 0, train_yolov3.py:527-530)
 * says so with this call. */
int vy_net_invalidate_split_weights(vy_net* net);

/* Diagnostics of the chain-preserving stream-K conv launches (csrc/conv_igemm.hip; no counterpart in the reference).
 * enabled: 1 if the bind-time probe saw the workgroup placement the schedule is built for (MI355X, SPX mode: 8 XCDs,
 * blocks L and L + 8 on one XCD, 256 CUs) — otherwise every conv is a plain launch.  flags_offset / n_flags: where the
 * hand-off flags live in the bound workspace (32-bit words, all zero between launches; after ANY entry point of the
 * handle has returned an error the next forward / training step zeroes them before it launches).  Tests only. */
int vy_net_streamk_state(const vy_net* net, int32_t* enabled, size_t* flags_offset, int32_t* n_flags);

/* Number of anchors N = 3 * sum_i (H/s_i)(W/s_i) for the planned shape. */
int32_t vy_net_num_anchors(const vy_net* net);

/* net(x) outside autograd — YOLOV3T.hybrid_forward inference branch, yolo3.py:1076-1206:
 * Darknet-53 stages -> 3 detection blocks/outputs -> decode -> box_nms -> first post_nms rows.
 *   x        device, (batch,3,H,W) fp32 NCHW
 *   ids      device, (batch,post_nms,1)     scores  device, (batch,post_nms,1)
 *   bboxes   device, (batch,post_nms,4)     corner format, input-pixel units, un-clipped
 *   keep_idx device, (batch,post_nms) int32, nullable: row index into the reference's
 *            pre-NMS (B, N*C, 6) detection tensor for every returned row (-1 for filler).
 * With nms_thresh outside (0,1) the reference skips box_nms and the slice (yolo3.py:1197-1202): the
 * outputs then have vy_net_num_anchors()*num_class rows — the (B, N*C, 6) detection tensor itself in its
 * class-major row order — and keep_idx is the row number.
 * Asynchronous on `stream`. */
int vy_net_forward_infer(vy_net* net, const float* x, float* ids, float* scores, float* bboxes,
                         int32_t* keep_idx, void* stream);

/* Route tensors.  The three outputs of Darknet-53 that the heads read — features[:15], [15:24], [24:] of
 * extract_base_features.py:120-160 (saved there as <id>_F1/F2/F3.npy) — as device fp32 NCHW:
 *   f0 (batch, 256, ceil(H/8), ceil(W/8))   f1 (batch, 512, ceil(H/16), ceil(W/16))   f2 (batch, 1024, ceil(H/32), ceil(W/32))
 * for the (batch, H, W) the workspace is planned for.  No entry writes into a caller's route buffer that it reads. */
/* Full nets: the backbone alone (stem and stages, on the ordinary plan — no vy_net_set_keep_activations needed), then
 * the routes copied out: what extract_base_features.py:120-160 computes per batch.  No head conv, no detection tail.
 * Asynchronous on `stream`. */
int vy_net_forward_features(vy_net* net, const float* x, float* f0, float* f1, float* f2, void* stream);
/* Heads-only nets: net(f1, f2, f3) outside autograd — YOLOV3_noback.hybrid_forward's inference branch
 * (train_yolov3.py:444-460 validates this way).  Outputs and the NMS-disabled raw-tensor rule as
 * vy_net_forward_infer.  Asynchronous on `stream`. */
int vy_net_forward_infer_routes(vy_net* net, const float* f0, const float* f1, const float* f2, float* ids, float* scores,
                                float* bboxes, int32_t* keep_idx, void* stream);

/* Windowed heads-only nets (vy_net_create_heads_window): a bank of stored per-frame routes and a table of clips.
 *   f0 (n_frames, 256, ceil(H/8), ceil(W/8))   f1 (n_frames, 512, ceil(H/16), ceil(W/16))   f2 (n_frames, 1024, ceil(H/32), ceil(W/32))
 * device fp32 NCHW, dense; table: host array of batch * k entries in [0, n_frames), clip b = frames table[b * k + t], t < k,
 * pooled in that order (TemporalPooling 'direct', layers.py:193-204: mean = x0 + x1 + ... then / k; max keeps the earliest
 * frame's bits on a tie).  A frame may repeat in a row.  One launch gathers, pools and transposes all three routes into the
 * planes the heads read: bit for bit what vy_net_forward_infer_routes gives for the pooled routes, and what
 * vy_net_forward_infer of a window net gives for the clips those frames came from.  batch * k <= VY_VIDEO_TABLE_MAX (the
 * table travels in the kernel arguments: the library holds no device memory for it, copies nothing and does not
 * synchronise); the table is range-checked before anything is launched (VY_ERR_INVALID) and consumed before the call
 * returns.  The banks are only read.  Outputs as vy_net_forward_infer at batch clips.  Asynchronous on `stream`. */
int vy_net_forward_infer_bank(vy_net* net, const float* f0, const float* f1, const float* f2, int32_t n_frames,
                              const int32_t* table, float* ids, float* scores, float* bboxes, int32_t* keep_idx,
                              void* stream);

/* Video plans: a window net (vy_net_create_window) run over a video, the backbone once per frame.
 * detect_yolo3.py with --window k,step builds one k-frame clip per frame of a video (datasets/imgnetvid.py:480-506: centred
 * on the frame, frames `step` apart, clamped at the ends), so consecutive clips share frames and the clip entries above run
 * Darknet-53 on each frame up to k times.  With the early join a frame's three routes do not depend on its clip, so a video
 * plan keeps them in a ring of `ring` slots in the workspace: vy_net_video_push runs the backbone on `frames` single
 * frames and stores their routes in the slots the caller names, vy_net_video_detect pools `clips` windows out of the slots
 * the caller names and runs the heads on them — bit for bit what vy_net_forward_infer gives for the materialised clips.
 * The library does not track which frame sits in which slot: that is the caller's bookkeeping.  frames, clips, ring >= 1;
 * frames <= VY_VIDEO_TABLE_MAX and clips * k <= VY_VIDEO_TABLE_MAX (the tables travel in the kernel arguments: no copy,
 * no synchronisation inside a call).  Every entry: VY_ERR_STATE on a net that is not a window net, doing nothing. */
#define VY_VIDEO_TABLE_MAX 512
/* Bytes of the workspace of a video plan (the ring included); 0 plus vy_last_error on a bad request. */
size_t vy_net_video_workspace_bytes(const vy_net* net, int32_t frames, int32_t clips, int32_t ring, int32_t height,
                                    int32_t width);
/* Binds (and zeroes, borders included, as vy_net_bind_workspace) a video plan.  The net then serves the video entries and
 * the taps only: vy_net_forward_infer and the training entries return VY_ERR_STATE until vy_net_bind_workspace /
 * vy_net_bind_train bind a clip plan again — which in turn ends the video plan; the ring's contents do not survive.
 * Like vy_net_bind_workspace it ends a training plan bound before it: the training step entries return VY_ERR_STATE
 * until vy_net_bind_train is called again. */
int vy_net_bind_video(vy_net* net, void* dev_ws, size_t bytes, int32_t frames, int32_t clips, int32_t ring, int32_t height,
                      int32_t width, void* stream);
/* The per-frame half of detect_yolo3.py's loop: stem and stages on x (frames, 3, height, width), then the three routes of
 * frame f go to ring slot slots[f] (host array of `frames` entries in [-1, ring); -1: the frame is padding and is not
 * stored).  No head conv, no detection tail.  Asynchronous on `stream`; `slots` is consumed before the call returns. */
int vy_net_video_push(vy_net* net, const float* x, const int32_t* slots, void* stream);
/* The per-clip half: for clip b the routes of slots table[b * k + t], t < k (host array, entries in [0, ring); a slot may
 * repeat: clamped ends of a video), are pooled in that order (TemporalPooling 'direct', layers.py:193-204) and the heads
 * and the detection tail run on the `clips` clips.  Outputs as vy_net_forward_infer at batch = clips.  Asynchronous. */
int vy_net_video_detect(vy_net* net, const int32_t* table, float* ids, float* scores, float* bboxes, int32_t* keep_idx,
                        void* stream);
/* Test tap: the three routes held in `slot` as NCHW (1, 256, ..), (1, 512, ..), (1, 1024, ..) — what
 * vy_net_forward_features exports for that frame (extract_base_features.py:120-160). */
int vy_net_video_read_slot(vy_net* net, int32_t slot, float* f0, float* f1, float* f2, void* stream);

/* Hier-video plans: a hierarchical net (vy_net_create_hier / _hier_join) run over a video, each level once per frame.
 * detect_yolo3.py --window T,step gives a hierarchical net one T-frame clip per frame too (T = 3^n_pools; the table of the video plans above),
 * and the clip entries then run the stem T times and pool i's group of cells T / 3^(i+1) times per emitted frame.  Extend
 * every level to the frame positions u of the video: level 0 at u is the stem on frame clamp(u, 0, N - 1), level L at u the
 * cells of that group on join(level L-1 at u - d, u, u + d) with d = step * 3^(L-1), operands in that order.  Level n at
 * u = i is then bit for bit what the clip of frame i gives, clamps included — eval-mode BatchNorm is per frame and a conv's
 * result does not depend on its batch.  A hier-video plan runs a chunk of `centres` consecutive frames i = a .. a + centres
 * - 1: with h_L = step * (3^L - 1) / 2, level L is held at the centres + 2 (h_n - h_L) consecutive positions from
 * a - (h_n - h_L) on, so every join is a dilated triple, dst[p] = join(src[p], src[p + d], src[p + 2d]).  Nothing is kept
 * between calls: the caller hands every chunk its centres + 2 h_n level-0 frames, clamped where they leave the video.
 * centres in [1, VY_VIDEO_TABLE_MAX], step in [1, VY_HIER_VIDEO_STEP_MAX].  Every entry: VY_ERR_STATE on a net that is not
 * hierarchical, doing nothing. */
#define VY_HIER_VIDEO_STEP_MAX 64
/* frames_in = centres + 2 h_n = centres + step * (3^n_pools - 1): the frames a vy_net_hier_video_detect call takes. */
int vy_net_hier_video_frames(const vy_net* net, int32_t centres, int32_t step, int32_t* frames_in);
/* Bytes of the workspace of a hier-video plan; 0 plus vy_last_error on a request it refuses. */
size_t vy_net_hier_video_workspace_bytes(const vy_net* net, int32_t centres, int32_t step, int32_t height, int32_t width);
/* Binds (and zeroes, as vy_net_bind_workspace) a hier-video plan.  The net then serves vy_net_hier_video_detect and the
 * taps only — vy_net_read_head at batch = centres, vy_net_read_activation each tap with the frames of its level, "hpool.i" /
 * "hjoin.i" the joined planes as ever — and vy_net_profile_infer, which then times the launches of a
 * vy_net_hier_video_detect call on its x (the joins under their labels "hpool.i" / "hjoin.i", bytes: the source plane and
 * the destination once each): vy_net_forward_infer and the training entries return VY_ERR_STATE until
 * vy_net_bind_workspace / vy_net_bind_train bind a clip plan again, which ends this one.  Like vy_net_bind_workspace it
 * ends a training plan bound before it. */
int vy_net_bind_hier_video(vy_net* net, void* dev_ws, size_t bytes, int32_t centres, int32_t step, int32_t height,
                           int32_t width, void* stream);
/* One chunk: x (frames_in, 3, height, width), frame j the video's frame clamp(a - h_n + j, 0, N - 1).  Outputs as
 * vy_net_forward_infer at batch = centres, row-block c the detections of frame a + c.  x is only read.  Asynchronous. */
int vy_net_hier_video_detect(vy_net* net, const float* x, float* ids, float* scores, float* bboxes, int32_t* keep_idx,
                             void* stream);

/* The detection tail ALONE, on caller-supplied prediction-conv outputs: YOLOOutputV3.hybrid_forward's inference branch
 * (yolo3.py:158-197: decode, x C tile, class-major rows) for the three scales, their concat (yolo3.py:1195), box_nms and
 * the slice (yolo3.py:1197-1206) — what `net.yolo_outputs[i](pred)` + `F.contrib.box_nms` compute in the reference.
 *   head_i   device, (batch, 3*(5+C), H_i, W_i) fp32 NCHW for strides 32, 16, 8 (the layout vy_net_read_head returns),
 *            H_i x W_i of the bound workspace's plan
 * Outputs as vy_net_forward_infer (nms_thresh outside (0,1): the (B, N*C, 6) detection tensor itself).  This is the
 * operator-level door the golden-vector kit uses (tests/golden/make_mxnet_goldens.py: hand-built logits decide threshold
 * strictness, tie order and the top-k cut on the SAME kernels a forward runs); it overwrites the head planes of the
 * workspace.  Asynchronous on `stream`. */
int vy_net_detect_heads(vy_net* net, const float* head0, const float* head1, const float* head2, float* ids,
                        float* scores, float* bboxes, int32_t* keep_idx, void* stream);

/* Debug / parity taps (asynchronous on `stream`, valid after a forward on the same stream):
 * copy head i's prediction-conv output (yolo3.py:154 `pred`) to dst as (batch, 3*(5+C), H_i, W_i)
 * NCHW — i = 0,1,2 for strides 32,16,8. */
int vy_net_read_head(vy_net* net, int32_t i, float* dst_dev, void* stream);
/* copy the activation of feature cell `name` ("stages.0.14", "yolo_blocks.1.tip", ...) to dst
 * as NCHW; returns its channel count / height / width through the out pointers.  With dst != NULL it needs a plan
 * that keeps every plane (vy_net_set_keep_activations, or a training plan): VY_ERR_STATE otherwise. */
int vy_net_read_activation(vy_net* net, const char* name, float* dst_dev, int32_t* c, int32_t* h,
                           int32_t* w, void* stream);

/* Per-launch device timing of the last forward: runs one forward with HIP events recorded on
 * `stream` around every kernel launch and returns, for launch j < *n, its name, the kernel
 * time in ms and its algorithmic FLOPs (2*MAC; 0 for non-conv launches).  Synchronises. */
typedef struct vy_launch_stat {
  char name[64];
  float ms;
  double flops;
  double bytes;   /* algorithmic HBM bytes (inputs read once + outputs written once) */
} vy_launch_stat;
int vy_net_profile_infer(vy_net* net, const float* x, float* ids, float* scores, float* bboxes,
                         vy_launch_stat* stats, int32_t* n, void* stream);

/* A HIP stream owned by the caller and created by the library (hipStreamCreateWithFlags, non-blocking):
 * its own hardware queue, for callers that run two launch sequences side by side — the reference's
 * `for x in data:` loop over per-device batches (detect_yolo3.py:211-222) on ONE device's two half
 * batches.  (torch's pooled streams may share the default stream's queue.) */
int vy_stream_create(void** stream);
int vy_stream_destroy(void* stream);

/* Frame pre-processing in front of the path: (batch,H,W,3) uint8 HWC device
 * frames -> (batch,3,H,W) fp32 NCHW, y = (x/255 - mean[c]) / std[c] — mx.nd.image.to_tensor +
 * mx.nd.image.normalize at models/definitions/yolo/transforms.py:331-334.  mean3/std3 are host
 * pointers to 3 floats.  Any height, width >= 1 and any byte address of frames_hwc are accepted: where
 * height*width is a multiple of 4, frames_hwc is 4-byte and out_nchw 16-byte aligned, a thread converts 4
 * pixels with 32-bit loads; otherwise a thread converts one pixel with byte loads, the same arithmetic per value.
 * Frames that are not at the network size yet: vy_preprocess_resize_frames below. */
int vy_preprocess_frames(const uint8_t* frames_hwc, float* out_nchw, int32_t batch, int32_t height,
                         int32_t width, const float* mean3, const float* std3, void* stream);

/* The whole YOLO3VideoInferenceTransform.__call__ (models/definitions/yolo/transforms.py:316-350) in one
 * launch: (batch, src_height, src_width, 3) uint8 device frames -> resize to (height, width) as
 * timage.imresize(frame, width, height, interp=9) does (:325-327: OpenCV INTER_AREA when both sides shrink,
 * INTER_CUBIC when both grow, INTER_LINEAR otherwise, on uint8 with OpenCV's fixed-point / float arithmetic
 * [UPSTREAM-RECALLED: gluoncv, mxnet and OpenCV are not available here; oracle/resize_oracle.py states the
 * arithmetic and tests/test_resize_oracle.py cross-checks it against torch / exact area definitions]) -> the
 * uint8 value the reference's resized NDArray would hold -> to_tensor + normalize -> (batch,3,height,width)
 * fp32 NCHW.  The resized frame itself is never materialised.  Fractional area shrink factors above 10 on
 * either axis are rejected; integer factors on both axes are block means of any size.  Frames already at
 * (height, width) are copied (cv::resize to the same size), at any size: vy_preprocess_frames. */
int vy_preprocess_resize_frames(const uint8_t* frames_hwc, int32_t src_height, int32_t src_width, float* out_nchw,
                                int32_t batch, int32_t height, int32_t width, const float* mean3, const float* std3,
                                void* stream);

/* The frames side of YOLO3VideoTrainTransform.__call__ (models/definitions/yolo/transforms.py:199-245) for a batch of
 * clips in one launch: colour distortion -> expansion onto a filled canvas -> crop -> resize with one of five
 * interpolations -> horizontal flip -> to_tensor -> normalize.  The random draws are the caller's
 * (videoyolo_amd.transforms.YOLO3VideoTrainTransform.draw); a vy_train_aug holds one sample's.  No intermediate image
 * exists: a thread per destination pixel walks back to its source taps.  After the colour step the reference's frames are
 * float32, so nothing is rounded or clamped on the way [UPSTREAM-RECALLED arithmetic, DESIGN.md §13;
 * tests/train_transform_ref.py states it op by op and is what the tests compare with, bit for bit].
 *
 * Geometry of a descriptor: the sample's k frames (src_h, src_w, 3) uint8 lie one after another from byte src_offset of
 * `frames`; the source is pasted at (paste_x, paste_y) into a canvas_w x canvas_h canvas of the fill colour (no
 * expansion: the canvas is the source, paste 0); the crop rectangle (crop_x, crop_y, crop_w, crop_h) of the canvas is
 * resized to (height, width) with `interp` (0 nearest, 1 linear, 2 cubic, 3 area, 4 Lanczos-4; OpenCV's numbering) and
 * mirrored when `flip`.  Colour ops run in the order listed on every source pixel read (the fill is not distorted):
 *   VY_AUG_BRIGHTNESS  v + a          VY_AUG_CONTRAST  v * a
 *   VY_AUG_SATURATION  g = ((r * 0.299 + g * 0.587) + b * 0.114) * b_arg ; v * a + g      (b_arg = 1 - alpha)
 *   VY_AUG_HUE         out[c] = (r * hue[0][c] + g * hue[1][c]) + b * hue[2][c] */
#define VY_AUG_BRIGHTNESS 1
#define VY_AUG_CONTRAST 2
#define VY_AUG_SATURATION 3
#define VY_AUG_HUE 4
#define VY_AUG_MAX_OPS 4
typedef struct vy_train_aug {
  int64_t src_offset;
  int32_t src_h, src_w;
  int32_t paste_x, paste_y;
  int32_t canvas_w, canvas_h;
  int32_t crop_x, crop_y, crop_w, crop_h;
  int32_t interp, flip;
  int32_t num_ops;
  int32_t op[VY_AUG_MAX_OPS];
  float a[VY_AUG_MAX_OPS];
  float b[VY_AUG_MAX_OPS];
  float hue[3][3];
} vy_train_aug;
/* The descriptors travel in the kernel arguments (no device memory of the library's, no copy, no synchronisation):
 * VY_AUG_CHUNK of them (144 bytes each) fit the 4 KB argument segment, and a larger batch goes out as several launches. */
#define VY_AUG_CHUNK 24
/* frames: device bytes; augs: HOST array of `batch` descriptors; out: device (batch, k, 3, height, width) fp32;
 * fill3 / mean3 / std3: host pointers to 3 floats (the fill in 0..255 units, mean * 255 in the reference).  Every
 * descriptor is checked before anything is launched — sizes >= 1, the paste and the crop inside the canvas, interp in
 * 0..4, known op codes, at most VY_AUG_MAX_OPS of them, a non-negative offset — else VY_ERR_INVALID and no launch. */
int vy_train_transform(const uint8_t* frames, const vy_train_aug* augs, int32_t batch, int32_t k, float* out,
                       int32_t height, int32_t width, const float* fill3, const float* mean3, const float* std3,
                       void* stream);

/* Mixup in the same launch: gluoncv.data.MixupDetection.__getitem__ (the wrapper train_yolov3.py:227-229, 571-581 puts
 * round its dataset) blends two images on a zero canvas of the larger height and width, both at the origin, and rounds the
 * blend back to uint8 before the transform sees it [UPSTREAM-RECALLED: gluoncv is not available here; restated from
 * memory, DESIGN.md §18].  Here nothing is blended ahead of the launch: a vy_train_mix beside a sample's vy_train_aug names
 * its two sources and the kernel blends every pixel it reads, before the colour ops:
 *   l1 = (float)lambd, l2 = (float)(1.0 - lambd)            the subtraction in double, by the caller
 *   both sources cover the pixel    m = (float)p1 * l1 + (float)p2 * l2     each product rounded to fp32, then added
 *   only the first                  m = (float)p1 * l1
 *   only the second                 m = 0.0f + (float)p2 * l2
 *   neither                         m = 0
 *   the mixed pixel is (uint8)m, truncated toward zero (not rounded); it cannot leave [0, 255]
 * Unlike gluoncv, which mixes single images, a clip is mixed frame t with frame t (both sources hold k frames).
 *
 * The first source's k frames (h1, w1, 3) lie from byte src_offset of the sample's vy_train_aug, the second's (h2, w2, 3)
 * from byte src2_offset; the aug's src_h x src_w is the mix canvas, max(h1, h2) x max(w1, w2), and everything else in the
 * vy_train_aug means what it means for vy_train_transform with the canvas as the source.  src2_offset = -1: no second
 * source — the sample is read as vy_train_transform reads it (src_h x src_w = h1 x w1; h2, w2, l1 and l2 are not used
 * but are checked like the others), so a batch may hold mixed and unmixed samples. */
typedef struct vy_train_mix {
  int64_t src2_offset;
  int32_t h1, w1;
  int32_t h2, w2;
  float l1, l2;
} vy_train_mix;
/* Both descriptors travel in the kernel arguments, 144 + 32 bytes a sample: VY_MIX_CHUNK samples per launch. */
#define VY_MIX_CHUNK 22
/* vy_train_transform with a HOST array of `batch` vy_train_mix beside augs.  Every descriptor is checked before anything
 * is launched: what vy_train_transform checks, and all four extents >= 1, src_h x src_w equal to the larger of the two
 * extents (to the first's when there is no second source), src2_offset >= 0 or exactly -1, 0 <= l1, l2 <= 1 — else
 * VY_ERR_INVALID naming the descriptor, and no launch. */
int vy_train_transform_mix(const uint8_t* frames, const vy_train_aug* augs, const vy_train_mix* mixes, int32_t batch,
                           int32_t k, float* out, int32_t height, int32_t width, const float* fill3, const float* mean3,
                           const float* std3, void* stream);
/* Host-only (no device is touched): include/vy_math.h's vy_lanczos4_weights, the eight Lanczos-4 tap weights the
 * kernel uses for the fractional position x, for checkers. */
void vy_math_lanczos4(float x, float* w8);

/* The matching step of the ImageNet-VID motion / area mAP (metrics/imgnetvid.py:191-276, vid_eval_motion) for a batch of
 * frames on the device: in every (motion range, area range) slice a frame's detections claim its ground truths greedily
 * in score order.  videoyolo_amd/metrics.py states the rule (vid_match_host); the kernel (csrc/vid_metric.hip) walks one
 * (frame, slice) chain per lane, all float64, and gives the same values.  Needs no vy_net.
 *
 * Detections — device arrays over all rows of the batch: det_box (n, 4) float64 corners, det_label (n) int32, det_score
 * (n) float64; frame i owns rows det_off[i] .. det_off[i + 1], ALREADY in descending score order.  A row with a negative
 * label or a score that is not >= conf_thresh is skipped wherever it lies: its outputs are 0.
 * Ground truths — device tables over a whole dataset of n_gt_frames frames: gt_box (G, 4) float64, gt_label (G) int32,
 * gt_thr (G) the IoU a match needs, gt_motion (G) motion IoU, and gt_nig (n_gt_frames, n_motion) int32, per frame and
 * motion range the number of its ground truths outside the range (its own count: with a class map the reference counts
 * the unmapped list).  Row r owns ground truths gt_off[r] .. gt_off[r + 1]; frame i of the batch is row gt_frame[i].
 * motion_ranges (n_motion, 2) and area_ranges (n_area, 2) are [lo, hi] pairs, both ends inside; empty_weight (n_motion)
 * is the false-positive weight of an unmatched detection in a frame without ground truth.  Slice s = motion * n_area +
 * area.  det_off, gt_frame, gt_off, the ranges and empty_weight are HOST arrays and travel in the kernel arguments,
 * VY_VID_CHUNK frames per launch.
 * flags: device scratch of flags_bytes >= (ground truths of the batch's frames) * n_motion * n_area bytes, one detected
 * flag per (ground truth, slice); the kernel clears what it uses.  tp (n, slices) uint8 and fp (n, slices) float64,
 * device: every element of the batch's rows is written.
 * Checked before anything is launched, else VY_ERR_INVALID: null pointers, negative counts, 1..VY_VID_MAX_RANGES ranges
 * of each kind with lo <= hi, ascending det_off, gt_frame inside the table, ascending gt_off at every row used, enough
 * flag bytes.  No frames or no rows: VY_OK without a launch.  Asynchronous on `stream`; no device memory of the
 * library's, no copy, no synchronisation. */
#define VY_VID_MAX_RANGES 8
#define VY_VID_CHUNK 64
int vy_vid_match(int32_t n_frames, const int64_t* det_off, const double* det_box, const int32_t* det_label,
                 const double* det_score, double conf_thresh, const int32_t* gt_frame, int32_t n_gt_frames,
                 const int64_t* gt_off, const double* gt_box, const int32_t* gt_label, const double* gt_thr,
                 const double* gt_motion, const int32_t* gt_nig, int32_t n_motion, const double* motion_ranges,
                 int32_t n_area, const double* area_ranges, const double* empty_weight, uint8_t* flags,
                 int64_t flags_bytes, uint8_t* tp, double* fp, void* stream);

/* The matching step of the PASCAL-VOC mAP (metrics/pascalvoc.py:84-170, VOCMApMetric.update; the metric both drivers
 * build, train_yolov3.py:181 and detect_yolo3.py:183, and validate() feeds per batch, train_yolov3.py:434-490) for a batch
 * of images on the device, one launch.  videoyolo_amd/metrics.py states the rule (voc_match_host); the kernel
 * (csrc/voc_metric.hip) runs one 256-thread workgroup per image and gives the same values.  Needs no vy_net.
 *
 * Detections — device arrays as the detector returns them: det_box (batch, rows, 4) fp32 corners, det_label (batch, rows)
 * fp32 class index, det_score (batch, rows) fp32, in any order; a row whose label is not >= 0 is padding wherever it lies.
 * Ground truths — device arrays: gt_box (batch, n_gt, 4) fp32, gt_label (batch, n_gt) int32, ALREADY class-mapped, < 0 =
 * skip, gt_difficult (batch, n_gt) bytes, non-zero = difficult, or NULL (none is).
 * Per row: its candidate is the ground truth of its own label with the largest IoU (fp32, no +1 pixel offset, in
 * pairwise_iou's operation order; the first index on a tie, a NaN IoU counting as the largest), or none when that IoU
 * < iou_thresh (false for NaN).  best (batch, rows) int32: the candidate's index in the image's n_gt, or -1.
 * flags (batch, rows) int8: -2 padding; 0 no candidate; -1 the candidate is difficult; else 1 unless another row of the image
 * with the same candidate comes before this one (a higher score; at equal scores the lower row), then 0.  Every element of
 * both outputs is written, in input row order.
 * rows <= VY_VOC_ROWS_MAX per image: score and candidate of every row of an image are held in LDS, 8 bytes per row, 8 KiB
 * at the limit.  n_gt is not limited.
 * Checked before anything is launched, else VY_ERR_INVALID: null pointers (gt_difficult excepted), negative counts, rows
 * above the limit, iou_thresh not finite.  batch == 0 or rows == 0: VY_OK without a launch.  Asynchronous on `stream`; no
 * device memory of the library's, no copy, no synchronisation. */
#define VY_VOC_ROWS_MAX 1024
int vy_voc_match(int32_t batch, int32_t rows, int32_t n_gt, const float* det_box, const float* det_label,
                 const float* det_score, const float* gt_box, const int32_t* gt_label, const uint8_t* gt_difficult,
                 float iou_thresh, int32_t* best, int8_t* flags, void* stream);

/* The per-frame mean AP (detect_yolo3.py:451-534, add_metrics_to_predictions: metric.reset(); metric.update(one frame);
 * metric.get() per frame, the eighth column of its prediction files and what summary.txt ranks clips by) for a batch of
 * images on the device, one launch, from the flags of the match above.  videoyolo_amd/metrics.py states the rule
 * (frame_map_host); the kernel (csrc/voc_metric.hip) runs one 256-thread workgroup per image.  Needs no vy_net.
 *
 * det_label, det_score (batch, rows) fp32 and flags (batch, rows) int8 as given to and written by the match (1 TP, 0 FP,
 * -1 matched a difficult ground truth: neither, -2 padding); gt_label (batch, n_gt) int32 class-mapped, < 0 = skip;
 * gt_difficult (batch, n_gt) bytes or NULL — the same arrays.
 * Per image: class c has npos = its ground truths that are not difficult; only classes with npos > 0 are averaged (one
 * without a detection with AP 0; one with detections and npos = 0 not at all).  A class's rows rank by score descending, at
 * equal scores the lower row first; tp / fp at a row count the flag-1 / flag-0 rows at or ahead of it, prec = tp / (tp + fp)
 * (0 / 0 -> 0), rec = tp / npos.  use_07 == 0, area AP: the sum over the class's TP rows of (tp / npos - (tp - 1) / npos) x
 * the largest prec at or behind the row.  use_07 != 0, 11-point AP: for k = 0..10, t = 0.0 + k * 0.1, ap += (the largest
 * prec over rows with rec >= t, else 0) / 11.  All float64, the divides correctly rounded.
 * frame_ap (batch) float64: the sum of the classes' AP / their number, NaN when there is none.  frame_classes (batch)
 * int32: that number.  The sum is formed in a fixed order without floating-point atomics: an image's value is the same
 * bits on every run and in any batch.
 * rows <= VY_VOC_ROWS_MAX per image: 25 bytes of LDS per row, 25 KiB at the limit.  n_gt is not limited; counting the
 * scored classes costs up to n_gt^2 / 256 label reads per lane and image.
 * Checked before anything is launched, else VY_ERR_INVALID: null pointers (gt_difficult excepted), negative counts, rows
 * above the limit.  batch == 0: VY_OK without a launch; rows == 0 is launched (0.0 with ground truth, NaN without).
 * Asynchronous on `stream`; no device memory of the library's, no copy, no synchronisation. */
int vy_voc_frame_ap(int32_t batch, int32_t rows, int32_t n_gt, const float* det_label, const float* det_score,
                    const int8_t* flags, const int32_t* gt_label, const uint8_t* gt_difficult, int32_t use_07,
                    double* frame_ap, int32_t* frame_classes, void* stream);

/* The matching step of the COCO detection metric (metrics/mscoco.py, COCODetectionMetric: the second metric the detect
 * driver builds by default, detect_yolo3.py:185; the reference hands the evaluation to pycocotools' COCOeval, iouType
 * 'bbox', whose per-image rule is restated in videoyolo_amd/metrics.py, coco_match_host, [UPSTREAM-RECALLED]) for a batch
 * of images on the device, one launch per VY_COCO_CHUNK images.  The kernel (csrc/coco_metric.hip) runs one 256-thread
 * workgroup per image and gives coco_match_host's values.  Needs no vy_net.
 *
 * Detections — device arrays: det_xywh (batch, rows, 4) float64 [x, y, w, h], det_cat (batch, rows) int32 category index
 * (a position in the ground-truth file's sorted category ids), < 0 = the row takes no part wherever it lies, det_score
 * (batch, rows) float64, in any order.
 * Ground truths — device tables over a whole dataset of n_images images: gt_xywh (G, 4) float64, gt_cat (G) int32 category
 * index (< 0: never matched), gt_area (G) float64 the file's area, gt_crowd (G) bytes, gt_id (G) int64 the annotation's
 * id.  Row r owns ground truths gt_off[r] .. gt_off[r + 1]; image i of the batch is row gt_image[i].  iou_thrs (n_thr)
 * and area_ranges (n_area, 2), [lo, hi] with both ends inside, are float64.  gt_image, gt_off, iou_thrs and area_ranges
 * are HOST arrays and travel in the kernel arguments.
 * Per image and category the kept rows are taken in stable descending score order (a NaN last), the first max_det of
 * them; in every (area range, threshold) pair they claim ground truths of their category as COCOeval.evaluateImg does.
 * rank (batch, rows) int32: the row's position in that order, -1 for a row that takes no part or whose position is
 * >= max_det.  flags (batch, rows, n_area, n_thr) bytes: bit 0 the row is matched to an annotation whose id is not 0,
 * bit 1 the row is ignored; 0 where rank is -1.  Every element of both is written, in input row order.
 * taken: device scratch of taken_bytes >= (ground truths of the batch's images) * n_area * n_thr bytes; the kernel clears
 * what it uses.  rows <= VY_COCO_ROWS_MAX per image (score, category and order table in LDS, 16 bytes per row).
 * Checked before anything is launched, else VY_ERR_INVALID: null pointers, negative counts, rows above the limit,
 * 1..VY_COCO_MAX_THRS finite thresholds, 1..VY_COCO_MAX_RANGES ranges with lo <= hi, gt_image inside the table, ascending
 * gt_off at every row used, enough taken bytes.  batch == 0 or rows == 0: VY_OK without a launch.  Asynchronous on
 * `stream`; no device memory of the library's, no copy, no synchronisation. */
#define VY_COCO_ROWS_MAX 1024
#define VY_COCO_MAX_THRS 16
#define VY_COCO_MAX_RANGES 8
#define VY_COCO_CHUNK 128
int vy_coco_match(int32_t batch, int32_t rows, const double* det_xywh, const int32_t* det_cat, const double* det_score,
                  const int32_t* gt_image, int32_t n_images, const int64_t* gt_off, const double* gt_xywh,
                  const int32_t* gt_cat, const double* gt_area, const uint8_t* gt_crowd, const int64_t* gt_id,
                  int32_t n_thr, const double* iou_thrs, int32_t n_area, const double* area_ranges, int32_t max_det,
                  uint8_t* taken, int64_t taken_bytes, int32_t* rank, uint8_t* flags, void* stream);

/* Prefetch target generation on the device: YOLOV3PrefetchTargetGenerator.forward,
 * models/definitions/yolo/yolo_target.py:31-148 (called per sample from the DataLoader transform,
 * transforms.py:259-277), for a whole batch.  gt_boxes (batch,num_gt,4) corner pixels of the
 * (height,width) network input, gt_ids (batch,num_gt) class index as fp32, gt_mixratio (batch,num_gt)
 * or NULL; a row with any negative coordinate ends that image's list (:107-108).  Outputs, all fp32
 * device buffers fully written: objness_t (batch,N,1), centers_t / scales_t / weights_t (batch,N,2),
 * clas_t (batch,N,num_class), N = vy_net_num_anchors order (stride 32,16,8 -> cell -> anchor) — exactly
 * the five tensors vy_net_train_forward takes.  Anchors are the yolo3_darknet53 table (wrappers.py:80-84). */
int vy_prefetch_targets(const float* gt_boxes, const float* gt_ids, const float* gt_mixratio, int32_t batch,
                        int32_t num_gt, int32_t height, int32_t width, int32_t num_class, float* objness_t,
                        float* centers_t, float* scales_t, float* weights_t, float* clas_t, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training step.  Reference call pattern, train_yolov3.py:623-634:
 *     with autograd.record():
 *         obj, ctr, scl, cls = net(x, gt_boxes, obj_t, centers_t, scales_t, weights_t, clas_t)
 *         autograd.backward(obj + ctr + scl + cls)
 *     trainer.step(batch_size)
 * The caller owns two more device buffers of vy_net_param_bytes each (gradients, SGD momentum;
 * same element offsets as the parameter buffer: one contiguous range for the RCCL all-reduce) and a
 * training workspace (activations, raw conv outputs / their gradients, gradient planes, scratch).
 * ---------------------------------------------------------------------------------------------- */
/* Training shapes: height and width multiples of 32, as train_yolov3.py produces them (0 / VY_ERR_UNSUPPORTED
 * otherwise). */
size_t vy_net_train_workspace_bytes(const vy_net* net, int32_t batch, int32_t height, int32_t width);
/* Binds the training workspace (also serves inference at that shape), the gradient buffer and the
 * momentum buffer (the caller zero-initialises the momentum once); zeroes the workspace
 * asynchronously on `stream`.  The training plan holds while this bind is the net's last: after vy_net_bind_workspace
 * or vy_net_bind_video, at whatever shape, vy_net_train_forward* / vy_net_train_mode_forward* return VY_ERR_STATE
 * ("training workspace not bound") until vy_net_bind_train is called again. */
int vy_net_bind_train(vy_net* net, void* dev_ws, size_t bytes, int32_t batch, int32_t height,
                      int32_t width, void* dev_grads, void* dev_momentum, void* stream);

/* The regions a plan carves out of the workspace, one per call, in offset order: region `index` of the clip plan
 * (VY_PLAN_CLIP: what vy_net_workspace_bytes sizes; frames, ring ignored), the training plan (VY_PLAN_TRAIN: the clip plan
 * with every plane kept, then the training regions), the video plan (VY_PLAN_VIDEO: batch counts clips) or the hier-video
 * plan (VY_PLAN_HIER_VIDEO: batch counts the centres, frames is the step, ring ignored) of the shape.
 * name: the carve — "fold", "det.state" .. "det.score", "sk.flags", "sk.slabs", "ck", "wsplit:<cell>", "wino:<cell>",
 * "plane:<the first cell that writes the slot>", "ring"; "dgrad_image:<cell>", "grad:<plane>", "z:<cell>", "train.save" ..
 * "train.chunk", "wgrad_table:<cell>".  bytes: what the plan means the kernels to use, from offset on; span: the bytes up
 * to the next region's offset (to the plan's total for the last one): bytes, the rounding to 256 and the guard gap.
 * With VY_PLAN_GUARD=<n> in the environment when the net is created (0, the default, or a multiple of 256 up to 1 MiB;
 * anything else counts as 0) every region is followed by n bytes that no launch may touch; the sizing queries and the
 * binds count them in.  A host-side query like the sizing queries: it needs no device and no bound workspace, plans anew
 * and changes nothing on the handle.  VY_ERR_RANGE for an index past the last region, VY_ERR_INVALID for a shape the
 * matching sizing query refuses.  Tests only. */
enum vy_plan_kind { VY_PLAN_CLIP = 0, VY_PLAN_TRAIN = 1, VY_PLAN_VIDEO = 2, VY_PLAN_HIER_VIDEO = 3 };
typedef struct vy_plan_region {
  char name[96];
  size_t offset, bytes, span;
} vy_plan_region;
int vy_net_plan_region(const vy_net* net, int32_t plan, int32_t batch, int32_t height, int32_t width, int32_t frames,
                       int32_t ring, int32_t index, vy_plan_region* out);

/* YOLOV3T(ignore_iou_thresh=0.7) (yolo3.py:962) and net._target_generator._label_smooth
 * (train_yolov3.py:499-500, yolo_target.py:272-278). */
int vy_net_set_train_options(vy_net* net, float ignore_iou_thresh, int32_t label_smooth);

/* net(x, gt_boxes, *fixed_targets) under autograd.record() — yolo3.py:1126-1187 with BatchNorm on
 * batch statistics (running stats updated, momentum 0.9), YOLOV3TargetMerger (yolo_target.py:
 * 226-281) and YOLOV3Loss.  Also computes d(sum of the four losses)/d(raw predictions), so that
 * vy_net_train_backward only has to walk the network.
 *   x (B,3,H,W)  gt_boxes (B,M,4) corner px, -1 padded   obj_t (B,N,1)  centers_t/scales_t/weights_t
 *   (B,N,2)  clas_t (B,N,C) — N anchors in the reference order (stride 32,16,8; cell; anchor)
 *   losses: device (4,B): obj, center, scale, cls per sample.
 *   M <= 4096 (more is an error return): the loss kernel stages one image's gt rows in LDS, 16 M bytes next to its 64
 *   static ones — 65,600 bytes at the cap, inside the 160 KiB a workgroup may hold on gfx950 (granted there:
 *   tests/test_gpu_loss_cells.py runs the cap and cap + 1). */
int vy_net_train_forward(vy_net* net, const float* x, const float* gt_boxes, int32_t M,
                         const float* obj_t, const float* centers_t, const float* scales_t,
                         const float* weights_t, const float* clas_t, float* losses, void* stream);
/* ... of a heads-only net on the three route tensors (train_yolov3.py:595-606 with --features_dir). */
int vy_net_train_forward_routes(vy_net* net, const float* f0, const float* f1, const float* f2, const float* gt_boxes,
                                int32_t M, const float* obj_t, const float* centers_t, const float* scales_t,
                                const float* weights_t, const float* clas_t, float* losses, void* stream);

/* ... of a windowed heads-only net on a bank of per-frame routes and a table (vy_net_forward_infer_bank). */
int vy_net_train_forward_bank(vy_net* net, const float* f0, const float* f1, const float* f2, int32_t n_frames,
                              const int32_t* table, const float* gt_boxes, int32_t M, const float* obj_t,
                              const float* centers_t, const float* scales_t, const float* weights_t, const float* clas_t,
                              float* losses, void* stream);

/* net(x) under autograd.train_mode() without recording — yolo3.py:1189-1192, the branch the DataLoader
 * transform drives (transforms.py:190-193): the network runs with BatchNorm on batch statistics (running
 * stats updated, as mxnet's BatchNorm does whenever is_training), and the per-anchor tensors of
 * YOLOOutputV3's training return (yolo3.py:179-182) come back concatenated over the scales (stride 32, 16,
 * 8 -> cell -> anchor):  box_preds (B,N,4) decoded corner boxes, centers (B,N,2) / scales (B,N,2) /
 * objness (B,N,1) / class_pred (B,N,C) RAW predictions.  Items 1-3 of the reference's 8-tuple (anchors,
 * offsets, fake feature maps) are constants of the input shape and are built by the host mirror.
 * Needs the training workspace (vy_net_bind_train).  All outputs are device buffers. */
int vy_net_train_mode_forward(vy_net* net, const float* x, float* box_preds, float* centers, float* scales,
                              float* objness, float* class_pred, void* stream);
/* ... of a heads-only net on the three route tensors. */
int vy_net_train_mode_forward_routes(vy_net* net, const float* f0, const float* f1, const float* f2, float* box_preds,
                                     float* centers, float* scales, float* objness, float* class_pred, void* stream);
/* ... of a windowed heads-only net on a bank of per-frame routes and a table. */
int vy_net_train_mode_forward_bank(vy_net* net, const float* f0, const float* f1, const float* f2, int32_t n_frames,
                                   const int32_t* table, float* box_preds, float* centers, float* scales, float* objness,
                                   float* class_pred, void* stream);

/* autograd.backward(sum_losses) (train_yolov3.py:631): fills the gradient buffer (every trainable
 * tensor, device layout) from the state left by the last vy_net_train_forward.  `x` is the same
 * image batch (needed by the stem's weight gradient). */
int vy_net_train_backward(vy_net* net, const float* x, void* stream);
/* ... of a heads-only net: the head cells' gradients only — no data gradient into the routes (yolo_blocks.0.body.0 gets
 * none, yolo_blocks.1/2.body.0 only that of the upsampled-transition channels of their concat input).  The routes are the
 * ones of the recorded forward; nothing is read from them here.  Also the backward of a windowed heads-only net
 * (vy_net_train_forward_bank), which ignores f0, f1, f2: NULL is allowed there. */
int vy_net_train_backward_routes(vy_net* net, const float* f0, const float* f1, const float* f2, void* stream);

/* Per-parameter optimizer attributes: Parameter.lr_mult / wd_mult (train_yolov3.py:496-497) and
 * grad_req = 'null' (enabled = 0; wrappers.py:55-57 freeze_base). */
int vy_net_param_set_opt(vy_net* net, int32_t i, float lr_mult, float wd_mult, int32_t enabled);

/* trainer.step(batch_size) for Trainer('sgd', {wd, momentum}) (train_yolov3.py:527-530,634):
 * g = rescale_grad*grad + wd*w ; mom = momentum*mom - lr*g ; w += mom.  rescale_grad = 1/batch_size.
 * Gradients must already be summed across ranks (all-reduce of the gradient buffer). */
int vy_net_sgd_step(vy_net* net, float lr, float momentum, float wd, float rescale_grad, void* stream);

/* Gradient of parameter i in the REFERENCE layout to host memory (tests / checkpoints). */
int vy_net_grad_get(vy_net* net, int32_t i, float* host_dst, void* stream);

/* Parity tap: gradient w.r.t. the output of cell `name` after vy_net_train_backward, as NCHW at the
 * resolution the output is stored (x2 for the transition cells). */
int vy_net_read_grad_activation(vy_net* net, const char* name, float* dst_dev, void* stream);

/* Test-only taps of the training step (per-cell parity checks; off the step's path).  Cell `name` (as in
 * vy_net_conv_info), one of:
 *   VY_TAP_Z             the cell's raw conv-output plane with its border, NCHW (B, Cout, H+2, W+2): z after
 *                        vy_net_train_forward, dz after vy_net_train_backward (BatchNorm cells only)
 *   VY_TAP_BN            [4][Cout]: the saved batch mean, the saved invstd, and the scale / shift the forward apply
 *                        and the backward kernels used (BatchNorm cells only)
 *   VY_TAP_GRAD_PADDED   the gradient of the cell's output channels with the border of their plane, NCHW
 *                        (B, Cout, Ho+2, Wo+2) at the resolution the output is stored (x2 for the transitions)
 *   VY_TAP_INPUT_PADDED  the input view the cell's conv reads, border included, NCHW (B, Cin, Hi+2, Wi+2) (not the stem)
 * dims (int32[4], may be NULL) receives the tensor's shape; dst_dev NULL: shape only. */
#define VY_TAP_Z 0
#define VY_TAP_BN 1
#define VY_TAP_GRAD_PADDED 2
#define VY_TAP_INPUT_PADDED 3
int vy_net_read_train_tap(vy_net* net, const char* name, int32_t which, float* dst_dev, int32_t* dims, void* stream);

/* Host-only: the accumulation plan of conv i in the bound training plan — the weight gradient's split-K (pixel splits,
 * pixels per split; the stem: the fp32 accumulators a block adds, the pixels one of them sums) and the BatchNorm backward's image rows per
 * partial chunk (0: no BatchNorm).  Any pointer may be NULL. */
int vy_net_train_conv_plan(const vy_net* net, int32_t i, int32_t* wgrad_splits, int32_t* wgrad_k_per_split,
                           int32_t* bn_bwd_rows_per_chunk);

/* SyncBatchNorm(num_devices) (train_yolov3.py:352-354).  With world > 1 the BatchNorm layers that
 * the reference builds with the passed norm_layer — the stem and the five stride-2 convs of
 * Darknet-53 (three_darknet.py:163-181; the residual blocks hard-code BatchNorm, :193-194, and
 * wrappers.py:101-103 does not forward norm_layer to YOLOV3T) — call `cb` to sum their [2][C]
 * double-precision statistics over all ranks, forward and backward.  cb(user, device_ptr, count)
 * must all-reduce (sum) `count` doubles in place, ordered with the stream passed to the step. */
typedef int (*vy_allreduce_cb)(void* user, void* dev_ptr, int64_t count);
int vy_net_set_sync_bn(vy_net* net, int32_t world, vy_allreduce_cb cb, void* user);

/* Bucketed gradient exchange: during vy_net_train_backward `cb(user, elem_offset, elem_count)` is
 * called each time a contiguous range of the gradient buffer is final (heads first, then Darknet
 * stages 2, 1, 0), after the kernels producing it were enqueued — the caller records an event and
 * all-reduces that range on a side stream, overlapping the rest of the backward pass. */
typedef int (*vy_grad_bucket_cb)(void* user, int64_t elem_offset, int64_t elem_count);
int vy_net_set_grad_bucket_cb(vy_net* net, vy_grad_bucket_cb cb, void* user);

#ifdef __cplusplus
}
#endif
#endif /* VYOLO_H */
