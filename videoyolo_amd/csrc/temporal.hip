// temporal.hip — early temporal join of a k-frame clip net (YOLOV3T with k_join_pos='early', yolo3.py:1106-1121):
// TemporalPooling 'direct' (layers.py:193-204) of the three Darknet-53 routes over each clip's k frames.  The backbone ran
// on B*k frames (TimeDistributed 'reshape1', layers.py:240-248: frame t of clip b is frame b*k + t); its per-frame route
// planes are pooled into the planes the heads read, where a single-frame net's backbone writes them: channels [128, 384)
// of the stride-8 concat plane, [256, 768) of the stride-16 one, and a pooled 1024-channel stride-32 plane.
//
// Arithmetic (a project choice, restated by the test references):
//   mean  forward  fp32 acc = x0; acc += x1; ...; out = acc / (float)k, in frame order (the library is built with
//                  -ffp-contract=off)
//         backward every frame gets g / (float)k                                            [UPSTREAM-RECALLED]
//   max   forward  strict > in frame order: on ties the earliest frame's bits are kept
//         backward every frame whose value equals the max (x_t == pooled, IEEE equality) gets the full g, the others 0 —
//                  mxnet's reduce-max backward, not torch's amax, which splits g among ties       [UPSTREAM-RECALLED]
//
// Streaming kernels: one lane owns 4 consecutive channels (16-B accesses, cs and co multiples of 4, plane offsets 256-B
// aligned) of one pooled pixel and loops over the clip's k frames; consecutive lanes walk the channels, then the pixels, so
// a wave moves 1 KiB contiguous per frame.  Forward: k reads, one write.  Backward: the pooled gradient (and, for max, the
// pooled value) is read once per lane, then each frame's value is read (max) and its gradient written — every byte moves
// once (a lane per frame re-read the pooled planes k times: 0.35-0.58 of the copy rate).  Only interior pixels of the
// route's channels are written; borders and the concat planes' transition channels never are.
#include "kernels.h"
#include "../../include/vyolo.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

struct Item {
  int r;
  long long i;  // index inside route r
};

__device__ inline Item locate(const WindowPoolArgs& a, long long g) {
  Item t;
  t.r = 0;
  while (t.r + 1 < a.n && g >= a.item_end[t.r]) ++t.r;
  t.i = g - (t.r ? a.item_end[t.r - 1] : 0);
  return t;
}

template <int kJoin>
__global__ __launch_bounds__(256) void window_pool_kernel(WindowPoolArgs a) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.item_end[a.n - 1]) return;
  const Item it = locate(a, g);
  const PoolRoute& r = a.r[it.r];
  const int C4 = r.C >> 2;
  long long i = it.i;
  const int q = (int)(i % C4);
  i /= C4;
  const int HW = r.H * r.W;
  const int p = (int)(i % HW);
  const int b = (int)(i / HW);
  const int y = p / r.W, x = p - y * r.W;
  const long long fs = (long long)(r.H + 2) * (r.W + 2);     // pixels per frame, border included
  const long long pix = (long long)(y + 1) * (r.W + 2) + x + 1;
  const float* src = r.src + ((long long)b * a.k * fs + pix) * r.s_cs + 4 * q;
  const long long fstep = fs * r.s_cs;
  f32x4 acc = *reinterpret_cast<const f32x4*>(src);
  for (int t = 1; t < a.k; ++t) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(src + t * fstep);
    if (kJoin == VY_JOIN_MAX) {
      if (v.x > acc.x) acc.x = v.x;
      if (v.y > acc.y) acc.y = v.y;
      if (v.z > acc.z) acc.z = v.z;
      if (v.w > acc.w) acc.w = v.w;
    } else {
      acc.x = acc.x + v.x;
      acc.y = acc.y + v.y;
      acc.z = acc.z + v.z;
      acc.w = acc.w + v.w;
    }
  }
  if (kJoin == VY_JOIN_MEAN) {
    const float kf = (float)a.k;
    acc.x = acc.x / kf;
    acc.y = acc.y / kf;
    acc.z = acc.z / kf;
    acc.w = acc.w / kf;
  }
  *reinterpret_cast<f32x4*>(r.dst + ((long long)b * fs + pix) * r.d_cs + r.d_co + 4 * q) = acc;
}

template <int kJoin>
__global__ __launch_bounds__(256) void window_pool_bwd_kernel(WindowPoolArgs a) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.item_end[a.n - 1]) return;
  const Item it = locate(a, g);
  const PoolRoute& r = a.r[it.r];
  const int C4 = r.C >> 2;
  long long i = it.i;
  const int q = (int)(i % C4);
  i /= C4;
  const int HW = r.H * r.W;
  const int p = (int)(i % HW);
  const int b = (int)(i / HW);
  const int y = p / r.W, x = p - y * r.W;
  const long long fs = (long long)(r.H + 2) * (r.W + 2);
  const long long pix = (long long)(y + 1) * (r.W + 2) + x + 1;
  const long long so = ((long long)b * a.k * fs + pix) * r.s_cs + 4 * q;  // frame b*k, then + t * fstep
  const long long fstep = fs * r.s_cs;
  const long long po = ((long long)b * fs + pix) * r.d_cs + r.d_co + 4 * q;
  const f32x4 gp = *reinterpret_cast<const f32x4*>(r.gdst + po);
  if (kJoin == VY_JOIN_MAX) {
    const f32x4 m = *reinterpret_cast<const f32x4*>(r.dst + po);
    for (int t = 0; t < a.k; ++t) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(r.src + so + t * fstep);
      f32x4 o;
      o.x = v.x == m.x ? gp.x : 0.0f;
      o.y = v.y == m.y ? gp.y : 0.0f;
      o.z = v.z == m.z ? gp.z : 0.0f;
      o.w = v.w == m.w ? gp.w : 0.0f;
      *reinterpret_cast<f32x4*>(r.gsrc + so + t * fstep) = o;
    }
  } else {
    const float kf = (float)a.k;
    f32x4 o;
    o.x = gp.x / kf;
    o.y = gp.y / kf;
    o.z = gp.z / kf;
    o.w = gp.w / kf;
    for (int t = 0; t < a.k; ++t) *reinterpret_cast<f32x4*>(r.gsrc + so + t * fstep) = o;
  }
}

hipError_t launch(WindowPoolArgs a, bool bwd, hipStream_t s) {
  if (a.n < 1 || a.n > 3 || a.B < 1 || a.k < 1 || (a.join != VY_JOIN_MAX && a.join != VY_JOIN_MEAN))
    return hipErrorInvalidValue;
  long long items = 0;
  for (int i = 0; i < a.n; ++i) {
    const PoolRoute& r = a.r[i];
    if (!r.src || !r.dst || (bwd && (!r.gsrc || !r.gdst)) || r.H < 1 || r.W < 1 || r.C < 4 || r.C % 4 || r.s_cs % 4 ||
        r.d_cs % 4 || r.d_co % 4 || r.C > r.s_cs || r.d_co + r.C > r.d_cs)
      return hipErrorInvalidValue;
    items += (long long)a.B * r.H * r.W * (r.C / 4);
    a.item_end[i] = items;
  }
  const long long blocks = (items + 255) / 256;
  if (blocks >= (1ll << 31)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks), block(256);
  if (bwd) {
    if (a.join == VY_JOIN_MAX)
      hipLaunchKernelGGL(window_pool_bwd_kernel<VY_JOIN_MAX>, grid, block, 0, s, a);
    else
      hipLaunchKernelGGL(window_pool_bwd_kernel<VY_JOIN_MEAN>, grid, block, 0, s, a);
  } else {
    if (a.join == VY_JOIN_MAX)
      hipLaunchKernelGGL(window_pool_kernel<VY_JOIN_MAX>, grid, block, 0, s, a);
    else
      hipLaunchKernelGGL(window_pool_kernel<VY_JOIN_MEAN>, grid, block, 0, s, a);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t vy_launch_window_pool(const WindowPoolArgs& a, hipStream_t s) { return launch(a, false, s); }
hipError_t vy_launch_window_pool_bwd(const WindowPoolArgs& a, hipStream_t s) { return launch(a, true, s); }
