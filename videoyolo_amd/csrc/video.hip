// video.hip — the per-frame route ring of a video plan.  A window net run over a video (detect_yolo3.py --window k,step:
// one clip per frame, datasets/imgnetvid.py:480-506) sees every frame in up to k clips; with the early join the stages are
// TimeDistributed, so a frame's three routes are the same bits in every clip.  The backbone therefore runs once per frame,
// ring_push keeps the routes in a ring of slots in HBM, and ring_pool gathers each clip's k slots and pools them — with
// window_pool's arithmetic (temporal.hip), bit for bit — into the planes the heads read.
//
// Ring layout: slot s = the three routes (stride 8, 16, 32) back to back, each tight NHWC (H x W x C) without borders —
// only ring_pool and the test tap read a slot.  slot_stride floats per slot, a multiple of 64 (256 B).
//
// Streaming kernels in the shape of window_pool_kernel: one lane owns 4 consecutive channels (16 B) of one pixel,
// consecutive lanes walk the channels, then the pixels; all three routes in one launch.  The frame -> slot and
// clip -> slots tables are kernel arguments (VY_RING_TABLE_MAX entries: the library owns no device memory and copies
// nothing per call); every slot is range-checked on the host before the launch.
#include "kernels.h"
#include "../../include/vyolo.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

struct Item {
  const RingRoute* r;
  int q, p, b;  // channel quad, pixel (row-major interior), frame / clip
};

__device__ inline Item locate(const RingRoute* r, const long long* item_end, int n, long long g) {
  int ri = 0;
  while (ri + 1 < n && g >= item_end[ri]) ++ri;
  const long long i = g - (ri ? item_end[ri - 1] : 0);
  Item t;
  t.r = r + ri;
  const int C4 = t.r->C >> 2;
  const int HW = t.r->H * t.r->W;
  if (item_end[n - 1] < (1ll << 31)) {  // (uniform) 32-bit divisions: a lane moves 32 ... 64 B, 64-bit ones would cost more than that
    const unsigned j = (unsigned)i, pj = j / (unsigned)C4;
    t.q = (int)(j - pj * (unsigned)C4);
    t.b = (int)(pj / (unsigned)HW);
    t.p = (int)(pj - (unsigned)t.b * (unsigned)HW);
  } else {
    const long long pj = i / C4;
    t.q = (int)(i - pj * C4);
    t.b = (int)(pj / HW);
    t.p = (int)(pj - (long long)t.b * HW);
  }
  return t;
}

// bordered plane: float offset of interior pixel p of image b
__device__ inline long long plane_pix(const RingRoute& r, int b, int p) {
  const int y = p / r.W, x = p - y * r.W;
  return (long long)b * (r.H + 2) * (r.W + 2) + (long long)(y + 1) * (r.W + 2) + x + 1;
}

__global__ __launch_bounds__(256) void ring_push_kernel(RingPushArgs a) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.item_end[a.n - 1]) return;
  const Item it = locate(a.r, a.item_end, a.n, g);
  const RingRoute& r = *it.r;
  const int slot = a.slot[it.b];
  if (slot < 0) return;  // tail padding: the frame is not stored
  const f32x4 v = *reinterpret_cast<const f32x4*>(r.plane + plane_pix(r, it.b, it.p) * r.s_cs + 4 * it.q);
  *reinterpret_cast<f32x4*>(r.ring + slot * a.slot_stride + (long long)it.p * r.C + 4 * it.q) = v;
}

template <int kJoin>
__global__ __launch_bounds__(256) void ring_pool_kernel(RingPoolArgs a) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.item_end[a.n - 1]) return;
  const Item it = locate(a.r, a.item_end, a.n, g);
  const RingRoute& r = *it.r;
  const int* row = a.table + it.b * a.k;
  const float* src = r.ring + (long long)it.p * r.C + 4 * it.q;
  f32x4 acc = *reinterpret_cast<const f32x4*>(src + row[0] * a.slot_stride);
  for (int t = 1; t < a.k; ++t) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(src + row[t] * a.slot_stride);
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
  *reinterpret_cast<f32x4*>(r.dst + plane_pix(r, it.b, it.p) * r.d_cs + r.d_co + 4 * it.q) = acc;
}

__global__ __launch_bounds__(256) void ring_read_kernel(const float* __restrict__ src, int HW, int C, float* __restrict__ chw) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long long)HW * C) return;
  const int p = (int)(g % HW), c = (int)(g / HW);
  chw[g] = src[(long long)p * C + c];
}

// geometry shared by both launches; fills item_end for `batch` images per route
bool routes_ok(const RingRoute* r, int n, int batch, bool pool, long long slot_stride, long long* item_end) {
  if (n < 1 || n > 3 || batch < 1 || slot_stride < 4 || slot_stride % 4) return false;
  long long items = 0;
  for (int i = 0; i < n; ++i) {
    const RingRoute& q = r[i];
    if (!q.ring || q.H < 1 || q.W < 1 || q.C < 4 || q.C % 4) return false;
    if (pool ? (!q.dst || q.d_cs % 4 || q.d_co % 4 || q.d_co + q.C > q.d_cs) : (!q.plane || q.s_cs % 4 || q.C > q.s_cs))
      return false;
    if ((q.ring - r[0].ring) + (long long)q.H * q.W * q.C > slot_stride) return false;  // the route lies inside its slot
    items += (long long)batch * q.H * q.W * (q.C / 4);
    item_end[i] = items;
  }
  return (items + 255) / 256 < (1ll << 31);
}

}  // namespace

hipError_t vy_launch_ring_push(const RingPushArgs& a0, hipStream_t s) {
  RingPushArgs a = a0;
  if (a.F < 1 || a.F > VY_RING_TABLE_MAX || a.R < 1 || !routes_ok(a.r, a.n, a.F, false, a.slot_stride, a.item_end))
    return hipErrorInvalidValue;
  for (int f = 0; f < a.F; ++f)
    if (a.slot[f] < -1 || a.slot[f] >= a.R) return hipErrorInvalidValue;
  const long long items = a.item_end[a.n - 1];
  hipLaunchKernelGGL(ring_push_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t vy_launch_ring_pool(const RingPoolArgs& a0, hipStream_t s) {
  RingPoolArgs a = a0;
  if (a.B < 1 || a.k < 1 || (long long)a.B * a.k > VY_RING_TABLE_MAX || a.R < 1 ||
      (a.join != VY_JOIN_MAX && a.join != VY_JOIN_MEAN) || !routes_ok(a.r, a.n, a.B, true, a.slot_stride, a.item_end))
    return hipErrorInvalidValue;
  for (int i = 0; i < a.B * a.k; ++i)
    if (a.table[i] < 0 || a.table[i] >= a.R) return hipErrorInvalidValue;
  const long long items = a.item_end[a.n - 1];
  const dim3 grid((unsigned)((items + 255) / 256)), block(256);
  if (a.join == VY_JOIN_MAX)
    hipLaunchKernelGGL(ring_pool_kernel<VY_JOIN_MAX>, grid, block, 0, s, a);
  else
    hipLaunchKernelGGL(ring_pool_kernel<VY_JOIN_MEAN>, grid, block, 0, s, a);
  return hipGetLastError();
}

hipError_t vy_launch_ring_read(const float* slot_route, int H, int W, int C, float* chw, hipStream_t s) {
  if (!slot_route || !chw || H < 1 || W < 1 || C < 1) return hipErrorInvalidValue;
  const long long items = (long long)H * W * C;
  hipLaunchKernelGGL(ring_read_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, slot_route, H * W, C, chw);
  return hipGetLastError();
}
