// hier.hip — the temporal pooling inside the backbone of a hierarchical net (HDarknet with h_join_type='max',
// h_darknet.py:103-188): between two groups of Darknet-53 cells, consecutive triples of frames of one plane are reduced
// with an element-wise max into a plane of a third of the frames.  The regrouping of the reference is hard-wired to 3
// (reshape(0, 0, -1, 3, 0, 0)): pooled frame n of the flat frame axis is the max of frames 3n, 3n + 1, 3n + 2.
//
// Arithmetic: temporal.hip's max, restated.
//   forward  strict > in frame order: on ties the earliest frame's bits are kept
//   backward every frame whose value equals the max (x_t == pooled, IEEE equality) gets the full g, the others +0 — written,
//            never accumulated: mxnet's reduce-max backward, not torch's amax, which splits g among ties   [UPSTREAM-RECALLED]
//
// Streaming kernels for the largest planes of the net (the first pool of a 9-frame net at 416x416, 16 clips reads 144
// full-resolution frames of 32 channels).  One launch per plane; the grid is (chunks of a row, rows, pooled frames), so a lane
// finds its place with shifts and one 32-bit multiply: no search, no division.  A lane owns 4 consecutive channels (16-B
// accesses) of one pooled pixel, consecutive lanes walk the channels and then the pixels of the row: a wave moves 1 KiB
// contiguous per frame, and the three frames are unrolled, their loads issued before the first compare.  Forward: three reads,
// one write.  Backward: pooled gradient and pooled value read once, three values read, three gradients written.  Interiors
// only: the borders of both planes stay the zeros of the bind (the pooled plane feeds a padded 3x3 stride-2 conv), and of
// a destination wider than C (route 0 in its concat plane) only the channels [d_co, d_co + C) are written.
#include "kernels.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

// where lane `i` of row y of pooled frame n lives: float offsets of the first of the three source frames and of the
// destination; false: past the end of the row
__device__ inline bool locate(const HierPoolArgs& a, long long* so, long long* po) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.row_items) return false;
  const unsigned px = i >> a.c4_shift, q = i & ((1u << a.c4_shift) - 1u);
  const unsigned in_frame = (blockIdx.y + 1u) * (unsigned)(a.W + 2) + px + 1u;  // pixel inside a frame, border included
  const long long n = blockIdx.z;
  *so = (3 * n * a.frame_pixels + in_frame) * a.s_cs + 4u * q;
  *po = (n * a.frame_pixels + in_frame) * a.d_cs + a.d_co + 4u * q;
  return true;
}

__global__ __launch_bounds__(256) void hier_pool_kernel(HierPoolArgs a) {
  long long so, po;
  if (!locate(a, &so, &po)) return;
  const long long fstep = a.frame_pixels * a.s_cs;
  const f32x4 v0 = *reinterpret_cast<const f32x4*>(a.src + so);
  const f32x4 v1 = *reinterpret_cast<const f32x4*>(a.src + so + fstep);
  const f32x4 v2 = *reinterpret_cast<const f32x4*>(a.src + so + 2 * fstep);
  f32x4 m = v0;
  if (v1.x > m.x) m.x = v1.x;
  if (v1.y > m.y) m.y = v1.y;
  if (v1.z > m.z) m.z = v1.z;
  if (v1.w > m.w) m.w = v1.w;
  if (v2.x > m.x) m.x = v2.x;
  if (v2.y > m.y) m.y = v2.y;
  if (v2.z > m.z) m.z = v2.z;
  if (v2.w > m.w) m.w = v2.w;
  *reinterpret_cast<f32x4*>(a.dst + po) = m;
}

__device__ inline f32x4 where_equal(const f32x4 v, const f32x4 m, const f32x4 g) {
  f32x4 o;
  o.x = v.x == m.x ? g.x : 0.0f;
  o.y = v.y == m.y ? g.y : 0.0f;
  o.z = v.z == m.z ? g.z : 0.0f;
  o.w = v.w == m.w ? g.w : 0.0f;
  return o;
}

__global__ __launch_bounds__(256) void hier_pool_bwd_kernel(HierPoolArgs a) {
  long long so, po;
  if (!locate(a, &so, &po)) return;
  const long long fstep = a.frame_pixels * a.s_cs;
  const f32x4 g = *reinterpret_cast<const f32x4*>(a.gdst + po);
  const f32x4 m = *reinterpret_cast<const f32x4*>(a.dst + po);
  const f32x4 v0 = *reinterpret_cast<const f32x4*>(a.src + so);
  const f32x4 v1 = *reinterpret_cast<const f32x4*>(a.src + so + fstep);
  const f32x4 v2 = *reinterpret_cast<const f32x4*>(a.src + so + 2 * fstep);
  *reinterpret_cast<f32x4*>(a.gsrc + so) = where_equal(v0, m, g);
  *reinterpret_cast<f32x4*>(a.gsrc + so + fstep) = where_equal(v1, m, g);
  *reinterpret_cast<f32x4*>(a.gsrc + so + 2 * fstep) = where_equal(v2, m, g);
}

hipError_t launch(HierPoolArgs a, bool bwd, hipStream_t s) {
  if (!a.src || !a.dst || (bwd && (!a.gsrc || !a.gdst)) || a.frames < 1 || a.frames > 65535 || a.H < 1 || a.H > 65535 ||
      a.W < 1 || a.C < 4 || (a.C & (a.C - 1)) || a.s_cs % 4 || a.d_cs % 4 || a.d_co % 4 || a.C > a.s_cs ||
      a.d_co + a.C > a.d_cs)
    return hipErrorInvalidValue;
  a.c4_shift = 0;
  while ((4 << a.c4_shift) < a.C) ++a.c4_shift;
  const long long items = (long long)a.W * (a.C / 4);
  if (items >= (1ll << 31)) return hipErrorInvalidValue;
  a.row_items = (unsigned)items;
  a.frame_pixels = (long long)(a.H + 2) * (a.W + 2);
  const dim3 grid((unsigned)((items + 255) / 256), (unsigned)a.H, (unsigned)a.frames), block(256);
  if (bwd)
    hipLaunchKernelGGL(hier_pool_bwd_kernel, grid, block, 0, s, a);
  else
    hipLaunchKernelGGL(hier_pool_kernel, grid, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t vy_launch_hier_pool(const HierPoolArgs& a, hipStream_t s) { return launch(a, false, s); }
hipError_t vy_launch_hier_pool_bwd(const HierPoolArgs& a, hipStream_t s) { return launch(a, true, s); }
