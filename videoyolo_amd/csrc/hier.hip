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
//
// The learned join ('conv': `_conv1d`, layers.py:50-60) runs in the same place on the same lane map: a depthwise 3-tap
// filter over the frames of a triple, then BatchNorm and LeakyReLU.  Inference is one launch (hier_join_kernel: three reads,
// one write); training writes z and per-block statistics rows (hier_join_raw_kernel) for the BatchNorm kernels every cell
// uses, and the backward (hier_join_bwd_kernel) writes the three frames' gradients and per-block rows of the weight gradient.
#include "kernels.h"
#include "../../include/vy_math.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

// where lane `i` of row y of pooled frame n lives: float offsets of the first of the three source frames and of the
// destination; false: past the end of the row
// (zo: of the same pixel in a join's z plane — the pooled frames, C channels, tight)
__device__ inline bool locate(const HierPoolArgs& a, long long* so, long long* po, long long* zo = nullptr) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.row_items) return false;
  const unsigned px = i >> a.c4_shift, q = i & ((1u << a.c4_shift) - 1u);
  const unsigned in_frame = (blockIdx.y + 1u) * (unsigned)(a.W + 2) + px + 1u;  // pixel inside a frame, border included
  const long long n = blockIdx.z;
  *so = (3 * n * a.frame_pixels + in_frame) * a.s_cs + 4u * q;
  *po = (n * a.frame_pixels + in_frame) * a.d_cs + a.d_co + 4u * q;
  if (zo) *zo = (n * a.frame_pixels + in_frame) * a.C + 4u * q;
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

// ---- the learned join (`_conv1d`, layers.py:50-60: Conv3D (3, 1, 1) with groups = C, no bias, under TimeDistributed): per
// channel a 3-tap filter over the frames of a triple.  The pinned arithmetic, frame order 0, 1, 2:
//   z = fmaf(w2, x2, fmaf(w1, x1, w0 * x0))
// w0 * x0 is rounded to fp32 on its own: the library is built with -ffp-contract=off, and the product is a statement of its
// own so that no other grouping can be read into it.
__device__ inline float join_z(float w0, float w1, float w2, float x0, float x1, float x2) {
  const float p0 = w0 * x0;
  return fmaf(w2, x2, fmaf(w1, x1, p0));
}

// the (C, 3) weights of a lane's four channels: twelve consecutive floats, three 16-byte loads; w[t] = frame t's four
struct JoinW {
  f32x4 w[3];
};
__device__ inline JoinW join_weights(const float* w, unsigned c) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(w + 3u * c);
  const f32x4 b = *reinterpret_cast<const f32x4*>(w + 3u * c + 4u);
  const f32x4 d = *reinterpret_cast<const f32x4*>(w + 3u * c + 8u);
  JoinW o;
  o.w[0] = f32x4{a.x, a.w, b.z, d.y};
  o.w[1] = f32x4{a.y, b.x, b.w, d.z};
  o.w[2] = f32x4{a.z, b.y, d.x, d.w};
  return o;
}
__device__ inline f32x4 join_z4(const JoinW& k, const f32x4 v0, const f32x4 v1, const f32x4 v2) {
  f32x4 z;
  z.x = join_z(k.w[0].x, k.w[1].x, k.w[2].x, v0.x, v1.x, v2.x);
  z.y = join_z(k.w[0].y, k.w[1].y, k.w[2].y, v0.y, v1.y, v2.y);
  z.z = join_z(k.w[0].z, k.w[1].z, k.w[2].z, v0.z, v1.z, v2.z);
  z.w = join_z(k.w[0].w, k.w[1].w, k.w[2].w, v0.w, v1.w, v2.w);
  return z;
}
// first channel of the lane's four
__device__ inline unsigned lane_channel(const HierPoolArgs& a) {
  return 4u * ((blockIdx.x * 256u + threadIdx.x) & ((1u << a.c4_shift) - 1u));
}

// inference: three reads, one write; weights and the folded affine are five cached 16-byte loads per lane
__global__ __launch_bounds__(256) void hier_join_kernel(HierJoinArgs j) {
  const HierPoolArgs& a = j.g;
  long long so, po;
  if (!locate(a, &so, &po)) return;
  const long long fstep = a.frame_pixels * a.s_cs;
  const f32x4 v0 = *reinterpret_cast<const f32x4*>(a.src + so);
  const f32x4 v1 = *reinterpret_cast<const f32x4*>(a.src + so + fstep);
  const f32x4 v2 = *reinterpret_cast<const f32x4*>(a.src + so + 2 * fstep);
  const unsigned c = lane_channel(a);
  const JoinW k = join_weights(j.w, c);
  const f32x4 sc = *reinterpret_cast<const f32x4*>(j.scale + c);
  const f32x4 sh = *reinterpret_cast<const f32x4*>(j.shift + c);
  const f32x4 z = join_z4(k, v0, v1, v2);
  f32x4 y;
  y.x = vy_leaky(fmaf(z.x, sc.x, sh.x));
  y.y = vy_leaky(fmaf(z.y, sc.y, sh.y));
  y.z = vy_leaky(fmaf(z.z, sc.z, sh.z));
  y.w = vy_leaky(fmaf(z.w, sc.w, sh.w));
  *reinterpret_cast<f32x4*>(a.dst + po) = y;
}

// The per-block rows of the two training kernels.  Every lane leaves K doubles in LDS (lanes past the end of the row:
// zeros), column-major so that the writes do not collide; column `col` of the block's row is then the sum, over the block's
// pixels in lane order, of value `k` of the lanes that hold channel quad `q` — a fixed order, in double.
template <int K>
struct JoinSums {
  double v[K][256];
  __device__ void put(int k, double x) { v[k][threadIdx.x] = x; }
  __device__ double sum(const HierPoolArgs& a, unsigned q, int k) const {
    double s = 0.0;
    for (unsigned l = q; l < 256u; l += 1u << a.c4_shift) s += v[k][l];
    return s;
  }
};
__device__ inline long long block_row() {
  return ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
}

// training forward: z into its plane, and the block's [2][C] sums of z and z^2
__global__ __launch_bounds__(256) void hier_join_raw_kernel(HierJoinArgs j) {
  __shared__ JoinSums<8> sums;
  const HierPoolArgs& a = j.g;
  long long so, po, zo;
  f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
  if (locate(a, &so, &po, &zo)) {
    const long long fstep = a.frame_pixels * a.s_cs;
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(a.src + so);
    const f32x4 v1 = *reinterpret_cast<const f32x4*>(a.src + so + fstep);
    const f32x4 v2 = *reinterpret_cast<const f32x4*>(a.src + so + 2 * fstep);
    z = join_z4(join_weights(j.w, lane_channel(a)), v0, v1, v2);
    *reinterpret_cast<f32x4*>(j.z + zo) = z;
  }
  const float ze[4] = {z.x, z.y, z.z, z.w};
  for (int e = 0; e < 4; ++e) {
    sums.put(e, (double)ze[e]);
    sums.put(4 + e, (double)ze[e] * (double)ze[e]);
  }
  __syncthreads();
  double* const row = j.partials + block_row() * (2ll * a.C);
  for (unsigned col = threadIdx.x; col < 2u * (unsigned)a.C; col += 256u) {
    const unsigned sq = col >= (unsigned)a.C, ch = col - sq * (unsigned)a.C;
    row[col] = sums.sum(a, ch >> 2, (int)(4u * sq + (ch & 3u)));
  }
}

// backward: dz and the three frames read once; gx_t = w_t * dz written to the three frames of the pre-pool gradient plane;
// the block's [C][3] sums of x_t * dz (the products exact in double)
__global__ __launch_bounds__(256) void hier_join_bwd_kernel(HierJoinArgs j) {
  __shared__ JoinSums<12> sums;
  const HierPoolArgs& a = j.g;
  long long so, po, zo;
  f32x4 dz = {0.0f, 0.0f, 0.0f, 0.0f}, v[3] = {dz, dz, dz};
  if (locate(a, &so, &po, &zo)) {
    const long long fstep = a.frame_pixels * a.s_cs;
    dz = *reinterpret_cast<const f32x4*>(j.z + zo);
#pragma unroll
    for (int t = 0; t < 3; ++t) v[t] = *reinterpret_cast<const f32x4*>(a.src + so + t * fstep);
    const JoinW k = join_weights(j.w, lane_channel(a));
#pragma unroll
    for (int t = 0; t < 3; ++t) *reinterpret_cast<f32x4*>(a.gsrc + so + t * fstep) = k.w[t] * dz;
  }
  const float de[4] = {dz.x, dz.y, dz.z, dz.w};
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const float xe[4] = {v[t].x, v[t].y, v[t].z, v[t].w};
    for (int e = 0; e < 4; ++e) sums.put(3 * e + t, (double)xe[e] * (double)de[e]);
  }
  __syncthreads();
  double* const row = j.partials + block_row() * (3ll * a.C);
  for (unsigned col = threadIdx.x; col < 3u * (unsigned)a.C; col += 256u) {
    const unsigned ch = col / 3u, t = col - 3u * ch;
    row[col] = sums.sum(a, ch >> 2, (int)(3u * (ch & 3u) + t));
  }
}

// the geometry every launcher checks and fills in (the pointers: the caller's to check)
bool geometry(HierPoolArgs& a, dim3* grid) {
  if (a.frames < 1 || a.frames > 65535 || a.H < 1 || a.H > 65535 || a.W < 1 || a.C < 4 || (a.C & (a.C - 1)) || a.s_cs % 4 ||
      a.d_cs % 4 || a.d_co % 4 || a.C > a.s_cs || a.d_co + a.C > a.d_cs)
    return false;
  a.c4_shift = 0;
  while ((4 << a.c4_shift) < a.C) ++a.c4_shift;
  const long long items = (long long)a.W * (a.C / 4);
  if (items >= (1ll << 31)) return false;
  a.row_items = (unsigned)items;
  a.frame_pixels = (long long)(a.H + 2) * (a.W + 2);
  *grid = dim3((unsigned)((items + 255) / 256), (unsigned)a.H, (unsigned)a.frames);
  return true;
}

hipError_t launch(HierPoolArgs a, bool bwd, hipStream_t s) {
  dim3 grid;
  if (!a.src || !a.dst || (bwd && (!a.gsrc || !a.gdst)) || !geometry(a, &grid)) return hipErrorInvalidValue;
  if (bwd)
    hipLaunchKernelGGL(hier_pool_bwd_kernel, grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(hier_pool_kernel, grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

// mode 0: inference, 1: training forward, 2: backward.  C <= 1024: a block holds whole pixels (C / 4 lanes each)
hipError_t launch_join(HierJoinArgs j, int mode, hipStream_t s) {
  dim3 grid;
  const bool ptrs = j.g.src && j.w && (mode == 0 ? j.g.dst && j.scale && j.shift : j.z && j.partials && (mode == 1 || j.g.gsrc));
  if (!ptrs || j.g.C > 1024 || !geometry(j.g, &grid)) return hipErrorInvalidValue;
  if ((long long)grid.x * grid.y * grid.z >= (1ll << 31)) return hipErrorInvalidValue;  // (the rows are counted in an int)
  if (mode == 0)
    hipLaunchKernelGGL(hier_join_kernel, grid, dim3(256), 0, s, j);
  else if (mode == 1)
    hipLaunchKernelGGL(hier_join_raw_kernel, grid, dim3(256), 0, s, j);
  else
    hipLaunchKernelGGL(hier_join_bwd_kernel, grid, dim3(256), 0, s, j);
  return hipGetLastError();
}

}  // namespace

hipError_t vy_launch_hier_pool(const HierPoolArgs& a, hipStream_t s) { return launch(a, false, s); }
hipError_t vy_launch_hier_pool_bwd(const HierPoolArgs& a, hipStream_t s) { return launch(a, true, s); }
hipError_t vy_launch_hier_join(const HierJoinArgs& a, hipStream_t s) { return launch_join(a, 0, s); }
hipError_t vy_launch_hier_join_raw(const HierJoinArgs& a, hipStream_t s) { return launch_join(a, 1, s); }
hipError_t vy_launch_hier_join_bwd(const HierJoinArgs& a, hipStream_t s) { return launch_join(a, 2, s); }

