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
//
// Over a whole video (a hier-video plan) consecutive clips share their triples, so both inference joins exist in a dilated
// form as well — frames p, p + d, p + 2d of one plane — behind the five kernels above, which carry no dilation.
#include <cstring>

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

// the max of three operands in frame order: strict >, so on ties the earliest operand's bits are kept
__device__ inline f32x4 max3(const f32x4 v0, const f32x4 v1, const f32x4 v2) {
  f32x4 m = v0;
  if (v1.x > m.x) m.x = v1.x;
  if (v1.y > m.y) m.y = v1.y;
  if (v1.z > m.z) m.z = v1.z;
  if (v1.w > m.w) m.w = v1.w;
  if (v2.x > m.x) m.x = v2.x;
  if (v2.y > m.y) m.y = v2.y;
  if (v2.z > m.z) m.z = v2.z;
  if (v2.w > m.w) m.w = v2.w;
  return m;
}

__global__ __launch_bounds__(256) void hier_pool_kernel(HierPoolArgs a) {
  long long so, po;
  if (!locate(a, &so, &po)) return;
  const long long fstep = a.frame_pixels * a.s_cs;
  const f32x4 v0 = *reinterpret_cast<const f32x4*>(a.src + so);
  const f32x4 v1 = *reinterpret_cast<const f32x4*>(a.src + so + fstep);
  const f32x4 v2 = *reinterpret_cast<const f32x4*>(a.src + so + 2 * fstep);
  *reinterpret_cast<f32x4*>(a.dst + po) = max3(v0, v1, v2);
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
// the folded BatchNorm affine and LeakyReLU(0.1) of the inference join
__device__ inline f32x4 join_apply4(const f32x4 z, const f32x4 sc, const f32x4 sh) {
  f32x4 y;
  y.x = vy_leaky(fmaf(z.x, sc.x, sh.x));
  y.y = vy_leaky(fmaf(z.y, sc.y, sh.y));
  y.z = vy_leaky(fmaf(z.z, sc.z, sh.z));
  y.w = vy_leaky(fmaf(z.w, sc.w, sh.w));
  return y;
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
  *reinterpret_cast<f32x4*>(a.dst + po) = join_apply4(join_z4(k, v0, v1, v2), sc, sh);
}

// ---- the dilated joins of a hier-video plan (vy_net_bind_hier_video): the same two inference joins, but destination
// frame p is made of source frames p, p + d, p + 2d (in that order) of a plane that holds frames + 2d frames, d = a.dil —
// consecutive clips of a video share their triples, so every level is computed once per frame position.  Same lane map,
// borders, channel strides and d_co as above; a locate of their own, so that the five kernels above carry no dilation.
__device__ inline bool locate_dilated(const HierPoolArgs& a, unsigned z, long long* so, long long* po) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.row_items) return false;
  const unsigned px = i >> a.c4_shift, q = i & ((1u << a.c4_shift) - 1u);
  const unsigned in_frame = (blockIdx.y + 1u) * (unsigned)(a.W + 2) + px + 1u;
  const long long n = z;
  *so = (n * a.frame_pixels + in_frame) * a.s_cs + 4u * q;
  *po = (n * a.frame_pixels + in_frame) * a.d_cs + a.d_co + 4u * q;
  return true;
}

// the join's per-lane constants (the max: none)
struct JoinK {
  JoinW k;
  f32x4 sc, sh;
};
template <bool CONV>
__device__ inline JoinK join_constants(const HierJoinArgs& j) {
  JoinK c = {};
  if (CONV) {
    const unsigned ch = lane_channel(j.g);
    c.k = join_weights(j.w, ch);
    c.sc = *reinterpret_cast<const f32x4*>(j.scale + ch);
    c.sh = *reinterpret_cast<const f32x4*>(j.shift + ch);
  }
  return c;
}
template <bool CONV>
__device__ inline f32x4 join3(const JoinK& c, const f32x4 v0, const f32x4 v1, const f32x4 v2) {
  return CONV ? join_apply4(join_z4(c.k, v0, v1, v2), c.sc, c.sh) : max3(v0, v1, v2);
}

// three reads, one write: the grid's z is the destination frame.  The correctness baseline of the chain walk below, which
// is what a net launches (VY_HIER_CHAIN=0 launches this one)
template <bool CONV>
__global__ __launch_bounds__(256) void hier_dilated_kernel(HierJoinArgs j) {
  const HierPoolArgs& a = j.g;
  long long so, po;
  if (!locate_dilated(a, blockIdx.z, &so, &po)) return;
  const long long fstep = (long long)a.dil * a.frame_pixels * a.s_cs;
  const f32x4 v0 = *reinterpret_cast<const f32x4*>(a.src + so);
  const f32x4 v1 = *reinterpret_cast<const f32x4*>(a.src + so + fstep);
  const f32x4 v2 = *reinterpret_cast<const f32x4*>(a.src + so + 2 * fstep);
  *reinterpret_cast<f32x4*>(a.dst + po) = join3<CONV>(join_constants<CONV>(j), v0, v1, v2);
}

// The chain walk: destination frames p = r (mod d) form a chain whose consecutive members share two operands, so a lane
// walks a chain and keeps the two previous operands in registers — every source frame of a chain is read once.  Chains are
// cut into segments of kChainSeg destination frames (the grid's z is segment * d + r): the grid stays full when there
// are few chains, and a segment re-reads only its first two operands, (kChainSeg + 2) / kChainSeg source reads per write.
// Measured (profiles/hier_video_step.txt, 16 centres at 416x416): hpool.0 at 0.90 / 0.85 / 0.88 of the copy rate of its
// algorithmic bytes at T = 9 / 27 / 81, where the three reads reach 0.72 / 0.66 / 0.70.
constexpr int kChainSeg = 8;
template <bool CONV>
__global__ __launch_bounds__(256) void hier_dilated_chain_kernel(HierJoinArgs j) {
  const HierPoolArgs& a = j.g;
  const unsigned d = (unsigned)a.dil, seg = blockIdx.z / d, r = blockIdx.z - seg * d;
  const unsigned first = seg * (unsigned)kChainSeg * d + r;  // this lane's first destination frame
  if (first >= (unsigned)a.frames) return;
  long long so, po;
  if (!locate_dilated(a, first, &so, &po)) return;
  const long long sstep = (long long)d * a.frame_pixels * a.s_cs, dstep = (long long)d * a.frame_pixels * a.d_cs;
  const JoinK c = join_constants<CONV>(j);
  f32x4 v0 = *reinterpret_cast<const f32x4*>(a.src + so);
  f32x4 v1 = *reinterpret_cast<const f32x4*>(a.src + so + sstep);
  const unsigned left = ((unsigned)a.frames - first + d - 1u) / d;  // members of the chain from `first` on
  const int n = (int)(left < (unsigned)kChainSeg ? left : (unsigned)kChainSeg);
  for (int k = 0; k < n; ++k) {
    const f32x4 v2 = *reinterpret_cast<const f32x4*>(a.src + so + (k + 2) * sstep);
    *reinterpret_cast<f32x4*>(a.dst + po + k * dstep) = join3<CONV>(c, v0, v1, v2);
    v0 = v1;
    v1 = v2;
  }
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

// the dilated inference joins: conv = the learned join (else the max, whose w / scale / shift stay null); chain: the chain walk
hipError_t launch_dilated(HierJoinArgs j, bool conv, bool chain, hipStream_t s) {
  dim3 grid;
  HierPoolArgs& a = j.g;
  const bool ptrs = a.src && a.dst && (!conv || (j.w && j.scale && j.shift));
  // (the source plane holds frames + 2 dil frames: the caller's plan says so)
  if (!ptrs || a.dil < 1 || a.dil > 65535 || (conv && a.C > 1024) || !geometry(a, &grid)) return hipErrorInvalidValue;
  if (chain) {
    const long long d = a.dil, members = (a.frames + d - 1) / d;  // of the longest chain
    const long long z = d * ((members + kChainSeg - 1) / kChainSeg);
    if (z > 65535) return hipErrorInvalidValue;
    grid.z = (unsigned)z;
    if (conv)
      hipLaunchKernelGGL(hier_dilated_chain_kernel<true>, grid, dim3(256), 0, s, j);
    else
      hipLaunchKernelGGL(hier_dilated_chain_kernel<false>, grid, dim3(256), 0, s, j);
  } else if (conv) {
    hipLaunchKernelGGL(hier_dilated_kernel<true>, grid, dim3(256), 0, s, j);
  } else {
    hipLaunchKernelGGL(hier_dilated_kernel<false>, grid, dim3(256), 0, s, j);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t vy_launch_hier_pool_dilated(const HierPoolArgs& a, int chain, hipStream_t s) {
  HierJoinArgs j;
  memset(&j, 0, sizeof j);
  j.g = a;
  return launch_dilated(j, false, chain != 0, s);
}
hipError_t vy_launch_hier_join_dilated(const HierJoinArgs& a, int chain, hipStream_t s) {
  return launch_dilated(a, true, chain != 0, s);
}
hipError_t vy_launch_hier_pool(const HierPoolArgs& a, hipStream_t s) { return launch(a, false, s); }
hipError_t vy_launch_hier_pool_bwd(const HierPoolArgs& a, hipStream_t s) { return launch(a, true, s); }
hipError_t vy_launch_hier_join(const HierJoinArgs& a, hipStream_t s) { return launch_join(a, 0, s); }
hipError_t vy_launch_hier_join_raw(const HierJoinArgs& a, hipStream_t s) { return launch_join(a, 1, s); }
hipError_t vy_launch_hier_join_bwd(const HierJoinArgs& a, hipStream_t s) { return launch_join(a, 2, s); }

