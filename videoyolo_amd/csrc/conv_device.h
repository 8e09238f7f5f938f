// conv_device.h — device-side helpers shared by the implicit-GEMM conv kernels (conv_igemm.hip, conv_split.hip,
// conv_wino.hip) and the weight gradients (wgrad.hip, wgrad_split.hip), and the ordered column sum of the training
// step's reductions (train_kernels.hip).
#pragma once
#include "kernels.h"
#include "../../include/vy_math.h"

#include <type_traits>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))

// One LDS-DMA instruction (global_load_lds_dwordx4: 64 lanes x 16 B -> 1 KiB at lds_base + lane*16), issued
// as inline asm so that hipcc does not serialise it against the surrounding ds_reads (it would wait
// vmcnt(0) before every LDS read that follows a DMA it knows about).  Ordering is by hand: every wave
// executes `s_waitcnt vmcnt(0)` before the barrier that precedes the first read of the tile.
__device__ __forceinline__ void lds_dma16(const float* gptr, unsigned lds_addr) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(gptr), "s"(lds_addr) : "memory", "m0");
#endif
}

// The same with the address split into a wave-uniform 64-bit base (SGPR pair) and a per-lane 32-bit byte offset:
// the base advances per k-step with two scalar adds, the per-lane offsets never change inside the k-loop — no
// vector instruction per DMA (the fp32 MFMA shares the vector pipe's FMA hardware: every VALU instruction in the
// loop is paid in matrix time, tools/probe/coissue_probe.hip).
__device__ __forceinline__ void lds_dma16_s(unsigned voff, const float* sbase, unsigned lds_addr) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_addr)
               : "memory", "m0");
#endif
}

// fp32 access through a buffer descriptor (the raw_buffer builtins move 32-bit integers): byte offset
// `voff` per lane + uniform `soff`; an offset past the descriptor's range reads 0 / is not written
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ float buf_load_f32(__amdgpu_buffer_rsrc_t rsrc, unsigned voff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, 0, 0));
}
__device__ __forceinline__ void buf_store_f32(float v, __amdgpu_buffer_rsrc_t rsrc, unsigned voff, int soff) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsrc, voff, soff, 0);
}
// 16-byte write-through store / L1-bypassing load (aux 16 = sc1): the pair that hands bytes to another workgroup inside a
// launch without an agent-scope release (an L2 write-back of the whole XCD) or acquire — MI355X_MICROARCH.md, visibility
typedef unsigned vy_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void buf_store_f32x4_sc1(f32x4 v, __amdgpu_buffer_rsrc_t rsrc, unsigned voff) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(vy_u32x4, v), rsrc, voff, 0, 16);
}
__device__ __forceinline__ f32x4 buf_load_f32x4_sc1(__amdgpu_buffer_rsrc_t rsrc, unsigned voff) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, 0, 16));
}
// the same with the default cache policy (write-through L1, write-back L2): bytes the SAME lanes read back later
__device__ __forceinline__ void buf_store_f32x4(f32x4 v, __amdgpu_buffer_rsrc_t rsrc, unsigned voff) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(vy_u32x4, v), rsrc, voff, 0, 0);
}
__device__ __forceinline__ f32x4 buf_load_f32x4(__amdgpu_buffer_rsrc_t rsrc, unsigned voff) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, 0, 0));
}
#endif

__device__ __forceinline__ unsigned fd_div(unsigned n, const VyFastDiv f) {
  const unsigned t = __umulhi(f.m, n);
  return (t + ((n - t) >> f.s1)) >> f.s2;
}

// workgroup barrier that waits for this wave's LDS traffic only (not for outstanding global loads: the deep
// pipeline below keeps LDS-DMA of later k-steps in flight across it)
__device__ __forceinline__ void lds_barrier() {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#endif
}

// ---- what the three conv kernels do around their k-loops: ONE definition each of the block order, the pixel of a GEMM
// row, the row tables, the epilogue and the batch-statistics sums.  `Args` is ConvArgs in the address space the caller
// reads it from (a kernel parameter, or the kernarg segment for the stream-K instances, which re-read it per work item):
// always passed on by reference, never copied.  Everything derived from the thread index comes in as an argument, so a
// caller that made it opaque per item keeps it un-hoisted.  The register allocation of the callers is held to
// profiles/conv_shared_parts.txt (tools/asm_counts.py): it is sensitive to how this code is written, not only to what it
// computes — see the notes at conv_epilogue and at MfmaCd32.

// XCD-aware order: blocks L, L+8, ... share an XCD (L2); give each XCD a contiguous run of tiles (stream-K: of the
// k-step sequence) with n fastest so neighbours in time re-use the same A rows and the whole W panel.
__device__ __forceinline__ int vy_xcd_tile(const int L, const int nblk) {
  const int q = nblk >> 3, r = nblk & 7, xcd = L & 7, idx = L >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// GEMM row m -> pixel (b, y, x) of the logical LH x LW grid
// (two multiply-highs instead of two emulated 32-bit divisions per row: the prologue is on the critical path of
// the short launches at small batches)
struct ConvPixel {
  int b, y, x;
};
template <typename Args>
__device__ __forceinline__ ConvPixel conv_pixel(const int m, Args& a) {
  const int t = (int)fd_div((unsigned)m, a.fd_lw);
  const int x = m - t * a.LW;
  const int b = (int)fd_div((unsigned)t, a.fd_lh);
  const int y = t - b * a.LH;
  return {b, y, x};
}
// ... its pixel index in the output plane (and in the addend plane, which has the output's pixel map) ...
template <typename Args>
__device__ __forceinline__ long long conv_out_pixel(const ConvPixel p, Args& a) {
  return (long long)(p.b * a.o_Hp + p.y * a.o_s + a.o_oy) * a.o_Wp + p.x * a.o_s + a.o_ox;
}
// ... and the element offset of its centre pixel's first channel in the A operand plane
template <typename Args>
__device__ __forceinline__ long long conv_in_offset(const ConvPixel p, Args& a) {
  return ((long long)(p.b * a.a_Hp + p.y * a.a_s + a.a_oy) * a.a_Wp + p.x * a.a_s + a.a_ox) * a.a_cs + a.a_co;
}
// x2-replicated store (nearest upsample fused, layers.py:11-20) cropped to the route's size (slice_like,
// yolo3.py:1177): bit 0 / bit 1 drop the pixel's second column / second row
template <typename Args>
__device__ __forceinline__ unsigned conv_ups2_crop(const ConvPixel p, Args& a) {
  return (2 * p.x + 1 >= a.o_Wp - 2 ? 1u : 0u) | (2 * p.y + 1 >= a.o_Hp - 2 ? 2u : 0u);
}
// A 64-bit value that every lane of the wave computed alike, as a wave-uniform one (an SGPR pair): two readfirstlanes.
// The compiler cannot see the uniformity itself once a division was expanded into vector code on the way to the value
template <typename T>  // long long or unsigned long long
__device__ __forceinline__ T vy_uniform64(const T v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return ((T)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)v);
#else
  return v;
#endif
}
// output pixel of a tile's first row (m0 < M always): wave-uniform
template <typename Args>
__device__ __forceinline__ long long conv_tile_pix0(const int m0, Args& a) {
  return vy_uniform64(conv_out_pixel(conv_pixel(m0, a), a));
}

// Row tables of a tile: in_off = element offset of the row's A pixel; o_off / r_off = byte offset of the row's output
// pixel (and of its addend pixel) relative to the tile's first pixel; kInvalidRow for rows past M.  The epilogue
// addresses memory through buffer descriptors based at the tile's first pixel: 32-bit offsets (one v_add per element
// instead of 64-bit multiply-adds), and an offset with bit 31 set is out of range for the descriptor, so the
// hardware drops the store / returns 0 for the load — no per-element branches.  With ups == 2 the two low bits of
// the (4-byte aligned) output offset carry conv_ups2_crop.
constexpr unsigned kInvalidRow = 0x80000000u;
template <int BM, int NT, typename Args>
__device__ __forceinline__ void conv_row_tables(Args& a, const int tid, const int m0, const long long pix0, long long* in_off,
                                                unsigned* o_off, unsigned* r_off) {
  for (int rr = tid; rr < BM; rr += NT) {
    const int m = m0 + rr;
    const ConvPixel p = conv_pixel(m < a.M ? m : a.M - 1, a);
    in_off[rr] = conv_in_offset(p, a);
    const unsigned rel = (unsigned)(conv_out_pixel(p, a) - pix0);
    unsigned oo_row = (m < a.M) ? rel * (unsigned)a.o_cs * 4u : kInvalidRow;
    if (a.ups == 2 && m < a.M) oo_row |= conv_ups2_crop(p, a);
    o_off[rr] = oo_row;
    r_off[rr] = (m < a.M) ? rel * (unsigned)a.r_cs * 4u : kInvalidRow;
  }
}

// C/D register maps of the two MFMA shapes the kernels use.  A lane holds ONE column of a TS x TS tile, col(lane), and
// NR of its rows: accumulator register r is row row(row0, group(lane), r) of the tile whose first row is row0.  The
// kernels compute a lane's column and row group once, at their top, and hand both to the functions below (recomputed
// from the lane inside the epilogue they cost the exact kernel a VGPR and the Winograd kernel 24 more LDS reads); row()
// takes row0 so that the sum associates as (row0 + row in tile) + 4 grp, the form the LDS offsets fold best from.
struct MfmaCd32 {  // v_mfma_f32_32x32x*: 16 registers
  static constexpr int TS = 32, NR = 16;
  static __device__ __forceinline__ int col(const int lane) { return lane & 31; }
  static __device__ __forceinline__ int group(const int lane) { return lane >> 5; }
  static __device__ __forceinline__ int row(const int row0, const int grp, const int r) {
    return row0 + (r & 3) + 8 * (r >> 2) + 4 * grp;
  }
};
struct MfmaCd16 {  // v_mfma_f32_16x16x*: 4 registers
  static constexpr int TS = 16, NR = 4;
  static __device__ __forceinline__ int col(const int lane) { return lane & 15; }
  static __device__ __forceinline__ int group(const int lane) { return lane >> 4; }
  static __device__ __forceinline__ int row(const int row0, const int grp, const int r) { return row0 + 4 * grp + r; }
};

#if defined(__HIP_DEVICE_COMPILE__)
// The epilogue's descriptors, based at the tile's first pixel and column (see the row tables above)
constexpr int kRsrcFlags = 0x00020000;  // raw dword buffer, gfx9 data format 32
template <typename Args>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t conv_out_rsrc(Args& a, const long long pix0, const int n0) {
  return __builtin_amdgcn_make_buffer_rsrc(a.out + (pix0 * a.o_cs + a.o_co + n0), 0, 0x7fffffff, kRsrcFlags);
}
template <typename Args>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t conv_res_rsrc(Args& a, const long long pix0, const int n0) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.res ? a.res + (pix0 * a.r_cs + a.r_co + n0) : a.in), 0,
                                           0x7fffffff, kRsrcFlags);
}

// The epilogue of a tile: affine (folded BN or bias) -> leaky -> + addend -> store (x1 or x2-replicated).  The wave
// (wm, wn) holds TM x TN MFMA tiles of Map's shape; tile (i, j) covers rows (wm * TM + i) * TS ... and columns
// (wn * TN + j) * TS ... of the block tile; lcol / lgrp: the lane's Map::col / Map::group.  The caller's own variables
// are taken by reference, as a lambda in the caller would capture them: taken by value, conv_split_kernel<128, 128>
// came out with a different instruction mix.
template <typename Map, int TM, int TN, typename Args, typename Acc>
__device__ __forceinline__ void conv_epilogue(Args& a, const Acc (&acc)[TM][TN], unsigned* const& o_off, unsigned* const& r_off,
                                              const long long& pix0, const int& n0, const int& wm, const int& wn, const int& lcol,
                                              const int& lgrp) {
  constexpr int TS = Map::TS, NR = Map::NR;
  const __amdgpu_buffer_rsrc_t out_rsrc = conv_out_rsrc(a, pix0, n0);
  const __amdgpu_buffer_rsrc_t res_rsrc = conv_res_rsrc(a, pix0, n0);
  const int ups_dx = a.o_cs * 4, ups_dy = a.o_Wp * a.o_cs * 4;
  // The epilogue variant (which of scale / shift / leaky / addend / x2-replicate apply) is uniform for the
  // launch; it is resolved ONCE, outside the element loops, into a straight-line instance per combination —
  // with the tests inside the loops hipcc emitted a branch (and a serialising wait) per element.
  auto epilogue = [&](auto has_scale_, auto has_shift_, auto leaky_, auto has_res_, auto ups2_) {
    constexpr bool has_scale = decltype(has_scale_)::value, has_shift = decltype(has_shift_)::value;
    constexpr bool leaky = decltype(leaky_)::value, has_res = decltype(has_res_)::value, ups2 = decltype(ups2_)::value;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int ncol = (wn * TN + j) * TS + lcol;
      const int n = n0 + ncol;
      const bool nvalid = n < a.N;
      const int nc = nvalid ? n : a.N - 1;
      // the lane's column offset with bit 31 set for a column past N; added to a row offset with a SATURATING add, so
      // that "invalid row" + "invalid column" stays out of the descriptor's range (one instruction per address)
      const unsigned colc = (unsigned)ncol * 4u | (nvalid ? 0u : kInvalidRow);
      float sc = 1.0f, sh = 0.0f;
      if (has_scale) sc = a.scale[nc];
      if (has_scale || has_shift) sh = a.shift[nc];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        unsigned oo[NR];
        float rv[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const int row = Map::row((wm * TM + i) * TS, lgrp, r);
          oo[r] = __builtin_elementwise_add_sat(o_off[row], colc);
          if (has_res) rv[r] = buf_load_f32(res_rsrc, __builtin_elementwise_add_sat(r_off[row], colc));
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          float vv = acc[i][j][r];
          if (has_scale)
            vv = fmaf(vv, sc, sh);
          else if (has_shift)
            vv = vv + sh;
          if (leaky) vv = vy_leaky(vv);
          if (has_res) vv = vv + rv[r];
          if (!ups2) {
            buf_store_f32(vv, out_rsrc, oo[r], 0);
          } else {  // an offset with bit 31 set is out of the descriptor's range: that store is dropped
            const unsigned base = oo[r] & ~3u;
            const unsigned no_dx = (oo[r] & 1u) << 31, no_dy = (oo[r] & 2u) << 30;
            buf_store_f32(vv, out_rsrc, base, 0);
            buf_store_f32(vv, out_rsrc, base | no_dx, ups_dx);
            buf_store_f32(vv, out_rsrc, base | no_dy, ups_dy);
            buf_store_f32(vv, out_rsrc, base | no_dx | no_dy, ups_dy + ups_dx);
          }
        }
      }
    }
  };
  using T = std::true_type;
  using F = std::false_type;
  const bool f_scale = a.scale != nullptr, f_shift = a.shift != nullptr, f_leaky = a.leaky != 0;
  const bool f_res = a.res != nullptr, f_ups2 = a.ups == 2;
  if (f_scale && f_shift && f_leaky && !f_ups2) {           // conv + BN + leaky (+ residual): inference cells
    if (f_res) epilogue(T{}, T{}, T{}, T{}, F{});
    else epilogue(T{}, T{}, T{}, F{}, F{});
  } else if (f_scale && f_shift && f_leaky && !f_res) {     // transition cells: x2-replicated store
    epilogue(T{}, T{}, T{}, F{}, T{});
  } else if (!f_scale && !f_leaky && !f_ups2) {             // raw conv (training forward) / bias / gradients (+ accumulate)
    if (f_shift) {
      if (f_res) epilogue(F{}, T{}, F{}, T{}, F{});
      else epilogue(F{}, T{}, F{}, F{}, F{});
    } else {
      if (f_res) epilogue(F{}, F{}, F{}, T{}, F{});
      else epilogue(F{}, F{}, F{}, F{}, F{});
    }
  } else {
    __builtin_trap();  // no launch site builds any other combination (vy_conv_epilogue_supported, kernels.h)
  }
}

// train-mode BatchNorm: per-tile column sums of the raw accumulators of a 32x32-MFMA tile into a.stats
// ([tile_m][2][N]; deterministic: fixed order inside the tile, tiles are combined in order by the finalize kernel).
// `smem`: the block's LDS from its start — the operand stages, reused as [WM][2][BN] doubles.  (conv_igemm.hip keeps
// these statements in line: see there.)
template <int BN, int WM, int TM, int TN, typename Args, typename Acc>
__device__ __forceinline__ void conv_bn_stats(Args& a, const Acc (&acc)[TM][TN], unsigned* const& o_off, unsigned char* const& smem,
                                              const int& tile_m, const int& n0, const int& wm, const int& wn, const int& lcol,
                                              const int& lgrp, const int& tid) {
  // double accumulation: var = E[x^2] - mean^2 cancels badly in fp32 when |mean| >> std, and the
  // batch statistics must round to the same fp32 mean / var as the CPU checker's
  double s1[TN], s2[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    s1[j] = 0.0;
    s2[j] = 0.0;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = MfmaCd32::row((wm * TM + i) * 32, lgrp, r);
        const double vv = o_off[row] != kInvalidRow ? (double)acc[i][j][r] : 0.0;
        s1[j] += vv;
        s2[j] += vv * vv;
      }
    s1[j] += __shfl_xor(s1[j], 32);
    s2[j] += __shfl_xor(s2[j], 32);
  }
  __syncthreads();  // every wave is past its last LDS tile read
  double* red = reinterpret_cast<double*>(smem);  // [WM][2][BN]
  if (lgrp == 0) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = (wn * TN + j) * 32 + lcol;
      red[(wm * 2 + 0) * BN + col] = s1[j];
      red[(wm * 2 + 1) * BN + col] = s2[j];
    }
  }
  __syncthreads();
  if (tid < BN && n0 + tid < a.N) {
    double t1 = 0.0, t2 = 0.0;
#pragma unroll
    for (int w = 0; w < WM; ++w) {
      t1 += red[(w * 2 + 0) * BN + tid];
      t2 += red[(w * 2 + 1) * BN + tid];
    }
    a.stats[((long long)tile_m * 2 + 0) * a.N + n0 + tid] = t1;
    a.stats[((long long)tile_m * 2 + 1) * a.N + n0 + tid] = t2;
  }
}
#endif  // __HIP_DEVICE_COMPILE__

// The weight gradients' view of output pixel p of a conv (wgrad.hip, the pixel table): the byte offset of its dz vector
// inside the dz plane and of its (stride-scaled) centre pixel inside the input plane, both zero-bordered
struct WgradPix {
  unsigned long long zo, ao;
};
__device__ __forceinline__ WgradPix wgrad_pixel_offsets(int p, int Ho, int Wo, int z_cs, int a_Hp, int a_Wp, int a_cs, int stride) {
  const int x = p % Wo, t = p / Wo, y = t % Ho, b = t / Ho;
  WgradPix o;
  o.zo = ((unsigned long long)(b * (Ho + 2) + y + 1) * (Wo + 2) + x + 1) * z_cs * 4ull;
  o.ao = ((unsigned long long)(b * a_Hp + y * stride + 1) * a_Wp + x * stride + 1) * a_cs * 4ull;
  return o;
}

// ---- what the two weight-gradient kernels (wgrad.hip, wgrad_split.hip) do around their k-loops, ONE definition each.
// The k-loops themselves share nothing: one stages by LDS-DMA from the pixel table, the other splits in registers.

// Block -> (split, tile) and the split's pixel range.  All tiles of a split read the same pixel range: every n-tile its dz
// rows, every o-tile the input taps.  Blocks are dealt round-robin over the 8 XCDs (each with its own L2), so in launch
// order every XCD saw every split and each re-read went out to the fabric (round 2: 22.6 GB per step against 5.2 GB
// algorithmic).  So the linear block index goes through vy_xcd_tile: an XCD works through a CONTIGUOUS run of (split,
// tile) pairs, tile fastest — whole splits per XCD, their re-reads served by that XCD's L2.
// Grid: x over the tiles_m * tiles_n tiles of BM x BN, y over the splits; KP = pixels per k-step.
struct WgradTile {
  int split, o0, n0;  // the block's split, first output channel (slab row) and first GEMM column n = tap * Cin + cin
  int Ntot;           // k * k * Cin: the slab's row length
  int p_begin, T;     // first pixel of the split, and its k-steps of KP pixels
};
template <int BM, int BN, int KP>
__device__ __forceinline__ WgradTile wgrad_tile(const WgradArgs& a, const int tiles_n) {
  const int gx = gridDim.x;
  const int v = vy_xcd_tile(blockIdx.y * gx + blockIdx.x, gx * gridDim.y);
  WgradTile t;
  t.split = v / gx;
  const int tile_id = v - t.split * gx;
  const int tile_m = tile_id / tiles_n, tile_n = tile_id - tile_m * tiles_n;
  t.o0 = tile_m * BM;
  t.n0 = tile_n * BN;
  t.Ntot = a.k * a.k * a.Cin;
  t.p_begin = t.split * a.k_per_split;
  int p_end = t.p_begin + a.k_per_split;
  if (p_end > a.M) p_end = a.M;
  t.T = (p_end - t.p_begin + KP - 1) / KP;
  return t;
}
// the split's slab [Cout][Ntot]
__device__ __forceinline__ float* wgrad_slab(const WgradArgs& a, const WgradTile& t) {
  return a.slabs + (long long)t.split * a.Cout * t.Ntot;
}

// byte offsets of the split's first pixel: the pixel table's entries are relative to it
__device__ __forceinline__ WgradPix wgrad_split_base(const WgradArgs& a, const WgradTile& t) {
  return wgrad_pixel_offsets(t.p_begin, a.Ho, a.Wo, a.z_cs, a.a_Hp, a.a_Wp, a.a_cs, a.stride);
}

// GEMM column bn of a staging lane (the first of its chunk; a chunk lies inside one tap, Cin being a multiple of 32) ->
// tap offset (dy, dx) and input channel.  Columns past k*k*Cin: tap 0 / channel 0 (the column is never stored)
struct WgradCol {
  bool ok;
  int tap, cin, dy, dx;
};
__device__ __forceinline__ WgradCol wgrad_column(const WgradArgs& a, const int bn, const int Ntot) {
  WgradCol c;
  c.ok = bn < Ntot;
  c.tap = c.ok ? bn / a.Cin : 0;
  c.cin = c.ok ? bn - c.tap * a.Cin : 0;
  const int pad = a.k >> 1;
  c.dy = a.k == 3 ? c.tap / 3 - pad : 0;
  c.dx = a.k == 3 ? c.tap % 3 - pad : 0;
  return c;
}

// Slab row (output channel) of accumulator register r of a 32x32 MFMA tile (MfmaCd32: grp = the lane's row group).
// IL = 1: the tile covers rows row0 .. row0 + 31.  IL = 2: tile i of a pair whose operand rows were read interleaved
// (wgrad_kernel's ds_read_b64: MFMA tile i holds the rows {2 l + i} of the pair's 64)
template <int IL = 1>
__device__ __forceinline__ int wgrad_slab_row(const int row0, const int grp, const int r, const int i = 0) {
  return row0 + IL * MfmaCd32::row(0, grp, r) + i;
}

// ---- the ordered column sum: the second stage of the training step's reductions (train_kernels.hip: BatchNorm
// statistics, BN-backward sums, bias and stem gradients).  A first stage leaves partial rows
// [n_part][n_cols] in a fixed layout; a block of COLS columns x G row groups then adds them in ONE fixed tree: row group g
// adds rows t0+g, t0+g+G, t0+g+2G, ... in that order (colsum_rows), then group 0 adds the G group sums in group order
// (colsum_finish).  No atomics, nothing that depends on which block finishes first: a training step is bit-reproducible
// run to run, and every caller gives the same bits as the others would for the same rows.  The float64 cell tests
// (tests/test_gpu_train_cells.py and its siblings) pass a reordered tree within their tolerances, so they do not hold
// the order; tools/train_bits.py does, and the SyncBatchNorm statistics exchange relies on every rank summing alike.
// Geometry (COLS x G), the accumulator type Acc and the loads in flight U are compile-time arguments of the call.
// (wgrad.hip's slab_reduce_wide_kernel adds the split-K slabs by a variant of this tree and keeps its own loop: see there.)

// The rows of NC columns at once (their loads interleaved): p[k] points at column k's element of row 0, rs = row stride
// in elements, t = the thread's first row (t0 + g), t1 = end of the row range.  U changes how many loads are in flight
// (the loop is latency-bound), never the order of the additions.
template <int G, int U, int NC, typename Acc, typename T>
__device__ __forceinline__ void colsum_rows(const T* const (&p)[NC], const long long rs, int t, const int t1, Acc (&acc)[NC]) {
  for (; t + (U - 1) * G < t1; t += U * G) {
    T v[NC][U];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int k = 0; k < NC; ++k) v[k][u] = p[k][(long long)(t + u * G) * rs];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int k = 0; k < NC; ++k) acc[k] += (Acc)v[k][u];
  }
  if (U > 1)
    for (; t < t1; t += G)
#pragma unroll
      for (int k = 0; k < NC; ++k) acc[k] += (Acc)p[k][(long long)t * rs];
}
// The finish: every thread of the block (column cx, row group g) hands in its group sums; after it group 0 holds the
// columns' totals in acc.  Contains the block's barrier: call it outside any column bound.
template <int G, int COLS, int NC, typename Acc>
__device__ __forceinline__ void colsum_finish(Acc (&acc)[NC], const int cx, const int g) {
  __shared__ Acc red[NC][G][COLS + 1];
#pragma unroll
  for (int k = 0; k < NC; ++k) red[k][g][cx] = acc[k];
  __syncthreads();
  if (g != 0) return;
#pragma unroll
  for (int k = 0; k < NC; ++k) acc[k] = 0;
#pragma unroll 8
  for (int r = 0; r < G; ++r)
#pragma unroll
    for (int k = 0; k < NC; ++k) acc[k] += red[k][r][cx];
}
