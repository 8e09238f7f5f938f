// routes.hip — the three Darknet-53 route tensors across the API (the heads-only net, the features-only forward):
// dense NCHW fp32 (the reference's layout: extract_base_features.py saves features[:15] / [15:24] / [24:] as they come
// out of the backbone) <-> the interior of a slice of a zero-bordered NHWC activation plane.  Moving a route
// in or out is a transpose per frame: [C][H*W] <-> [H*W][C] with the plane's row pitch (W + 2) * cs and its border.
//
// One launch moves all three routes.  A 256-thread block owns one 64-channel x 64-pixel tile of one frame of one route
// (pixels are the flattened y * W + x of the frame, so a tile may span image rows):
//   NCHW side   a channel's 64 pixels are 256 contiguous bytes: 16 lanes x 16-B loads / stores per channel row when H*W is
//               a multiple of 4 (every row then starts 16-B aligned); otherwise one dword per lane, 64 lanes on one row
//               (still 256 contiguous bytes per wave instruction)
//   plane side  a pixel's 64 channels are 256 contiguous bytes: 16 lanes x 16-B accesses per pixel, always aligned
//               (cs and co are multiples of 4, the plane offsets 256-B aligned)
//   LDS         the tile as [64 channels][64 pixels], the 16-B pixel slots of channel c XOR-swizzled by (c / 4) % 16: a row
//               access (one channel, 4 pixels per lane) stays one aligned 16-B slot, and the 16 lanes of a column access (one
//               pixel, 4 channels per lane) land on 16 different slots (2-way on 32 banks instead of 16-way)
// Only interior pixels of channels [co, co + C) are touched: import never writes a border or any other channel of the
// plane (the concat planes' upsampled-transition range [0, co) is the transition conv's), export never writes outside
// the caller's dense tensor.
//
// route_import_pool is route_import over a window of stored frames: a block owns the same tile of one CLIP, keeps its
// share of the tile in registers as accumulators over the clip's k frames of the bank (temporal.hip's arithmetic, in
// table order; the loads of frame t + 1 are issued before frame t is reduced), and only the pooled tile goes through
// the LDS and out, once.  k reads and one write per element, no per-frame plane in between.
#include "kernels.h"
#include "../../include/vyolo.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kTileC = 64, kTileP = 64;

// LDS index of (channel c, tile pixel pp)
__device__ inline int lds_at(int c, int pp) { return c * kTileP + (pp ^ (((c >> 2) & 15) << 2)); }

// which route, frame, channel tile and pixel tile block `bid` owns
struct TileRef {
  int r, b, c0, p0;
};
template <typename Args>
__device__ inline TileRef locate(const Args& a, int bid) {
  TileRef t;
  t.r = 0;
  while (t.r + 1 < a.n && bid >= a.tile_end[t.r]) ++t.r;
  const RouteXfer& x = a.r[t.r];
  int i = bid - (t.r ? a.tile_end[t.r - 1] : 0);
  const int pt = (x.H * x.W + kTileP - 1) / kTileP, ct = x.C / kTileC;
  t.p0 = (i % pt) * kTileP;
  i /= pt;
  t.c0 = (i % ct) * kTileC;
  t.b = i / ct;
  return t;
}

template <bool kImport>
__global__ __launch_bounds__(256) void route_xfer_kernel(RouteArgs a) {
  __shared__ __attribute__((aligned(16))) float tile[kTileC * kTileP];
  const TileRef t = locate(a, (int)blockIdx.x);  // block-uniform: every branch below is too
  const RouteXfer& x = a.r[t.r];
  const int HW = x.H * x.W, tid = (int)threadIdx.x;
  float* nchw = x.nchw + ((long long)t.b * x.C + t.c0) * HW + t.p0;  // (b, c0, p0)
  const long long frame = (long long)t.b * (x.H + 2) * (x.W + 2);
  const bool vec = (HW & 3) == 0;
  const int np = min(kTileP, HW - t.p0);  // pixels of this tile (a multiple of 4 when vec)
  // plane address of tile pixel `pp`, channel c0 of the route (co + c0 of the plane)
  auto plane_at = [&](int pp) {
    const int p = t.p0 + pp, y = p / x.W, xx = p - y * x.W;
    return x.plane + (frame + (long long)(y + 1) * (x.W + 2) + xx + 1) * x.cs + x.co + t.c0;
  };
  if (kImport) {
    if (vec) {
      for (int k = tid; k < kTileC * (kTileP / 4); k += 256) {
        const int c = k >> 4, q = (k & 15) * 4;
        if (q < np) *reinterpret_cast<f32x4*>(&tile[lds_at(c, q)]) = *reinterpret_cast<const f32x4*>(nchw + (long long)c * HW + q);
      }
    } else {
      for (int k = tid; k < kTileC * kTileP; k += 256) {
        const int c = k >> 6, pp = k & 63;
        if (pp < np) tile[lds_at(c, pp)] = nchw[(long long)c * HW + pp];
      }
    }
    __syncthreads();
    for (int k = tid; k < kTileP * (kTileC / 4); k += 256) {
      const int pp = k >> 4, c = (k & 15) * 4;
      if (pp >= np) continue;
      f32x4 v;
      v.x = tile[lds_at(c + 0, pp)];
      v.y = tile[lds_at(c + 1, pp)];
      v.z = tile[lds_at(c + 2, pp)];
      v.w = tile[lds_at(c + 3, pp)];
      *reinterpret_cast<f32x4*>(plane_at(pp) + c) = v;
    }
  } else {
    for (int k = tid; k < kTileP * (kTileC / 4); k += 256) {
      const int pp = k >> 4, c = (k & 15) * 4;
      if (pp >= np) continue;
      const f32x4 v = *reinterpret_cast<const f32x4*>(plane_at(pp) + c);
      tile[lds_at(c + 0, pp)] = v.x;
      tile[lds_at(c + 1, pp)] = v.y;
      tile[lds_at(c + 2, pp)] = v.z;
      tile[lds_at(c + 3, pp)] = v.w;
    }
    __syncthreads();
    if (vec) {
      for (int k = tid; k < kTileC * (kTileP / 4); k += 256) {
        const int c = k >> 4, q = (k & 15) * 4;
        if (q < np) *reinterpret_cast<f32x4*>(nchw + (long long)c * HW + q) = *reinterpret_cast<const f32x4*>(&tile[lds_at(c, q)]);
      }
    } else {
      for (int k = tid; k < kTileC * kTileP; k += 256) {
        const int c = k >> 6, pp = k & 63;
        if (pp < np) nchw[(long long)c * HW + pp] = tile[lds_at(c, pp)];
      }
    }
  }
}

// one frame's share of a tile: kN values per lane (vector path: 4 x 16 B; dword path: 16 x 4 B)
template <int kN, typename V>
struct Frag {
  V v[kN];
};

template <int kJoin>
__device__ inline float reduce(float acc, float v) {
  if (kJoin == VY_JOIN_MAX) return v > acc ? v : acc;  // strict: the earliest frame's bits survive a tie
  return acc + v;
}
template <int kJoin>
__device__ inline f32x4 reduce(f32x4 acc, f32x4 v) {
  acc.x = reduce<kJoin>(acc.x, v.x);
  acc.y = reduce<kJoin>(acc.y, v.y);
  acc.z = reduce<kJoin>(acc.z, v.z);
  acc.w = reduce<kJoin>(acc.w, v.w);
  return acc;
}

// pool the k frames of `row` over this lane's share of the tile; load(frame, frag) reads one frame's share
template <int kJoin, int kN, typename V, typename Load>
__device__ inline void pool_frames(const int* row, int k, Frag<kN, V>& acc, Load load) {
  load(row[0], acc);
  if (k > 1) {
    Frag<kN, V> cur, nxt;
    load(row[1], cur);
    for (int t = 2; t < k; ++t) {
      load(row[t], nxt);  // in flight while frame t - 1 is reduced
#pragma unroll
      for (int j = 0; j < kN; ++j) acc.v[j] = reduce<kJoin>(acc.v[j], cur.v[j]);
      cur = nxt;
    }
#pragma unroll
    for (int j = 0; j < kN; ++j) acc.v[j] = reduce<kJoin>(acc.v[j], cur.v[j]);
  }
  if (kJoin == VY_JOIN_MEAN) {
    const float kf = (float)k;
#pragma unroll
    for (int j = 0; j < kN; ++j) acc.v[j] = acc.v[j] / kf;
  }
}

template <int kJoin>
__global__ __launch_bounds__(256) void route_import_pool_kernel(RoutePoolArgs a) {
  __shared__ __attribute__((aligned(16))) float tile[kTileC * kTileP];
  const TileRef t = locate(a, (int)blockIdx.x);  // block-uniform: every branch below is too
  const RouteXfer& x = a.r[t.r];
  const int HW = x.H * x.W, tid = (int)threadIdx.x;
  const long long fstride = (long long)x.C * HW;                   // floats per frame of the bank
  const float* bank = x.nchw + (long long)t.c0 * HW + t.p0;        // (frame 0, c0, p0)
  const long long frame = (long long)t.b * (x.H + 2) * (x.W + 2);
  const int* row = a.table + t.b * a.k;
  const int np = min(kTileP, HW - t.p0);  // pixels of this tile (a multiple of 4 on the vector path)
  if ((HW & 3) == 0) {  // every frame of the bank and every channel row starts 16-B aligned
    const int c = tid >> 4, q = (tid & 15) * 4;  // channels c, c + 16, c + 32, c + 48; pixels [q, q + 4)
    Frag<4, f32x4> acc;
    pool_frames<kJoin>(row, a.k, acc, [&](int f, Frag<4, f32x4>& o) {
      const float* src = bank + f * fstride + (long long)c * HW + q;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        o.v[j] = q < np ? *reinterpret_cast<const f32x4*>(src + (long long)(16 * j) * HW) : f32x4{0.f, 0.f, 0.f, 0.f};
    });
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4*>(&tile[lds_at(c + 16 * j, q)]) = acc.v[j];
  } else {
    const int c = tid >> 6, pp = tid & 63;  // channels c, c + 4, ..., c + 60; pixel pp
    Frag<16, float> acc;
    pool_frames<kJoin>(row, a.k, acc, [&](int f, Frag<16, float>& o) {
      const float* src = bank + f * fstride + (long long)c * HW + pp;
#pragma unroll
      for (int j = 0; j < 16; ++j) o.v[j] = pp < np ? src[(long long)(4 * j) * HW] : 0.f;
    });
#pragma unroll
    for (int j = 0; j < 16; ++j) tile[lds_at(c + 4 * j, pp)] = acc.v[j];
  }
  __syncthreads();
  for (int i = tid; i < kTileP * (kTileC / 4); i += 256) {
    const int pp = i >> 4, c = (i & 15) * 4;
    if (pp >= np) continue;
    f32x4 v;
    v.x = tile[lds_at(c + 0, pp)];
    v.y = tile[lds_at(c + 1, pp)];
    v.z = tile[lds_at(c + 2, pp)];
    v.w = tile[lds_at(c + 3, pp)];
    const int p = t.p0 + pp, y = p / x.W, xx = p - y * x.W;
    *reinterpret_cast<f32x4*>(x.plane + (frame + (long long)(y + 1) * (x.W + 2) + xx + 1) * x.cs + x.co + t.c0 + c) = v;
  }
}

// the routes' geometry, checked; fills tile_end for `batch` frames / clips per route and returns the tiles (0: invalid)
long long count_tiles(const RouteXfer* r, int n, int batch, int* tile_end) {
  if (n < 1 || n > 3 || batch < 1) return 0;
  long long tiles = 0;
  for (int i = 0; i < n; ++i) {
    const RouteXfer& x = r[i];
    if (!x.plane || !x.nchw || x.H < 1 || x.W < 1 || x.C < kTileC || x.C % kTileC || x.cs % 4 || x.co % 4 ||
        x.co + x.C > x.cs)
      return 0;
    tiles += (long long)batch * (x.C / kTileC) * ((x.H * x.W + kTileP - 1) / kTileP);
    if (tiles >= (1ll << 31)) return 0;
    tile_end[i] = (int)tiles;
  }
  return tiles;
}

hipError_t launch(RouteArgs a, bool import, hipStream_t s) {
  const long long tiles = count_tiles(a.r, a.n, a.B, a.tile_end);
  if (!tiles) return hipErrorInvalidValue;
  if (import)
    hipLaunchKernelGGL(route_xfer_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(route_xfer_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t vy_launch_route_import(const RouteArgs& a, hipStream_t s) { return launch(a, true, s); }
hipError_t vy_launch_route_export(const RouteArgs& a, hipStream_t s) { return launch(a, false, s); }

hipError_t vy_launch_route_import_pool(const RoutePoolArgs& a0, hipStream_t s) {
  RoutePoolArgs a = a0;
  if (a.k < 1 || a.T < 1 || a.B < 1 || (long long)a.B * a.k > VY_ROUTE_TABLE_MAX ||
      (a.join != VY_JOIN_MAX && a.join != VY_JOIN_MEAN))
    return hipErrorInvalidValue;
  for (int i = 0; i < a.B * a.k; ++i)
    if (a.table[i] < 0 || a.table[i] >= a.T) return hipErrorInvalidValue;
  const long long tiles = count_tiles(a.r, a.n, a.B, a.tile_end);
  if (!tiles) return hipErrorInvalidValue;
  if (a.join == VY_JOIN_MAX)
    hipLaunchKernelGGL(route_import_pool_kernel<VY_JOIN_MAX>, dim3((unsigned)tiles), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(route_import_pool_kernel<VY_JOIN_MEAN>, dim3((unsigned)tiles), dim3(256), 0, s, a);
  return hipGetLastError();
}
