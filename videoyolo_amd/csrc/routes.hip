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
#include "kernels.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kTileC = 64, kTileP = 64;

// LDS index of (channel c, tile pixel pp)
__device__ inline int lds_at(int c, int pp) { return c * kTileP + (pp ^ (((c >> 2) & 15) << 2)); }

// which route, frame, channel tile and pixel tile block `bid` owns
struct TileRef {
  int r, b, c0, p0;
};
__device__ inline TileRef locate(const RouteArgs& a, int bid) {
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

hipError_t launch(RouteArgs a, bool import, hipStream_t s) {
  if (a.n < 1 || a.n > 3 || a.B < 1) return hipErrorInvalidValue;
  long long tiles = 0;
  for (int i = 0; i < a.n; ++i) {
    RouteXfer& x = a.r[i];
    if (!x.plane || !x.nchw || x.H < 1 || x.W < 1 || x.C < kTileC || x.C % kTileC || x.cs % 4 || x.co % 4 ||
        x.co + x.C > x.cs)
      return hipErrorInvalidValue;
    tiles += (long long)a.B * (x.C / kTileC) * ((x.H * x.W + kTileP - 1) / kTileP);
    if (tiles >= (1ll << 31)) return hipErrorInvalidValue;
    a.tile_end[i] = (int)tiles;
  }
  if (import)
    hipLaunchKernelGGL(route_xfer_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(route_xfer_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t vy_launch_route_import(const RouteArgs& a, hipStream_t s) { return launch(a, true, s); }
hipError_t vy_launch_route_export(const RouteArgs& a, hipStream_t s) { return launch(a, false, s); }
