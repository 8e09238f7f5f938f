// augment.hip — the frames side of the reference's training transform, YOLO3VideoTrainTransform.__call__
// (models/definitions/yolo/transforms.py:199-245): random_color_distort -> random_expand -> crop -> imresize with a
// random interpolation -> flip -> to_tensor -> normalize, for a batch of k-frame clips in ONE launch.  The random draws
// are made on the host (videoyolo_amd/transforms.py, `draw`) and arrive as one vy_train_aug per sample in the kernel
// arguments.  One thread per destination pixel (three channels), grid (ceil(W / 256), H, samples * k) like
// resize_normalize_kernel of preproc.hip; every branch on a sample's parameters is uniform across the block.
//
// A thread un-flips its column, computes its taps in CROP coordinates (tap indices clamp to the crop: the reference
// resizes the cropped array), moves each tap into the canvas by the crop offset, and reads it: inside the pasted source
// rectangle the uint8 pixel, colour-distorted in fp32 in the drawn order; outside it the fill, undistorted (the expansion
// follows the colour step).  That bounds test is also what keeps every read inside the sample's frames.  Nothing is
// rounded to uint8 and nothing is clamped: after random_color_distort the reference's frames are float32, so imresize
// runs cv::resize on CV_32FC3 and to_tensor only divides.
//
// Arithmetic [UPSTREAM-RECALLED, restated from memory like preproc.hip; DESIGN.md §13].  Built with -ffp-contract=off:
// every value is the stated sequence of fp32 operations, which tests/train_transform_ref.py repeats in numpy.
//   taps      rows first: r_j = (P(j,0) * a0 + P(j,1) * a1) + ..., then out = (r_0 * b0 + r_1 * b1) + ...
//   nearest   s = min(floor(d * scale), ssize - 1); scale = ssize / dsize in double
//   linear    f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s; s < 0 -> (0, 0); s >= ssize - 1 -> (ssize - 1, 0);
//             weights (1 - f, f) on taps s, min(s + 1, ssize - 1)
//   cubic     Keys, A = -0.75, taps s - 1 .. s + 2, interpolateCubic's operation order
//   Lanczos-4 taps s - 3 .. s + 4, vy_lanczos4_weights (include/vy_math.h)
//   area      both scales >= 1 with integer factors: one running sum over the block, row-major, times 1.f / area;
//             both >= 1, fractional: computeResizeAreaTab's weights, the span walked in a loop (any shrink factor);
//             a side enlarged: the linear arithmetic with s = floor(d * scale),
//             f = (float)((d + 1) - (s + 1) * inv_scale), f = f <= 0 ? 0 : f - floor(f)
//   same size nearest with scale 1, which is a copy
//
// Mixup (vy_train_transform_mix) [UPSTREAM-RECALLED: gluoncv.data.MixupDetection.__getitem__, restated from
// memory].  The MIX instantiation treats src_h x src_w as the mix canvas: two sources of their own extents, both at the
// canvas origin, and inside the canvas a pixel is read from up to two of them and blended BEFORE the colour ops:
//   l1 = (float)lambd, l2 = (float)(1.0 - lambd)       (the subtraction in double, on the host)
//   both cover      m = (float)p1 * l1 + (float)p2 * l2   (each product rounded to fp32, then added)
//   first only      m = (float)p1 * l1
//   second only     m = 0.0f + (float)p2 * l2
//   neither         m = 0
//   mixed pixel     (uint8)m, truncated toward zero, not rounded; it cannot leave [0, 255]
// That uint8 value is what the colour step converts to float.  A sample without a second source takes the plain read.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <type_traits>

#include "../../include/vy_math.h"
#include "vy_support.h"

namespace {

enum { kNearest = 0, kLinear = 1, kCubic = 2, kAreaFrac = 3, kLanczos = 4, kAreaInt = 5, kAreaLinear = 6 };

struct AugArgs {
  const uint8_t* src;
  float* dst;       // (n, k, 3, H, W), already offset to this chunk's first sample
  int n, k, H, W;
  float fill[3], mean[3], stdv[3];
  vy_train_aug d[VY_AUG_CHUNK];  // interp holds the kernel's mode (kNearest .. kAreaLinear)
};

static_assert(sizeof(vy_train_aug) == 144 && sizeof(AugArgs) <= 4096, "the descriptors must fit the argument segment");

// the mix launch's arguments: the same head, and a vy_train_mix beside every vy_train_aug
struct MixArgs {
  const uint8_t* src;
  float* dst;
  int n, k, H, W;
  float fill[3], mean[3], stdv[3];
  vy_train_aug d[VY_MIX_CHUNK];
  vy_train_mix m[VY_MIX_CHUNK];
};

static_assert(sizeof(vy_train_mix) == 32 && sizeof(MixArgs) <= 4096, "the mix descriptors must fit the argument segment");

struct Px {
  float c[3];
};

// frame t of a sample of the mix launch: the first source's frame, the second's (null for a sample without a second
// source) and the sample's vy_train_mix.  The plain launch's frame is the bare pointer.
struct MixFrame {
  const uint8_t* S;
  const uint8_t* S2;
  vy_train_mix m;
};

// the uint8 pixel (x, y) of the mix canvas as floats: the truncated blend of the sources that cover (x, y); each read
// stays inside its own source's frame.  A sample without a second source takes the plain read (the canvas is its source).
__device__ __forceinline__ void mixed_pixel(const vy_train_aug& d, const MixFrame& F, int x, int y, float& r, float& g,
                                            float& b) {
  if (F.S2 == nullptr) {  // uniform: the sample's
    const uint8_t* q = F.S + ((long long)y * d.src_w + x) * 3;
    r = (float)q[0];
    g = (float)q[1];
    b = (float)q[2];
    return;
  }
  const vy_train_mix& m = F.m;
  r = g = b = 0.0f;
  if (x < m.w1 && y < m.h1) {
    const uint8_t* q = F.S + ((long long)y * m.w1 + x) * 3;
    r = (float)q[0] * m.l1;
    g = (float)q[1] * m.l1;
    b = (float)q[2] * m.l1;
  }
  if (x < m.w2 && y < m.h2) {
    const uint8_t* q = F.S2 + ((long long)y * m.w2 + x) * 3;
    r = r + (float)q[0] * m.l2;
    g = g + (float)q[1] * m.l2;
    b = b + (float)q[2] * m.l2;
  }
  r = (float)(int)r;  // (uint8)m: truncated toward zero, 0 <= m < 256
  g = (float)(int)g;
  b = (float)(int)b;
}

// the pixel at crop coordinates (cx, cy) of frame `S`: the distorted source inside the paste, the fill outside it
// (the mix launch: the paste is the mix canvas)
template <class Args, class Src>
__device__ __forceinline__ Px fetch(const Args& a, const vy_train_aug& d, Src S, int cx, int cy) {
  const int x = cx + d.crop_x - d.paste_x, y = cy + d.crop_y - d.paste_y;
  Px p;
  if (x < 0 || y < 0 || x >= d.src_w || y >= d.src_h) {
    p.c[0] = a.fill[0];
    p.c[1] = a.fill[1];
    p.c[2] = a.fill[2];
    return p;
  }
  // MIX is the frame's type, and the plain read stays written out here: through a helper shared with the mix launch the
  // plain instantiation no longer compiled to the code it was (1.5 - 2.7 % slower on linear and Lanczos-4)
  constexpr bool MIX = std::is_same<Src, MixFrame>::value;
  float r, g, b;
  if constexpr (MIX) {
    mixed_pixel(d, S, x, y, r, g, b);
  } else {
    const uint8_t* q = S + ((long long)y * d.src_w + x) * 3;
    r = (float)q[0];
    g = (float)q[1];
    b = (float)q[2];
  }
#pragma unroll
  for (int i = 0; i < VY_AUG_MAX_OPS; ++i) {  // unrolled: constant indices keep the descriptor in registers
    if (i >= d.num_ops) break;
    const float u = d.a[i];
    switch (d.op[i]) {
      case VY_AUG_BRIGHTNESS:
        r = r + u;
        g = g + u;
        b = b + u;
        break;
      case VY_AUG_CONTRAST:
        r = r * u;
        g = g * u;
        b = b * u;
        break;
      case VY_AUG_SATURATION: {
        float gray = (r * 0.299f + g * 0.587f) + b * 0.114f;
        gray = gray * d.b[i];
        r = r * u + gray;
        g = g * u + gray;
        b = b * u + gray;
        break;
      }
      default: {  // VY_AUG_HUE (op codes are validated on the host)
        const float o0 = (r * d.hue[0][0] + g * d.hue[1][0]) + b * d.hue[2][0];
        const float o1 = (r * d.hue[0][1] + g * d.hue[1][1]) + b * d.hue[2][1];
        const float o2 = (r * d.hue[0][2] + g * d.hue[1][2]) + b * d.hue[2][2];
        r = o0;
        g = o1;
        b = o2;
        break;
      }
    }
  }
  p.c[0] = r;
  p.c[1] = g;
  p.c[2] = b;
  return p;
}

__device__ __forceinline__ int clampi(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

__device__ __forceinline__ void src_coord(int d, double scale, int& s, float& f) {
  f = (float)(((double)d + 0.5) * scale - 0.5);
  s = (int)floorf(f);
  f -= (float)s;
}

// N taps (index clamped to [0, ssize - 1], fp32 weight) of destination index d along one axis
template <int MODE, int N>
__device__ __forceinline__ void axis_taps(int d, int ssize, int dsize, int idx[N], float w[N]) {
  const double scale = (double)ssize / (double)dsize;
  if constexpr (MODE == kNearest) {
    const int s = (int)floor((double)d * scale);
    idx[0] = s < ssize - 1 ? s : ssize - 1;
    w[0] = 1.0f;
  } else if constexpr (MODE == kLinear || MODE == kAreaLinear) {
    int s;
    float f;
    if constexpr (MODE == kLinear) {
      src_coord(d, scale, s, f);
    } else {
      const double inv_scale = (double)dsize / (double)ssize;
      s = (int)floor((double)d * scale);
      f = (float)((double)(d + 1) - (double)(s + 1) * inv_scale);
      f = f <= 0.0f ? 0.0f : f - floorf(f);
    }
    if (s < 0) {
      s = 0;
      f = 0.0f;
    }
    if (s >= ssize - 1) {
      s = ssize - 1;
      f = 0.0f;
    }
    idx[0] = s;
    idx[N - 1] = s + 1 < ssize ? s + 1 : ssize - 1;
    w[0] = 1.0f - f;
    w[N - 1] = f;
  } else if constexpr (MODE == kCubic) {
    int s;
    float x;
    src_coord(d, scale, s, x);
    const float A = -0.75f;
    w[0] = ((A * (x + 1.0f) - 5.0f * A) * (x + 1.0f) + 8.0f * A) * (x + 1.0f) - 4.0f * A;
    w[1] = ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f;
    w[2] = ((A + 2.0f) * (1.0f - x) - (A + 3.0f)) * (1.0f - x) * (1.0f - x) + 1.0f;
    w[N - 1] = 1.0f - w[0] - w[1] - w[2];
#pragma unroll
    for (int t = 0; t < N; ++t) idx[t] = clampi(s - 1 + t, ssize);
  } else {
    int s;
    float x;
    src_coord(d, scale, s, x);
    vy_lanczos4_weights(x, w);
#pragma unroll
    for (int t = 0; t < N; ++t) idx[t] = clampi(s - 3 + t, ssize);
  }
}

template <int MODE, int N, class Args, class Src>
__device__ __forceinline__ Px resample(const Args& a, const vy_train_aug& d, Src S, int ux, int dy) {
  int xi[N], yi[N];
  float xw[N], yw[N];
  axis_taps<MODE, N>(ux, d.crop_w, a.W, xi, xw);
  axis_taps<MODE, N>(dy, d.crop_h, a.H, yi, yw);
  Px acc;
#pragma unroll 1
  for (int j = 0; j < N; ++j) {  // a rolled loop over the rows (their taps are uniform: dy is the block's)
    int y = yi[0];
    float wy = yw[0];
#pragma unroll
    for (int t = 1; t < N; ++t)
      if (t == j) {
        y = yi[t];
        wy = yw[t];
      }
    Px row;
#pragma unroll
    for (int t = 0; t < N; ++t) {
      const Px p = fetch(a, d, S, xi[t], y);
#pragma unroll
      for (int c = 0; c < 3; ++c) row.c[c] = t == 0 ? p.c[c] * xw[0] : row.c[c] + p.c[c] * xw[t];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) acc.c[c] = j == 0 ? row.c[c] * wy : acc.c[c] + row.c[c] * wy;
  }
  return acc;
}

// computeResizeAreaTab for one destination index as a span: source indices first .. last, with the weight of the first
// (when it is a partial head cell), of the whole cells, and of the last (when it is a partial tail cell)
struct AreaSpan {
  int first, last, s1, s2;
  float wh, wb, wt;
  __device__ __forceinline__ float weight(int s) const { return s < s1 ? wh : (s < s2 ? wb : wt); }
};

__device__ __forceinline__ AreaSpan area_span(int d, int ssize, int dsize) {
  const double scale = (double)ssize / (double)dsize;
  const double f1 = (double)d * scale, f2 = f1 + scale;
  const double cell = fmin(scale, (double)ssize - f1);
  int s1 = (int)ceil(f1), s2 = (int)floor(f2);
  s2 = s2 < ssize - 1 ? s2 : ssize - 1;
  s1 = s1 < s2 ? s1 : s2;
  AreaSpan a;
  a.s1 = s1;
  a.s2 = s2;
  const bool head = (double)s1 - f1 > 1e-3, tail = f2 - (double)s2 > 1e-3;
  a.first = head ? s1 - 1 : s1;
  a.last = tail ? s2 : s2 - 1;
  a.wh = (float)(((double)s1 - f1) / cell);
  a.wb = (float)(1.0 / cell);
  a.wt = (float)(fmin(fmin(f2 - (double)s2, 1.0), cell) / cell);
  return a;
}

__device__ __forceinline__ const uint8_t* frame_of(const AugArgs& a, const vy_train_aug& d, int sample, int t) {
  return a.src + d.src_offset + (long long)t * d.src_h * d.src_w * 3;
}

__device__ __forceinline__ MixFrame frame_of(const MixArgs& a, const vy_train_aug& d, int sample, int t) {
  MixFrame F;
  F.m = a.m[sample];  // uniform, like d
  F.S = a.src + d.src_offset + (long long)t * F.m.h1 * F.m.w1 * 3;
  F.S2 = F.m.src2_offset < 0 ? nullptr : a.src + F.m.src2_offset + (long long)t * F.m.h2 * F.m.w2 * 3;
  return F;
}

// Args = AugArgs is the plain transform; Args = MixArgs blends two sources in source_pixel()
template <class Args>
__global__ __launch_bounds__(256) void train_transform_kernel(Args a) {
  const int dx = blockIdx.x * 256 + threadIdx.x;
  if (dx >= a.W) return;
  const int dy = blockIdx.y, frame = blockIdx.z;
  const int sample = frame / a.k, t = frame - sample * a.k;
  const vy_train_aug d = a.d[sample];  // uniform: the descriptor sits in scalar registers
  const auto S = frame_of(a, d, sample, t);
  const int ux = d.flip ? a.W - 1 - dx : dx;
  Px v;
  switch (d.interp) {
    case kNearest:
      v = resample<kNearest, 1>(a, d, S, ux, dy);
      break;
    case kLinear:
      v = resample<kLinear, 2>(a, d, S, ux, dy);
      break;
    case kAreaLinear:
      v = resample<kAreaLinear, 2>(a, d, S, ux, dy);
      break;
    case kCubic:
      v = resample<kCubic, 4>(a, d, S, ux, dy);
      break;
    case kLanczos:
      v = resample<kLanczos, 8>(a, d, S, ux, dy);
      break;
    case kAreaInt: {
      const int ix = d.crop_w / a.W, iy = d.crop_h / a.H;
      float sum[3] = {0.0f, 0.0f, 0.0f};
      for (int yy = 0; yy < iy; ++yy)
        for (int xx = 0; xx < ix; ++xx) {
          const Px p = fetch(a, d, S, ux * ix + xx, dy * iy + yy);
#pragma unroll
          for (int c = 0; c < 3; ++c) sum[c] = sum[c] + p.c[c];
        }
      const float scale = 1.0f / (float)(ix * iy);
#pragma unroll
      for (int c = 0; c < 3; ++c) v.c[c] = sum[c] * scale;
      break;
    }
    default: {  // kAreaFrac
      const AreaSpan xs = area_span(ux, d.crop_w, a.W), ys = area_span(dy, d.crop_h, a.H);
      float acc[3] = {0.0f, 0.0f, 0.0f};
      for (int sy = ys.first; sy <= ys.last; ++sy) {
        float buf[3] = {0.0f, 0.0f, 0.0f};
        for (int sx = xs.first; sx <= xs.last; ++sx) {
          const Px p = fetch(a, d, S, sx, sy);
          const float wx = xs.weight(sx);
#pragma unroll
          for (int c = 0; c < 3; ++c) buf[c] = buf[c] + p.c[c] * wx;
        }
        const float wy = ys.weight(sy);
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = sy == ys.first ? wy * buf[c] : acc[c] + wy * buf[c];
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) v.c[c] = acc[c];
      break;
    }
  }
  const long long hw = (long long)a.H * a.W;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    a.dst[((long long)frame * 3 + c) * hw + (long long)dy * a.W + dx] = (v.c[c] / 255.0f - a.mean[c]) / a.stdv[c];
}

// the kernel's mode of a validated descriptor: OpenCV's dispatch of cv::resize(CV_32FC3) on the crop
int kernel_mode(const vy_train_aug& d, int H, int W) {
  if (d.crop_h == H && d.crop_w == W) return kNearest;  // cv::resize to the same size is a copy
  if (d.interp != 3) return d.interp;
  const double sx = (double)d.crop_w / W, sy = (double)d.crop_h / H;
  if (sx >= 1.0 && sy >= 1.0) {
    const int ix = (int)nearbyint(sx), iy = (int)nearbyint(sy);
    const bool whole = fabs(sx - ix) < 2.220446049250313e-16 && fabs(sy - iy) < 2.220446049250313e-16;
    return whole ? kAreaInt : kAreaFrac;
  }
  return kAreaLinear;
}

// what is wrong with a descriptor, or null
const char* invalid(const vy_train_aug& d) {
  if (d.src_offset < 0) return "negative source offset";
  if (d.src_h < 1 || d.src_w < 1 || d.canvas_h < 1 || d.canvas_w < 1 || d.crop_h < 1 || d.crop_w < 1) return "a size below 1";
  if (d.paste_x < 0 || d.paste_y < 0 || (long long)d.paste_x + d.src_w > d.canvas_w ||
      (long long)d.paste_y + d.src_h > d.canvas_h)
    return "the paste leaves the canvas";
  if (d.crop_x < 0 || d.crop_y < 0 || (long long)d.crop_x + d.crop_w > d.canvas_w ||
      (long long)d.crop_y + d.crop_h > d.canvas_h)
    return "the crop leaves the canvas";
  if (d.interp < 0 || d.interp > 4) return "interp outside 0..4";
  if (d.num_ops < 0 || d.num_ops > VY_AUG_MAX_OPS) return "bad op count";
  for (int j = 0; j < d.num_ops; ++j)
    if (d.op[j] < VY_AUG_BRIGHTNESS || d.op[j] > VY_AUG_HUE) return "unknown op code";
  return nullptr;
}

// what is wrong with a mix descriptor beside its (valid) vy_train_aug, or null
const char* invalid(const vy_train_aug& d, const vy_train_mix& m) {
  if (m.h1 < 1 || m.w1 < 1 || m.h2 < 1 || m.w2 < 1) return "a source extent below 1";
  if (m.src2_offset < -1) return "negative second source offset";
  if (!(m.l1 >= 0.0f && m.l1 <= 1.0f) || !(m.l2 >= 0.0f && m.l2 <= 1.0f)) return "a mix ratio outside [0, 1]";
  if (m.src2_offset < 0) {
    if (d.src_h != m.h1 || d.src_w != m.w1) return "src_h x src_w is not the first source's extent (no second source)";
  } else if (d.src_h != std::max(m.h1, m.h2) || d.src_w != std::max(m.w1, m.w2)) {
    return "src_h x src_w is not the larger of the two extents";
  }
  return nullptr;
}

// the launches of a validated batch, CHUNK samples each (mixes is null for the plain launch)
template <class Args, int CHUNK>
int launch_chunks(const uint8_t* frames, const vy_train_aug* augs, const vy_train_mix* mixes, int batch, int k, float* out,
                  int height, int width, const float* fill3, const float* mean3, const float* std3, void* stream) {
  Args a;
  a.src = frames;
  a.k = k;
  a.H = height;
  a.W = width;
  for (int c = 0; c < 3; ++c) {
    a.fill[c] = fill3[c];
    a.mean[c] = mean3[c];
    a.stdv[c] = std3[c];
  }
  const long long per_sample = (long long)k * 3 * height * width;
  for (int i0 = 0; i0 < batch; i0 += CHUNK) {
    a.n = std::min(batch - i0, CHUNK);
    a.dst = out + (long long)i0 * per_sample;
    for (int i = 0; i < a.n; ++i) {
      a.d[i] = augs[i0 + i];
      a.d[i].interp = kernel_mode(augs[i0 + i], height, width);
      if constexpr (std::is_same<Args, MixArgs>::value) a.m[i] = mixes[i0 + i];
    }
    for (int i = a.n; i < CHUNK; ++i) {
      memset(&a.d[i], 0, sizeof(vy_train_aug));
      if constexpr (std::is_same<Args, MixArgs>::value) memset(&a.m[i], 0, sizeof(vy_train_mix));
    }
    hipLaunchKernelGGL(train_transform_kernel<Args>, dim3((width + 255) / 256, height, a.n * k), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

}  // namespace

extern "C" void vy_math_lanczos4(float x, float* w8) { vy_lanczos4_weights(x, w8); }

extern "C" int vy_train_transform(const uint8_t* frames, const vy_train_aug* augs, int32_t batch, int32_t k, float* out,
                                  int32_t height, int32_t width, const float* fill3, const float* mean3,
                                  const float* std3, void* stream) {
  if (!frames || !augs || !out || !fill3 || !mean3 || !std3 || batch < 1 || k < 1 || height < 1 || width < 1)
    return fail(VY_ERR_INVALID, "vy_train_transform: bad argument");
  if (k > 2048) return fail(VY_ERR_INVALID, "vy_train_transform: k above 2048");  // a chunk's frames are the grid's z
  for (int i = 0; i < batch; ++i)
    if (const char* why = invalid(augs[i])) return fail(VY_ERR_INVALID, "vy_train_transform: descriptor %d: %s", i, why);
  return launch_chunks<AugArgs, VY_AUG_CHUNK>(frames, augs, nullptr, batch, k, out, height, width, fill3, mean3, std3,
                                                     stream);
}

extern "C" int vy_train_transform_mix(const uint8_t* frames, const vy_train_aug* augs, const vy_train_mix* mixes,
                                      int32_t batch, int32_t k, float* out, int32_t height, int32_t width,
                                      const float* fill3, const float* mean3, const float* std3, void* stream) {
  if (!frames || !augs || !mixes || !out || !fill3 || !mean3 || !std3 || batch < 1 || k < 1 || height < 1 || width < 1)
    return fail(VY_ERR_INVALID, "vy_train_transform_mix: bad argument");
  for (int i = 0; i < batch; ++i) {
    const char* why = invalid(augs[i]);
    if (!why) why = invalid(augs[i], mixes[i]);
    if (why) return fail(VY_ERR_INVALID, "vy_train_transform_mix: descriptor %d: %s", i, why);
  }
  if (k > 2048) return fail(VY_ERR_INVALID, "vy_train_transform_mix: k above 2048");  // a chunk's frames are the grid's z
  return launch_chunks<MixArgs, VY_MIX_CHUNK>(frames, augs, mixes, batch, k, out, height, width, fill3, mean3, std3,
                                                    stream);
}
