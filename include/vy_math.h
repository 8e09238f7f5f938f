/*
 * vy_math.h — exactly-reproducible fp32 scalar math shared by the HIP kernels and by
 * host-side code (BN folding, tests).
 *
 * Every function is a fixed sequence of IEEE-754 binary32 operations (add, mul, fma,
 * correctly rounded divide / sqrt, integer bit moves), so it returns bit-identical
 * results on gfx950 (hipcc -ffp-contract=off, correctly rounded divide/sqrt, f32
 * denormals kept) and on an x86 host (gcc -mfma -ffp-contract=off).  Nothing here
 * calls libm's expf/logf, whose results differ between libraries by an ulp or two;
 * that freedom is what would make "bit-exact NMS indices" a matter of luck.
 *
 * Replaces (numerically, to ~1-2 ulp) the mxnet operators the reference calls at
 *   models/definitions/yolo/yolo3.py:172-175  (F.sigmoid, F.exp in YOLOOutputV3)
 *   models/definitions/layers.py:68-69        (BatchNorm eval affine, LeakyReLU(0.1))
 */
#ifndef VY_MATH_H
#define VY_MATH_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define VY_HD __host__ __device__ __forceinline__
#define VY_UNROLL _Pragma("unroll") /* small fixed loops over register arrays: constant indices on the device */
#else
#define VY_HD static inline
#define VY_UNROLL
#endif

VY_HD float vy_bits_to_f32(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}
VY_HD uint32_t vy_f32_to_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

/* exp(x): Cody-Waite reduction by ln2 (two-constant split), degree-6 polynomial in
 * Horner form with explicit fmaf, scale by 2^n through the exponent field.
 * x > 88.5 -> +inf, x < -86 -> 0 (no denormal results; the detector never needs them). */
VY_HD float vy_expf(float x) {
  if (x > 88.5f) return vy_bits_to_f32(0x7f800000u);
  if (!(x >= -86.0f)) return (x != x) ? x : 0.0f;
  const float kLog2e = 1.44269504088896341f;
  const float kLn2Hi = 0.693359375f;
  const float kLn2Lo = -2.12194440e-4f;
  const float kMagic = 12582912.0f; /* 1.5 * 2^23: round-to-nearest-even to integer */
  float t = fmaf(x, kLog2e, kMagic);
  float n = t - kMagic;
  float r = fmaf(n, -kLn2Hi, x);
  r = fmaf(n, -kLn2Lo, r);
  float p = 1.9875691500e-4f;
  p = fmaf(p, r, 1.3981999507e-3f);
  p = fmaf(p, r, 8.3334519073e-3f);
  p = fmaf(p, r, 4.1665795894e-2f);
  p = fmaf(p, r, 1.6666665459e-1f);
  p = fmaf(p, r, 5.0000001201e-1f);
  float r2 = r * r;
  p = fmaf(p, r2, r);
  p = p + 1.0f;
  int32_t ni = (int32_t)n;
  if (ni > 127) { /* only x in (88.03, 88.5]: split the scale so the exponent add cannot wrap */
    p = p * 2.0f;
    ni -= 1;
  }
  uint32_t u = vy_f32_to_bits(p) + ((uint32_t)ni << 23);
  return vy_bits_to_f32(u);
}

/* sigmoid(x) = 1 / (1 + exp(-x))   (mxnet's formula; correctly rounded divide) */
VY_HD float vy_sigmoidf(float x) { return 1.0f / (1.0f + vy_expf(-x)); }

/* log(x) for x > 0 (used by the loss: log1p(exp(-|x|)) is evaluated as vy_logf(1 + e)).
 * Reduction x = m * 2^e with m in [sqrt(1/2), sqrt(2)), then log(m) = 2 atanh(s),
 * s = (m-1)/(m+1), odd polynomial in s. */
VY_HD float vy_logf(float x) {
  if (x != x || x < 0.0f) return vy_bits_to_f32(0x7fc00000u);
  if (x == 0.0f) return vy_bits_to_f32(0xff800000u);
  uint32_t u = vy_f32_to_bits(x);
  if (u >= 0x7f800000u) return x;
  int32_t e = 0;
  if (u < 0x00800000u) { /* denormal: scale up by 2^23 */
    x = x * 8388608.0f;
    u = vy_f32_to_bits(x);
    e = -23;
  }
  e += (int32_t)(u >> 23) - 127;
  uint32_t mant = (u & 0x007fffffu) | 0x3f800000u;
  float m = vy_bits_to_f32(mant);
  if (m > 1.41421356f) {
    m = m * 0.5f;
    e += 1;
  }
  float s = (m - 1.0f) / (m + 1.0f);
  float s2 = s * s;
  /* 2*atanh(s)/s = 2 + 2/3 s^2 + 2/5 s^4 + ... ; |s| <= 0.1716 so the s^16 term is < 1e-13 */
  float p = 0.13333333333f;
  p = fmaf(p, s2, 0.15384615385f);
  p = fmaf(p, s2, 0.18181818182f);
  p = fmaf(p, s2, 0.22222222222f);
  p = fmaf(p, s2, 0.28571428571f);
  p = fmaf(p, s2, 0.4f);
  p = fmaf(p, s2, 0.66666666667f);
  p = fmaf(p, s2, 2.0f);
  float lm = p * s;
  float fe = (float)e;
  float r = fmaf(fe, 0.693359375f, lm);
  r = fmaf(fe, -2.12194440e-4f, r);
  return r;
}

/* LeakyReLU(0.1): mxnet LeakyReLU(act_type='leaky', slope=0.1): x > 0 ? x : slope*x */
/* written as max(x, 0.1 x): the same value for every x (x > 0: x > 0.1 x; x < 0: 0.1 x > x; +-0 and NaN map to
 * themselves) in two instructions instead of three on the device epilogue */
VY_HD float vy_leaky(float x) { return fmaxf(x, 0.1f * x); }

/* BatchNorm (eval) folded into one fma: scale = gamma / sqrt(var + eps),
 * shift = beta - mean*scale.  Both sides (host fold, device fold kernel) use these. */
VY_HD float vy_bn_scale(float gamma, float var, float eps) { return gamma / sqrtf(var + eps); }
VY_HD float vy_bn_shift(float beta, float mean, float scale) { return fmaf(-mean, scale, beta); }

/* The pinned summation order of a forward convolution (oracle/ref_ops.c header): its K = taps x Cin
 * products (Cin counted in 32-channel k-steps, so K = taps * 32 * ceil(Cin / 32)) are summed as S independent fp32 fma
 * chains over S contiguous, equally long runs of k-steps, and the chains are then added in run order starting from +0:
 *     out = (((+0 + P0) + P1) + P2) + P3.
 * S depends on the layer's K only — never on the batch, the tile or the launch — so a frame gives the same bits whatever
 * it is batched with:  K >= 4096 -> 4 (the eight 3x3 cells on 512 channels: the longest chains of the net, on its smallest
 * maps), else 1.
 * Why not one chain everywhere (rounds 1-5): a single chain per output element is serial; one frame's 13x13 / 19x19 maps
 * give the chip 48 / 96 tiles of 64x64 for 256 CUs, each a 144-k-step chain — those launches are latency-bound.  Independent
 * runs can go to different workgroups: one 416x416 frame 1.95 -> 1.62 ms, one 608x608 frame 2.23 -> 1.99 ms.
 * Why not more runs, or runs for K >= 2048 too (measured, same box, profiles/r06_runs_ab.txt): a workgroup that computes
 * all runs of a tile itself — every launch at batch 64 — has to park each finished chain in memory (there are no registers
 * for a second accumulator tile) and read it back; all resident workgroups do that at the same moment, so it costs what
 * moving those bytes at HBM speed costs: 0.03 % of the batch-64 step per (launch x parked chain).  4 / 2 runs for
 * K >= 4096 / 2048: one 416 frame 1.50 ms but the batch-64 step -1.1 %; this rule: -0.7 %; two runs for K >= 4096: -0.35 %
 * (one 416 frame 1.75 ms). */
static inline int vy_conv_k_chunks(long long K) { return K >= 4096 ? 4 : 1; }
/* ... for a conv of `taps` taps over `cch` 32-channel k-steps per tap: the runs must be equally long and a multiple of four
 * k-steps (the kernels' LDS pipeline depth); a shape that is not (none of this net's) is summed as one chain. */
static inline int vy_conv_runs(int taps, int cch) {
  const int T = taps * cch, S = vy_conv_k_chunks((long long)T * 32);
  return (S > 1 && T % (4 * S) == 0) ? S : 1;
}

/* IoU of two corner-format boxes, no +1 offset (mxnet box_nms / box_iou, corner format).
 * Returns 0 when the union is not positive (mxnet: u <= 0 ? 0 : i/u). */
VY_HD float vy_box_iou(float ax1, float ay1, float ax2, float ay2, float bx1, float by1, float bx2,
                       float by2) {
  float iw = fminf(ax2, bx2) - fmaxf(ax1, bx1);
  float ih = fminf(ay2, by2) - fmaxf(ay1, by1);
  if (!(iw > 0.0f) || !(ih > 0.0f)) return 0.0f;
  float inter = iw * ih;
  float aa = (ax2 - ax1) * (ay2 - ay1);
  float ab = (bx2 - bx1) * (by2 - by1);
  float uni = (aa + ab) - inter;
  return (uni <= 0.0f) ? 0.0f : inter / uni;
}

/* The same with the +1 pixel convention (boxes as inclusive pixel ranges): +1 on the overlap's width and height and on
 * both boxes' widths and heights.  [UPSTREAM-RECALLED] box_nms is recalled to use none; vy_semantics.nms_iou_plus_one
 * selects this one.  Operation for operation in fp32: iw = (min - max) + 1, areas (x2 - x1 + 1) * (y2 - y1 + 1),
 * uni = (aa + ab) - inter; 0 without a positive overlap or with uni <= 0. */
VY_HD float vy_box_iou_plus1(float ax1, float ay1, float ax2, float ay2, float bx1, float by1, float bx2,
                             float by2) {
  float iw = (fminf(ax2, bx2) - fmaxf(ax1, bx1)) + 1.0f;
  float ih = (fminf(ay2, by2) - fmaxf(ay1, by1)) + 1.0f;
  if (!(iw > 0.0f) || !(ih > 0.0f)) return 0.0f;
  float inter = iw * ih;
  float aa = ((ax2 - ax1) + 1.0f) * ((ay2 - ay1) + 1.0f);
  float ab = ((bx2 - bx1) + 1.0f) * ((by2 - by1) + 1.0f);
  float uni = (aa + ab) - inter;
  return (uni <= 0.0f) ? 0.0f : inter / uni;
}

/* sin(a), cos(a) for a in [0, pi/4]: Taylor polynomials in Horner form with explicit fmaf (truncation below 2e-10,
 * under half an ulp of the results, which lie in [0, 0.71] and [0.70, 1]). */
VY_HD float vy_sin_q(float a) {
  const float z = a * a;
  float p = 2.7557319224e-6f;      /* 1/9! */
  p = fmaf(p, z, -1.9841269841e-4f); /* -1/7! */
  p = fmaf(p, z, 8.3333333333e-3f);  /* 1/5! */
  p = fmaf(p, z, -1.6666666667e-1f); /* -1/3! */
  return fmaf(a * z, p, a);
}
VY_HD float vy_cos_q(float a) {
  const float z = a * a;
  float p = -2.7557319224e-7f;     /* -1/10! */
  p = fmaf(p, z, 2.4801587302e-5f);  /* 1/8! */
  p = fmaf(p, z, -1.3888888889e-3f); /* -1/6! */
  p = fmaf(p, z, 4.1666666667e-2f);  /* 1/4! */
  p = fmaf(p, z, -0.5f);
  return fmaf(z, p, 1.0f);
}

/* The eight Lanczos-4 weights of the taps s-3 .. s+4 for the fractional source position x in [0, 1): OpenCV's
 * interpolateLanczos4 [UPSTREAM-RECALLED] — x < FLT_EPSILON gives a unit weight at tap 3; otherwise tap i, at distance
 * d = x + 3 - i, gets sin(pi d) sin(pi d / 4) / d^2 up to a factor common to the taps, and the weights are divided by
 * their sum.  sin(pi d) = +-sin(pi x) is that common factor; sin(pi d / 4) is one of +-sin / +-cos of v = x pi/4 and of
 * u = (1 - x) pi/4.  OpenCV forms the numerators in double from ONE sin / cos pair (of -(x + 3) pi/4) through an angle
 * sum; that sum cancels for the taps next to the sample (d -> 0), harmlessly in double and ruinously in fp32, so here
 * each of u and v gets its own polynomial pair and no numerator is a difference. */
VY_HD void vy_lanczos4_weights(float x, float w[8]) {
  /* x >= 1 is the sample one tap further on (position s + 1, x = 0): a source coordinate a hair below an integer
   * rounds to floor + 1.0f in float.  Without this, tap 4 would be 0 / 0. */
  if (x < 1.1920928955e-7f || x >= 1.0f) {
    const int unit = x >= 1.0f ? 4 : 3;
    VY_UNROLL
    for (int i = 0; i < 8; ++i) w[i] = i == unit ? 1.0f : 0.0f;
    return;
  }
  const float kPi4 = 0.78539816339744831f;
  const float v = x * kPi4, u = (1.0f - x) * kPi4;
  const float sv = vy_sin_q(v), cv = vy_cos_q(v), su = vy_sin_q(u), cu = vy_cos_q(u);
  const float num[8] = {-su, cv, -cu, sv, su, -cv, cu, -sv};
  float sum = 0.0f;
  VY_UNROLL
  for (int i = 0; i < 8; ++i) {
    const float d = x + (float)(3 - i);
    w[i] = num[i] / (d * d);
    sum = sum + w[i];
  }
  sum = 1.0f / sum;
  VY_UNROLL
  for (int i = 0; i < 8; ++i) w[i] = w[i] * sum;
}

#endif /* VY_MATH_H */
