// coco_metric.hip — the matching step of the COCO detection metric (the reference's metrics/mscoco.py hands it to
// pycocotools' COCOeval.evaluateImg, iouType 'bbox'; [UPSTREAM-RECALLED]) for a batch of images, one launch per
// VY_COCO_CHUNK images.  videoyolo_amd/metrics.py states the rule (coco_match_host) and is what the tests hold this kernel
// to, value for value.
//
// One 256-thread workgroup per image, three steps with a barrier between them:
//   0. score and category of every row of the image go to LDS.
//   1. ranks: a lane owns a row (block-stride loop above 256 rows) and counts, against every row in LDS (every lane the
//      same address: a broadcast read), the kept rows that come before it in the stable descending score order — all of
//      them for its position, those of its own category for its rank.  rows^2 comparisons, no sort.  order[position] = row
//      goes to LDS; a row whose rank reaches max_det is marked there and takes no part in the matching.
//   2. chains: in every (area range, IoU threshold) pair the image's detections claim its ground truths in score order;
//      that chain is sequential and every pair's chain is independent of every other's, as are the chains of different
//      categories.  A lane owns one (range, threshold) chain — 40 at COCO's defaults — and the lanes left over take the
//      same chains for other categories: lane / chains owns the categories c % (256 / chains).  The lane walks the rows in
//      score order and, for a row of category c, the image's ground truths of category c twice, the ones not ignored in
//      its range first, then the ignored ones; the second walk is skipped when the first found a match (COCOeval sorts the
//      ignored ones last and breaks at the first of them).  The IoU is recomputed per pair in float64 rather than stored.
//      "Taken" is one byte per (ground truth of the batch, chain) in the caller's scratch; a lane clears the bytes it will
//      read before it starts, so the scratch needs no preparation and there is no limit on ground truths per image.
// Outputs are in input row order.  Plain vector stores, no atomics.  LDS: 16 bytes per row, 16 KiB at VY_COCO_ROWS_MAX.
//
// The per-image offsets travel in the kernel arguments like vy_vid_match's: no device memory of the library's, no copy, no
// synchronisation.
//
// Arithmetic: float64 in metrics.py's operation order; built with -ffp-contract=off, and the float64 divide is correctly
// rounded, so every IoU equals numpy's.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "vy_support.h"

namespace {

struct CocoImage {
  long long gt0, taken0;  // first ground-truth row of the image (dataset table), first taken row (batch-local)
  int gt_n, pad;
};

struct CocoArgs {
  const double* det_xywh;
  const int32_t* det_cat;
  const double* det_score;
  const double* gt_xywh;
  const int32_t* gt_cat;
  const double* gt_area;
  const uint8_t* gt_crowd;
  const int64_t* gt_id;
  uint8_t* taken;
  int32_t* rank;
  uint8_t* flags;
  double thr[VY_COCO_MAX_THRS];
  double a_lo[VY_COCO_MAX_RANGES], a_hi[VY_COCO_MAX_RANGES];
  long long det0;  // first detection row of the chunk's first image
  int rows, n_thr, n_area, max_det;
  CocoImage im[VY_COCO_CHUNK];
};
static_assert(sizeof(CocoArgs) <= 4096, "the image table must fit the kernel argument segment");

__global__ __launch_bounds__(256) void coco_match_kernel(const CocoArgs a) {
  __shared__ double s_score[VY_COCO_ROWS_MAX];
  __shared__ int32_t s_cat[VY_COCO_ROWS_MAX];
  __shared__ int32_t s_order[VY_COCO_ROWS_MAX];
  const CocoImage im = a.im[blockIdx.x];
  const int rows = a.rows, T = a.n_thr, C = a.n_area * a.n_thr;
  const long long d0 = a.det0 + (long long)blockIdx.x * rows;

  for (int r = threadIdx.x; r < rows; r += 256) {
    s_score[r] = a.det_score[d0 + r];
    s_cat[r] = a.det_cat[d0 + r];
    s_order[r] = -1;
  }
  __syncthreads();

  // ranks: argsort(-score, kind='mergesort') over the kept rows — descending, a NaN last, equal scores in row order
  for (int r = threadIdx.x; r < rows; r += 256) {
    const int c = s_cat[r];
    int rank = -1;
    if (c >= 0) {
      const double s = s_score[r];
      const bool nan = s != s;
      int pos = 0;
      rank = 0;
      for (int j = 0; j < rows; ++j) {
        const int cj = s_cat[j];
        const double sj = s_score[j];
        const bool before = cj >= 0 && (sj != sj ? (nan && j < r) : (nan || sj > s || (sj == s && j < r)));
        pos += before ? 1 : 0;
        rank += (before && cj == c) ? 1 : 0;
      }
      s_order[pos] = rank < a.max_det ? r : -1;
      if (rank >= a.max_det) rank = -1;
    }
    a.rank[d0 + r] = rank;
    if (rank < 0) {  // no chain visits this row
      uint8_t* const f = a.flags + (d0 + r) * C;
      for (int q = 0; q < C; ++q) f[q] = 0;
    }
  }
  __syncthreads();

  const int groups = 256 / C;  // C <= 128: at least two
  const int group = threadIdx.x / C, chain = threadIdx.x - group * C;
  if (group >= groups) return;
  const int ai = chain / T, ti = chain - ai * T;
  const double lo = a.a_lo[ai], hi = a.a_hi[ai];
  const double start = fmin(a.thr[ti], 1.0 - 1e-10);
  uint8_t* const taken = a.taken + im.taken0 * C + chain;  // taken[k * C]: ground truth k taken in this chain
  const int32_t* const gcat = a.gt_cat + im.gt0;
  for (int k = 0; k < im.gt_n; ++k) {
    const int c = gcat[k];
    if (c >= 0 && c % groups == group) taken[(long long)k * C] = 0;
  }

  for (int p = 0; p < rows; ++p) {
    const int r = s_order[p];
    if (r < 0) continue;
    const int c = s_cat[r];
    if (c % groups != group) continue;
    const long long d = d0 + r;
    const double dx = a.det_xywh[d * 4], dy = a.det_xywh[d * 4 + 1], dw = a.det_xywh[d * 4 + 2], dh = a.det_xywh[d * 4 + 3];
    const double da = dw * dh;
    double best = start;
    int m = -1;
    bool m_ig = false;
    for (int pass = 0; pass < 2 && m < 0; ++pass) {
      for (int k = 0; k < im.gt_n; ++k) {
        if (gcat[k] != c) continue;
        const long long g = im.gt0 + k;
        const bool crowd = a.gt_crowd[g] != 0;
        const double area = a.gt_area[g];
        const bool ig = crowd || area < lo || area > hi;
        if (ig != (pass == 1)) continue;
        if (taken[(long long)k * C] && !crowd) continue;
        const double gx = a.gt_xywh[g * 4], gy = a.gt_xywh[g * 4 + 1], gw = a.gt_xywh[g * 4 + 2], gh = a.gt_xywh[g * 4 + 3];
        double w = fmin(dx + dw, gx + gw) - fmax(dx, gx);
        double h = fmin(dy + dh, gy + gh) - fmax(dy, gy);
        if (w <= 0.0) w = 0.0;
        if (h <= 0.0) h = 0.0;
        const double inter = w * h;
        const double uni = crowd ? da : (da + gw * gh) - inter;
        const double iou = inter / uni;
        if (iou < best) continue;
        best = iou;
        m = k;
        m_ig = ig;
      }
    }
    bool matched = false, dig = false;
    if (m >= 0) {
      dig = m_ig;
      matched = a.gt_id[im.gt0 + m] != 0;  // COCOeval reads "matched" off the annotation's id: id 0 counts as none
      taken[(long long)m * C] = 1;
    }
    if (!matched && (da < lo || da > hi)) dig = true;
    a.flags[d * C + chain] = (uint8_t)((matched ? 1 : 0) | (dig ? 2 : 0));
  }
}

}  // namespace

extern "C" int vy_coco_match(int32_t batch, int32_t rows, const double* det_xywh, const int32_t* det_cat,
                             const double* det_score, const int32_t* gt_image, int32_t n_images, const int64_t* gt_off,
                             const double* gt_xywh, const int32_t* gt_cat, const double* gt_area, const uint8_t* gt_crowd,
                             const int64_t* gt_id, int32_t n_thr, const double* iou_thrs, int32_t n_area,
                             const double* area_ranges, int32_t max_det, uint8_t* taken, int64_t taken_bytes,
                             int32_t* rank, uint8_t* flags, void* stream) {
  if (!det_xywh || !det_cat || !det_score || !gt_image || !gt_off || !gt_xywh || !gt_cat || !gt_area || !gt_crowd ||
      !gt_id || !iou_thrs || !area_ranges || !rank || !flags)
    return fail(VY_ERR_INVALID, "vy_coco_match: null pointer");
  if (batch < 0 || rows < 0 || n_images < 0 || max_det < 0 || taken_bytes < 0)
    return fail(VY_ERR_INVALID, "vy_coco_match: negative count");
  if (rows > VY_COCO_ROWS_MAX)
    return fail(VY_ERR_INVALID, "vy_coco_match: %d rows per image, above VY_COCO_ROWS_MAX = %d", rows, VY_COCO_ROWS_MAX);
  if (n_thr < 1 || n_thr > VY_COCO_MAX_THRS || n_area < 1 || n_area > VY_COCO_MAX_RANGES)
    return fail(VY_ERR_INVALID, "vy_coco_match: between 1 and %d IoU thresholds and 1 and %d area ranges",
                VY_COCO_MAX_THRS, VY_COCO_MAX_RANGES);
  for (int i = 0; i < n_thr; ++i)
    if (!std::isfinite(iou_thrs[i])) return fail(VY_ERR_INVALID, "vy_coco_match: IoU threshold %d is not finite", i);
  for (int i = 0; i < n_area; ++i)
    if (!(area_ranges[2 * i] <= area_ranges[2 * i + 1]))
      return fail(VY_ERR_INVALID, "vy_coco_match: area range %d: lo > hi", i);
  const int C = n_thr * n_area;
  long long taken_rows = 0;
  for (int i = 0; i < batch; ++i) {
    const int r = gt_image[i];
    if (r < 0 || r >= n_images)
      return fail(VY_ERR_INVALID, "vy_coco_match: image %d: ground-truth row %d outside [0, %d)", i, r, n_images);
    if (gt_off[r] < 0 || gt_off[r + 1] < gt_off[r] || gt_off[r + 1] > gt_off[n_images] ||
        gt_off[r + 1] - gt_off[r] > INT32_MAX)
      return fail(VY_ERR_INVALID, "vy_coco_match: ground-truth offsets do not ascend at row %d", r);
    taken_rows += gt_off[r + 1] - gt_off[r];
  }
  if (taken_rows * C > taken_bytes || (taken_rows > 0 && !taken))
    return fail(VY_ERR_INVALID, "vy_coco_match: %lld taken bytes needed, %lld given", taken_rows * C,
                (long long)taken_bytes);
  if (batch == 0 || rows == 0) return VY_OK;

  CocoArgs a;
  memset(&a, 0, sizeof(a));
  a.det_xywh = det_xywh, a.det_cat = det_cat, a.det_score = det_score;
  a.gt_xywh = gt_xywh, a.gt_cat = gt_cat, a.gt_area = gt_area, a.gt_crowd = gt_crowd, a.gt_id = gt_id;
  a.taken = taken, a.rank = rank, a.flags = flags;
  for (int i = 0; i < n_thr; ++i) a.thr[i] = iou_thrs[i];
  for (int i = 0; i < n_area; ++i) a.a_lo[i] = area_ranges[2 * i], a.a_hi[i] = area_ranges[2 * i + 1];
  a.rows = rows, a.n_thr = n_thr, a.n_area = n_area, a.max_det = max_det;
  long long taken0 = 0;
  for (int i0 = 0; i0 < batch; i0 += VY_COCO_CHUNK) {
    const int n = std::min(batch - i0, (int)VY_COCO_CHUNK);
    a.det0 = (long long)i0 * rows;
    for (int i = 0; i < VY_COCO_CHUNK; ++i) {
      CocoImage& im = a.im[i];
      im.gt0 = im.taken0 = 0, im.gt_n = im.pad = 0;
      if (i >= n) continue;
      const int r = gt_image[i0 + i];
      im.gt0 = gt_off[r], im.gt_n = (int)(gt_off[r + 1] - gt_off[r]);
      im.taken0 = taken0;
      taken0 += im.gt_n;
    }
    hipLaunchKernelGGL(coco_match_kernel, dim3(n), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    HIP_TRY(hipGetLastError());
  }
  return VY_OK;
}
