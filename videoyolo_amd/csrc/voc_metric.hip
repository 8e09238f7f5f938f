// voc_metric.hip — the matching step of the PASCAL-VOC mAP (the reference's metrics/pascalvoc.py VOCMApMetric.update,
// :84-170) for a batch of images in one launch.  videoyolo_amd/metrics.py states the rule (voc_match_host) and is what the
// tests hold this kernel to, value for value.
//
// Unlike the ImageNet-VID rule (vid_metric.hip) this one has no sequential chain: a detection's candidate ground truth is
// the argmax of its IoU over the ground truths of its class, whether or not an earlier detection took it.  "Taken" is then
// one question — does a detection of the same image with the same candidate come earlier in score order — which needs no
// sort.  One 256-thread workgroup per image, two phases around one barrier:
//   1. candidates: a lane owns a detection row (block-stride loop above 256 rows) and walks the image's ground truths;
//      every lane reads the same ground-truth row, so the fetch is uniform.  Score and candidate go to LDS.
//   2. claims: the lane scans the image's rows in LDS (every lane the same address: a broadcast read) for one with its
//      candidate that comes before it.  rows^2 comparisons per image, 10^4 at the detector's 100 rows.
// Outputs are in input row order: no sort, no gather, no atomics, no limit on ground truths.  LDS: 8 bytes per row,
// 8 KiB at VY_VOC_ROWS_MAX.
//
// Arithmetic: fp32 in pairwise_iou's operation order; built with -ffp-contract=off and the correctly rounded divide
// (include/vy_math.h), so every IoU equals numpy's float32 value, NaN and signed zero included.
//
// Further down: frame_ap_kernel (vy_voc_frame_ap), the per-frame mean AP computed from these flags.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/vyolo.h"
#include "vy_support.h"

namespace {

struct VocRow {
  float score;
  int best;
};

// np.maximum / np.minimum: a NaN on either side gives NaN
__device__ __forceinline__ float np_max(float a, float b) { return (a >= b || a != a) ? a : b; }
__device__ __forceinline__ float np_min(float a, float b) { return (a <= b || a != a) ? a : b; }

__global__ __launch_bounds__(256) void voc_match_kernel(int rows, int n_gt, const float* __restrict__ det_box,
                                                        const float* __restrict__ det_label,
                                                        const float* __restrict__ det_score,
                                                        const float* __restrict__ gt_box,
                                                        const int32_t* __restrict__ gt_label,
                                                        const uint8_t* __restrict__ gt_difficult, float iou_thresh,
                                                        int32_t* __restrict__ best_out, int8_t* __restrict__ flags) {
  __shared__ VocRow row[VY_VOC_ROWS_MAX];
  const long long d0 = (long long)blockIdx.x * rows, g0 = (long long)blockIdx.x * n_gt;
  const float* const gb = gt_box + g0 * 4;
  const int32_t* const gl = gt_label + g0;

  for (int r = threadIdx.x; r < rows; r += 256) {
    const float lab = det_label[d0 + r];
    int best = -1;
    if (lab >= 0.0f) {
      const int label = (int)lab;
      const float a0 = det_box[(d0 + r) * 4], a1 = det_box[(d0 + r) * 4 + 1], a2 = det_box[(d0 + r) * 4 + 2],
                  a3 = det_box[(d0 + r) * 4 + 3];
      const float area_a = (a2 - a0) * (a3 - a1);
      float top = 0.0f;
      for (int g = 0; g < n_gt; ++g) {
        if (gl[g] != label) continue;
        const float b0 = gb[g * 4LL], b1 = gb[g * 4LL + 1], b2 = gb[g * 4LL + 2], b3 = gb[g * 4LL + 3];
        const float lx = np_max(a0, b0), ly = np_max(a1, b1), hx = np_min(a2, b2), hy = np_min(a3, b3);
        const float inter = ((hx - lx) * (hy - ly)) * ((lx < hx && ly < hy) ? 1.0f : 0.0f);
        const float area_b = (b2 - b0) * (b3 - b1);
        const float iou = inter / ((area_a + area_b) - inter);
        // np.argmax: the first index of the largest value, a NaN being the largest
        if (best < 0 || iou > top || (iou != iou && top == top)) {
          top = iou;
          best = g;
        }
      }
      if (top < iou_thresh) best = -1;  // false for a NaN maximum: it keeps its match
    }
    row[r].score = det_score[d0 + r];
    row[r].best = best;
    best_out[d0 + r] = best;
    if (!(lab >= 0.0f)) flags[d0 + r] = -2;
  }
  __syncthreads();

  for (int r = threadIdx.x; r < rows; r += 256) {
    if (!(det_label[d0 + r] >= 0.0f)) continue;
    const VocRow me = row[r];
    int8_t flag = 0;
    if (me.best >= 0) {
      if (gt_difficult && gt_difficult[g0 + me.best]) {
        flag = -1;
      } else {
        bool taken = false;
        for (int j = 0; j < rows; ++j) {
          const VocRow o = row[j];
          taken |= o.best == me.best && (o.score > me.score || (o.score == me.score && j < r));
        }
        flag = taken ? 0 : 1;
      }
    }
    flags[d0 + r] = flag;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// frame_ap_kernel — the mean AP of every image on its own (the reference's detect_yolo3.py:451-534: reset / update with one
// frame / get, per frame), from the flags above.  videoyolo_amd/metrics.py states the rule (frame_map_host).
//
// A class's curve needs its rows in score order; a row's place in that order is a count, so again nothing is sorted.  One
// 256-thread workgroup per image, a lane owns a row (block-stride loop above 256 rows), three phases around barriers:
//   1. counts: the lane scans the image's rows in LDS (every lane the same address: a broadcast read) for the rows of its
//      class at or ahead of it — a higher score; at equal scores the lower row — and counts their TPs (flag 1) and FPs
//      (flag 0); a uniform walk over the image's ground truths counts npos, the non-difficult ones of its class.
//      prec = tp / (tp + fp) (0 / 0 -> 0) and rec = tp / npos go to LDS.
//   2. envelope: area AP — a TP row scans again for the largest prec of its class at or behind it and contributes
//      (tp / npos - (tp - 1) / npos) * that, the two quotients formed separately as numpy forms them.  11-point AP — the
//      first row of a class in score order scans its class once for the largest prec at rec >= t for each of the eleven
//      t = 0.0 + k * 0.1 and contributes ap = (..((0 + p0 / 11) + p1 / 11).. + p10 / 11), numpy's order.
//   3. the rows' contributions go to LDS and are added in a fixed order: lane t adds rows t, t + 256, ..., then a tree
//      over the 256 lanes.  No floating-point atomics: a frame's value is the same bits on every run and in any batch.
// Meanwhile a lane per ground truth counts the classes that are scored: a ground truth counts when it is not difficult and
// no earlier one of its label is — O(n_gt^2 / 256) label reads per image, every lane the same address, and no limit on
// n_gt.  frame_ap = (sum of contributions) / (that count); NaN when the count is 0.  A class with ground truth and no
// detection adds 0 to the sum and 1 to the count; one with detections and no such ground truth adds nothing to either.
//
// LDS: 25 bytes per row (score 4, class 4, flag 1, prec 8, rec / contribution 8): 25 KiB at VY_VOC_ROWS_MAX.
// Arithmetic: float64 throughout.  The 11-point compare rec >= t needs tp / npos correctly rounded (3 / 10 must be
// 0.3 < 0.30000000000000004): hipcc's default lowering of the f64 divide is correctly rounded, and this file is built
// without fast-math and with -ffp-contract=off.
constexpr int kRowsPerLane = VY_VOC_ROWS_MAX / 256;

__global__ __launch_bounds__(256) void frame_ap_kernel(int rows, int n_gt, const float* __restrict__ det_label,
                                                       const float* __restrict__ det_score,
                                                       const int8_t* __restrict__ flags,
                                                       const int32_t* __restrict__ gt_label,
                                                       const uint8_t* __restrict__ gt_difficult, int use_07,
                                                       double* __restrict__ frame_ap,
                                                       int32_t* __restrict__ frame_classes) {
  __shared__ double prec[VY_VOC_ROWS_MAX];
  __shared__ double aux[VY_VOC_ROWS_MAX];  // rec until the envelope phase is over, then the row's contribution
  __shared__ float score[VY_VOC_ROWS_MAX];
  __shared__ int cls[VY_VOC_ROWS_MAX];     // -1: not a detection
  __shared__ int8_t flag[VY_VOC_ROWS_MAX];
  __shared__ int n_scored;
  const int tid = threadIdx.x;
  const long long d0 = (long long)blockIdx.x * rows, g0 = (long long)blockIdx.x * n_gt;
  const int32_t* const gl = gt_label + g0;
  const uint8_t* const gd = gt_difficult ? gt_difficult + g0 : nullptr;

  if (tid == 0) n_scored = 0;
  for (int r = tid; r < rows; r += 256) {
    const float lab = det_label[d0 + r];
    const int8_t f = flags[d0 + r];
    const bool det = lab >= 0.0f && f != -2;
    score[r] = det_score[d0 + r];
    cls[r] = det ? (int)lab : -1;
    flag[r] = f;
  }
  __syncthreads();

  // the classes that are scored (an integer count: the order of the additions does not matter)
  int firsts = 0;
  for (int g = tid; g < n_gt; g += 256) {
    const int label = gl[g];
    if (label < 0 || (gd && gd[g])) continue;
    bool first = true;
    for (int j = 0; j < g; ++j) first &= !(gl[j] == label && !(gd && gd[j]));
    firsts += first ? 1 : 0;
  }
  if (firsts) atomicAdd(&n_scored, firsts);

  // 1. counts
  int tp_of[kRowsPerLane], npos_of[kRowsPerLane];
  bool leads[kRowsPerLane];
#pragma unroll
  for (int k = 0; k < kRowsPerLane; ++k) {
    const int r = tid + 256 * k;
    tp_of[k] = npos_of[k] = 0;
    leads[k] = false;
    if (r >= rows || cls[r] < 0) continue;
    const int c = cls[r];
    const float s = score[r];
    int tp = 0, fp = 0, ahead = 0;
    for (int j = 0; j < rows; ++j) {
      const float sj = score[j];
      const bool in = cls[j] == c && (sj > s || (sj == s && j <= r));
      const int fj = flag[j];
      ahead += in ? 1 : 0;
      tp += (in && fj == 1) ? 1 : 0;
      fp += (in && fj == 0) ? 1 : 0;
    }
    int npos = 0;
    for (int g = 0; g < n_gt; ++g) npos += (gl[g] == c && !(gd && gd[g])) ? 1 : 0;
    prec[r] = (tp + fp) > 0 ? (double)tp / (double)(tp + fp) : 0.0;
    aux[r] = npos > 0 ? (double)tp / (double)npos : 0.0;
    tp_of[k] = tp;
    npos_of[k] = npos;
    leads[k] = ahead == 1;
  }
  __syncthreads();

  // 2. envelope
  double part[kRowsPerLane];
#pragma unroll
  for (int k = 0; k < kRowsPerLane; ++k) {
    const int r = tid + 256 * k;
    part[k] = 0.0;
    if (r >= rows || cls[r] < 0 || npos_of[k] <= 0) continue;
    const int c = cls[r];
    if (!use_07) {
      if (flag[r] != 1) continue;
      const float s = score[r];
      double top = 0.0;
      for (int j = 0; j < rows; ++j) {
        const float sj = score[j];
        const bool in = cls[j] == c && (sj < s || (sj == s && j >= r));
        const double pj = prec[j];
        top = (in && pj > top) ? pj : top;
      }
      const double np = (double)npos_of[k];
      part[k] = ((double)tp_of[k] / np - (double)(tp_of[k] - 1) / np) * top;
    } else {
      if (!leads[k]) continue;
      double top[11];
#pragma unroll
      for (int t = 0; t < 11; ++t) top[t] = 0.0;
      for (int j = 0; j < rows; ++j) {
        if (cls[j] != c) continue;
        const double pj = prec[j], rj = aux[j];
#pragma unroll
        for (int t = 0; t < 11; ++t) top[t] = (rj >= 0.0 + (double)t * 0.1 && pj > top[t]) ? pj : top[t];
      }
      double ap = 0.0;
#pragma unroll
      for (int t = 0; t < 11; ++t) ap += top[t] / 11.0;
      part[k] = ap;
    }
  }
  __syncthreads();  // every rec has been read: aux now takes the contributions

  // 3. the sum, in a fixed order
  double mine = 0.0;
#pragma unroll
  for (int k = 0; k < kRowsPerLane; ++k) mine += part[k];
  aux[tid] = mine;
  __syncthreads();
  for (int half = 128; half > 0; half >>= 1) {
    if (tid < half) aux[tid] += aux[tid + half];
    __syncthreads();
  }
  if (tid == 0) {
    const int n = n_scored;
    frame_classes[blockIdx.x] = n;
    frame_ap[blockIdx.x] = n > 0 ? aux[0] / (double)n : (double)NAN;
  }
}

}  // namespace

extern "C" int vy_voc_frame_ap(int32_t batch, int32_t rows, int32_t n_gt, const float* det_label, const float* det_score,
                               const int8_t* flags, const int32_t* gt_label, const uint8_t* gt_difficult, int32_t use_07,
                               double* frame_ap, int32_t* frame_classes, void* stream) {
  if (!det_label || !det_score || !flags || !gt_label || !frame_ap || !frame_classes)
    return fail(VY_ERR_INVALID, "vy_voc_frame_ap: null pointer");
  if (batch < 0 || rows < 0 || n_gt < 0) return fail(VY_ERR_INVALID, "vy_voc_frame_ap: negative count");
  if (rows > VY_VOC_ROWS_MAX)
    return fail(VY_ERR_INVALID, "vy_voc_frame_ap: %d rows per image, above VY_VOC_ROWS_MAX = %d", rows, VY_VOC_ROWS_MAX);
  if (batch == 0) return VY_OK;
  // rows == 0 is launched too: an image with ground truth and no row scores 0, one without ground truth NaN
  hipLaunchKernelGGL(frame_ap_kernel, dim3(batch), dim3(256), 0, static_cast<hipStream_t>(stream), rows, n_gt, det_label,
                     det_score, flags, gt_label, gt_difficult, use_07 != 0, frame_ap, frame_classes);
  HIP_TRY(hipGetLastError());
  return VY_OK;
}

extern "C" int vy_voc_match(int32_t batch, int32_t rows, int32_t n_gt, const float* det_box, const float* det_label,
                            const float* det_score, const float* gt_box, const int32_t* gt_label,
                            const uint8_t* gt_difficult, float iou_thresh, int32_t* best, int8_t* flags, void* stream) {
  if (!det_box || !det_label || !det_score || !gt_box || !gt_label || !best || !flags)
    return fail(VY_ERR_INVALID, "vy_voc_match: null pointer");
  if (batch < 0 || rows < 0 || n_gt < 0) return fail(VY_ERR_INVALID, "vy_voc_match: negative count");
  if (rows > VY_VOC_ROWS_MAX)
    return fail(VY_ERR_INVALID, "vy_voc_match: %d rows per image, above VY_VOC_ROWS_MAX = %d", rows, VY_VOC_ROWS_MAX);
  if (!std::isfinite(iou_thresh)) return fail(VY_ERR_INVALID, "vy_voc_match: iou_thresh is not finite");
  if (batch == 0 || rows == 0) return VY_OK;
  hipLaunchKernelGGL(voc_match_kernel, dim3(batch), dim3(256), 0, static_cast<hipStream_t>(stream), rows, n_gt, det_box,
                     det_label, det_score, gt_box, gt_label, gt_difficult, iou_thresh, best, flags);
  HIP_TRY(hipGetLastError());
  return VY_OK;
}
