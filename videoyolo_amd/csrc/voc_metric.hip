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

}  // namespace

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
