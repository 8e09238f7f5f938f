// vid_metric.hip — the matching step of the ImageNet-VID motion / area mAP (the reference's metrics/imgnetvid.py
// vid_eval_motion, :191-276) for a batch of frames in one launch per VY_VID_CHUNK frames.  videoyolo_amd/metrics.py
// states the rule (vid_match_host) and is what the tests hold this kernel to, value for value.
//
// A frame's detections claim ground truths greedily in score order, separately in every (motion range, area range) slice:
// that chain is sequential, and every (frame, slice) pair is independent of every other.  One lane walks one chain.  The
// slice is the fastest lane index, so the lanes of a frame read the same detection and ground-truth rows (one fetch,
// broadcast) and write adjacent outputs: tp and fp are [det][slice].  The IoU is recomputed per pair — a dozen float64
// operations — rather than stored.  The detected flags are the caller's scratch, one byte per (ground truth of the batch,
// slice); a lane clears its own before it starts, so the scratch needs no preparation and no limit on ground truths per
// frame exists.  No LDS, no atomics, no cross-lane traffic.
//
// The per-frame offsets travel in the kernel arguments like vy_train_aug (augment.hip): no device memory of the library's,
// no copy, no synchronisation.
//
// Arithmetic: float64, the operation order of metrics.py; built with -ffp-contract=off, and the float64 divide is
// correctly rounded, so every value equals numpy's.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "vy_support.h"

namespace {

struct VidFrame {
  long long det0, gt0, flag0;  // first detection row, first ground-truth row, first flag row (batch-local)
  int det_n, gt_n, row, pad;   // row: the frame's row of gt_nig
};

struct VidArgs {
  const double* det_box;
  const int32_t* det_label;
  const double* det_score;
  const double* gt_box;
  const int32_t* gt_label;
  const double* gt_thr;
  const double* gt_motion;
  const int32_t* gt_nig;
  uint8_t* flags;
  uint8_t* tp;
  double* fp;
  double conf;
  double m_lo[VY_VID_MAX_RANGES], m_hi[VY_VID_MAX_RANGES], a_lo[VY_VID_MAX_RANGES], a_hi[VY_VID_MAX_RANGES];
  double empty_weight[VY_VID_MAX_RANGES];
  int n_motion, n_area, n_frames, pad;
  VidFrame f[VY_VID_CHUNK];
};
static_assert(sizeof(VidArgs) <= 4096, "the frame table must fit the kernel argument segment");

__global__ __launch_bounds__(256) void vid_match_kernel(const VidArgs a) {
  const int S = a.n_motion * a.n_area;
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int frame = t / S, slice = t - frame * S;
  if (frame >= a.n_frames) return;
  const VidFrame fr = a.f[frame];
  const int mi = slice / a.n_area, ai = slice - mi * a.n_area;
  const double m0 = a.m_lo[mi], m1 = a.m_hi[mi], a0 = a.a_lo[ai], a1 = a.a_hi[ai];
  uint8_t* const flag = a.flags + fr.flag0 * S + slice;  // flag[k * S]: ground truth k detected in this slice
  for (int k = 0; k < fr.gt_n; ++k) flag[(long long)k * S] = 0;
  // a miss that overlaps nothing more in range than out of range: the frame's share of out-of-range ground truths
  const double miss = fr.gt_n == 0 ? a.empty_weight[mi] : (double)a.gt_nig[(long long)fr.row * a.n_motion + mi] / (double)fr.gt_n;
  for (int j = 0; j < fr.det_n; ++j) {
    const long long d = fr.det0 + j;
    const int label = a.det_label[d];
    uint8_t tp = 0;
    double fp = 0.0;
    if (label >= 0 && a.det_score[d] >= a.conf) {
      const double b0 = a.det_box[d * 4], b1 = a.det_box[d * 4 + 1], b2 = a.det_box[d * 4 + 2], b3 = a.det_box[d * 4 + 3];
      const double bb_area = (b3 - b1 + 1.0) * (b2 - b0 + 1.0);
      double ovmax = -1.0, ovmax_ig = -1.0, ovmax_nig = -1.0;
      int kmax = -1;
      bool kmax_in = false;
      for (int k = 0; k < fr.gt_n; ++k) {
        const long long g = fr.gt0 + k;
        const double g0 = a.gt_box[g * 4], g1 = a.gt_box[g * 4 + 1], g2 = a.gt_box[g * 4 + 2], g3 = a.gt_box[g * 4 + 3];
        const double iw = fmin(b2, g2) - fmax(b0, g0) + 1.0, ih = fmin(b3, g3) - fmax(b1, g1) + 1.0;
        const double gt_area = (g2 - g0 + 1.0) * (g3 - g1 + 1.0);
        double ov = 0.0;
        if (iw > 0.0 && ih > 0.0) {
          const double ua = (b2 - b0 + 1.0) * (b3 - b1 + 1.0) + gt_area - iw * ih;
          ov = iw * ih / ua;
        }
        const double mo = a.gt_motion[g];
        const bool ig_motion = mo < m0 || mo > m1;
        if (ov >= a.gt_thr[g] && ov > ovmax && !flag[(long long)k * S] && label == a.gt_label[g]) {
          ovmax = ov;
          kmax = k;
          kmax_in = !ig_motion && !(gt_area < a0 || gt_area > a1);
        }
        if (ig_motion) {
          if (ov > ovmax_ig) ovmax_ig = ov;
        } else {
          if (ov > ovmax_nig) ovmax_nig = ov;
        }
      }
      if (kmax >= 0) {
        flag[(long long)kmax * S] = 1;
        tp = kmax_in ? 1 : 0;
      } else if (bb_area < a0 || bb_area > a1) {
        fp = 0.0;
      } else if (ovmax_nig > ovmax_ig) {
        fp = 1.0;
      } else if (ovmax_ig > ovmax_nig) {
        fp = 0.0;
      } else {
        fp = miss;
      }
    }
    a.tp[d * S + slice] = tp;
    a.fp[d * S + slice] = fp;
  }
}

}  // namespace

extern "C" int vy_vid_match(int32_t n_frames, const int64_t* det_off, const double* det_box, const int32_t* det_label,
                            const double* det_score, double conf_thresh, const int32_t* gt_frame, int32_t n_gt_frames,
                            const int64_t* gt_off, const double* gt_box, const int32_t* gt_label, const double* gt_thr,
                            const double* gt_motion, const int32_t* gt_nig, int32_t n_motion, const double* motion_ranges,
                            int32_t n_area, const double* area_ranges, const double* empty_weight, uint8_t* flags,
                            int64_t flags_bytes, uint8_t* tp, double* fp, void* stream) {
  if (!det_off || !det_box || !det_label || !det_score || !gt_frame || !gt_off || !gt_box || !gt_label || !gt_thr ||
      !gt_motion || !gt_nig || !motion_ranges || !area_ranges || !empty_weight || !tp || !fp)
    return fail(VY_ERR_INVALID, "vy_vid_match: null pointer");
  if (n_frames < 0 || n_gt_frames < 0 || flags_bytes < 0) return fail(VY_ERR_INVALID, "vy_vid_match: negative count");
  if (n_motion < 1 || n_motion > VY_VID_MAX_RANGES || n_area < 1 || n_area > VY_VID_MAX_RANGES)
    return fail(VY_ERR_INVALID, "vy_vid_match: between 1 and %d motion and area ranges", VY_VID_MAX_RANGES);
  for (int i = 0; i < n_motion; ++i)
    if (!(motion_ranges[2 * i] <= motion_ranges[2 * i + 1]))
      return fail(VY_ERR_INVALID, "vy_vid_match: motion range %d: lo > hi", i);
  for (int i = 0; i < n_area; ++i)
    if (!(area_ranges[2 * i] <= area_ranges[2 * i + 1])) return fail(VY_ERR_INVALID, "vy_vid_match: area range %d: lo > hi", i);
  if (n_frames == 0) return VY_OK;
  if (det_off[0] < 0) return fail(VY_ERR_INVALID, "vy_vid_match: negative detection offset");
  const int S = n_motion * n_area;
  long long flag_rows = 0;
  for (int i = 0; i < n_frames; ++i) {
    if (det_off[i + 1] < det_off[i] || det_off[i + 1] - det_off[i] > INT32_MAX)
      return fail(VY_ERR_INVALID, "vy_vid_match: detection offsets do not ascend at frame %d", i);
    const int r = gt_frame[i];
    if (r < 0 || r >= n_gt_frames) return fail(VY_ERR_INVALID, "vy_vid_match: frame %d: ground-truth row %d outside [0, %d)", i, r, n_gt_frames);
    if (gt_off[r] < 0 || gt_off[r + 1] < gt_off[r] || gt_off[r + 1] > gt_off[n_gt_frames] || gt_off[r + 1] - gt_off[r] > INT32_MAX)
      return fail(VY_ERR_INVALID, "vy_vid_match: ground-truth offsets do not ascend at row %d", r);
    flag_rows += gt_off[r + 1] - gt_off[r];
  }
  if (flag_rows * S > flags_bytes || (flag_rows > 0 && !flags))
    return fail(VY_ERR_INVALID, "vy_vid_match: %lld flag bytes needed, %lld given", flag_rows * S, (long long)flags_bytes);
  if (det_off[n_frames] == det_off[0]) return VY_OK;

  VidArgs a;
  a.det_box = det_box, a.det_label = det_label, a.det_score = det_score;
  a.gt_box = gt_box, a.gt_label = gt_label, a.gt_thr = gt_thr, a.gt_motion = gt_motion, a.gt_nig = gt_nig;
  a.flags = flags, a.tp = tp, a.fp = fp;
  a.conf = conf_thresh;
  for (int i = 0; i < VY_VID_MAX_RANGES; ++i) {
    a.m_lo[i] = i < n_motion ? motion_ranges[2 * i] : 0.0, a.m_hi[i] = i < n_motion ? motion_ranges[2 * i + 1] : 0.0;
    a.a_lo[i] = i < n_area ? area_ranges[2 * i] : 0.0, a.a_hi[i] = i < n_area ? area_ranges[2 * i + 1] : 0.0;
    a.empty_weight[i] = i < n_motion ? empty_weight[i] : 0.0;
  }
  a.n_motion = n_motion, a.n_area = n_area, a.pad = 0;
  long long flag0 = 0;
  for (int i0 = 0; i0 < n_frames; i0 += VY_VID_CHUNK) {
    a.n_frames = std::min(n_frames - i0, (int)VY_VID_CHUNK);
    for (int i = 0; i < a.n_frames; ++i) {
      const int r = gt_frame[i0 + i];
      VidFrame& f = a.f[i];
      f.det0 = det_off[i0 + i], f.det_n = (int)(det_off[i0 + i + 1] - det_off[i0 + i]);
      f.gt0 = gt_off[r], f.gt_n = (int)(gt_off[r + 1] - gt_off[r]);
      f.flag0 = flag0, f.row = r, f.pad = 0;
      flag0 += f.gt_n;
    }
    for (int i = a.n_frames; i < VY_VID_CHUNK; ++i) memset(&a.f[i], 0, sizeof(VidFrame));
    const int lanes = a.n_frames * S;
    hipLaunchKernelGGL(vid_match_kernel, dim3((lanes + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    HIP_TRY(hipGetLastError());
  }
  return VY_OK;
}
