// Flickr30k Entities Recall@k on the device (host side: mq_det_amd/evaluation.py FlickrRecallEvaluator).
//
// mq_flickr_recall: Flickr30kEntitiesRecallEvaluator.evaluate's inner loop (flickr_eval.py:362-380 with box_iou :152-202) for every phrase.
// One wave per phrase.  The phrase's predicted boxes are its D detection rows, already in score-descending order, followed by the dummy
// box [0, 0, 0, 0] that flickr_post_process appends (engine/inference.py:333-334): D + 1 list entries, the dummy counts towards k.  Lane l
// owns the entries l, l + 64, ...; the ground truths pass through LDS 64 at a time, so neither side has a cap.  The IoU is in fp64 with
// the reference's operations one by one (no contraction): area = (x2 - x1) * (y2 - y1) without + 1, width and height of the
// intersection clipped at 0 separately, iou = inter / ((area1 + area2) - inter).
// `ious[:k].max() >= thr` needs no maximum: it holds iff some IoU of the first k entries is >= thr and none of them is NaN (numpy's max
// returns NaN as soon as one entry is NaN -- a zero-area ground truth against a zero-area box gives 0 / 0 --, and NaN >= thr is a miss).
// So every lane keeps two bit sets over the k values (an IoU >= thr seen / a NaN seen among the entries below k) and two ballots per k
// finish the phrase: hits[p] bit j = hit at ks[j] (ks[j] = -1: all entries).
//
// mq_flickr_tally: RecallTracker (:220-255) as integers.  One lane per phrase; the implicit category "all" (column 0) is summed over the
// wave with ballots first, the phrase's own categories (CSR cat_off / cat_idx, a category listed twice counts twice like in the
// reference's loop) go straight to integer atomics: positives [NK, C] and totals [C] do not depend on the schedule.
#include "common.h"

MQ_NAMESPACE_BEGIN
#ifdef MQ_PRIMARY_UNIT                                     // fp64 / integer data only: one copy, in the fp16 translation unit

#define FLICKR_MAX_K 30                                    // k values per call: one bit each in hits[p]

// np.maximum / np.minimum: a NaN operand gives NaN (fmax / fmin would drop it)
__device__ __forceinline__ double flickr_max(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }
__device__ __forceinline__ double flickr_min(double a, double b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }

__global__ __launch_bounds__(64) void flickr_recall_kernel(const int* __restrict__ phrase_dt, const int* __restrict__ phrase_gt,
                                                           const float* __restrict__ dt_box, const double* __restrict__ gt_box,
                                                           const int* __restrict__ ks, int NK, const double* __restrict__ iou_thr, int* __restrict__ hits) {
#pragma clang fp contract(off)
  const double thr = iou_thr[0];
  __shared__ double gt_s[64 * 4];
  __shared__ double ga_s[64];
  const int p = blockIdx.x, lane = threadIdx.x;
  const int ds = phrase_dt[2 * p], D = phrase_dt[2 * p + 1], gs = phrase_gt[2 * p], G = phrase_gt[2 * p + 1];
  unsigned ge_bits = 0, nan_bits = 0;
  for (int g0 = 0; g0 < G; g0 += 64) {
    const int gn = min(64, G - g0);
    __syncthreads();                                       // the previous tile is read
    if (lane < gn) {
      const double* gb = gt_box + (long)(gs + g0 + lane) * 4;
      const double x1 = gb[0], y1 = gb[1], x2 = gb[2], y2 = gb[3];
      gt_s[lane * 4] = x1, gt_s[lane * 4 + 1] = y1, gt_s[lane * 4 + 2] = x2, gt_s[lane * 4 + 3] = y2;
      ga_s[lane] = (x2 - x1) * (y2 - y1);
    }
    __syncthreads();
    for (int e = lane; e <= D; e += 64) {                  // entry D is the dummy box
      double x1 = 0, y1 = 0, x2 = 0, y2 = 0;
      if (e < D) {
        const float* db = dt_box + (long)(ds + e) * 4;
        x1 = db[0], y1 = db[1], x2 = db[2], y2 = db[3];
      }
      const double a1 = (x2 - x1) * (y2 - y1);
      bool ge = false, nan = false;
      for (int g = 0; g < gn; ++g) {
        const double lx = flickr_max(x1, gt_s[g * 4]), ly = flickr_max(y1, gt_s[g * 4 + 1]);
        const double rx = flickr_min(x2, gt_s[g * 4 + 2]), ry = flickr_min(y2, gt_s[g * 4 + 3]);
        double w = rx - lx, h = ry - ly;
        w = w < 0 ? 0 : w;                                 // clip(min = 0)
        h = h < 0 ? 0 : h;
        const double inter = w * h;
        const double uni = a1 + ga_s[g] - inter;
        const double iou = inter / uni;
        ge |= iou >= thr;
        nan |= iou != iou;
      }
      for (int j = 0; j < NK; ++j) {
        const int k = ks[j];
        if (k < 0 || e < k) {
          ge_bits |= (unsigned)ge << j;
          nan_bits |= (unsigned)nan << j;
        }
      }
    }
  }
  int out = 0;
  for (int j = 0; j < NK; ++j) {
    const unsigned long long bg = __ballot(ge_bits >> j & 1), bn = __ballot(nan_bits >> j & 1);
    if (bg != 0 && bn == 0) out |= 1 << j;
  }
  if (lane == 0) hits[p] = out;
}

__global__ __launch_bounds__(256) void flickr_tally_kernel(const int* __restrict__ hits, const int* __restrict__ cat_off,
                                                           const int* __restrict__ cat_idx, unsigned long long* __restrict__ positives,
                                                           unsigned long long* __restrict__ totals, int P, int NK, int C) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = p < P;
  const int lane = threadIdx.x & 63;
  const int h = live ? hits[p] : 0;
  const int nlive = __popcll(__ballot(live));
  if (lane == 0 && nlive) atomicAdd(totals, (unsigned long long)nlive);
  for (int j = 0; j < NK; ++j) {
    const int n = __popcll(__ballot(live && (h >> j & 1)));
    if (lane == 0 && n) atomicAdd(positives + (long)j * C, (unsigned long long)n);
  }
  if (!live) return;
  for (int i = cat_off[p]; i < cat_off[p + 1]; ++i) {
    const int c = cat_idx[i];
    if (c < 0 || c >= C) continue;                         // (the host wrapper checks the table; never an out-of-bounds atomic)
    atomicAdd(totals + c, 1ull);
    for (int j = 0; j < NK; ++j)
      if (h >> j & 1) atomicAdd(positives + (long)j * C + c, 1ull);
  }
}

extern "C" int mq_flickr_recall(const int* phrase_dt, const int* phrase_gt, const float* dt_box, const double* gt_box, const int* ks,
                                const double* iou_thr, int* hits, int P, int NK, void* stream) {
  if (NK < 1 || NK > FLICKR_MAX_K) return -1;
  if (P <= 0) return 0;
  return mq_launch<flickr_recall_kernel>(dim3(P), dim3(64), 0, (hipStream_t)stream, phrase_dt, phrase_gt, dt_box, gt_box, ks, NK, iou_thr, hits);
}

extern "C" int mq_flickr_tally(const int* hits, const int* cat_off, const int* cat_idx, unsigned long long* positives,
                               unsigned long long* totals, int P, int NK, int C, void* stream) {
  if (NK < 1 || NK > FLICKR_MAX_K || C < 1) return -1;
  if (P <= 0) return 0;
  return mq_launch<flickr_tally_kernel>(dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, hits, cat_off, cat_idx, positives, totals,
                                        P, NK, C);
}

#endif
MQ_NAMESPACE_END
