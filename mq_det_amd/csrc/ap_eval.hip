// AP on the device: LVIS Fixed AP and COCO-style AP (host side: mq_det_amd/evaluation.py LvisFixedAPEvaluator / CocoAPEvaluator).  One match
// kernel and one accumulate kernel; the two protocols are template arguments.
//
// ap_match_kernel<Rules>: LVISEval.evaluate_img (lvis_eval.py:318-410) / pycocotools' COCOeval.evaluateImg (cocoeval.py:236-313) for every
// (image, category) pair, all 4 area ranges x 10 IoU thresholds at once.  One 64-lane workgroup per pair; lane l < 40 owns (area l / 10,
// threshold l % 10) and runs that greedy scan in the reference's order: detections by score (the host sorted them; under COCO it also cut
// the pair to maxDets[-1] = 100), ground truths in annotation-file order, non-ignored ones first.  The IoU is pycocotools' bbIou (maskApi.c)
// in fp64 with the reference's operation order (no contraction).  The per-detection results of the 40 lanes are gathered with two ballots:
// dt_bits[d] = (matched bits, ignored bits), bit = area * 10 + threshold.
//
// Rules: what a protocol sets.
//   crowd    false (LVIS): the per-ground-truth byte is `ignore` -- the ground truth is ignored in every area range, nothing else.
//            true (COCO): the byte is `iscrowd` -- ignored in every area range as well, and its IoU has the detection's area as denominator
//            (bbIou, iscrowd = 1) and it stays available after a match: many detections may take it.  The crowd bit of the flag byte is only
//            ever set under crowd, so both tests fold away in the LVIS instantiation.
//   fast_gt  ground truths per pair on the fast path (below): 512 (LVIS), 256 (COCO).
// The not-exhaustive byte per pair (pair_nel: an unmatched detection of such a pair is ignored) is LVIS's alone; COCO passes null.
//
// Fast path and LDS: a pair with at most fast_gt ground truths keeps its taken flags in LDS (fast_gt / 32 words per lane), the ground truths'
// flags (fast_gt bytes) and the fp64 IoUs of AP_TILE / G detections at a time (16 KB), computed once for the 40 scans.  With 256 that is
// 18.3 KB per one-wave workgroup, 8 workgroups per CU -- the scans are dependent LDS reads, so what hides their latency is the other
// workgroups of the CU, and a larger tile would take them away (COCO pairs have a handful of ground truths and at most 100 detections: one
// tile); with LVIS's 512 it is 20.5 KB, 7 workgroups.  A pair with more ground truths takes the slow path:
// taken flags in the global workspace ws (one byte per lane and ground truth) and every IoU computed where it is read.  The number of
// detections of a pair is not bounded on either path (tiles / a plain loop).  Both paths give the same bits.
//
// ap_accumulate_kernel<NM>: LVISEval.accumulate (:412-523) / COCOeval.accumulate (:315-420) per (category, maxDets slice) workgroup and
// (area, threshold) lane: the category's detections in the reference's order (the host's order[] permutation: score descending, image, rank
// in the pair) -- for NM = 3 (COCO, maxDets {1, 10, 100}) those whose rank in their pair is below the slice's maxDets, for NM = 1 (LVIS,
// max_dets = -1) all of them, no rank read --; tp / fp running sums, pr = tp / (fp + tp + eps), rc = tp / num_gt, the right-to-left precision
// envelope and the 101-point searchsorted lookup.  The envelope is only needed at the lookup points: the forward pass keeps the running
// maximum of pr between consecutive lookup points (LDS), a backward pass over the 101 points folds them into suffix maxima.
#include "common.h"

MQ_NAMESPACE_BEGIN
#ifdef MQ_PRIMARY_UNIT                                     // fp64 / integer data only: one copy, in the fp16 translation unit

#define AP_NT 10                                           // IoU thresholds
#define AP_NA 4                                            // area ranges
#define AP_NR 101                                          // recall thresholds
#define AP_LANES (AP_NT * AP_NA)                           // lanes with a scan of their own
#define AP_TILE 2048                                       // fp64 IoUs staged per tile (16 KB)
#define AP_F_NZ 16                                         // gt flags: bit a = ignored in area range a, then id != 0 and iscrowd
#define AP_F_CROWD 32

struct LvisRules {
  static constexpr bool crowd = false;
  static constexpr int fast_gt = 512;
};
struct CocoRules {
  static constexpr bool crowd = true;
  static constexpr int fast_gt = 256;
};

__device__ __forceinline__ double ap_iou(const float* __restrict__ db, const double* __restrict__ gb, bool crowd) {
#pragma clang fp contract(off)                           // bbIou's operations one by one
  const double dx = db[0], dy = db[1], dw = db[2], dh = db[3];
  const double gx = gb[0], gy = gb[1], gw = gb[2], gh = gb[3];
  const double ga = gw * gh, da = dw * dh;
  const double w = fmin(dw + dx, gw + gx) - fmax(dx, gx);
  if (w <= 0) return 0.0;
  const double h = fmin(dh + dy, gh + gy) - fmax(dy, gy);
  if (h <= 0) return 0.0;
  const double i = w * h;
  const double u = crowd ? da : da + ga - i;
  return i / u;
}

template <class Rules>
__device__ __forceinline__ int ap_gt_flags(const double* __restrict__ gt_area, const unsigned char* __restrict__ gt_ign,
                                           const unsigned char* __restrict__ gt_nz, const double* __restrict__ area_rng, long g) {
  const double ar = gt_area[g];
  const bool ign = gt_ign[g] != 0;                         // LVIS: ignore, COCO: iscrowd
  int f = (gt_nz[g] ? AP_F_NZ : 0) | (Rules::crowd && ign ? AP_F_CROWD : 0);
  for (int a = 0; a < AP_NA; ++a)
    if (ign || ar < area_rng[2 * a] || ar > area_rng[2 * a + 1]) f |= 1 << a;
  return f;
}

template <class Rules>
__global__ __launch_bounds__(64) void ap_match_kernel(const int* __restrict__ pair_dt, const int* __restrict__ pair_gt,
                                                      const unsigned char* __restrict__ pair_nel, const float* __restrict__ dt_box,
                                                      const double* __restrict__ gt_box, const double* __restrict__ gt_area,
                                                      const unsigned char* __restrict__ gt_ign, const unsigned char* __restrict__ gt_nz,
                                                      const double* __restrict__ area_rng, const double* __restrict__ iou_thr,
                                                      unsigned long long* __restrict__ dt_bits, int* __restrict__ gt_count,
                                                      unsigned char* __restrict__ ws, long Ng) {
#pragma clang fp contract(off)
  constexpr int FAST_GT = Rules::fast_gt;
  __shared__ double iou_s[AP_TILE];                        // [tile detections][G]
  __shared__ unsigned taken_s[(FAST_GT / 32) * 64];        // [word][lane]
  __shared__ unsigned char flag_s[FAST_GT];
  const int p = blockIdx.x, lane = threadIdx.x;
  const int ds = pair_dt[2 * p], D = pair_dt[2 * p + 1], gs = pair_gt[2 * p], G = pair_gt[2 * p + 1];
  const bool fast = G <= FAST_GT;
  const int a = lane / AP_NT, t = lane % AP_NT;
  const bool active = lane < AP_LANES;
  const int abit = active ? 1 << a : 0;
  double lo = 0, hi = 0, thr = 0;
  if (active) {
    lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
    const double cap = 1 - 1e-10;                          // min([iou_thr, 1 - 1e-10])
    thr = cap < iou_thr[t] ? cap : iou_thr[t];
  }
  if (lane < AP_NA) {                                      // non-ignored ground truths of the pair per area range
    int n = 0;
    for (int g = 0; g < G; ++g) n += !(ap_gt_flags<Rules>(gt_area, gt_ign, gt_nz, area_rng, gs + g) & (1 << lane));
    gt_count[p * AP_NA + lane] = n;
  }
  if (D == 0) return;
  unsigned char* tk = ws + (long)lane * Ng + gs;           // slow path: this lane's taken flags
  if (fast) {
    for (int g = lane; g < G; g += 64) flag_s[g] = (unsigned char)ap_gt_flags<Rules>(gt_area, gt_ign, gt_nz, area_rng, gs + g);
    for (int w = 0; w < (G + 31) / 32; ++w) taken_s[w * 64 + lane] = 0;
  } else if (active) {
    for (int g = 0; g < G; ++g) tk[g] = 0;
  }
  const int TD = fast && G > 0 ? AP_TILE / G : 64;
  const bool nel = pair_nel != nullptr && pair_nel[p] != 0;
  for (int d0 = 0; d0 < D; d0 += TD) {
    const int td = min(TD, D - d0);
    __syncthreads();                                       // flag_s written / the previous tile's scans done
    if (fast && G > 0) {
      for (int e = lane; e < td * G; e += 64) {
        const int g = e % G;
        iou_s[e] = ap_iou(dt_box + (long)(ds + d0 + e / G) * 4, gt_box + (long)(gs + g) * 4, Rules::crowd && (flag_s[g] & AP_F_CROWD) != 0);
      }
    }
    __syncthreads();
    for (int dd = 0; dd < td; ++dd) {
      const long d = ds + d0 + dd;
      bool matched = false, ignored = false;
      if (active) {
        const float* db = dt_box + d * 4;
        double cur = thr;
        int m = -1;
        // two passes = the reference's scan over the ground truths sorted ignored-last: once a non-ignored match exists the scan breaks
        // at the first ignored ground truth it does not skip, so the ignored ones are only scanned when the first pass found nothing
        for (int pass = 0; pass < 2 && m < 0; ++pass) {
          for (int g = 0; g < G; ++g) {
            int fl;                                        // a crowd is never taken
            if (fast) {
              fl = flag_s[g];
              if (((fl & abit) != 0) != (pass == 1)) continue;
              if (!(Rules::crowd && (fl & AP_F_CROWD)) && (taken_s[(g >> 5) * 64 + lane] >> (g & 31) & 1)) continue;
            } else {
              fl = ap_gt_flags<Rules>(gt_area, gt_ign, gt_nz, area_rng, gs + g);
              if (((fl & abit) != 0) != (pass == 1)) continue;
              if (!(Rules::crowd && (fl & AP_F_CROWD)) && tk[g]) continue;
            }
            const double v = fast ? iou_s[dd * G + g] : ap_iou(db, gt_box + (long)(gs + g) * 4, Rules::crowd && (fl & AP_F_CROWD) != 0);
            if (v < cur) continue;
            cur = v;
            m = g;
          }
        }
        if (m >= 0) {
          if (fast) taken_s[(m >> 5) * 64 + lane] |= 1u << (m & 31);
          else tk[m] = 1;
          const int fl = fast ? flag_s[m] : ap_gt_flags<Rules>(gt_area, gt_ign, gt_nz, area_rng, gs + m);
          matched = (fl & AP_F_NZ) != 0;                   // dtm holds the ground truth's id: an id of 0 reads as unmatched
          ignored = (fl & abit) != 0;
        }
        if (!matched) {
          const double da = (double)db[2] * (double)db[3];
          if (da < lo || da > hi || nel) ignored = true;
        }
      }
      const unsigned long long bm = __ballot(matched), bi = __ballot(ignored);
      if (lane == 0) {
        dt_bits[2 * d] = bm;
        dt_bits[2 * d + 1] = bi;
      }
    }
  }
}

// grid (K, NM); rank / max_dets are read for NM > 1 only.  precision [10, 101, K, 4, NM], recall [10, K, 4, NM] (NM = 1: LVIS's layout)
template <int NM>
__global__ __launch_bounds__(64) void ap_accumulate_kernel(const int* __restrict__ cat_off, const int* __restrict__ order,
                                                           const int* __restrict__ rank, const unsigned long long* __restrict__ dt_bits,
                                                           const int* __restrict__ num_gt, const int* __restrict__ max_dets,
                                                           const double* __restrict__ rec_thr, double* __restrict__ precision,
                                                           double* __restrict__ recall, int K) {
#pragma clang fp contract(off)
  __shared__ double seg_s[AP_NR * 64];                     // [recall point][lane]: max of pr from the point's index to the next point's
  __shared__ unsigned long long bits_s[2 * 64];
  __shared__ int rank_s[64];                               // not referenced for NM = 1: no LDS there
  const int k = blockIdx.x, mi = blockIdx.y, lane = threadIdx.x;
  const int a = lane / AP_NT, t = lane % AP_NT;
  const int off = cat_off[k], n = cat_off[k + 1] - off;
  int md = 0;
  if constexpr (NM > 1) md = max_dets[mi];
  const int ng = lane < AP_LANES ? num_gt[k * AP_NA + a] : 0;
  const bool active = lane < AP_LANES && ng > 0;
  const double eps = 2.220446049250313e-16;                // np.spacing(1)
  double tp = 0, fp = 0, seg = 0;
  int r = 0, open = -1;
  for (int c0 = 0; c0 < n; c0 += 64) {
    const int cn = min(64, n - c0);
    __syncthreads();
    if (lane < cn) {
      const long j = order[off + c0 + lane];
      bits_s[lane] = dt_bits[2 * j];
      bits_s[64 + lane] = dt_bits[2 * j + 1];
      if constexpr (NM > 1) rank_s[lane] = rank[j];
    }
    __syncthreads();
    if (!active) continue;
    for (int i = 0; i < cn; ++i) {
      if constexpr (NM > 1)
        if (rank_s[i] >= md) continue;                     // e['dtMatches'][:, 0:maxDet]
      const bool m = bits_s[i] >> lane & 1, ig = bits_s[64 + i] >> lane & 1;
      if (!ig) {
        if (m) tp += 1;
        else fp += 1;
      }
      const double pr = tp / (fp + tp + eps);
      const double rc = tp / ng;
      if (r < AP_NR && rc >= rec_thr[r]) {                 // searchsorted(rc, rec_thrs, "left") reaches this detection
        if (open >= 0) seg_s[open * 64 + lane] = seg;
        while (r < AP_NR && rc >= rec_thr[r]) {
          seg_s[r * 64 + lane] = -1.0;                     // empty segment (pr >= 0)
          ++r;
        }
        open = r - 1;
        seg = pr;
      } else if (pr > seg) {
        seg = pr;
      }
    }
  }
  if (lane >= AP_LANES) return;
  const long KAM = (long)K * AP_NA * NM;
  const long col = ((long)k * AP_NA + a) * NM + mi;
  if (!active) {                                           // num_gt == 0: the reference leaves -1
    for (int q = 0; q < AP_NR; ++q) precision[((long)t * AP_NR + q) * KAM + col] = -1.0;
    recall[t * KAM + col] = -1.0;
    return;
  }
  if (open >= 0) seg_s[open * 64 + lane] = seg;
  recall[t * KAM + col] = tp / ng;                         // rc[-1], or 0 without detections
  double env = -1.0;
  for (int q = AP_NR - 1; q >= 0; --q) {
    double v = 0.0;                                        // recall levels past the end of rc
    if (q < r) {
      env = fmax(env, seg_s[q * 64 + lane]);
      v = env;
    }
    precision[((long)t * AP_NR + q) * KAM + col] = v;
  }
}

template <class Rules>
static int ap_match(const int* pair_dt, const int* pair_gt, const unsigned char* pair_nel, const float* dt_box, const double* gt_box,
                    const double* gt_area, const unsigned char* gt_ign, const unsigned char* gt_nz, const double* area_rng,
                    const double* iou_thr, unsigned long long* dt_bits, int* gt_count, unsigned char* ws, int P, long Ng, void* stream) {
  if (P <= 0) return 0;
  if (Ng < 0) return -1;
  return mq_launch<ap_match_kernel<Rules>>(dim3(P), dim3(64), 0, (hipStream_t)stream, pair_dt, pair_gt, pair_nel, dt_box, gt_box, gt_area,
                                           gt_ign, gt_nz, area_rng, iou_thr, dt_bits, gt_count, ws, Ng);
}

template <int NM>
static int ap_accumulate(const int* cat_off, const int* order, const int* rank, const unsigned long long* dt_bits, const int* num_gt,
                         const int* max_dets, const double* rec_thr, double* precision, double* recall, int K, void* stream) {
  if (K <= 0) return 0;
  return mq_launch<ap_accumulate_kernel<NM>>(dim3(K, NM), dim3(64), 0, (hipStream_t)stream, cat_off, order, rank, dt_bits, num_gt, max_dets,
                                             rec_thr, precision, recall, K);
}

extern "C" int mq_lvis_match(const int* pair_dt, const int* pair_gt, const unsigned char* pair_nel, const float* dt_box, const double* gt_box,
                             const double* gt_area, const unsigned char* gt_ign, const unsigned char* gt_nz, const double* area_rng,
                             const double* iou_thr, unsigned long long* dt_bits, int* gt_count, unsigned char* ws, int P, long Ng, void* stream) {
  return ap_match<LvisRules>(pair_dt, pair_gt, pair_nel, dt_box, gt_box, gt_area, gt_ign, gt_nz, area_rng, iou_thr, dt_bits, gt_count, ws, P, Ng,
                             stream);
}

extern "C" int mq_coco_match(const int* pair_dt, const int* pair_gt, const float* dt_box, const double* gt_box, const double* gt_area,
                             const unsigned char* gt_crowd, const unsigned char* gt_nz, const double* area_rng, const double* iou_thr,
                             unsigned long long* dt_bits, int* gt_count, unsigned char* ws, int P, long Ng, void* stream) {
  return ap_match<CocoRules>(pair_dt, pair_gt, nullptr, dt_box, gt_box, gt_area, gt_crowd, gt_nz, area_rng, iou_thr, dt_bits, gt_count, ws, P, Ng,
                             stream);
}

extern "C" int mq_lvis_accumulate(const int* cat_off, const int* order, const unsigned long long* dt_bits, const int* num_gt,
                                  const double* rec_thr, double* precision, double* recall, int K, void* stream) {
  return ap_accumulate<1>(cat_off, order, nullptr, dt_bits, num_gt, nullptr, rec_thr, precision, recall, K, stream);
}

extern "C" int mq_coco_accumulate(const int* cat_off, const int* order, const int* rank, const unsigned long long* dt_bits, const int* num_gt,
                                  const int* max_dets, const double* rec_thr, double* precision, double* recall, int K, void* stream) {
  return ap_accumulate<3>(cat_off, order, rank, dt_bits, num_gt, max_dets, rec_thr, precision, recall, K, stream);
}

#endif
MQ_NAMESPACE_END
