// Test-time augmentation (TEST.USE_MULTISCALE): the device image ingest and the device merge of the per-transform detections.
//
// mq_tta_ingest_fwd: B ragged RGB uint8 HWC images -> the fp32 NCHW zero-padded canvas of one scale, plain and (optionally) flipped, in one
// launch.  Resampling is PIL's uint8 BILINEAR resize, bit for bit (libImaging/Resample.c: two separable passes, horizontal first into a
// rounded and clamped uint8 intermediate, 22-bit fixed-point coefficients, accumulation from 1 << 21, clamp(acc >> 22, 0, 255)).  The
// coefficient tables are built on the host in float64 (mq_det_amd/tta.py: pil_coeffs); a pass PIL skips is an identity table (one tap of
// weight 1 << 22), which gives the same bytes.  The kernel does integer math only, then the fp32 ToTensor / Normalize of the reference.
//
// mq_tta_merge_*: box_aug.py merge_result_from_multi_scales with SPECIAL_NMS = 'none', after the per-transform un-flip / area band /
// rescale, as four launches around mq_ml_nms (nms.hip).  Every sort is a rank by counting over a total order, so the result does not
// depend on the schedule.
//
// mq_tta_merge_special / mq_tta_merge_finalize_special: the same merge with SPECIAL_NMS = 'soft-nms', 'vote' or 'soft-vote': the per-class
// step in place of mq_ml_nms, one workgroup per (image, class), and a finalize whose cut ranks the new scores (see "special merges" below;
// ties on equal scores go to the lower original row, where the reference's order is whatever numpy's unstable argsort leaves).
//
// mq_tta_merge_nms: the per-class NMS of the 'none' merge for lists mq_ml_nms's N^2 bit mask cannot take (the un-suppressed candidates of
// TEST.USE_MULTISCALE: transforms x 5 x PRE_NMS_TOP_N rows per image), one workgroup per (image, class), the same keep flags byte for
// byte (see "per-class NMS, any N" below).
#include "common.h"
#include "box_iou.h"

MQ_NAMESPACE_BEGIN
#ifdef MQ_PRIMARY_UNIT                                     // uint8 / fp32 / int data only: one copy, in the fp16 translation unit

// ---------------------------------------------------------------------------------------------------------------- ingest
// meta [B, 16] int32 per image: 0 H_in, 1 W_in, 2 H_out, 3 W_out, 4 x-table column offset, 5 x-coefficient offset, 6 x taps,
// 7 y-table row offset, 8 y-coefficient offset, 9 y taps.  bounds: (first input index, taps used) per output index; coef: taps ints each.
#define TTA_TW 64                                          // output columns per workgroup (one per lane of a wave)

__device__ __forceinline__ int tta_clip8(int acc) {
  const int v = acc >> 22;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__global__ __launch_bounds__(256) void tta_ingest_kernel(const unsigned char* __restrict__ src, const long* __restrict__ src_off,
                                                         const int* __restrict__ meta, const int* __restrict__ bounds,
                                                         const int* __restrict__ coef, float* __restrict__ out, float* __restrict__ out_flip,
                                                         int* __restrict__ err, int Hp, int Wp, int TH, int R, float m0, float m1, float m2, float s0, float s1,
                                                         float s2, int bgr, int x255) {
#pragma clang fp contract(off)                           // the reference's fp32 ops one by one: no fma of the x 255 into the - mean
  extern __shared__ __attribute__((aligned(16))) unsigned char tmp_s[];   // [R][TTA_TW][3] horizontal-pass rows of the tile
  const int b = blockIdx.z, x0 = blockIdx.x * TTA_TW, y0 = blockIdx.y * TH, tid = threadIdx.x;
  const int* mb = meta + b * 16;
  const int Wi = mb[1], Ho = mb[2], Wo = mb[3], xbo = mb[4], xko = mb[5], xks = mb[6], ybo = mb[7], yko = mb[8], yks = mb[9];
  const long plane = (long)Hp * Wp;
  float* ob = out + (long)b * 3 * plane;
  float* fb = out_flip ? out_flip + (long)b * 3 * plane : nullptr;
  const int lx = tid & (TTA_TW - 1), x = x0 + lx;
  const int rows = min(TH, Ho - y0);                      // output rows of the tile inside the image (<= 0: padding only)
  int ry0 = 0;
  if (rows > 0) {
    ry0 = bounds[(ybo + y0) * 2];
    int ry1 = ry0;                                        // one past the last input row the tile's rows read
    for (int r = 0; r < rows; ++r) ry1 = max(ry1, bounds[(ybo + y0 + r) * 2] + bounds[(ybo + y0 + r) * 2 + 1]);
    int nr = ry1 - ry0;                                   // <= R: the host sized R from the same tables
    if (nr > R) {                                         // never with the host's tables: reported (the wrapper raises), LDS stays in bounds
      if (tid == 0) atomicAdd(err, 1);
      nr = R;
    }
    const unsigned char* sb = src + src_off[b];
    for (int e = tid; e < nr * TTA_TW; e += 256) {        // horizontal pass: input rows ry0 .. ry1 - 1, the tile's 64 output columns
      const int r = e / TTA_TW, c = e % TTA_TW, xo = x0 + c;
      if (xo >= Wo) continue;
      const int xmin = bounds[(xbo + xo) * 2], n = bounds[(xbo + xo) * 2 + 1];
      const int* k = coef + xko + (long)xo * xks;
      const unsigned char* p = sb + ((long)(ry0 + r) * Wi + xmin) * 3;
      int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
      for (int j = 0; j < n; ++j) {
        const int w = k[j];
        a0 += (int)p[j * 3 + 0] * w;
        a1 += (int)p[j * 3 + 1] * w;
        a2 += (int)p[j * 3 + 2] * w;
      }
      unsigned char* t = tmp_s + (r * TTA_TW + c) * 3;
      t[0] = (unsigned char)tta_clip8(a0);
      t[1] = (unsigned char)tta_clip8(a1);
      t[2] = (unsigned char)tta_clip8(a2);
    }
  }
  __syncthreads();
  const float mean[3] = {m0, m1, m2}, stdv[3] = {s0, s1, s2};
  if (x >= Wp) return;
  for (int ly = tid / TTA_TW; ly < TH; ly += 256 / TTA_TW) {   // vertical pass + normalisation: lane = column, waves = rows
    const int y = y0 + ly;
    if (y >= Hp) break;
    const long o = (long)y * Wp;
    if (ly >= rows || x >= Wo) {                          // padding of to_image_list: zero in both canvases
      for (int c = 0; c < 3; ++c) {
        ob[c * plane + o + x] = 0.f;
        if (fb) fb[c * plane + o + x] = 0.f;
      }
      continue;
    }
    const int ymin = bounds[(ybo + y) * 2] - ry0, n = bounds[(ybo + y) * 2 + 1];
    const int* k = coef + yko + (long)y * yks;
    int acc[3] = {1 << 21, 1 << 21, 1 << 21};
    for (int j = 0; j < n; ++j) {
      const unsigned char* t = tmp_s + ((ymin + j) * TTA_TW + lx) * 3;
      const int w = k[j];
      acc[0] += (int)t[0] * w;
      acc[1] += (int)t[1] * w;
      acc[2] += (int)t[2] * w;
    }
    const long xf = o + (Wo - 1 - x);                     // RandomHorizontalFlip(1.0) happens before the padding
    for (int c = 0; c < 3; ++c) {
      const int sc = bgr ? 2 - c : c;                     // Normalize: image[[2, 1, 0]] for 'bgr' formats
      float v = (float)tta_clip8(acc[sc]) / 255.f;       // ToTensor: correctly rounded division
      if (x255) v = v * 255.f;
      v = (v - mean[c]) / stdv[c];
      ob[c * plane + o + x] = v;
      if (fb) fb[c * plane + xf] = v;
    }
  }
}

// src: the B images packed, image b at src + src_off[b] ([H_in, W_in, 3] uint8); out / out_flip [B, 3, Hp, Wp] fp32 (out_flip may be NULL).
// mean / stdv: HOST float[3].  TH output rows per workgroup and R = the largest input-row window of a tile (host: mq_det_amd/tta.py); LDS = R * 192 bytes.
extern "C" int mq_tta_ingest_fwd(const unsigned char* src, const long* src_off, const int* meta, const int* bounds, const int* coef,
                                 float* out, float* out_flip, int* err, int B, int Hp, int Wp, int TH, int R, const float* mean, const float* stdv,
                                 int bgr, int x255, void* stream) {
  if (B <= 0) return 0;
  if (TH < 1 || R < 1 || Hp < 1 || Wp < 1 || B > 65535) return -1;
  const size_t smem = (size_t)R * TTA_TW * 3;
  if (smem > 160 * 1024) return -1;
  dim3 grid((Wp + TTA_TW - 1) / TTA_TW, (Hp + TH - 1) / TH, B);
  return mq_launch<tta_ingest_kernel>(grid, dim3(256), smem, (hipStream_t)stream, src, src_off, meta, bounds, coef, out, out_flip, err, Hp, Wp, TH, R, mean[0], mean[1], mean[2], stdv[0], stdv[1], stdv[2], bgr, x255);
}

// ---------------------------------------------------------------------------------------------------------------- merge
// 1. per row of every transform: un-flip, area band, rescale, class filter -> compacted-by-flag rows [B, N] (N = T * K, row t * K + k)
__global__ __launch_bounds__(256) void tta_prep_kernel(const float* __restrict__ packed, const int* __restrict__ counts,
                                                       const float* __restrict__ tparam, const float* __restrict__ band,
                                                       const int* __restrict__ cls_rank, int n_cls, float* __restrict__ boxes,
                                                       float* __restrict__ scores, int* __restrict__ labels, unsigned char* __restrict__ valid,
                                                       int* __restrict__ nvalid, int* __restrict__ ndrop, int T, int B, int K) {
#pragma clang fp contract(off)
  const int b = blockIdx.y, N = T * K, n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const int t = n / K, k = n % K;
  const long o = (long)b * N + n;
  valid[o] = 0;
  if (k >= counts[t * B + b]) return;
  const float* p = packed + (((long)t * B + b) * K + k) * 6;
  const float* tp = tparam + ((long)t * B + b) * 4;         // (flip: scaled width, else -1; width ratio; height ratio; -)
  float x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
  const float s = p[4];
  const int l = (int)p[5];
  if (tp[0] >= 0.f) {                                      // BoxList.transpose(FLIP_LEFT_RIGHT), TO_REMOVE = 1
    const float w = tp[0], nx1 = (w - x2) - 1.f, nx2 = (w - x1) - 1.f;
    x1 = nx1;
    x2 = nx2;
  }
  if (band) {                                              // remove_boxes: strictly inside (min^2, max^2)
    const float a = (x2 - x1 + 1.f) * (y2 - y1 + 1.f);
    if (!(a > band[t * 2] && a < band[t * 2 + 1])) return;
  }
  if (!(s == s)) return;                                   // a NaN score has no place in a total order
  if (l < 0 || l >= n_cls || cls_rank[l] < 0) {           // labels outside SELECT_CLASSES / range(1, NUM_CLASSES)
    atomicAdd(ndrop + b, 1);
    return;
  }
  const float rw = tp[1], rh = tp[2];                      // BoxList.resize
  boxes[o * 4 + 0] = x1 * rw;
  boxes[o * 4 + 1] = y1 * rh;
  boxes[o * 4 + 2] = x2 * rw;
  boxes[o * 4 + 3] = y2 * rh;
  scores[o] = s;
  labels[o] = l;
  valid[o] = 1;
  atomicAdd(nvalid + b, 1);
}

// 2. rank of every valid row in (score descending, row ascending) -> the score-sorted lists mq_ml_nms sweeps
__global__ __launch_bounds__(256) void tta_rank_score_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                             const int* __restrict__ labels, const unsigned char* __restrict__ valid,
                                                             float* __restrict__ boxes_s, float* __restrict__ scores_s, int* __restrict__ labels_s,
                                                             int* __restrict__ src_s, int N) {
  __shared__ float ss[256];
  __shared__ int sv[256];
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  const long base = (long)b * N;
  const bool mine = i < N && valid[base + i];
  const float si = mine ? scores[base + i] : 0.f;
  int rank = 0;
  for (int j0 = 0; j0 < N; j0 += 256) {
    const int j = j0 + threadIdx.x;
    __syncthreads();
    sv[threadIdx.x] = j < N ? valid[base + j] : 0;
    ss[threadIdx.x] = j < N ? scores[base + j] : 0.f;
    __syncthreads();
    if (mine) {
      const int m = min(256, N - j0);
      for (int q = 0; q < m; ++q)
        rank += sv[q] && (ss[q] > si || (ss[q] == si && j0 + q < i));
    }
  }
  if (!mine) return;
  const long o = base + rank;
  for (int c = 0; c < 4; ++c) boxes_s[o * 4 + c] = boxes[(base + i) * 4 + c];
  scores_s[o] = si;
  labels_s[o] = labels[base + i];
  src_s[o] = i;
}

// 3. the top-N cut (box_aug.py: kthvalue(scores, n - PRE_NMS_TOP_N + 1), keep >=): with the kept rows in score order the threshold is the
//    score of the top_n-th kept row.  One workgroup per image -> thr [B] (-inf: no cut)
__global__ __launch_bounds__(256) void tta_cut_kernel(const float* __restrict__ scores_s, const unsigned char* __restrict__ keep,
                                                      const int* __restrict__ nvalid, float* __restrict__ thr, int N, int top_n) {
  __shared__ int cnt[256];
  __shared__ int total_s;
  const int b = blockIdx.x, n = nvalid[b], tid = threadIdx.x;
  const int per = (n + 255) / 256, i0 = min(n, tid * per), i1 = min(n, i0 + per);
  const unsigned char* kb = keep + (long)b * N;
  int c = 0;
  for (int i = i0; i < i1; ++i) c += kb[i] != 0;
  cnt[tid] = c;
  __syncthreads();
  if (tid == 0) {                                          // exclusive prefix over the 256 chunks
    int acc = 0;
    for (int q = 0; q < 256; ++q) {
      const int v = cnt[q];
      cnt[q] = acc;
      acc += v;
    }
    total_s = acc;
    if (!(top_n > 0 && acc > top_n)) thr[b] = -__builtin_inff();
  }
  __syncthreads();
  if (top_n > 0 && total_s > top_n) {
    int seen = cnt[tid];
    if (seen < top_n && seen + c >= top_n)                 // this chunk holds the top_n-th kept row
      for (int i = i0; i < i1; ++i)
        if (kb[i] && ++seen == top_n) {
          thr[b] = scores_s[(long)b * N + i];
          break;
        }
  }
}

// 4. rank of every surviving row in (position of its label in the class list, original row ascending) -> the output lists, int64 labels
__global__ __launch_bounds__(256) void tta_rank_final_kernel(const float* __restrict__ boxes_s, const float* __restrict__ scores_s,
                                                             const int* __restrict__ labels_s, const int* __restrict__ src_s,
                                                             const unsigned char* __restrict__ keep, const int* __restrict__ nvalid,
                                                             const float* __restrict__ thr, const int* __restrict__ cls_rank,
                                                             float* __restrict__ boxes_o,
                                                             float* __restrict__ scores_o, long long* __restrict__ labels_o,
                                                             int* __restrict__ counts, int N) {
  __shared__ int sl[256], sr[256], sf[256];
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x, n = nvalid[b];
  const long base = (long)b * N;
  const float th = thr[b];
  const bool mine = i < n && keep[base + i] && scores_s[base + i] >= th;
  const int lab = mine ? labels_s[base + i] : 0, li = mine ? cls_rank[lab] : 0, ri = mine ? src_s[base + i] : 0;
  int rank = 0;
  for (int j0 = 0; j0 < n; j0 += 256) {
    const int j = j0 + threadIdx.x;
    __syncthreads();
    const bool fj = j < n && keep[base + j] && scores_s[base + j] >= th;
    sf[threadIdx.x] = fj;
    sl[threadIdx.x] = fj ? cls_rank[labels_s[base + j]] : 0;
    sr[threadIdx.x] = fj ? src_s[base + j] : 0;
    __syncthreads();
    if (mine) {
      const int m = min(256, n - j0);
      for (int q = 0; q < m; ++q)
        rank += sf[q] && (sl[q] < li || (sl[q] == li && sr[q] < ri));
    }
  }
  if (!mine) return;
  atomicAdd(counts + b, 1);
  const long o = base + rank;
  for (int c = 0; c < 4; ++c) boxes_o[o * 4 + c] = boxes_s[(base + i) * 4 + c];
  scores_o[o] = scores_s[base + i];
  labels_o[o] = lab;
}

// packed [T, B, K, 6] fp32 rows (x1, y1, x2, y2, score, label) of T transforms, counts [T, B] int32 live rows; tparam [T, B, 4] fp32
// (scaled width when the transform is flipped, else -1; width ratio; height ratio; unused); band [T, 2] fp32 squared (min, max) or NULL;
// cls_rank [n_cls] int32: position of label l in the class list, -1 = dropped.  Work arrays (N = T * K): boxes / boxes_s [B, N, 4] fp32, scores / scores_s [B, N] fp32, labels / labels_s / src_s
// [B, N] int32, valid [B, N] uint8; nvalid / ndrop [B] int32 ZEROED by the caller.  -> rows sorted for mq_ml_nms, nvalid, ndrop.
extern "C" int mq_tta_merge_prep(const float* packed, const int* counts, const float* tparam, const float* band, const int* cls_rank,
                                 int n_cls, float* boxes, float* scores, int* labels, unsigned char* valid, float* boxes_s,
                                 float* scores_s, int* labels_s, int* src_s, int* nvalid, int* ndrop, int T, int B, int K, void* stream) {
  const long N = (long)T * K;
  if (B <= 0 || N <= 0) return 0;
  if (N > (1 << 24) || B > 65535) return -1;
  dim3 grid((unsigned)((N + 255) / 256), B);
  hipLaunchKernelGGL(tta_prep_kernel, grid, dim3(256), 0, (hipStream_t)stream, packed, counts, tparam, band, cls_rank, n_cls, boxes, scores,
                     labels, valid, nvalid, ndrop, T, B, K);
  MQ_CHECK_LAUNCH();
  hipLaunchKernelGGL(tta_rank_score_kernel, grid, dim3(256), 0, (hipStream_t)stream, boxes, scores, labels, valid, boxes_s, scores_s,
                     labels_s, src_s, (int)N);
  MQ_CHECK_LAUNCH();
  return 0;
}

// after mq_ml_nms(boxes_s, labels_s, nvalid) -> keep [B, N]: the top_n cut and the output order (class-list position, row).  thr [B] fp32 work; boxes_o [B, N, 4],
// scores_o [B, N] fp32, labels_o [B, N] int64; counts [B] int32 ZEROED by the caller -> live rows of every image.
extern "C" int mq_tta_merge_finalize(const float* boxes_s, const float* scores_s, const int* labels_s, const int* src_s,
                                     const unsigned char* keep, const int* nvalid, float* thr, const int* cls_rank, float* boxes_o, float* scores_o,
                                     long long* labels_o, int* counts, int B, int N, int top_n, void* stream) {
  if (B <= 0 || N <= 0) return 0;
  if (B > 65535) return -1;
  hipLaunchKernelGGL(tta_cut_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, scores_s, keep, nvalid, thr, N, top_n);
  MQ_CHECK_LAUNCH();
  hipLaunchKernelGGL(tta_rank_final_kernel, dim3((N + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, boxes_s, scores_s, labels_s, src_s,
                     keep, nvalid, thr, cls_rank, boxes_o, scores_o, labels_o, counts, N);
  MQ_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------- special merges
// TEST.SPECIAL_NMS = 'soft-nms' / 'vote' / 'soft-vote' (box_aug.py:209-349, csrc/cpu/soft_nms.cpp): the per-class step between
// mq_tta_merge_prep and the output ranking, one workgroup per (image, class-list position).  The workgroup gathers its class's rows from the
// image's score-sorted list in list order (position = number of earlier rows of the class: a count, not a race), stages them -- box, +1
// area, score, list index, original row, state -- in LDS, or, when the class has more than `cap` rows, in its own slice of a global
// workspace (slice start = rows of earlier classes, so the slices are disjoint), and runs the reference's loop on the staged rows:
//   soft-nms   pick the live row of the highest current score; every other live row s <- float(s * exp(-ovr^2 / sigma)) with the fp32 +1
//              IoU and the fp64 factor; s < thresh discards the row; the picks, in pick order, with their decayed scores
//   vote       the first live row (rows are in score order) heads a cluster of every live row with IoU >= thresh; a cluster of one passes
//              through, a larger one becomes sum(b s) / sum(s) with the head's score; clusters in cluster order
//   soft-vote  vote, plus every non-head member with s (1 - ovr) >= aux (MODEL.RETINANET.INFERENCE_TH) as a row of its own box and that
//              score; the class's rows re-sorted by score
// Every output row takes the slot of one input row (a cluster its head's), so the capacity stays N.  -> per slot: box, score, keep flag and
// seq, the row's place inside its class, which mq_tta_merge_finalize_special ranks by.
// IoUs are the reference's fp32 operations in its order with contraction off: every >= of the voting modes is numpy's.  The voted box is
// summed in fp64 in a fixed order (per thread by ascending row, then a fixed tree) and rounded once; the reference sums in fp32.
// TIES: on equal scores the reference's order follows numpy's unstable argsort and soft-NMS's swap-with-last; here the LOWER ORIGINAL ROW
// goes first (list order for the votes, the staged original row for soft-NMS's pick and soft-vote's final sort).
#define TTA_SP_WORDS 9                                     // 4-byte words staged per row
#define TTA_SP_MAX_CAP 4096                                // rows of the LDS path at most: 144 KB
enum { TTA_SOFT_NMS = 1, TTA_VOTE = 2, TTA_SOFT_VOTE = 3 };
enum { TTA_DEAD = 0, TTA_LIVE = 1, TTA_OUT = 4 };

// The class segment of one workgroup (256 threads) of tta_special_kernel / tta_nms_kernel: lab = the labels of the image's score-sorted
// list, n = min(max(nvalid[b], 0), N) its rows, c = the workgroup's position in the class list.
// position of label l in the class list; -1: a label of no class (outside [0, L), or dropped by cls_rank)
__device__ __forceinline__ int tta_cls_pos(const int* __restrict__ cls_rank, int L, int l) { return (l >= 0 && l < L) ? cls_rank[l] : -1; }

// -> m, the rows of position c (the same in every thread), and st, where the workgroup stages them, WORDS words a row: the dynamic LDS
// when m <= cap, else the class's slice of the workspace ws [B, N, WORDS] (counted in nws); the slice starts at the rows of the earlier
// positions.  base = b * N; cnt_s: LDS int [2].
template <int WORDS>
__device__ __forceinline__ int tta_class_rows(const int* __restrict__ lab, const int* __restrict__ cls_rank, int L, int n, int c, int cap,
                                              float* lds, float* ws, long base, int* nws, int* cnt_s, float*& st) {
  const int tid = threadIdx.x;
  if (tid < 2) cnt_s[tid] = 0;
  __syncthreads();
  int mc = 0, oc = 0;
  for (int j = tid; j < n; j += 256) {
    const int p = tta_cls_pos(cls_rank, L, lab[j]);
    mc += p == c;
    oc += p >= 0 && p < c;
  }
  atomicAdd(&cnt_s[0], mc);
  atomicAdd(&cnt_s[1], oc);
  __syncthreads();
  const int m = cnt_s[0], off = cnt_s[1];
  st = lds;
  if (m > cap) {
    if (tid == 0) atomicAdd(nws, 1);
    st = ws + (base + off) * WORDS;
  }
  return m;
}

// store(j, k) for every row j of position c: k = the rows of the class before j in the list (a ballot prefix over the four waves: a
// count, not a race).  wcnt: LDS int [4].
template <class Store>
__device__ __forceinline__ void tta_class_stage(const int* __restrict__ lab, const int* __restrict__ cls_rank, int L, int n, int c, int* wcnt,
                                                Store store) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int run = 0;
  for (int j0 = 0; j0 < n; j0 += 256) {
    const int j = j0 + tid;
    const bool mine = j < n && tta_cls_pos(cls_rank, L, lab[j]) == c;
    const unsigned long long bal = __ballot(mine);
    if (lane == 0) wcnt[wv] = __popcll(bal);
    __syncthreads();
    int k = run + __popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < wv; ++w) k += wcnt[w];
    run += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    if (mine) store(j, k);
    __syncthreads();
  }
}

__device__ __forceinline__ float tta_iou1(float ax1, float ay1, float ax2, float ay2, float aa, float bx1, float by1, float bx2, float by2,
                                          float ba) {
#pragma clang fp contract(off)                           // soft_nms.cpp:77-86 / box_aug.py:252-260, one operation at a time
  const float xx1 = ax1 < bx1 ? bx1 : ax1, yy1 = ay1 < by1 ? by1 : ay1;
  const float xx2 = bx2 < ax2 ? bx2 : ax2, yy2 = by2 < ay2 ? by2 : ay2;
  float w = (xx2 - xx1) + 1.f, h = (yy2 - yy1) + 1.f;
  w = w > 0.f ? w : 0.f;
  h = h > 0.f ? h : 0.f;
  const float inter = w * h;
  return inter / ((aa + ba) - inter);
}

__device__ __forceinline__ double tta_wave_sum(double v) {
  for (int d = 32; d; d >>= 1) v += __shfl_down(v, d);
  return v;                                                // lane 0: the wave's sum, always the same tree
}

__global__ __launch_bounds__(256) void tta_special_kernel(const float* __restrict__ boxes_s, const float* __restrict__ scores_s,
                                                          const int* __restrict__ labels_s, const int* __restrict__ src_s,
                                                          const int* __restrict__ nvalid, const int* __restrict__ cls_rank,
                                                          float* __restrict__ boxes_m, float* __restrict__ scores_m,
                                                          unsigned char* __restrict__ keep, int* __restrict__ seq, float* __restrict__ ws,
                                                          int* __restrict__ nws, int N, int L, int mode, float thresh, float aux, int cap) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float sp_s[];             // [TTA_SP_WORDS][m] when the class fits
  __shared__ int cnt_s[2], wcnt[4], red_k[4], red_r[4];
  __shared__ float red_s[4];
  __shared__ double red_d[5][4];
  const int b = blockIdx.y, c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = min(max(nvalid[b], 0), N);
  const long base = (long)b * N;
  const int* lab = labels_s + base;
  float* st;
  const int m = tta_class_rows<TTA_SP_WORDS>(lab, cls_rank, L, n, c, cap, sp_s, ws, base, nws, cnt_s, st);
  if (m == 0) return;
  float *X1 = st, *Y1 = st + m, *X2 = st + 2 * (long)m, *Y2 = st + 3 * (long)m, *AR = st + 4 * (long)m, *SC = st + 5 * (long)m;
  int *IDX = (int*)(st + 6 * (long)m), *SRC = (int*)(st + 7 * (long)m), *FL = (int*)(st + 8 * (long)m);
  tta_class_stage(lab, cls_rank, L, n, c, wcnt, [&](int j, int k) {
    const float x1 = boxes_s[(base + j) * 4 + 0], y1 = boxes_s[(base + j) * 4 + 1], x2 = boxes_s[(base + j) * 4 + 2],
                y2 = boxes_s[(base + j) * 4 + 3];
    X1[k] = x1;
    Y1[k] = y1;
    X2[k] = x2;
    Y2[k] = y2;
    AR[k] = ((x2 - x1) + 1.f) * ((y2 - y1) + 1.f);
    SC[k] = scores_s[base + j];
    IDX[k] = j;
    SRC[k] = src_s[base + j];
    FL[k] = TTA_LIVE;
  });

  if (mode == TTA_SOFT_NMS) {
    const double sigma = (double)aux;
    for (int picks = 0;; ++picks) {
      // the live row of the highest current score, the lower original row on a tie
      float bs = 0.f;
      int bk = -1, br = 0;
      for (int k = tid; k < m; k += 256)
        if (FL[k] == TTA_LIVE) {
          const float s = SC[k];
          const int r = SRC[k];
          if (bk < 0 || s > bs || (s == bs && r < br)) bs = s, bk = k, br = r;
        }
      for (int d = 32; d; d >>= 1) {
        const float os = __shfl_down(bs, d);
        const int ok = __shfl_down(bk, d), orow = __shfl_down(br, d);
        if (ok >= 0 && (bk < 0 || os > bs || (os == bs && orow < br))) bs = os, bk = ok, br = orow;
      }
      if (lane == 0) red_s[wv] = bs, red_k[wv] = bk, red_r[wv] = br;
      __syncthreads();
      bs = red_s[0], bk = red_k[0], br = red_r[0];
      for (int w = 1; w < 4; ++w)
        if (red_k[w] >= 0 && (bk < 0 || red_s[w] > bs || (red_s[w] == bs && red_r[w] < br))) bs = red_s[w], bk = red_k[w], br = red_r[w];
      if (bk < 0) break;                                   // nothing live: done (the same answer in every thread)
      const float hx1 = X1[bk], hy1 = Y1[bk], hx2 = X2[bk], hy2 = Y2[bk], ha = AR[bk];
      if (tid == 0) {                                      // the pick is never checked against the threshold
        const long o = base + IDX[bk];
        FL[bk] = TTA_OUT;
        boxes_m[o * 4 + 0] = hx1;
        boxes_m[o * 4 + 1] = hy1;
        boxes_m[o * 4 + 2] = hx2;
        boxes_m[o * 4 + 3] = hy2;
        scores_m[o] = bs;
        keep[o] = 1;
        seq[o] = picks;
      }
      for (int k = tid; k < m; k += 256)
        if (k != bk && FL[k] == TTA_LIVE) {
          const float ovr = tta_iou1(hx1, hy1, hx2, hy2, ha, X1[k], Y1[k], X2[k], Y2[k], AR[k]);
          const float s = (float)((double)SC[k] * exp(-((double)ovr * (double)ovr) / sigma));
          SC[k] = s;
          if (s < thresh) {
            FL[k] = TTA_DEAD;
            keep[base + IDX[k]] = 0;
          }
        }
      __syncthreads();
    }
    return;
  }

  // vote / soft-vote
  int head = 0;
  for (;;) {
    while (head < m && FL[head] != TTA_LIVE) ++head;       // rows are in score order: the first live row heads the next cluster
    if (head >= m) break;
    const float hx1 = X1[head], hy1 = Y1[head], hx2 = X2[head], hy2 = Y2[head], ha = AR[head], hs = SC[head];
    double a0 = 0., a1 = 0., a2 = 0., a3 = 0., as = 0.;
    int members = 0;
    if (tid == 0) {                                        // the head is a member of its own cluster (ovr = 1)
      a0 = (double)hx1 * hs, a1 = (double)hy1 * hs, a2 = (double)hx2 * hs, a3 = (double)hy2 * hs, as = hs;
      members = 1;
    }
    for (int k = head + 1 + tid; k < m; k += 256)
      if (FL[k] == TTA_LIVE) {
        const float x1 = X1[k], y1 = Y1[k], x2 = X2[k], y2 = Y2[k], s = SC[k];
        const float ovr = tta_iou1(hx1, hy1, hx2, hy2, ha, x1, y1, x2, y2, AR[k]);
        if (!(ovr >= thresh)) continue;
        a0 += (double)x1 * s, a1 += (double)y1 * s, a2 += (double)x2 * s, a3 += (double)y2 * s, as += s;
        ++members;
        const long o = base + IDX[k];
        const float soft = s * (1.f - ovr);
        if (mode == TTA_SOFT_VOTE && soft >= aux) {        // the member stays as a row of its own with the softened score
          FL[k] = TTA_OUT;
          SC[k] = soft;
          for (int q = 0; q < 4; ++q) boxes_m[o * 4 + q] = boxes_s[o * 4 + q];
          scores_m[o] = soft;
          keep[o] = 1;
        } else {
          FL[k] = TTA_DEAD;
          keep[o] = 0;
        }
      }
    a0 = tta_wave_sum(a0), a1 = tta_wave_sum(a1), a2 = tta_wave_sum(a2), a3 = tta_wave_sum(a3), as = tta_wave_sum(as);
    for (int d = 32; d; d >>= 1) members += __shfl_down(members, d);
    if (lane == 0) red_d[0][wv] = a0, red_d[1][wv] = a1, red_d[2][wv] = a2, red_d[3][wv] = a3, red_d[4][wv] = as, red_k[wv] = members;
    __syncthreads();
    if (tid == 0) {
      const long o = base + IDX[head];
      float ob[4] = {hx1, hy1, hx2, hy2};
      if (red_k[0] + red_k[1] + red_k[2] + red_k[3] > 1) {
        const double den = ((red_d[4][0] + red_d[4][1]) + red_d[4][2]) + red_d[4][3];
        for (int q = 0; q < 4; ++q) ob[q] = (float)((((red_d[q][0] + red_d[q][1]) + red_d[q][2]) + red_d[q][3]) / den);
      }
      for (int q = 0; q < 4; ++q) boxes_m[o * 4 + q] = ob[q];
      scores_m[o] = hs;
      keep[o] = 1;
      seq[o] = head;                                       // vote: cluster order
      FL[head] = TTA_OUT;
    }
    __syncthreads();
  }
  if (mode == TTA_SOFT_VOTE)                               // the class's rows by (score descending, original row ascending)
    for (int k = tid; k < m; k += 256)
      if (FL[k] == TTA_OUT) {
        const float s = SC[k];
        const int r = SRC[k];
        int rank = 0;
        for (int q = 0; q < m; ++q) rank += FL[q] == TTA_OUT && (SC[q] > s || (SC[q] == s && SRC[q] < r));
        seq[base + IDX[k]] = rank;
      }
}

// the top-N cut when the scores are no longer in list order: the kept row with exactly top_n - 1 kept rows ahead of it in (score
// descending, slot ascending) holds kthvalue(scores, n - top_n + 1) -> thr [B] (-inf: no cut)
__global__ __launch_bounds__(256) void tta_cut_rank_kernel(const float* __restrict__ scores_m, const unsigned char* __restrict__ keep,
                                                           const int* __restrict__ nvalid, float* __restrict__ thr, int N, int top_n) {
  __shared__ float ss[256];
  __shared__ int sf[256];
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x, n = nvalid[b];
  const long base = (long)b * N;
  const bool mine = i < n && keep[base + i];
  const float si = mine ? scores_m[base + i] : 0.f;
  int rank = 0, total = 0;
  for (int j0 = 0; j0 < n; j0 += 256) {
    const int j = j0 + threadIdx.x;
    __syncthreads();
    const bool fj = j < n && keep[base + j];
    sf[threadIdx.x] = fj;
    ss[threadIdx.x] = fj ? scores_m[base + j] : 0.f;
    __syncthreads();
    const int m = min(256, n - j0);
    for (int q = 0; q < m; ++q) {
      total += sf[q];
      rank += sf[q] && (ss[q] > si || (ss[q] == si && j0 + q < i));
    }
  }
  if (!(top_n > 0 && total > top_n)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) thr[b] = -__builtin_inff();
    return;
  }
  if (mine && rank == top_n - 1) thr[b] = si;
}

// The rows mq_tta_merge_prep left (boxes_s / scores_s / labels_s / src_s [B, N], nvalid [B]) -> per slot boxes_m [B, N, 4], scores_m [B, N]
// fp32, keep [B, N] uint8, seq [B, N] int32 (written for the first nvalid[b] slots of image b).  L = length of the class list (cls_rank
// maps a label to 0 .. L - 1); mode 1 soft-nms (aux = sigma), 2 vote, 3 soft-vote (aux = MODEL.RETINANET.INFERENCE_TH > 0); thresh > 0.
// cap: rows of a class staged in LDS at most (1 .. 4096); a larger class works in ws [B, N, 9] fp32 (may be NULL when N <= cap) and is
// counted in nws [1] int32 (ZEROED by the caller).  -1: arguments out of range.
extern "C" int mq_tta_merge_special(const float* boxes_s, const float* scores_s, const int* labels_s, const int* src_s, const int* nvalid,
                                    const int* cls_rank, float* boxes_m, float* scores_m, unsigned char* keep, int* seq, float* ws, int* nws,
                                    int B, int N, int L, int mode, float thresh, float aux, int cap, void* stream) {
  if (B <= 0 || N <= 0 || L <= 0) return 0;
  if (B > 65535 || N > (1 << 24) || mode < TTA_SOFT_NMS || mode > TTA_SOFT_VOTE || !(thresh > 0.f) || cap < 1 || cap > TTA_SP_MAX_CAP) return -1;
  if ((mode == TTA_SOFT_VOTE || mode == TTA_SOFT_NMS) && !(aux > 0.f)) return -1;
  if (N > cap && !ws) return -1;
  const size_t smem = (size_t)(cap < N ? cap : N) * TTA_SP_WORDS * sizeof(float);
  return mq_launch<tta_special_kernel>(dim3(L, B), dim3(256), smem, (hipStream_t)stream, boxes_s, scores_s, labels_s, src_s, nvalid, cls_rank,
                                       boxes_m, scores_m, keep, seq, ws, nws, N, L, mode, thresh, aux, cap);
}

// mq_tta_merge_finalize for the rows of mq_tta_merge_special: the cut over the new scores, then the output order (class-list position, seq).
extern "C" int mq_tta_merge_finalize_special(const float* boxes_m, const float* scores_m, const int* labels_s, const int* seq,
                                             const unsigned char* keep, const int* nvalid, float* thr, const int* cls_rank, float* boxes_o,
                                             float* scores_o, long long* labels_o, int* counts, int B, int N, int top_n, void* stream) {
  if (B <= 0 || N <= 0) return 0;
  if (B > 65535) return -1;
  const dim3 grid((N + 255) / 256, B);
  hipLaunchKernelGGL(tta_cut_rank_kernel, grid, dim3(256), 0, (hipStream_t)stream, scores_m, keep, nvalid, thr, N, top_n);
  MQ_CHECK_LAUNCH();
  hipLaunchKernelGGL(tta_rank_final_kernel, grid, dim3(256), 0, (hipStream_t)stream, boxes_m, scores_m, labels_s, seq, keep, nvalid, thr,
                     cls_rank, boxes_o, scores_o, labels_o, counts, N);
  MQ_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------- per-class NMS, any N
// mq_tta_merge_nms: what mq_ml_nms (nms.hip) answers -- greedy suppression in list order between rows of equal label at iou > thresh --
// without its [N, N / 64] bit mask, for the candidate lists of TEST.USE_MULTISCALE (transforms x 5 x PRE_NMS_TOP_N rows per image).  The
// class segment of tta_special_kernel (tta_class_rows / tta_class_stage): one workgroup per (image, class-list position), the class's rows
// gathered in list order and staged -- box, +1 area, list index -- in LDS, or in the class's own slice of a global workspace when it has
// more than `cap` rows.
// The sweep takes 256 rows at a time, one per thread:
//   a. every row is tested against the heads kept so far (a compact list, read at the same address by every lane; no barrier per head),
//   b. the four waves resolve their 64 rows one after the other: row j of the wave is final once rows 0 .. j - 1 are, and a kept j
//      suppresses the later lanes; the survivors are appended to the kept list in lane order (ballot prefix), then the later waves of
//      the chunk catch up on the appended heads.
// The kept list is compacted IN PLACE over the staged rows (kept head k <= its own row's slot, and every thread holds its row in
// registers from the top of the chunk); in the workspace path the first 6 * cap / 5 heads live in the idle LDS instead.
// Every decision is taken on final flags behind a barrier or inside one wave in lane order: no race decides an order.  The IoU is
// box_iou_area (box_iou.h), the one nms.hip's mask kernel evaluates.
#define TTA_NMS_WORDS 6                                    // 4-byte words staged per row: x1 y1 x2 y2 area index

__global__ __launch_bounds__(256) void tta_nms_kernel(const float* __restrict__ boxes_s, const int* __restrict__ labels_s,
                                                      const int* __restrict__ nvalid, const int* __restrict__ cls_rank,
                                                      unsigned char* __restrict__ keep, float* __restrict__ ws, int* __restrict__ nws, int N,
                                                      int L, float thresh, int cap) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float sp_s[];             // [TTA_NMS_WORDS][m] when the class fits, else kept heads [5][kc]
  __shared__ int cnt_s[2], wcnt[4], nk_s;
  const int b = blockIdx.y, c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = min(max(nvalid[b], 0), N);
  const long base = (long)b * N;
  for (long j = (long)n + c * 256 + tid; j < N; j += (long)L * 256) keep[base + j] = 0;   // rows past the list: not kept (the blocks of an image share them out)
  const int* lab = labels_s + base;
  if (c == 0)                                              // a label outside the class list (mq_tta_merge_prep leaves none): not kept
    for (int j = tid; j < n; j += 256)
      if (tta_cls_pos(cls_rank, L, lab[j]) < 0) keep[base + j] = 0;
  if (tid == 0) nk_s = 0;
  float* st;
  const int m = tta_class_rows<TTA_NMS_WORDS>(lab, cls_rank, L, n, c, cap, sp_s, ws, base, nws, cnt_s, st);
  if (m == 0) return;
  const bool in_lds = m <= cap;
  float *X1 = st, *Y1 = st + m, *X2 = st + 2 * (long)m, *Y2 = st + 3 * (long)m, *AR = st + 4 * (long)m;
  int* IDX = (int*)(st + 5 * (long)m);
  // kept heads: slot k < kc in K*, the rest in place in the staged arrays (the LDS path: all of them, K* == the staged arrays)
  const int kc = in_lds ? m : (cap * TTA_NMS_WORDS) / 5;
  float *K1 = in_lds ? X1 : sp_s, *K2 = in_lds ? Y1 : sp_s + kc, *K3 = in_lds ? X2 : sp_s + 2 * kc, *K4 = in_lds ? Y2 : sp_s + 3 * kc,
        *KA = in_lds ? AR : sp_s + 4 * kc;
  tta_class_stage(lab, cls_rank, L, n, c, wcnt, [&](int j, int k) {
    const float x1 = boxes_s[(base + j) * 4 + 0], y1 = boxes_s[(base + j) * 4 + 1], x2 = boxes_s[(base + j) * 4 + 2],
                y2 = boxes_s[(base + j) * 4 + 3];
    X1[k] = x1;
    Y1[k] = y1;
    X2[k] = x2;
    Y2[k] = y2;
    AR[k] = (x2 - x1 + 1.f) * (y2 - y1 + 1.f);
    IDX[k] = j;
  });

  int nk = 0;                                              // kept heads so far (the same in every thread)
  for (int r0 = 0; r0 < m; r0 += 256) {
    const int r = r0 + tid;
    const bool have = r < m;
    float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f, ar = 0.f;
    int idx = 0;
    if (have) x1 = X1[r], y1 = Y1[r], x2 = X2[r], y2 = Y2[r], ar = AR[r], idx = IDX[r];
    int alive = have, done = 0;                            // done: kept heads this row has been tested against
    for (int s = 0; s < 4; ++s) {
      if (wv >= s) {
        int k = done;
        const int k_lds = min(nk, kc);
        for (; alive && k < k_lds; ++k)
          if (box_iou_area(K1[k], K2[k], K3[k], K4[k], KA[k], x1, y1, x2, y2, ar) > thresh) alive = 0;
        for (k = max(k, kc); alive && k < nk; ++k)
          if (box_iou_area(X1[k], Y1[k], X2[k], Y2[k], AR[k], x1, y1, x2, y2, ar) > thresh) alive = 0;
        done = nk;
      }
      if (wv == s) {
        for (int j = 0; j < 64; ++j) {                     // row j of the wave is final here: rows 0 .. j - 1 have had their say
          const int aj = __shfl(alive, j);
          const float jx1 = __shfl(x1, j), jy1 = __shfl(y1, j), jx2 = __shfl(x2, j), jy2 = __shfl(y2, j), ja = __shfl(ar, j);
          if (aj && alive && lane > j && box_iou_area(jx1, jy1, jx2, jy2, ja, x1, y1, x2, y2, ar) > thresh) alive = 0;
        }
        const unsigned long long bal = __ballot(alive);
        if (have) keep[base + idx] = (unsigned char)alive;
        if (alive) {
          const int k = nk + __popcll(bal & ((1ull << lane) - 1ull));      // <= r: the slot of a row that is already in registers
          if (k < kc) K1[k] = x1, K2[k] = y1, K3[k] = x2, K4[k] = y2, KA[k] = ar;
          else X1[k] = x1, Y1[k] = y1, X2[k] = x2, Y2[k] = y2, AR[k] = ar;
        }
        if (lane == 0) nk_s = nk + __popcll(bal);
      }
      __syncthreads();
      nk = nk_s;
    }
  }
}

// The per-class NMS of the merge at any row count: boxes_s [B, N, 4] fp32 / labels_s [B, N] int32 / nvalid [B] int32 as mq_tta_merge_prep
// leaves them (score-sorted, every label l of a live row with 0 <= l < L and cls_rank[l] >= 0) -> keep [B, N] uint8, all of it written,
// byte for byte mq_ml_nms(boxes_s, labels_s, nvalid, thresh).  L = length of cls_rank; cap: rows of a class staged in LDS at most
// (1 .. 4096); a larger class works in ws [B, N, 6] fp32 (may be NULL when N <= cap) and is counted in nws [1] int32 (ZEROED by the
// caller).  N <= 2^24, B <= 65535.  -1: arguments out of range.
extern "C" int mq_tta_merge_nms(const float* boxes_s, const int* labels_s, const int* nvalid, const int* cls_rank, unsigned char* keep,
                                float* ws, int* nws, int B, int N, int L, float thresh, int cap, void* stream) {
  if (B <= 0 || N <= 0) return 0;
  if (B > 65535 || N > (1 << 24) || L <= 0 || L > (1 << 24) || !(thresh > 0.f) || cap < 1 || cap > TTA_SP_MAX_CAP) return -1;
  if (N > cap && !ws) return -1;
  const size_t smem = (size_t)(cap < N ? cap : N) * TTA_NMS_WORDS * sizeof(float);
  return mq_launch<tta_nms_kernel>(dim3(L, B), dim3(256), smem, (hipStream_t)stream, boxes_s, labels_s, nvalid, cls_rank, keep, ws, nws, N, L,
                                   thresh, cap);
}
#endif

MQ_NAMESPACE_END
