// Test-time augmentation (TEST.USE_MULTISCALE): the device image ingest and the device merge of the per-transform detections.
//
// mq_tta_ingest_fwd: B ragged RGB uint8 HWC images -> the fp32 NCHW zero-padded canvas of one scale, plain and (optionally) flipped, in one
// launch.  Resampling is PIL's uint8 BILINEAR resize, bit for bit (libImaging/Resample.c: two separable passes, horizontal first into a
// rounded and clamped uint8 intermediate, 22-bit fixed-point coefficients, accumulation from 1 << 21, clamp(acc >> 22, 0, 255)).  The
// coefficient tables are built on the host in float64 (mq_det_amd/tta.py: pil_coeffs); a pass PIL skips is an identity table (one tap of
// weight 1 << 22), which gives the same bytes.  The kernel does integer math only, then the fp32 ToTensor / Normalize of the reference.
//
// mq_tta_merge_*: box_aug.py merge_result_from_multi_scales with SPECIAL_NMS = 'none', after the per-transform un-flip / area band /
// rescale, as four launches around mq_ml_nms (post.hip).  Every sort is a rank by counting over a total order, so the result does not
// depend on the schedule.
#include "common.h"

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
#endif

MQ_NAMESPACE_END
