// The ATSS training objective of MQ-GLIP, evaluated forward-only on gfx950 (host side: mq_det_amd/losses.py).
//
// Reference: rpn/loss.py ATSSLossComputation.prepare_targets (:655-832) and __call__ (:850-1201) with USE_DOT_PRODUCT_TOKEN_LOSS and one
// anchor per location.  The reference loops over images in Python, builds dense [A, G] IoU and distance matrices, takes a topk per
// level, scatters into an [A G] vector, and then makes about ten element-wise passes over the materialised [B, A, 256] fp32 logits.
// Here:
//   mq_atss_assign_fwd       two launches.  (1) one workgroup per gt box: per level the min(TOPK, n) anchors nearest to the box centre are
//                            found by repeated "smallest key above the previous one" over the level (key = distance bits << 32 | anchor
//                            index, so a tie goes to the lower index and keys are unique), their IoUs give mean + unbiased std = the
//                            box's threshold; only the threshold and the k-th key per (gt, level) are written.  (2) one thread per
//                            (image, anchor) walks the image's gts in order: candidate iff key <= k-th key, IoU >= threshold, centre
//                            inside by more than 0.01; the highest IoU wins, a tie goes to the lower gt.  Keys and IoUs come from the same
//                            inline functions in both launches (no contraction), so both see the same bits.  No atomics, no [A G] tensor.
//   mq_atss_box_loss_fwd     one thread per (image, anchor): label, BoxCoder.encode target, centerness target; GIoU / centerness terms
//                            of the positives as per-workgroup partial sums, then one fixed-order pass over the partials.
//   mq_token_focal_loss_fwd  the dot-product token loss on the operands of mq_align_fused_fwd: a workgroup owns 128 pyramid tokens of one
//                            image (8 waves x 16 rows, A fragments in registers), the live text rows pass through LDS in chunks of 128
//                            (row pitch 264: conflict-free b128 fragment reads, align_fused.hip), v_mfma_f32_16x16x32 forms 16 x 16 logits
//                            per step and the epilogue turns them into focal-loss terms at once: + bias, clamp, target from the matched
//                            gt's positive-map row (background: 1 at the last column of the full caption), BCE-with-logits x (1 - p_t)^gamma
//                            x alpha_t, summed per lane, wave and workgroup.  The logits never reach memory.
// Every sum that reaches a result is: lanes in a fixed order, wave_sum's butterfly, the waves of a workgroup in order, then
// atss_reduce_kernel over the partials in a fixed order (fp64 accumulators).  No floating-point atomics: results are the same bits from run to run.
//
// What bounds them: (1) of the assignment is TOPK x levels passes of one workgroup over the anchors (L2 hits) with one barrier each --
// latency of 45 small reductions per gt, the gts in parallel; (2) and the box loss read every anchor once per image plus the image's gt
// list (wave-uniform loads); the token loss reads tok once (512 B per token) and is MFMA / transcendental bound: 2 exp-class and 1 log-class
// evaluation per live (token, text column) pair.
#include "common.h"

MQ_NAMESPACE_BEGIN

#define AL_THREADS 256
#define AL_WAVES (AL_THREADS / 64)
#define AL_MAXLVL 8
#define AL_MAXK 64                                          // largest ATSS.TOPK
#define AL_NSUM 5                                           // box-loss sums: positives, S ct, S ct (1 - GIoU), S BCE(ctr, ct), S (1 - GIoU)

// out[j] = sum_i partials[i * W + j], i in a fixed order: thread t takes i = t, t + 256, ... in fp64, then a fixed tree over the threads
__global__ __launch_bounds__(AL_THREADS) void atss_reduce_kernel(const float* __restrict__ partials, int n, int W, float* __restrict__ out) {
  __shared__ double red[AL_THREADS];
  const int tid = threadIdx.x;
  for (int j = 0; j < W; ++j) {
    double s = 0.0;
    for (int i = tid; i < n; i += AL_THREADS) s += (double)partials[(long)i * W + j];
    red[tid] = s;
    __syncthreads();
    for (int st = AL_THREADS / 2; st > 0; st >>= 1) {
      if (tid < st) red[tid] += red[tid + st];
      __syncthreads();
    }
    if (tid == 0) out[j] = (float)red[0];
    __syncthreads();
  }
}

#ifdef MQ_PRIMARY_UNIT                                      // fp32 / integer data only: one copy, in the fp16 translation unit

struct AtssLevels {
  int off[AL_MAXLVL + 1];
  int NL;
};

// boxlist_iou (structures/boxlist_ops.py:97-132, TO_REMOVE = 1), every operation rounded by itself
__device__ __forceinline__ float atss_iou(const float4_ a, const float4_ g) {
#pragma clang fp contract(off)
  const float area1 = (a[2] - a[0] + 1.f) * (a[3] - a[1] + 1.f);
  const float area2 = (g[2] - g[0] + 1.f) * (g[3] - g[1] + 1.f);
  const float w = fmaxf(fminf(a[2], g[2]) - fmaxf(a[0], g[0]) + 1.f, 0.f);
  const float h = fmaxf(fminf(a[3], g[3]) - fmaxf(a[1], g[1]) + 1.f, 0.f);
  const float inter = w * h;
  return inter / (area1 + area2 - inter);
}

// (squared centre distance, anchor index) as one ordered key: the square root of the reference is monotone, so the k nearest are the same set
__device__ __forceinline__ unsigned long long atss_key(const float4_ a, const float4_ g, int idx) {
#pragma clang fp contract(off)
  const float dx = (a[2] + a[0]) / 2.0f - (g[2] + g[0]) / 2.0f;
  const float dy = (a[3] + a[1]) / 2.0f - (g[3] + g[1]) / 2.0f;
  const float d2 = dx * dx + dy * dy;
  return ((unsigned long long)__builtin_bit_cast(unsigned, d2) << 32) | (unsigned)idx;
}

__device__ __forceinline__ unsigned long long atss_wave_min(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned hi = __shfl_xor((unsigned)(v >> 32), o), lo = __shfl_xor((unsigned)v, o);
    const unsigned long long w = ((unsigned long long)hi << 32) | lo;
    v = w < v ? w : v;
  }
  return v;
}

__global__ __launch_bounds__(AL_THREADS) void atss_thresh_kernel(const float* __restrict__ anchors, const float* __restrict__ gt, AtssLevels lv,
                                                                  int topk, float* __restrict__ thr, unsigned long long* __restrict__ kth) {
  __shared__ unsigned long long red[2][AL_WAVES];
  __shared__ int cand[AL_MAXLVL * AL_MAXK];
  __shared__ float ious[AL_MAXLVL * AL_MAXK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long q = blockIdx.x;
  const float4_ g = *(const float4_*)(gt + q * 4);
  int nc = 0, round = 0;                                    // uniform over the workgroup
  for (int l = 0; l < lv.NL; ++l) {
    const int lo = lv.off[l], n = lv.off[l + 1] - lo, k = topk < n ? topk : n;
    unsigned long long prev = 0;
    for (int j = 0; j < k; ++j, ++round) {
      unsigned long long best = ~0ull;                      // the smallest key above `prev` (keys are unique: the index is part of them)
      for (int i = tid; i < n; i += AL_THREADS) {
        const unsigned long long key = atss_key(*(const float4_*)(anchors + (long)(lo + i) * 4), g, lo + i);
        if ((j == 0 || key > prev) && key < best) best = key;
      }
      best = atss_wave_min(best);
      unsigned long long* r = red[round & 1];               // two buffers in turn: one barrier per round
      if (lane == 0) r[wave] = best;
      __syncthreads();
      best = r[0];
#pragma unroll
      for (int w = 1; w < AL_WAVES; ++w) best = r[w] < best ? r[w] : best;
      prev = best;
      if (tid == 0) cand[nc + j] = (int)(unsigned)(best & 0xffffffffull);
    }
    if (tid == 0) kth[q * lv.NL + l] = prev;
    nc += k;
  }
  __syncthreads();
  for (int i = tid; i < nc; i += AL_THREADS) ious[i] = atss_iou(*(const float4_*)(anchors + (long)cand[i] * 4), g);
  __syncthreads();
  if (tid == 0) {                                           // mean + unbiased std over <= 512 values, in order, fp64; each rounded to fp32 like the reference's
    double s = 0.0;
    for (int i = 0; i < nc; ++i) s += (double)ious[i];
    const double mean = nc > 0 ? s / nc : 0.0;
    double v = 0.0;
    for (int i = 0; i < nc; ++i) v += ((double)ious[i] - mean) * ((double)ious[i] - mean);
    const float sd = nc > 1 ? (float)sqrt(v / (nc - 1)) : __builtin_nanf("");      // torch.std of one value is NaN: nothing passes
    thr[q] = (float)mean + sd;
  }
}

__global__ __launch_bounds__(AL_THREADS) void atss_match_kernel(const float* __restrict__ anchors, const float* __restrict__ gt,
                                                                 const int* __restrict__ gt_off, AtssLevels lv, const float* __restrict__ thr,
                                                                 const unsigned long long* __restrict__ kth, int* __restrict__ matched, int A,
                                                                 int total_gt, int tiles) {
  const int b = blockIdx.x / tiles, i = (blockIdx.x - b * tiles) * AL_THREADS + threadIdx.x;
  if (i >= A) return;
  const float4_ a = *(const float4_*)(anchors + (long)i * 4);
  int l = 0;
#pragma unroll
  for (int k = 1; k < AL_MAXLVL; ++k) l += (k < lv.NL && i >= lv.off[k]);
  const float acx = (a[2] + a[0]) / 2.0f, acy = (a[3] + a[1]) / 2.0f;
  int g0 = gt_off[b], g1 = gt_off[b + 1];
  g0 = g0 < 0 ? 0 : g0;
  g1 = g1 > total_gt ? total_gt : g1;
  int best = -1;
  float best_iou = -1.0e8f;                                 // the reference's -INF
  for (int q = g0; q < g1; ++q) {
    const float4_ g = *(const float4_*)(gt + (long)q * 4);
    if (atss_key(a, g, i) > kth[(long)q * lv.NL + l]) continue;
    const float iou = atss_iou(a, g);
    if (!(iou >= thr[q])) continue;
    const float m = fminf(fminf(acx - g[0], acy - g[1]), fminf(g[2] - acx, g[3] - acy));
    if (!(m > 0.01f)) continue;
    if (iou > best_iou) {                                   // strict: a tie stays with the lower gt
      best_iou = iou;
      best = q - g0;
    }
  }
  matched[(long)b * A + i] = best;
}

static int atss_levels(const int* lvl_off, int NL, int A, AtssLevels& lv) {
  if (NL < 1 || NL > AL_MAXLVL) return -1;
  for (int i = 0; i <= AL_MAXLVL; ++i) lv.off[i] = lvl_off[i < NL ? i : NL];
  lv.NL = NL;
  if (lv.off[0] != 0 || lv.off[NL] != A) return -1;
  for (int i = 0; i < NL; ++i)
    if (lv.off[i + 1] < lv.off[i]) return -1;
  return 0;
}

extern "C" int mq_atss_assign_fwd(const float* anchors, const int* lvl_off, const float* gt, const int* gt_off, float* thr, long long* kth,
                                  int* matched, int B, int A, int NL, int total_gt, int topk, void* stream) {
  if (B <= 0 || A <= 0) return 0;
  AtssLevels lv;
  if (total_gt < 0 || topk < 1 || topk > AL_MAXK || atss_levels(lvl_off, NL, A, lv)) return -1;
  const hipStream_t st = (hipStream_t)stream;
  if (total_gt > 0) {
    const int rc = mq_launch<atss_thresh_kernel>(dim3((unsigned)total_gt), dim3(AL_THREADS), 0, st, anchors, gt, lv, topk, thr,
                                                 (unsigned long long*)kth);
    if (rc) return rc;
  }
  const int tiles = (A + AL_THREADS - 1) / AL_THREADS;
  if ((long)B * tiles > 0x7fffffffL) return -1;
  return mq_launch<atss_match_kernel>(dim3((unsigned)(B * tiles)), dim3(AL_THREADS), 0, st, anchors, gt, gt_off, lv, (const float*)thr,
                                      (const unsigned long long*)kth, matched, A, total_gt, tiles);
}

// BoxCoder(10, 10, 5, 5), TO_REMOVE = 1 (modeling/box_coder.py), in the reference's order of operations
__device__ __forceinline__ float4_ atss_encode(const float4_ g, const float4_ a) {
#pragma clang fp contract(off)
  const float ew = a[2] - a[0] + 1.f, eh = a[3] - a[1] + 1.f, ex = a[0] + 0.5f * ew, ey = a[1] + 0.5f * eh;
  const float gw = g[2] - g[0] + 1.f, gh = g[3] - g[1] + 1.f, gx = g[0] + 0.5f * gw, gy = g[1] + 0.5f * gh;
  return (float4_){10.f * (gx - ex) / ew, 10.f * (gy - ey) / eh, 5.f * logf(gw / ew), 5.f * logf(gh / eh)};
}
__device__ __forceinline__ float4_ atss_decode(const float4_ c, const float4_ a) {
#pragma clang fp contract(off)
  const float w = a[2] - a[0] + 1.f, h = a[3] - a[1] + 1.f, cx = a[0] + 0.5f * w, cy = a[1] + 0.5f * h;
  const float clip = 4.135166556742356f;                    // log(1000 / 16)
  const float dx = c[0] / 10.f, dy = c[1] / 10.f, dw = fminf(c[2] / 5.f, clip), dh = fminf(c[3] / 5.f, clip);
  const float px = dx * w + cx, py = dy * h + cy, pw = expf(dw) * w, ph = expf(dh) * h;
  return (float4_){px - 0.5f * pw, py - 0.5f * ph, px + 0.5f * pw - 1.f, py + 0.5f * ph - 1.f};
}

__global__ __launch_bounds__(AL_THREADS) void atss_box_loss_kernel(const float* __restrict__ anchors, const float* __restrict__ gt,
                                                                    const long long* __restrict__ labels, const int* __restrict__ gt_off,
                                                                    const int* __restrict__ matched, const float* __restrict__ reg,
                                                                    const float* __restrict__ ctr, long long* __restrict__ cls_out,
                                                                    float* __restrict__ reg_out, float* __restrict__ partials, int A,
                                                                    int total_gt, int tiles) {
  __shared__ float red[AL_WAVES][AL_NSUM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / tiles, i = (blockIdx.x - b * tiles) * AL_THREADS + tid;
  float s[AL_NSUM] = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (i < A) {
    const long o = (long)b * A + i;
    const float4_ a = *(const float4_*)(anchors + (long)i * 4);
    int g0 = gt_off[b], g1 = gt_off[b + 1];
    g0 = g0 < 0 ? 0 : g0;
    g1 = g1 > total_gt ? total_gt : g1;
    const int m = matched[o];
    const bool hit = m >= 0 && m < g1 - g0;
    const long long label = hit ? labels[g0 + m] : 0;
    // a background anchor carries the encoding of the image's FIRST gt, as the reference's max over a row of -INF returns index 0
    float4_ t = {0.f, 0.f, 0.f, 0.f};
    if (g1 > g0) t = atss_encode(*(const float4_*)(gt + (long)(g0 + (hit ? m : 0)) * 4), a);
    if (cls_out) cls_out[o] = label;
    if (reg_out) *(float4_*)(reg_out + o * 4) = t;
    if (reg && label > 0) {
      const float acx = (a[2] + a[0]) / 2.0f, acy = (a[3] + a[1]) / 2.0f;
      const float4_ tb = atss_decode(t, a);
      const float l_ = acx - tb[0], t_ = acy - tb[1], r_ = tb[2] - acx, b_ = tb[3] - acy;
      const float ct = sqrtf((fminf(l_, r_) / fmaxf(l_, r_)) * (fminf(t_, b_) / fmaxf(t_, b_)));
      float4_ pb = atss_decode(*(const float4_*)(reg + o * 4), a);
      pb[2] = fmaxf(pb[0], pb[2]);
      pb[3] = fmaxf(pb[1], pb[3]);
      const float pa = (pb[2] - pb[0]) * (pb[3] - pb[1]), ta = (tb[2] - tb[0]) * (tb[3] - tb[1]);
      const float ix1 = fmaxf(pb[0], tb[0]), iy1 = fmaxf(pb[1], tb[1]), ix2 = fminf(pb[2], tb[2]), iy2 = fminf(pb[3], tb[3]);
      const float inter = (iy2 > iy1 && ix2 > ix1) ? (ix2 - ix1) * (iy2 - iy1) : 0.f;
      const float ea = (fmaxf(pb[2], tb[2]) - fminf(pb[0], tb[0])) * (fmaxf(pb[3], tb[3]) - fminf(pb[1], tb[1])) + 1e-7f;
      const float un = pa + ta - inter + 1e-7f;
      const float gl = 1.f - (inter / un - (ea - un) / ea);
      const float x = ctr[o];
      s[0] = 1.f;
      s[1] = ct;
      s[2] = gl * ct;
      s[3] = fmaxf(x, 0.f) - x * ct + log1pf(expf(-fabsf(x)));
      s[4] = gl;
    }
  }
  if (!partials) return;                                    // uniform
#pragma unroll
  for (int j = 0; j < AL_NSUM; ++j) {
    const float v = wave_sum(s[j]);
    if (lane == 0) red[wave][j] = v;
  }
  __syncthreads();
  if (tid < AL_NSUM) {
    float v = red[0][tid];
#pragma unroll
    for (int w = 1; w < AL_WAVES; ++w) v += red[w][tid];
    partials[(long)blockIdx.x * AL_NSUM + tid] = v;
  }
}

extern "C" int mq_atss_box_loss_fwd(const float* anchors, const float* gt, const long long* labels, const int* gt_off, const int* matched,
                                    const float* reg, const float* ctr, long long* cls_out, float* reg_out, float* partials, float* sums,
                                    int B, int A, int total_gt, void* stream) {
  if (B <= 0 || A <= 0) return 0;
  if (total_gt < 0 || (reg != nullptr) != (ctr != nullptr) || (reg != nullptr) != (partials != nullptr) || (reg != nullptr) != (sums != nullptr))
    return -1;
  const int tiles = (A + AL_THREADS - 1) / AL_THREADS;
  if ((long)B * tiles > 0x7fffffffL) return -1;
  const hipStream_t st = (hipStream_t)stream;
  const int rc = mq_launch<atss_box_loss_kernel>(dim3((unsigned)(B * tiles)), dim3(AL_THREADS), 0, st, anchors, gt, labels, gt_off, matched, reg,
                                                 ctr, cls_out, reg_out, partials, A, total_gt, tiles);
  if (rc || !partials) return rc;
  return mq_launch<atss_reduce_kernel>(dim3(1), dim3(AL_THREADS), 0, st, (const float*)partials, B * tiles, AL_NSUM, sums);
}

#endif  // MQ_PRIMARY_UNIT

// ---------------------------------------------------------------------------------------------- dot-product token focal loss
constexpr int TF_C = 256, TF_KS = TF_C / 32, TF_PITCH = TF_C + 8, TF_NW = 8, TF_BM = 16 * TF_NW, TF_CH = 8;

struct TokenFocalParams {
  const half_t* tok;        // [B, N, 256]
  const half_t* tk;         // [B, T, 256]   projected text tokens / exp(log_scale)
  const float* tbias;       // [B, T]
  const int* matched;       // [B, N]        gt of the anchor inside its image, -1 background
  const float* posmap;      // [total_gt, Tpm]
  const int* gt_off;        // [B + 1]
  const int* mask;          // [B, T]        > 0: the text column counts
  float* partials;          // [B * tiles]
  int B, N, T, TL, Tpm, total_gt;
  float alpha, gamma;
};

// token_sigmoid_binary_focal_loss (layers/sigmoid_focal_loss.py:130-171) of one element
__device__ __forceinline__ float token_focal_term(float x, float t, float alpha, float gamma) {
  const float e = expf(-fabsf(x));
  const float ce = fmaxf(x, 0.f) - x * t + log1pf(e);
  const float p = (x >= 0.f ? 1.f : e) / (1.f + e);
  const float om = 1.f - (p * t + (1.f - p) * (1.f - t));
  float loss = ce * (gamma == 2.f ? om * om : powf(fmaxf(om, 0.f), gamma));
  if (alpha >= 0.f) loss *= alpha * t + (1.f - alpha) * (1.f - t);
  return loss;
}

__global__ __launch_bounds__(64 * TF_NW) void token_focal_kernel(TokenFocalParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  half_t* ts = (half_t*)smem;                                 // [16 TF_CH][TF_PITCH]: one chunk of live text rows
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tiles = (p.N + TF_BM - 1) / TF_BM;
  const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const int row0 = tile * TF_BM + wave * 16;                  // this wave's 16 tokens (rows >= N: clamped loads, no terms)
  const int nb = p.TL >> 4;                                   // live 16-column blocks of text tokens

  half8 a[TF_KS];
  {
    const long r = min(row0 + l15, p.N - 1);
    const half_t* src = p.tok + ((long)b * p.N + r) * TF_C + g * 8;
#pragma unroll
    for (int ks = 0; ks < TF_KS; ++ks) a[ks] = *(const half8*)(src + ks * 32);
  }
  // the lane's four accumulator rows 4 g + r: the positive-map row of the matched gt, or background
  const float* prow[4];
  bool valid[4];
  {
    int g0 = p.gt_off[b], g1 = p.gt_off[b + 1];
    g0 = g0 < 0 ? 0 : g0;
    g1 = g1 > p.total_gt ? p.total_gt : g1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = row0 + 4 * g + r;
      valid[r] = n < p.N;
      const int m = valid[r] ? p.matched[(long)b * p.N + n] : -1;
      prow[r] = (m >= 0 && m < g1 - g0) ? p.posmap + (long)(g0 + m) * p.Tpm : nullptr;
    }
  }
  const half_t* tkb = p.tk + (long)b * p.T * TF_C;
  const float* tb = p.tbias + (long)b * p.T;
  const int* mk = p.mask + (long)b * p.T;
  float sum = 0.f;
  for (int c0 = 0; c0 < nb; c0 += TF_CH) {
    const int nbc = nb - c0 < TF_CH ? nb - c0 : TF_CH;
    if (c0) __syncthreads();                                  // every wave is done with the previous chunk
    const int pieces = nbc * 16 * (TF_C / 8);
    for (int i = tid; i < pieces; i += 64 * TF_NW) {
      const int r = i >> 5, c8 = i & 31;
      *(half8*)(ts + r * TF_PITCH + c8 * 8) = *(const half8*)(tkb + (long)min(c0 * 16 + r, p.T - 1) * TF_C + c8 * 8);
    }
    __syncthreads();
#pragma unroll
    for (int cb = 0; cb < TF_CH; ++cb) {
      if (cb < nbc) {
        float4_ acc = {0.f, 0.f, 0.f, 0.f};
        const half_t* bp = ts + (cb * 16 + l15) * TF_PITCH + g * 8;
#pragma unroll
        for (int ks = 0; ks < TF_KS; ++ks) acc = mfma16(a[ks], *(const half8*)(bp + ks * 32), acc);
        // lane holds logits[row = 4 g + r][col]
        const int col = (c0 + cb) * 16 + l15;
        if (col < p.T && mk[col] > 0) {
          const float bias = tb[col];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (valid[r]) {
              const float v = fminf(fmaxf(acc[r] + bias, -50000.f), 50000.f);
              const float t = prow[r] ? (col < p.Tpm ? prow[r][col] : 0.f) : (col == p.Tpm - 1 ? 1.f : 0.f);
              sum += token_focal_term(v, t, p.alpha, p.gamma);
            }
          }
        }
      }
    }
  }
  __syncthreads();                                            // the text tile is no longer read: its first bytes carry the wave sums
  float* red = (float*)smem;
  sum = wave_sum(sum);
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  if (tid == 0) {
    float v = red[0];
#pragma unroll
    for (int w = 1; w < TF_NW; ++w) v += red[w];
    p.partials[blockIdx.x] = v;
  }
}

// see include/mqdet_hip.h
extern "C" int MQ_SYM(mq_token_focal_loss_fwd)(const void* tok, const void* tk, const float* tbias, const int* matched, const float* posmap,
                                               const int* gt_off, const int* text_mask, float* partials, float* loss, int B, int N, int T,
                                               int kv_max, int Tpm, int total_gt, float alpha, float gamma, void* stream) {
  if (B <= 0 || N <= 0) return 0;
  if (T <= 0 || Tpm <= 0 || total_gt < 0) return -1;
  TokenFocalParams p;
  p.tok = (const half_t*)tok; p.tk = (const half_t*)tk; p.tbias = tbias; p.matched = matched; p.posmap = posmap; p.gt_off = gt_off;
  p.mask = text_mask; p.partials = partials;
  const int live = (kv_max > 0 && kv_max < T) ? kv_max : T;
  p.B = B; p.N = N; p.T = T; p.TL = (live + 15) / 16 * 16; p.Tpm = Tpm; p.total_gt = total_gt; p.alpha = alpha; p.gamma = gamma;
  const int tiles = (N + TF_BM - 1) / TF_BM;
  if ((long)B * tiles > 0x7fffffffL) return -1;
  const int rows = (p.TL < 16 * TF_CH ? p.TL : 16 * TF_CH);
  const size_t smem = (size_t)rows * TF_PITCH * sizeof(half_t);
  const hipStream_t st = (hipStream_t)stream;
  const int rc = mq_launch<token_focal_kernel>(dim3((unsigned)(B * tiles)), dim3(64 * TF_NW), smem, st, p);
  if (rc) return rc;
  return mq_launch<atss_reduce_kernel>(dim3(1), dim3(AL_THREADS), 0, st, (const float*)partials, B * tiles, 1, loss);
}

MQ_NAMESPACE_END
