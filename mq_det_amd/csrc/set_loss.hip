// The set criterion of MQ-GroundingDINO, evaluated forward-only on gfx950 (host side: mq_det_amd/set_loss.py).
//
// Reference: groundingdino_new/models/GroundingDINO/matcher.py HungarianMatcher.forward (:49-86) and loss.py SetCriterion.loss_labels /
// loss_boxes (:42-91).  The reference builds a dense [B nq, sum G] cost over the whole batch, copies it to the host and runs scipy's
// linear_sum_assignment per image, once per decoder layer.  Here every decoder layer and image is handled in the same three launches:
//   mq_set_cost_fwd    a workgroup owns 64 queries of one (layer, image): the focal class term pos - neg is formed ONCE per (query, token)
//                      into LDS (token-major, pitch 65: the transposing write and the per-query read are both conflict-free), then each wave
//                      walks the image's gts: the gt's positive tokens come from a ballot over its positive-map row, a lane (= query) adds
//                      its LDS column entries of those tokens, + L1 + GIoU, and writes one 256-byte piece of the gt-major cost row.
//   mq_hungarian_fwd   one problem per single-wave workgroup: the shortest-augmenting-path algorithm of Crouse (what scipy's
//                      linear_sum_assignment implements), rows = gts.  Lane l owns the columns l, l + 64, ...: their path costs and duals
//                      are fp64 REGISTERS (16 columns a lane: nq <= 1024); the row duals and the three index arrays are 20 KB of LDS.  A
//                      step = one cost-row read + one (value, column) argmin by xor-shuffles, a tie to the lower column.  Every loop is
//                      counted (rows < G, steps <= row + 1, augmentation <= row + 1), a column index is range-checked before it is used,
//                      and a problem that reads a non-finite entry gives up: -1 for all its gts.
//   mq_set_loss_fwd    one wave per (layer, image, query) row: token focal terms over the live text columns, L1 and 1 - GIoU of a matched
//                      query; per-workgroup partials, then one fixed-order fp64 tree per layer.  No floating-point atomics anywhere: results are the
//                      same bits from run to run.
//
// What bounds them: the cost kernel evaluates 1 exp + 2 log per (query, token) and then reads LDS once per (query, gt, positive token); the
// solver is latency: per step <= 16 dependent-free L2 loads per lane, ~10 fp64 operations per column and 6 shuffle rounds of 12 bytes, in a
// chain of at most G (G + 1) / 2 steps per problem, the L B problems side by side; the loss kernel reads every logit once.
#include "common.h"

MQ_NAMESPACE_BEGIN

#ifdef MQ_PRIMARY_UNIT                                      // fp32 / integer data only: one copy, in the fp16 translation unit

#define SL_THREADS 256
#define SL_WAVES (SL_THREADS / 64)
#define SL_MAXQ 1024                                        // queries the solver takes: 16 columns per lane
#define SL_KMAX (SL_MAXQ / 64)
#define SL_TQ 64                                            // queries per workgroup of the cost kernel
#define SL_PITCH (SL_TQ + 1)
#define SL_MAXT 512                                         // text positions of the logits the cost kernel takes (LDS: T x 65 floats)
#define SL_ROWS 16                                          // (image, query) rows per workgroup of the loss kernel

// pos_cost_class - neg_cost_class of one logit (matcher.py:52-64, gamma = 2); x = -inf: p = 0, alpha (-log 1e-8)
__device__ __forceinline__ float set_class_term(float x, float alpha) {
  const float p = 1.f / (1.f + expf(-x));
  const float neg = (1.f - alpha) * (p * p) * (-logf(1.f - p + 1e-8f));
  const float pos = alpha * ((1.f - p) * (1.f - p)) * (-logf(p + 1e-8f));
  return pos - neg;
}

struct SetBox {
  float x0, y0, x1, y1, area;
};
__device__ __forceinline__ SetBox set_xyxy(const float4_ c) {
  SetBox o;
  o.x0 = c[0] - 0.5f * c[2]; o.y0 = c[1] - 0.5f * c[3]; o.x1 = c[0] + 0.5f * c[2]; o.y1 = c[1] + 0.5f * c[3];
  o.area = (o.x1 - o.x0) * (o.y1 - o.y0);
  return o;
}
// util/box_ops.py generalized_box_iou of one pair (its two 1e-6 terms)
__device__ __forceinline__ float set_giou(const SetBox a, const SetBox g) {
  const float iw = fmaxf(fminf(a.x1, g.x1) - fmaxf(a.x0, g.x0), 0.f), ih = fmaxf(fminf(a.y1, g.y1) - fmaxf(a.y0, g.y0), 0.f);
  const float inter = iw * ih, uni = a.area + g.area - inter;
  const float ew = fmaxf(fmaxf(a.x1, g.x1) - fminf(a.x0, g.x0), 0.f), eh = fmaxf(fmaxf(a.y1, g.y1) - fminf(a.y0, g.y0), 0.f);
  const float enc = ew * eh;
  return inter / (uni + 1e-6f) - (enc - uni) / (enc + 1e-6f);
}
__device__ __forceinline__ float set_l1(const float4_ a, const float4_ g) {
  return fabsf(a[0] - g[0]) + fabsf(a[1] - g[1]) + fabsf(a[2] - g[2]) + fabsf(a[3] - g[3]);
}
// the image's gt rows, clamped into the packed arrays
__device__ __forceinline__ void set_gt_range(const int* __restrict__ gt_off, int b, int total_gt, int& g0, int& g1) {
  g0 = gt_off[b];
  g1 = gt_off[b + 1];
  g0 = g0 < 0 ? 0 : (g0 > total_gt ? total_gt : g0);
  g1 = g1 < g0 ? g0 : (g1 > total_gt ? total_gt : g1);
}

__global__ __launch_bounds__(SL_THREADS) void set_cost_kernel(const float* __restrict__ logits, const float* __restrict__ boxes,
                                                              const float* __restrict__ gt, const float* __restrict__ posmap,
                                                              const int* __restrict__ gt_off, float* __restrict__ cost, int B, int nq, int T,
                                                              int Tpm, int total_gt, int tiles, float wc, float wb, float wg, float alpha) {
  extern __shared__ __attribute__((aligned(16))) float dcls[];   // [T][SL_PITCH]: pos - neg of (token, query of the tile)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lb = blockIdx.x / tiles, q0 = (blockIdx.x - lb * tiles) * SL_TQ;
  const int l = lb / B, b = lb - l * B;
  int g0, g1;
  set_gt_range(gt_off, b, total_gt, g0, g1);
  if (g1 == g0) return;                                     // uniform over the workgroup
  const int nqt = nq - q0 < SL_TQ ? nq - q0 : SL_TQ;
  const float* lg = logits + ((long)lb * nq + q0) * T;
  for (int i = tid; i < SL_TQ * T; i += SL_THREADS) {
    const int qq = i / T, t = i - qq * T;
    dcls[t * SL_PITCH + qq] = qq < nqt ? set_class_term(lg[i], alpha) : 0.f;
  }
  __syncthreads();
  const int q = q0 + lane;
  const bool live = q < nq;
  const float4_ qb = *(const float4_*)(boxes + ((long)lb * nq + (live ? q : nq - 1)) * 4);
  const SetBox qx = set_xyxy(qb);
  const float absent = set_class_term(-__builtin_inff(), alpha);      // a positive token the head did not compute: p = 0
  for (int g = g0 + wave; g < g1; g += SL_WAVES) {
    const float* prow = posmap + (long)g * Tpm;
    float sum = 0.f;
    int n = 0;
    for (int c0 = 0; c0 < Tpm; c0 += 64) {
      const int t = c0 + lane;
      unsigned long long m = __ballot(t < Tpm && prow[t] > 0.f);
      const int cnt = __popcll(m);
      n += cnt;
      for (int i = 0; i < cnt; ++i) {
        const int tt = c0 + __ffsll(m) - 1;
        m &= m - 1;
        sum += tt < T ? dcls[tt * SL_PITCH + lane] : absent;
      }
    }
    const float4_ gb = *(const float4_*)(gt + (long)g * 4);
    const float c = wb * set_l1(qb, gb) + wc * (sum / (float)n) + wg * (-set_giou(qx, set_xyxy(gb)));   // no positive token: NaN, as the reference's empty mean
    if (live) cost[((long)l * total_gt + g) * nq + q] = c;
  }
}

extern "C" int mq_set_cost_fwd(const float* logits, const float* boxes, const float* gt, const float* posmap, const int* gt_off, float* cost,
                               int L, int B, int nq, int T, int Tpm, int total_gt, float cost_class, float cost_bbox, float cost_giou,
                               float focal_alpha, void* stream) {
  if (nq <= 0 || T <= 0 || T > SL_MAXT || Tpm < T || total_gt < 0) return -1;
  if (L <= 0 || B <= 0 || total_gt == 0) return 0;
  const int tiles = (nq + SL_TQ - 1) / SL_TQ;
  if ((long)L * B * tiles > 0x7fffffffL) return -1;
  return mq_launch<set_cost_kernel>(dim3((unsigned)(L * B * tiles)), dim3(SL_THREADS), (size_t)T * SL_PITCH * sizeof(float), (hipStream_t)stream,
                                    logits, boxes, gt, posmap, gt_off, cost, B, nq, T, Tpm, total_gt, tiles, cost_class, cost_bbox, cost_giou,
                                    focal_alpha);
}

// ---------------------------------------------------------------------------------------------- rectangular linear sum assignment
struct SetBest {
  double v;
  int j;
};
// (value, column) minimum over the wave, a tie to the lower column
__device__ __forceinline__ SetBest set_wave_argmin(SetBest a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(a.v, o);
    const int oj = __shfl_xor(a.j, o);
    if (ov < a.v || (ov == a.v && oj < a.j)) {
      a.v = ov;
      a.j = oj;
    }
  }
  return a;
}

__global__ __launch_bounds__(64) void set_hungarian_kernel(const float* __restrict__ cost, const int* __restrict__ gt_off,
                                                           int* __restrict__ match_q, int* __restrict__ q2g, int B, int nq, int total_gt) {
  __shared__ double u[SL_MAXQ];                             // row (gt) duals
  __shared__ int row4col[SL_MAXQ], col4row[SL_MAXQ], path[SL_MAXQ];
  const int lane = threadIdx.x;
  const int l = blockIdx.x / B, b = blockIdx.x - l * B;
  int g0, g1;
  set_gt_range(gt_off, b, total_gt, g0, g1);
  const int G = g1 - g0, kmax = (nq + 63) >> 6;
  const float* C = cost + ((long)l * total_gt + g0) * nq;
  const double inf = (double)__builtin_inff();
  bool ok = G <= nq;                                        // uniform over the wave, like every branch below that holds a cross-lane operation
  double v[SL_KMAX];                                        // column duals of the lane's columns lane + 64 k
#pragma unroll
  for (int k = 0; k < SL_KMAX; ++k) {
    v[k] = 0.0;
    const int j = lane + 64 * k;
    if (j < nq) {
      row4col[j] = -1;
      col4row[j] = -1;
      path[j] = -1;
      u[j] = 0.0;
    }
  }
  __syncthreads();
  for (int row = 0; row < G && ok; ++row) {
    double sh[SL_KMAX];                                     // shortest path cost to each of the lane's columns
#pragma unroll
    for (int k = 0; k < SL_KMAX; ++k) sh[k] = inf;
    unsigned sc = 0;                                        // bit k: column lane + 64 k is in the tree
    double minval = 0.0;
    int i = row, sink = -1;
    for (int step = 0; step <= row && sink < 0; ++step) {   // a step adds one column to the tree: at most `row` assigned ones, then a free one
      const double ui = u[i];
      const float* cr = C + (long)i * nq;
      SetBest best = {inf, 0x7fffffff};
      bool bad = false;
#pragma unroll
      for (int k = 0; k < SL_KMAX; ++k) {
        const int j = lane + 64 * k;
        if (k < kmax && j < nq && !((sc >> k) & 1u)) {
          const float c = cr[j];
          bad |= !(fabsf(c) <= 3.4028235e38f);
          const double r = minval + (double)c - ui - v[k];
          if (r < sh[k]) {
            sh[k] = r;
            path[j] = i;
          }
          if (sh[k] < best.v) {                             // k ascending: a tie inside the lane stays with the lower column
            best.v = sh[k];
            best.j = j;
          }
        }
      }
      best = set_wave_argmin(best);
      if (__any(bad) || best.j >= nq) {                     // a non-finite entry, or no reachable column: give up before `j` is used
        ok = false;
        break;
      }
      minval = best.v;
      const int j = best.j;
      if (lane == (j & 63)) sc |= 1u << (j >> 6);
      const int r4 = row4col[j];
      if (r4 < 0) sink = j;
      else i = r4;
    }
    if (sink < 0) ok = false;
    if (!ok) break;
    // duals: the rows of the tree other than `row` are the rows the tree's assigned columns belong to
#pragma unroll
    for (int k = 0; k < SL_KMAX; ++k) {
      if ((sc >> k) & 1u) {
        const double d = minval - sh[k];
        v[k] -= d;
        const int r4 = row4col[lane + 64 * k];
        if (r4 >= 0) u[r4] += d;
      }
    }
    if (lane == 0) u[row] += minval;
    __syncthreads();                                        // `path` of this row is complete
    if (lane == 0) {                                        // augment along the path: at most row + 1 edges
      int j = sink;
      for (int s = 0; s <= row; ++s) {
        const int pi = path[j];
        if ((unsigned)pi >= (unsigned)G) break;
        row4col[j] = pi;
        const int t = col4row[pi];
        col4row[pi] = j;
        if (pi == row || (unsigned)t >= (unsigned)nq) break;
        j = t;
      }
    }
    __syncthreads();
  }
  __syncthreads();
  int* qg = q2g + ((long)l * B + b) * nq;
#pragma unroll
  for (int k = 0; k < SL_KMAX; ++k) {
    const int j = lane + 64 * k;
    if (j < nq) qg[j] = ok ? row4col[j] : -1;
  }
  int* mq = match_q + (long)l * total_gt + g0;
  for (int r = lane; r < G; r += 64) mq[r] = ok ? col4row[r] : -1;
}

extern "C" int mq_hungarian_fwd(const float* cost, const int* gt_off, int* match_q, int* q2g, int L, int B, int nq, int total_gt, int max_gt,
                                void* stream) {
  if (L <= 0 || B <= 0) return 0;
  if (nq <= 0 || total_gt < 0 || max_gt < 0) return -1;
  if (nq > SL_MAXQ) return -2;
  if (max_gt > nq) return -3;
  if ((long)L * B > 0x7fffffffL) return -1;
  return mq_launch<set_hungarian_kernel>(dim3((unsigned)(L * B)), dim3(64), 0, (hipStream_t)stream, cost, gt_off, match_q, q2g, B, nq, total_gt);
}

// ---------------------------------------------------------------------------------------------- loss sums
// token_sigmoid_binary_focal_loss (layers/sigmoid_focal_loss.py:130-171) of one element, as csrc/atss_loss.hip evaluates it
__device__ __forceinline__ float set_focal_term(float x, float t, float alpha, float gamma) {
  const float e = expf(-fabsf(x));
  const float ce = fmaxf(x, 0.f) - x * t + log1pf(e);
  const float p = (x >= 0.f ? 1.f : e) / (1.f + e);
  const float om = 1.f - (p * t + (1.f - p) * (1.f - t));
  float loss = ce * (gamma == 2.f ? om * om : powf(fmaxf(om, 0.f), gamma));
  if (alpha >= 0.f) loss *= alpha * t + (1.f - alpha) * (1.f - t);
  return loss;
}

__global__ __launch_bounds__(SL_THREADS) void set_loss_kernel(const float* __restrict__ logits, const float* __restrict__ boxes,
                                                              const float* __restrict__ gt, const float* __restrict__ posmap,
                                                              const int* __restrict__ gt_off, const int* __restrict__ mask,
                                                              const int* __restrict__ q2g, const int* __restrict__ match_q,
                                                              float* __restrict__ partials, int B, int nq, int T, int Tpm, int total_gt,
                                                              int tiles, float alpha, float gamma) {
  __shared__ float red[SL_WAVES][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l = blockIdx.x / tiles, tile = blockIdx.x - l * tiles;
  const long rows = (long)B * nq;
  float s[3] = {0.f, 0.f, 0.f};
  for (int rr = 0; rr < SL_ROWS / SL_WAVES; ++rr) {
    const long r = (long)tile * SL_ROWS + wave * (SL_ROWS / SL_WAVES) + rr;          // (image, query), uniform over the wave
    if (r >= rows) break;
    const int b = (int)(r / nq);
    int g0, g1;
    set_gt_range(gt_off, b, total_gt, g0, g1);
    const long row = (long)l * rows + r;
    const int m = q2g[row];
    const bool hit = m >= 0 && m < g1 - g0;
    const float* prow = posmap + (long)(g0 + (hit ? m : 0)) * Tpm;
    // a matched query whose positive-map row is empty gets the background target too (loss.py:60)
    bool pos = false;
    if (hit) {
      for (int t = lane; t < Tpm; t += 64) pos |= prow[t] > 0.f;
      pos = __any(pos);
    }
    const float* x = logits + row * T;
    const int* mk = mask + (long)b * T;
    for (int t = lane; t < T; t += 64) {
      if (mk[t] > 0) {                                      // a masked column is skipped before any arithmetic: its logit is -inf
        const float tg = pos ? (prow[t] > 0.f ? 1.f : 0.f) : (t == Tpm - 1 ? 1.f : 0.f);
        s[0] += set_focal_term(x[t], tg, alpha, gamma);
      }
    }
    if (lane == 0) {
      if (hit) {
        const float4_ qb = *(const float4_*)(boxes + row * 4), gb = *(const float4_*)(gt + (long)(g0 + m) * 4);
        s[1] += set_l1(qb, gb);
        s[2] += 1.f - set_giou(set_xyxy(qb), set_xyxy(gb));
      }
      if (g1 > g0 && match_q[(long)l * total_gt + g0] < 0) {            // the solver gave this problem up: the failure shows in the sums
        s[0] = s[1] = s[2] = __builtin_nanf("");
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float w = wave_sum(s[j]);
    if (lane == 0) red[wave][j] = w;
  }
  __syncthreads();
  if (tid < 3) {
    float w = red[0][tid];
#pragma unroll
    for (int k = 1; k < SL_WAVES; ++k) w += red[k][tid];
    partials[(long)blockIdx.x * 3 + tid] = w;
  }
}

// sums[l][j] = sum_i partials[l][i][j], as atss_reduce_kernel orders it: thread t takes i = t, t + 256, ... in fp64, then a fixed tree
__global__ __launch_bounds__(SL_THREADS) void set_reduce_kernel(const float* __restrict__ partials, int n, float* __restrict__ out) {
  __shared__ double red[SL_THREADS];
  const int tid = threadIdx.x;
  const float* p = partials + (long)blockIdx.x * n * 3;
  for (int j = 0; j < 3; ++j) {
    double s = 0.0;
    for (int i = tid; i < n; i += SL_THREADS) s += (double)p[(long)i * 3 + j];
    red[tid] = s;
    __syncthreads();
    for (int st = SL_THREADS / 2; st > 0; st >>= 1) {
      if (tid < st) red[tid] += red[tid + st];
      __syncthreads();
    }
    if (tid == 0) out[blockIdx.x * 3 + j] = (float)red[0];
    __syncthreads();
  }
}

extern "C" int mq_set_loss_fwd(const float* logits, const float* boxes, const float* gt, const float* posmap, const int* gt_off,
                               const int* text_mask, const int* q2g, const int* match_q, float* partials, float* sums, int L, int B, int nq,
                               int T, int Tpm, int total_gt, float alpha, float gamma, void* stream) {
  if (L <= 0) return 0;
  if (B <= 0 || nq <= 0 || T <= 0 || Tpm < T || total_gt < 0) return -1;
  const long tiles = ((long)B * nq + SL_ROWS - 1) / SL_ROWS;
  if (L * tiles > 0x7fffffffL) return -1;
  const hipStream_t st = (hipStream_t)stream;
  const int rc = mq_launch<set_loss_kernel>(dim3((unsigned)(L * tiles)), dim3(SL_THREADS), 0, st, logits, boxes, gt, posmap, gt_off, text_mask,
                                            q2g, match_q, partials, B, nq, T, Tpm, total_gt, (int)tiles, alpha, gamma);
  if (rc) return rc;
  return mq_launch<set_reduce_kernel>(dim3((unsigned)L), dim3(SL_THREADS), 0, st, (const float*)partials, (int)tiles, sums);
}

#endif  // MQ_PRIMARY_UNIT

MQ_NAMESPACE_END
