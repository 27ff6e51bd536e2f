// Region-word alignment scoring and ATSS post-processing kernels for gfx950 (thin, HBM-bound).
//
// mq_align_scores_fwd -- reference rpn/vldyhead.py:884-887 (+bias, clamp +-50000) followed by
//   rpn/inference.py:656-683: sigmoid, token -> class aggregation (convert_grounding_to_od_logits[_v2], :772-824:
//   agg 0 = MEAN, 1 = MAX, 2 = POWER = prod^(1/n); ONEHOT is MEAN over the one-token index the host builds for it),
//   threshold 0.05, x sigmoid(centerness).  The reference builds a dense [B, HW, 3000] (LVIS) score
//   tensor of which <= 40 columns are non-zero; here only the L labels of the caption are produced.
//     dot    : [B, HW, T] fp16 = feat . (proj_tokens / exp(log_scale))^T       (library GEMM outside; batch stride
//              dot_bs elements: a level's slice of the all-level [B, N, T] product)
//     tbias  : [B, T] fp32     = emb . bias_lang + bias0
//     tokidx : [L, MT] int32   token positions of each label (-1 padded); batch stride tok_bs elements (0: one caption
//              shared by the batch; L*MT: one caption per batch item -- chunk batching of the LVIS protocol)
//     ctr    : [B, HW] fp16/fp32 centerness logits
//     out    : [B, HW, L] fp32 = (cls > thr) ? cls * sigmoid(ctr) : -1 ;  cls_out (optional) = cls
//   One wave per location: 256 token logits -> LDS, lanes then average their label's tokens.
//
// mq_box_decode -- BoxCoder.decode (vldyhead.py:78-108), clip_to_image (bounding_box.py:221-232), sqrt
//   score (inference.py:707), label = class_idx + 1 (:696) for the top-k candidates of one level.
//
// The class-aware NMS that follows them (mq_ml_nms, mq_ml_nms_topk) is nms.hip.
#include "common.h"

MQ_NAMESPACE_BEGIN

template <typename TD>
__global__ __launch_bounds__(256) void align_scores_kernel(const TD* __restrict__ dot, const float* __restrict__ tbias,
                                                           const int* __restrict__ tokidx, const half_t* __restrict__ ctr,
                                                           float* __restrict__ out, float* __restrict__ cls_out,
                                                           int B, int HW, int T, int L, int MT, float thr, long dot_bs, long tok_bs,
                                                           int agg) {
  extern __shared__ float sig[];                 // [4][T]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long loc = (long)blockIdx.x * 4 + wave;
  if (loc >= (long)B * HW) return;
  const int b = loc / HW;
  const TD* drow = dot + (long)b * dot_bs + (loc - (long)b * HW) * T;
  const int* tix = tokidx + (long)b * tok_bs;
  float* sw = sig + wave * T;
  if ((T & 3) == 0 && (dot_bs & 3) == 0) {       // 8-byte (fp16) / 16-byte (fp32) loads: one per lane for T = 256
    for (int t = lane * 4; t < T; t += 256) {
      float d[4];
      if constexpr (sizeof(TD) == 2) {
        const half4 h = *(const half4*)(drow + t);
#pragma unroll
        for (int j = 0; j < 4; ++j) d[j] = (float)h[j];
      } else {
        const float4_ f = *(const float4_*)(drow + t);
#pragma unroll
        for (int j = 0; j < 4; ++j) d[j] = f[j];
      }
      const float4_ tb = *(const float4_*)(tbias + (long)b * T + t);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float v = d[j] + tb[j];
        v = fminf(fmaxf(v, -50000.f), 50000.f);
        sw[t + j] = 1.f / (1.f + __expf(-v));
      }
    }
  } else {
    for (int t = lane; t < T; t += 64) {
      float v = (float)drow[t] + tbias[(long)b * T + t];
      v = fminf(fmaxf(v, -50000.f), 50000.f);
      sw[t] = 1.f / (1.f + __expf(-v));
    }
  }
  wave_lds_fence();
  const float c = 1.f / (1.f + __expf(-(float)ctr[loc]));
  for (int l = lane; l < L; l += 64) {
    float s = agg == 2 ? 1.f : 0.f;
    int n = 0;
    for (int j = 0; j < MT; ++j) {
      int t = tix[l * MT + j];
      if (t >= 0) {
        const float v = sw[t];
        s = agg == 0 ? s + v : (agg == 1 ? fmaxf(s, v) : s * v);          // sigmoid outputs are >= 0: 0 is the identity of max
        ++n;
      }
    }
    float cls = 0.f;                                    // a label without tokens scores 0 (never a candidate)
    if (n > 0) cls = agg == 0 ? s / (float)n : (agg == 1 ? s : powf(s, 1.f / (float)n));
    if (cls_out) cls_out[loc * L + l] = cls;
    // candidates are decided by the class score alone (rpn/inference.py:677): keep them > 0 even if the product with a
    // vanishing centerness underflows, so that "value > 0" identifies a candidate downstream
    out[loc * L + l] = cls > thr ? fmaxf(cls * c, 1.17549435e-38f) : -1.f;
  }
}

extern "C" int MQ_SYM(mq_align_scores_fwd)(const void* dot, int dot_f32, const float* tbias, const int* tokidx, long tok_bs,
                                   const void* ctr, float* out, float* cls_out, int B, int HW, int T, int L, int MT, float thr,
                                   long dot_bs, int agg, void* stream) {
  if (B <= 0 || HW <= 0 || L <= 0) return 0;
  if (agg < 0 || agg > 2) return -1;
  long locs = (long)B * HW;
  const dim3 grid((unsigned)((locs + 3) / 4));
  const long dbs = dot_bs > 0 ? dot_bs : (long)HW * T;
  if (dot_f32)
    hipLaunchKernelGGL(align_scores_kernel<float>, grid, dim3(256), 4 * T * sizeof(float), (hipStream_t)stream, (const float*)dot,
                       tbias, tokidx, (const half_t*)ctr, out, cls_out, B, HW, T, L, MT, thr, dbs, tok_bs, agg);
  else
    hipLaunchKernelGGL(align_scores_kernel<half_t>, grid, dim3(256), 4 * T * sizeof(float), (hipStream_t)stream, (const half_t*)dot,
                       tbias, tokidx, (const half_t*)ctr, out, cls_out, B, HW, T, L, MT, thr, dbs, tok_bs, agg);
  MQ_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------------------------------------
template <typename TR>
__global__ void box_decode_kernel(const float* __restrict__ val, const long* __restrict__ flat, const TR* __restrict__ reg,
                                  const float* __restrict__ anchors, const int* __restrict__ label_ids,
                                  const float* __restrict__ im_wh, float* __restrict__ boxes, float* __restrict__ scores,
                                  int* __restrict__ labels, int B, int K, int HW, int L, long out_stride, long out_off, long lab_bs) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * K) return;
  const int b = i / K, k = i % K;
  const long o = (long)b * out_stride + out_off + k;
  const float v = val[i];
  if (!(v > 0.f)) {                       // not a candidate (score -1 filler)
    scores[o] = -1.f; labels[o] = 0;
    boxes[o * 4 + 0] = boxes[o * 4 + 1] = boxes[o * 4 + 2] = boxes[o * 4 + 3] = 0.f;
    return;
  }
  const long f = flat[i];
  const int loc = f / L, l = f % L;
  const TR* r = reg + ((long)b * HW + loc) * 4;
  const float* a = anchors + (long)loc * 4;
  const float w = a[2] - a[0] + 1.f, h = a[3] - a[1] + 1.f;
  const float cx = (a[2] + a[0]) * 0.5f, cy = (a[3] + a[1]) * 0.5f;
  const float lim = 4.135166556742356f;   // log(1000/16)
  const float dx = (float)r[0] / 10.f, dy = (float)r[1] / 10.f;
  const float dw = fminf((float)r[2] / 5.f, lim), dh = fminf((float)r[3] / 5.f, lim);
  const float pcx = dx * w + cx, pcy = dy * h + cy;
  const float pw = expf(dw) * w, ph = expf(dh) * h;
  const float W = im_wh[b * 2 + 0], H = im_wh[b * 2 + 1];
  boxes[o * 4 + 0] = fminf(fmaxf(pcx - 0.5f * (pw - 1.f), 0.f), W - 1.f);
  boxes[o * 4 + 1] = fminf(fmaxf(pcy - 0.5f * (ph - 1.f), 0.f), H - 1.f);
  boxes[o * 4 + 2] = fminf(fmaxf(pcx + 0.5f * (pw - 1.f), 0.f), W - 1.f);
  boxes[o * 4 + 3] = fminf(fmaxf(pcy + 0.5f * (ph - 1.f), 0.f), H - 1.f);
  scores[o] = sqrtf(v);
  labels[o] = label_ids[(long)b * lab_bs + l];
}

extern "C" int MQ_SYM(mq_box_decode)(const float* val, const long* flat, const void* reg, int reg_f32, const float* anchors, const int* label_ids,
                             long lab_bs, const float* im_wh, float* boxes, float* scores, int* labels, int B, int K, int HW,
                             int L, long out_stride, long out_off, void* stream) {
  if (B <= 0 || K <= 0) return 0;
  long n = (long)B * K;
  if (reg_f32)
    hipLaunchKernelGGL(box_decode_kernel<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, val, flat,
                       (const float*)reg, anchors, label_ids, im_wh, boxes, scores, labels, B, K, HW, L, out_stride, out_off, lab_bs);
  else
    hipLaunchKernelGGL(box_decode_kernel<half_t>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, val, flat,
                       (const half_t*)reg, anchors, label_ids, im_wh, boxes, scores, labels, B, K, HW, L, out_stride, out_off, lab_bs);
  MQ_CHECK_LAUNCH();
  return 0;
}

MQ_NAMESPACE_END
