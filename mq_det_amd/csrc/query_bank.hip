// The vision-query bank on the device: its admission loop (host side: mq_det_amd/query_bank.py QueryBank.update) and, at the end of the file,
// the selection of a forward's vision queries from it (mq_bank_select_fwd).
//
// mq_bank_admit: generalized_vl_rcnn_new.py:269-287 (== groundingdino.py:401-421) for a whole batch of candidates in one launch.  The host
// sorts the candidates' labels once (stable: candidates of a label keep their row order); workgroup b owns label `label_lo + b`, finds its
// segment of the sorted labels by two binary searches and walks the candidates IN ORDER -- a candidate admitted earlier in the call is part
// of the bank the later ones are compared against.  Labels are independent, so the sequential semantics of the reference hold exactly.
//
// Per candidate: stop when the label holds maxq rows; with `exclude` and a non-empty label bank the candidate is skipped when any row has
// cosine similarity > thr (strict; a NaN compares false, so the candidate is admitted, like `(similarity > thr).sum() > 0`).  The cosine
// is dot(c, r) / (max(|c|, 1e-12) max(|r|, 1e-12)) -- F.normalize's rule -- with 1 / max(|r|, 1e-12) of every bank row cached in inv_norm,
// so a comparison is ONE dot product: the bank rows are dealt out over the four waves, the row is read with 16-byte loads (1 KB per wave
// instruction at C = 256), the candidate sits in registers (C = 256) or comes from the cache, a per-lane partial dot and a wave reduction
// follow.  The any-hit flag crosses the waves through LDS with one barrier per candidate (three flags in rotation: the flag of candidate
// i + 1 is cleared while candidate i is decided, two barriers after its last reader).  An admitted row is copied bit for bit into a pool
// row taken with one atomic add by one lane; slot, inverse norm and count are plain stores by one lane; two more barriers make the new
// row visible to the next candidate's comparisons.
//
// What bounds it: the walk through one label's candidates is sequential, and each comparison pass reads the label's rows from L2 / HBM:
// n rows x D floats over four waves.  One launch replaces, per candidate, the dict path's two normalisations, einsum, compare, reduction,
// device->host sync and torch.cat of the label's whole tensor.
#include "common.h"

MQ_NAMESPACE_BEGIN
#ifdef MQ_PRIMARY_UNIT                                     // fp32 / integer data only: one copy, in the fp16 translation unit

#define BANK_WAVES 4
#define BANK_THREADS (BANK_WAVES * 64)

// first index in [0, n) whose value is >= v (n if none)
__device__ __forceinline__ int bank_lower_bound(const long long* __restrict__ a, int n, long long v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

template <bool VEC4>
__device__ __forceinline__ float bank_dot(const float* __restrict__ a, const float* __restrict__ b, int D, int lane) {
  float s = 0.f;
  if (VEC4) {
    for (int k = lane * 4; k < D; k += 256) {
      const float4_ x = *(const float4_*)(a + k), y = *(const float4_*)(b + k);
      s += x[0] * y[0] + x[1] * y[1] + x[2] * y[2] + x[3] * y[3];
    }
  } else {
    for (int k = lane; k < D; k += 64) s += a[k] * b[k];
  }
  return wave_sum(s);
}

template <bool VEC4>
__global__ __launch_bounds__(BANK_THREADS) void bank_admit_kernel(const float* __restrict__ cand, const long long* __restrict__ sorted_labels,
                                                                   const long long* __restrict__ order, float* pool, float* inv_norm,
                                                                   int* slots, int* __restrict__ counts, int* __restrict__ state, int N, int D,
                                                                   int pool_rows, int cap, int label_lo, int maxq, int exclude, float thr) {
  __shared__ int hit_s[3];
  __shared__ int prow_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long l = (long long)label_lo + blockIdx.x;
  const int lo = bank_lower_bound(sorted_labels, N, l), hi = bank_lower_bound(sorted_labels, N, l + 1);
  if (lo >= hi) return;                                    // no candidate of this label
  int* __restrict__ row_slots = slots + l * cap;
  int n = counts[l];
  if (tid < 3) hit_s[tid] = 0;
  __syncthreads();
  int it = 0;
  for (int j = lo; j < hi && n < maxq; ++j) {              // n is uniform over the workgroup; a full label ends the walk
    const float* __restrict__ c = cand + order[j] * D;
    // every wave computes the candidate's norm itself (same lanes, same order: the same bits in every wave)
    const float inv_c = 1.f / fmaxf(sqrtf(bank_dot<VEC4>(c, c, D, lane)), 1e-12f);
    if (exclude && n > 0) {
      bool hit = false;
      if (VEC4 && D == 256) {                              // the candidate in registers, one 16-byte load per lane and bank row
        const float4_ x = *(const float4_*)(c + lane * 4);
        for (int r = wave; r < n; r += BANK_WAVES) {
          const int prow = row_slots[r];
          const float4_ y = *(const float4_*)(pool + (long)prow * 256 + lane * 4);
          const float dot = wave_sum(x[0] * y[0] + x[1] * y[1] + x[2] * y[2] + x[3] * y[3]);
          hit |= dot * inv_c * inv_norm[prow] > thr;
        }
      } else {
        for (int r = wave; r < n; r += BANK_WAVES) {
          const int prow = row_slots[r];
          hit |= bank_dot<VEC4>(c, pool + (long)prow * D, D, lane) * inv_c * inv_norm[prow] > thr;
        }
      }
      const int p = it % 3;
      if (hit && lane == 0) hit_s[p] = 1;
      if (tid == 0) hit_s[(it + 1) % 3] = 0;               // last read two barriers ago
      __syncthreads();
      ++it;
      if (hit_s[p]) continue;                              // a similar row is in the bank already
    }
    if (tid == 0) prow_s = atomicAdd(&state[0], 1);        // the pool is append-only: one row per admitted candidate
    __syncthreads();
    const int prow = prow_s;
    if (prow >= pool_rows) {                               // the host sized the pool for every candidate of the call: not reached
      if (tid == 0) state[1] = 1;
      break;
    }
    float* __restrict__ dst = pool + (long)prow * D;
    if (VEC4) {
      for (int k = tid * 4; k < D; k += BANK_THREADS * 4) *(float4_*)(dst + k) = *(const float4_*)(c + k);
    } else {
      for (int k = tid; k < D; k += BANK_THREADS) dst[k] = c[k];
    }
    if (tid == 0) {
      row_slots[n] = prow;
      inv_norm[prow] = inv_c;
    }
    ++n;
    __syncthreads();                                       // the row, its slot and its norm before the next candidate's comparisons
  }
  if (tid == 0) counts[l] = n;
}

extern "C" int mq_bank_admit(const float* cand, const long long* sorted_labels, const long long* order, float* pool, float* inv_norm, int* slots,
                             int* counts, int* state, int N, int D, int pool_rows, int cap, int label_lo, int num_labels, int maxq, int exclude,
                             float thr, void* stream) {
  if (N <= 0 || num_labels <= 0) return 0;
  if (D <= 0 || label_lo < 0 || maxq > cap || pool_rows < 0) return -1;
  const bool vec4 = D % 4 == 0 && ((uintptr_t)cand | (uintptr_t)pool) % 16 == 0;
  if (vec4)
    hipLaunchKernelGGL(bank_admit_kernel<true>, dim3(num_labels), dim3(BANK_THREADS), 0, (hipStream_t)stream, cand, sorted_labels, order, pool,
                       inv_norm, slots, counts, state, N, D, pool_rows, cap, label_lo, maxq, exclude, thr);
  else
    hipLaunchKernelGGL(bank_admit_kernel<false>, dim3(num_labels), dim3(BANK_THREADS), 0, (hipStream_t)stream, cand, sorted_labels, order, pool,
                       inv_norm, slots, counts, state, N, D, pool_rows, cap, label_lo, maxq, exclude, thr);
  return (int)hipGetLastError();
}

// mq_bank_select_fwd: the consumer side (host: modeling/query_selector.py QuerySelector with a resident QueryBank).  The host has drawn, per
// item and label, which of the label's rows enter the forward; one launch turns those integer tables into what the GCP layers read:
//   * row tiles (blockIdx.x < row_tiles): SEL_ROWS consecutive rows of vision [I * V, C], one wave per row at a time.  Row (i, q * S + s) is
//     pool row slots[label, pos] of qsrc[i, q], scale s, read with 16-byte loads (1 KB per wave instruction at C = 256) and stored in the
//     output type, rounded to nearest-even like Tensor.to; a padding query, or one whose table entries do not name a row, gives zeros.
//   * index blocks (the rest of the grid): 256 token positions of one item each.  The item's qtok [Q, MT] goes through LDS in pieces of
//     SEL_CHUNK entries; every thread walks the queries in order and counts how often its token is listed, so its rows come out ascending
//     and a token listed twice gives each row twice, adjacent -- `sorted(owners[t])` of the dict path.  Smax is the host's exact maximum.
// Nothing here waits for another workgroup; the two parts write disjoint outputs.
#define SEL_THREADS 256
#define SEL_ROWS 16
#define SEL_CHUNK 2048

struct sel_bf16 { unsigned short bits; };
template <class O> struct alignas(4 * sizeof(O)) sel_vec4 { O v[4]; };

__device__ __forceinline__ void sel_cvt(float x, float& y) { y = x; }
__device__ __forceinline__ void sel_cvt(float x, _Float16& y) { y = (_Float16)x; }
__device__ __forceinline__ void sel_cvt(float x, sel_bf16& y) {            // c10::BFloat16's round-to-nearest-even
  const unsigned u = __builtin_bit_cast(unsigned, x);
  y.bits = x != x ? (unsigned short)0x7FC0 : (unsigned short)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// ADD (mq_bank_select_add_fwd, VISION_QUERY.ADD_VISION_LAYER): row v = q * S + s of an item, counted inside the item, gets row_add[v, :] added in
// fp32 before the one rounding to O.  Only a row that the tables name gets it -- a padding row stays zero, as the reference adds before
// pad_sequence -- and no addend row at or beyond add_rows is read (the host refuses such a call; here the row then goes without).  Without ADD
// the two arguments are not looked at and the code is that of mq_bank_select_fwd.
template <class O, bool VEC4, bool ADD>
__global__ __launch_bounds__(SEL_THREADS) void bank_select_kernel(const float* __restrict__ pool, const int* __restrict__ slots,
                                                                   const int* __restrict__ qsrc, const int* __restrict__ qtok,
                                                                   const float* __restrict__ row_add, int add_rows,
                                                                   O* __restrict__ vision, int* __restrict__ idx, int pool_rows, int num_labels,
                                                                   int cap, int I, int Q, int MT, int S, int C, int T, int Smax, int row_tiles) {
  __shared__ int tok_s[SEL_CHUNK];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < row_tiles) {
    const int lane = tid & 63, wave = tid >> 6;
    const long rows = (long)I * Q * S;
    for (int r = wave; r < SEL_ROWS; r += SEL_THREADS / 64) {
      const long row = (long)blockIdx.x * SEL_ROWS + r;      // = (i * Q + q) * S + s
      if (row >= rows) break;
      const long iq = row / S;
      const int s = (int)(row - iq * S);
      const int label = qsrc[iq * 2], pos = qsrc[iq * 2 + 1];
      const float* __restrict__ src = nullptr;
      if (label >= 0 && label < num_labels && pos >= 0 && pos < cap) {
        const int prow = slots[(long)label * cap + pos];
        if (prow >= 0 && prow < pool_rows) src = pool + ((long)prow * S + s) * C;
      }
      O* __restrict__ dst = vision + row * C;
      const float* __restrict__ add = nullptr;                 // decided once per row, outside the element loops
      if (ADD && src) {
        const long v = row - (iq / Q) * (long)Q * S;           // the row's place in its item
        if (v < add_rows) add = row_add + v * C;
      }
      if (VEC4) {
        for (int k = lane * 4; k < C; k += 256) {
          float4_ x = {0.f, 0.f, 0.f, 0.f};
          if (src) x = *(const float4_*)(src + k);
          if (ADD && add) {
            const float4_ a = *(const float4_*)(add + k);
            x[0] += a[0];
            x[1] += a[1];
            x[2] += a[2];
            x[3] += a[3];
          }
          sel_vec4<O> y;
          sel_cvt(x[0], y.v[0]);
          sel_cvt(x[1], y.v[1]);
          sel_cvt(x[2], y.v[2]);
          sel_cvt(x[3], y.v[3]);
          *(sel_vec4<O>*)(dst + k) = y;
        }
      } else {
        if (ADD && add) {
          for (int k = lane; k < C; k += 64) sel_cvt(src[k] + add[k], dst[k]);
        } else {
          for (int k = lane; k < C; k += 64) sel_cvt(src ? src[k] : 0.f, dst[k]);
        }
      }
    }
    return;
  }
  const int tblocks = (T + SEL_THREADS - 1) / SEL_THREADS;
  const int b = blockIdx.x - row_tiles, i = b / tblocks, t = (b - i * tblocks) * SEL_THREADS + tid;
  const int* __restrict__ tok = qtok + (long)i * Q * MT;
  int* __restrict__ out = idx + ((long)i * T + (t < T ? t : 0)) * Smax;      // written with t < T only
  const int total = Q * MT;
  int n = 0, q = 0, j = 0, mult = 0;
  for (int base = 0; base < total; base += SEL_CHUNK) {
    const int len = total - base < SEL_CHUNK ? total - base : SEL_CHUNK;
    __syncthreads();                                         // the previous piece has been read by every thread
    for (int e = tid; e < len; e += SEL_THREADS) tok_s[e] = tok[base + e];
    __syncthreads();
    if (t < T) {
      for (int e = 0; e < len; ++e) {
        mult += tok_s[e] == t;
        if (++j == MT) {                                     // query q is complete: its S rows, each `mult` times
          if (mult) {
            for (int s = 0; s < S; ++s)
              for (int m = 0; m < mult; ++m)
                if (n < Smax) out[n++] = q * S + s;
          }
          j = 0;
          mult = 0;
          ++q;
        }
      }
    }
  }
  if (t < T)
    for (; n < Smax; ++n) out[n] = -1;
}

template <class O, bool ADD>
static int bank_select_launch(const float* pool, const int* slots, const int* qsrc, const int* qtok, const float* row_add, int add_rows,
                              void* vision, int* idx, int pool_rows, int num_labels, int cap, int I, int Q, int MT, int S, int C, int T, int Smax,
                              hipStream_t stream) {
  const long rows = (long)I * Q * S;
  const long row_tiles = (rows + SEL_ROWS - 1) / SEL_ROWS, blocks = row_tiles + (long)I * ((T + SEL_THREADS - 1) / SEL_THREADS);
  if (blocks > 0x7fffffffL) return -1;
  const bool vec4 = C % 4 == 0 && ((uintptr_t)pool | (uintptr_t)vision | (ADD ? (uintptr_t)row_add : 0)) % 16 == 0;
  if (vec4)
    return mq_launch<bank_select_kernel<O, true, ADD>>(dim3((unsigned)blocks), dim3(SEL_THREADS), 0, stream, pool, slots, qsrc, qtok, row_add,
                                                       add_rows, (O*)vision, idx, pool_rows, num_labels, cap, I, Q, MT, S, C, T, Smax,
                                                       (int)row_tiles);
  return mq_launch<bank_select_kernel<O, false, ADD>>(dim3((unsigned)blocks), dim3(SEL_THREADS), 0, stream, pool, slots, qsrc, qtok, row_add,
                                                      add_rows, (O*)vision, idx, pool_rows, num_labels, cap, I, Q, MT, S, C, T, Smax,
                                                      (int)row_tiles);
}

template <bool ADD>
static int bank_select_any(const float* pool, const int* slots, const int* qsrc, const int* qtok, const float* row_add, int add_rows, void* vision,
                           int* idx, int pool_rows, int num_labels, int cap, int I, int Q, int MT, int S, int C, int T, int Smax, int out_type,
                           void* stream) {
  if (I <= 0) return 0;
  if (Q <= 0 || MT <= 0 || S < 1 || S > 8 || C <= 0 || T <= 0 || Smax <= 0 || pool_rows < 0 || num_labels < 0 || cap < 0) return -1;
  if ((long)Q * MT > 0x7fffffffL) return -1;
  if (ADD && (!row_add || add_rows < 0)) return -1;
  const hipStream_t st = (hipStream_t)stream;
  switch (out_type) {
    case 0:
      return bank_select_launch<float, ADD>(pool, slots, qsrc, qtok, row_add, add_rows, vision, idx, pool_rows, num_labels, cap, I, Q, MT, S, C, T,
                                            Smax, st);
    case 1:
      return bank_select_launch<_Float16, ADD>(pool, slots, qsrc, qtok, row_add, add_rows, vision, idx, pool_rows, num_labels, cap, I, Q, MT, S, C,
                                               T, Smax, st);
    case 2:
      return bank_select_launch<sel_bf16, ADD>(pool, slots, qsrc, qtok, row_add, add_rows, vision, idx, pool_rows, num_labels, cap, I, Q, MT, S, C,
                                               T, Smax, st);
  }
  return -1;
}

extern "C" int mq_bank_select_fwd(const float* pool, const int* slots, const int* qsrc, const int* qtok, void* vision, int* idx, int pool_rows,
                                  int num_labels, int cap, int I, int Q, int MT, int S, int C, int T, int Smax, int out_type, void* stream) {
  return bank_select_any<false>(pool, slots, qsrc, qtok, nullptr, 0, vision, idx, pool_rows, num_labels, cap, I, Q, MT, S, C, T, Smax, out_type,
                                stream);
}

extern "C" int mq_bank_select_add_fwd(const float* pool, const int* slots, const int* qsrc, const int* qtok, const float* row_add, int add_rows,
                                      void* vision, int* idx, int pool_rows, int num_labels, int cap, int I, int Q, int MT, int S, int C, int T,
                                      int Smax, int out_type, void* stream) {
  return bank_select_any<true>(pool, slots, qsrc, qtok, row_add, add_rows, vision, idx, pool_rows, num_labels, cap, I, Q, MT, S, C, T, Smax,
                               out_type, stream);
}

#endif
MQ_NAMESPACE_END
