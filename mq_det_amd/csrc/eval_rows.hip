// Evaluator rows from the packed detections of one forward, on the device (host side: mq_det_amd/evaluation.py `update_packed`,
// mq_det_amd/detection.py `evaluate_detection`).
//
// mq_eval_rows: packed [items, K2, 6] fp32 (x1, y1, x2, y2, score, label) and the RAW counts [items] int32 of `_rest_program` (low 16 bits =
// live rows, bit 16 = tie overflow; candidate mode: the plain count) -> rows [capacity, 7 | 8] fp32
// (image id, category, score, x, y, w, h [, mark]) of the live detections only, densely packed from row 0 in the order of the ENTRY TABLE
// (one entry per source item, in output order: image-major out of the forward's chunk-major items), the number of rows and the OR of the
// overflow bits.  The counts are read where they lie: nothing comes to the host.
//
// One launch, one workgroup per entry.  Every workgroup sums the clamped counts of the entries before its own (E is a few hundred: E
// 4-byte reads per workgroup, a handful per lane), so no second launch, no atomics and no zeroed buffer are needed and the row order does
// not depend on the schedule; the last entry's workgroup writes the two scalars.  Placeholder mode (COCO): an image -- a run of entries
// from one marked "first" to the next -- whose entries hold no live row at all emits the one row that CocoAPEvaluator.update appends for
// an empty BoxList, written by the workgroup of the image's first entry.
//
// Arithmetic: BoxList.resize (a multiply by the fp32 ratio) followed by convert_to_xywh (LVIS) / BoxList.convert("xywh") (COCO, + 1), every
// operation rounded by itself: contraction is off, `x2 * r - x1 * r` as an fma differs from torch in the last bit of most widths.
//
// Bounds: a count above K2 is clamped; an entry whose item lies outside [0, items) contributes no rows (the host refuses such a table before
// the launch); no row at or beyond `capacity` is written; rows behind the last one are left as they are.
#include "common.h"

MQ_NAMESPACE_BEGIN
#ifdef MQ_PRIMARY_UNIT                                     // fp32 / integer data only: one copy, in the fp16 translation unit

#define EVAL_ROWS_THREADS 256
#define EVAL_ROWS_CANDIDATE 1                              // flags: counts are plain numbers (TEST.USE_MULTISCALE), no overflow bit
#define EVAL_ROWS_PLUS_ONE 2                               //        legacy + 1 on width and height
#define EVAL_ROWS_PLACEHOLDER 4                            //        an image without a live row emits (id, NaN, 0, 0, 0, 0, 0, 1)

// entry table [E, 5] int32: (item, first entry of its image, image id, ratio_w, ratio_h), the last three as fp32 bits
#define EVAL_ROWS_ENTRY 5

__device__ __forceinline__ int eval_rows_count(const int* __restrict__ table, const int* __restrict__ counts, int j, int items, int K2,
                                               int candidate, int* over) {
  const int it = table[j * EVAL_ROWS_ENTRY];
  if (it < 0 || it >= items) return 0;
  const int raw = counts[it];
  int n = raw;
  if (!candidate) {
    n = raw & 0xFFFF;
    *over |= (raw >> 16) & 1;
  }
  return n < 0 ? 0 : (n > K2 ? K2 : n);
}

__device__ __forceinline__ int eval_rows_block_sum(int v, int* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();                                         // the previous reduction's result is read
  if (lane == 0) red[wave] = v;
  __syncthreads();
  int s = 0;
  for (int w = 0; w < EVAL_ROWS_THREADS / 64; ++w) s += red[w];
  return s;
}

__global__ __launch_bounds__(EVAL_ROWS_THREADS) void eval_rows_kernel(const float* __restrict__ packed, const int* __restrict__ counts,
                                                                      const int* __restrict__ table, const int* __restrict__ lbl_keys,
                                                                      const float* __restrict__ lbl_vals, int n_lbl, float* __restrict__ rows,
                                                                      int* __restrict__ n_rows, int* __restrict__ overflow, int E, int items,
                                                                      int K2, int cols, long capacity, int flags) {
#pragma clang fp contract(off)
  __shared__ int red[EVAL_ROWS_THREADS / 64];
  const int e = blockIdx.x, tid = threadIdx.x;
  const int candidate = flags & EVAL_ROWS_CANDIDATE, placeholder = flags & EVAL_ROWS_PLACEHOLDER;
  // the first entry of this entry's image: the last marked entry at or before e (entry 0 starts an image whatever its mark says)
  int start = 0;
  for (int j = e; j > 0; --j)
    if (table[j * EVAL_ROWS_ENTRY + 1]) {
      start = j;
      break;
    }
  // live rows before this entry, of them within its image, placeholder rows of the images before its image, overflow bits up to e
  int before = 0, inside = 0, holders = 0, over = 0;
  for (int j = tid; j < e; j += EVAL_ROWS_THREADS) {
    const int n = eval_rows_count(table, counts, j, items, K2, candidate, &over);
    before += n;
    if (j >= start) inside += n;
    if (placeholder && j < start && (j == 0 || table[j * EVAL_ROWS_ENTRY + 1])) {      // j starts an earlier image: is that image empty?
      int any = n, k = j + 1, dummy = 0;
      for (; !any && k < start && !table[k * EVAL_ROWS_ENTRY + 1]; ++k) any = eval_rows_count(table, counts, k, items, K2, candidate, &dummy);
      holders += !any;
    }
  }
  before = eval_rows_block_sum(before, red);
  inside = eval_rows_block_sum(inside, red);
  holders = eval_rows_block_sum(holders, red);
  over = eval_rows_block_sum(over, red);
  int mine_over = 0;
  const int mine = eval_rows_count(table, counts, e, items, K2, candidate, &mine_over);
  const long off = (long)before + holders;
  // whether this entry's image holds no live row (asked by its first entry, which then writes the placeholder, and by the last entry for the total)
  int empty = 0;
  if (placeholder && inside == 0 && mine == 0 && (e == start || e == E - 1)) {
    empty = 1;
    int dummy = 0;
    for (int k = e + 1; empty && k < E && !table[k * EVAL_ROWS_ENTRY + 1]; ++k)
      empty = !eval_rows_count(table, counts, k, items, K2, candidate, &dummy);
  }
  const int* ent = table + e * EVAL_ROWS_ENTRY;
  const float id = __builtin_bit_cast(float, ent[2]), rw = __builtin_bit_cast(float, ent[3]), rh = __builtin_bit_cast(float, ent[4]);
  if (tid == 0) {
    if (e == E - 1) {
      n_rows[0] = (int)(off + mine + empty);
      overflow[0] = (over | mine_over) ? 1 : 0;
    }
    if (empty && e == start && off < capacity) {
      float* r = rows + off * cols;
      r[0] = id, r[1] = __builtin_nanf(""), r[2] = 0.f, r[3] = 0.f, r[4] = 0.f, r[5] = 0.f, r[6] = 0.f;
      if (cols == 8) r[7] = 1.f;
    }
  }
  if (mine == 0) return;
  const float* src = packed + (long)ent[0] * K2 * 6;
  for (int i = tid; i < mine; i += EVAL_ROWS_THREADS) {
    const long row = off + i;
    if (row >= capacity) break;
    const float* p = src + (long)i * 6;
    const float x = p[0] * rw, y = p[1] * rh, xe = p[2] * rw, ye = p[3] * rh;
    float w = xe - x, h = ye - y;
    if (flags & EVAL_ROWS_PLUS_ONE) {
      w = w + 1.f;
      h = h + 1.f;
    }
    float cat = p[5];
    if (n_lbl >= 0) {                                      // label table (sorted keys); a label it lacks keeps its place with a NaN category
      const float lab = cat;
      cat = __builtin_nanf("");
      if (lab == lab && lab > -2147483648.f && lab < 2147483648.f) {
        const int key = (int)lab;                          // Tensor.long(): towards zero
        int lo = 0, hi = n_lbl;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (lbl_keys[mid] < key) lo = mid + 1; else hi = mid;
        }
        if (lo < n_lbl && lbl_keys[lo] == key) cat = lbl_vals[lo];
      }
    }
    float* r = rows + row * cols;
    r[0] = id, r[1] = cat, r[2] = p[4], r[3] = x, r[4] = y, r[5] = w, r[6] = h;
    if (cols == 8) r[7] = (inside == 0 && i == 0) ? 1.f : 0.f;
  }
}

extern "C" int mq_eval_rows(const float* packed, const int* counts, const int* table, const int* table_host, const int* lbl_keys,
                            const float* lbl_vals, int n_lbl, float* rows, int* n_rows, int* overflow, int E, int items, int K2, int cols,
                            long capacity, int flags, void* stream) {
  if (E < 1 || items < 1 || K2 < 1 || (cols != 7 && cols != 8) || capacity < 0) return -1;
  if (n_lbl > 0 && (!lbl_keys || !lbl_vals)) return -1;
  if (table_host)                                          // the host's copy of the table, when the caller has one: refuse before the launch
    for (int j = 0; j < E; ++j)
      if (table_host[j * EVAL_ROWS_ENTRY] < 0 || table_host[j * EVAL_ROWS_ENTRY] >= items) return -2;
  return mq_launch<eval_rows_kernel>(dim3(E), dim3(EVAL_ROWS_THREADS), 0, (hipStream_t)stream, packed, counts, table, lbl_keys, lbl_vals, n_lbl,
                                     rows, n_rows, overflow, E, items, K2, cols, capacity, flags);
}

#endif
MQ_NAMESPACE_END
