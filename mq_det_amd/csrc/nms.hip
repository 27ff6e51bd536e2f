// Class-aware NMS of the ATSS post-processing for gfx950.
//
// mq_ml_nms -- reference csrc/cuda/ml_nms.cu: IoU with the legacy +1 widths, 0 across labels (:15-26; box_iou.h), 64x64 bitmask
//   tiles (:28-75).  The reference copies the mask to the host and sweeps serially there (:117-140, a device sync per image); here the
//   sweep runs on the device, 64 boxes at a time (intra-chunk dependencies via wave shuffles).
//
// mq_ml_nms_topk -- the same NMS, but the sweep STOPS once `max_keep` boxes of an image are kept.  The boxes arrive sorted by score and
//   the caller only uses the max_keep highest-scoring survivors (ATSSPostProcessor.select_over_all_levels, rpn/inference.py:748-769:
//   NMS, then kthvalue / top DETECTIONS_PER_IMG): the first max_keep survivors of the sweep are exactly those, every later box is
//   irrelevant.  mq_ml_nms resolves all ~5000 candidates of an image -- a serial chain of ~80 chunks, 0.3 ms at the very end of the
//   step where nothing overlaps it (profiles/r02_call5); with 300 detections per image the sweep typically ends after 10 - 20 chunks.
//   keep[] is 0 for every box after the stopping chunk; the selected detections are identical to mq_ml_nms + top-k.
//   Default since round 3 (KERNELS["NMS_EARLY_STOP"] = 1; device parity: tests/test_gpu_parity.py test_opt_in_kernel[nms_early_stop]).
//
// Both entry points are one mask kernel and one sweep (nms_run below); the stop is a template flag of the five-wave sweep.
#include "common.h"
#include "box_iou.h"

MQ_NAMESPACE_BEGIN
#ifdef MQ_PRIMARY_UNIT                                     // NMS works on fp32 boxes: one copy, in the fp16 translation unit

// boxes sorted by score (descending) per image; rows >= nvalid[b] are ignored.
__global__ __launch_bounds__(64) void nms_mask_kernel(const float* __restrict__ boxes, const int* __restrict__ labels,
                                                      const int* __restrict__ nvalid, unsigned long long* __restrict__ mask,
                                                      int N, int col_blocks, float thr) {
  const int b = blockIdx.z, row_blk = blockIdx.y, col_blk = blockIdx.x;
  const int n = nvalid[b];
  if (row_blk * 64 >= n || col_blk * 64 >= n || col_blk < row_blk) {
    // upper-triangular only; untouched words must still read as 0
    int i = row_blk * 64 + threadIdx.x;
    if (i < N) mask[((long)b * N + i) * col_blocks + col_blk] = 0ULL;
    return;
  }
  __shared__ float cb[64 * 4];
  __shared__ int cl[64];
  const float* bb = boxes + (long)b * N * 4;
  const int* lb = labels + (long)b * N;
  const int cj = col_blk * 64 + threadIdx.x;
  if (cj < n) {
    cb[threadIdx.x * 4 + 0] = bb[cj * 4 + 0]; cb[threadIdx.x * 4 + 1] = bb[cj * 4 + 1];
    cb[threadIdx.x * 4 + 2] = bb[cj * 4 + 2]; cb[threadIdx.x * 4 + 3] = bb[cj * 4 + 3];
    cl[threadIdx.x] = lb[cj];
  }
  __syncthreads();
  const int i = row_blk * 64 + threadIdx.x;
  unsigned long long t = 0ULL;
  if (i < n) {
    float a[4] = {bb[i * 4 + 0], bb[i * 4 + 1], bb[i * 4 + 2], bb[i * 4 + 3]};
    int la = lb[i];
    int cols = min(64, n - col_blk * 64);
    int start = (row_blk == col_blk) ? threadIdx.x + 1 : 0;
    for (int j = start; j < cols; ++j)
      if (ml_iou(a, la, cb + j * 4, cl[j]) > thr) t |= 1ULL << j;
  }
  if (i < N) mask[((long)b * N + i) * col_blocks + col_blk] = t;
}

// one wave per image; lane owns remv words {lane, lane+64, ...}
template <int SLOTS>
__global__ __launch_bounds__(64) void nms_sweep_kernel(const unsigned long long* __restrict__ mask,
                                                       const int* __restrict__ nvalid, unsigned char* __restrict__ keep,
                                                       int N, int col_blocks) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = nvalid[b];
  const unsigned long long* mb = mask + (long)b * N * col_blocks;
  unsigned char* kb = keep + (long)b * N;
  unsigned long long remv[SLOTS];
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) remv[s] = 0ULL;
  const int nchunks = (n + 63) / 64;
  for (int c = 0; c < nchunks; ++c) {
    const int i = c * 64 + lane;
    // word c of remv lives in lane (c % 64), slot (c / 64)
    unsigned long long word = 0ULL;
#pragma unroll
    for (int s = 0; s < SLOTS; ++s)
      if (s == c / 64) word = remv[s];
    word = __shfl(word, c % 64);
    unsigned long long diag = (i < n) ? mb[(long)i * col_blocks + c] : 0ULL;
    int alive = (i < n) && !((word >> lane) & 1ULL);
    for (int j = 0; j < 64; ++j) {
      int aj = __shfl(alive, j);
      unsigned long long dj = __shfl(diag, j);
      if (aj && ((dj >> lane) & 1ULL)) alive = 0;          // only bits > j are ever set in row j's diagonal word
    }
    if (i < N) kb[i] = (unsigned char)alive;
    unsigned long long alive_mask = __ballot(alive);
    while (alive_mask) {
      int r = __ffsll((long long)alive_mask) - 1;
      alive_mask &= alive_mask - 1;
      const unsigned long long* row = mb + (long)(c * 64 + r) * col_blocks;
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) {
        int w = lane + 64 * s;
        if (w > c && w < col_blocks) remv[s] |= row[w];
      }
    }
  }
  for (int i = nchunks * 64 + lane; i < N; i += 64) kb[i] = 0;
}

// Same sweep, five waves per image: waves 1-4 stream the 64-row block of mask words of chunk c + 2 into LDS (coalesced
// 16-byte loads, all of a wave's loads in flight before the first store, triple-buffered) while wave 0 resolves chunk c
// out of LDS.  The one-wave version above follows every surviving row with a dependent global load (~0.5 us each,
// ~5000 candidates): 1.0 ms per forward, all of it on the critical path.
// STOP: the sweep ends after the chunk in which the max_keep-th box is kept (a flag in LDS that all five waves read after the
// per-chunk barrier); without it max_keep is not read.
template <int SLOTS, bool STOP>
__global__ __launch_bounds__(320) void nms_sweep_lds_kernel(const unsigned long long* __restrict__ mask,
                                                            const int* __restrict__ nvalid, unsigned char* __restrict__ keep,
                                                            int N, int col_blocks, int max_keep) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long rows_s[];      // [3][64 * col_blocks]
  __shared__ int stop_s[2];     // [c & 1]: set by wave 0 in iteration c once max_keep boxes are kept.  Two slots: wave 0 may be an
                                // iteration ahead of a loader wave that has not yet read the flag of the previous one
  typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
  const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = nvalid[b];
  const unsigned long long* mb = mask + (long)b * N * col_blocks;
  unsigned char* kb = keep + (long)b * N;
  const int nchunks = (n + 63) / 64;
  const int blk = 64 * col_blocks;                          // words per chunk block (even)
  auto stage = [&](int c) {                                 // loader waves: chunk c -> buffer c % 3
    if (c >= nchunks) return;
    const unsigned long long* src = mb + (long)c * blk;
    const int avail = (min(N, c * 64 + 64) - c * 64) * col_blocks;       // words of rows that exist in the workspace
    unsigned long long* dst = rows_s + (c % 3) * blk;
    const int lt = (wave - 1) * 64 + lane;                  // 0..255
    constexpr int U = 8;
    for (int base = 0; base < blk; base += 256 * 2 * U) {
      u64x2 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int idx = base + (u * 256 + lt) * 2;
        v[u] = (u64x2){0ULL, 0ULL};
        if (idx + 1 < avail) v[u] = *(const u64x2*)(src + idx);
        else if (idx < avail) v[u][0] = src[idx];             // odd tail: never read past the workspace
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int idx = base + (u * 256 + lt) * 2;
        if (idx < blk) *(u64x2*)(dst + idx) = v[u];
      }
    }
  };
  if (wave > 0) { stage(0); stage(1); }
  if (STOP && threadIdx.x < 2) stop_s[threadIdx.x] = 0;
  __syncthreads();
  int kept = 0, c_end = nchunks;                            // c_end: first chunk that was not resolved
  unsigned long long remv[SLOTS];
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) remv[s] = 0ULL;
  for (int c = 0; c < nchunks; ++c) {
    if (wave > 0) {
      stage(c + 2);                                         // buffer (c + 2) % 3 was last read for chunk c - 1
    } else {
      const unsigned long long* L = rows_s + (c % 3) * blk;
      const int i = c * 64 + lane;
      unsigned long long word = 0ULL;                      // word c of remv lives in lane (c % 64), slot (c / 64)
#pragma unroll
      for (int s = 0; s < SLOTS; ++s)
        if (s == c / 64) word = remv[s];
      word = __shfl(word, c % 64);
      const unsigned long long diag = (i < n) ? L[lane * col_blocks + c] : 0ULL;
      int alive = (i < n) && !((word >> lane) & 1ULL);
      for (int j = 0; j < 64; ++j) {
        const int aj = __shfl(alive, j);
        const unsigned long long dj = __shfl(diag, j);
        if (aj && ((dj >> lane) & 1ULL)) alive = 0;        // only bits > j are ever set in row j's diagonal word
      }
      if (i < N) kb[i] = (unsigned char)alive;
      const unsigned long long alive_mask = __ballot(alive);
      if (STOP) {
        // boxes are sorted by score: the first max_keep survivors ARE the top max_keep of the kept set -- nothing that comes later can
        // enter the final selection (rpn/inference.py:757-766 keeps the max_keep highest scores of the NMS output), so the sweep ends here
        kept += __popcll(alive_mask);
        if (kept >= max_keep && lane == 0) stop_s[c & 1] = 1;
      }
      // OR the rows of the survivors into remv: LDS reads are issued 8 rows at a time, the test is wave-uniform.
      // (words <= c are OR-ed too: they belong to chunks already resolved and are never read again)
      for (int r0 = 0; r0 < 64; r0 += 8) {
        if (((alive_mask >> r0) & 0xFFULL) == 0ULL) continue;
        unsigned long long v[8][SLOTS];
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
          for (int s = 0; s < SLOTS; ++s) {
            const int w = lane + 64 * s;
            v[k][s] = (w < col_blocks) ? L[(r0 + k) * col_blocks + w] : 0ULL;
          }
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if ((alive_mask >> (r0 + k)) & 1ULL) {
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) remv[s] |= v[k][s];
          }
      }
    }
    __syncthreads();
    if (STOP && stop_s[c & 1]) { c_end = c + 1; break; }           // block-uniform: every wave reads the flag after the same barrier
  }
  if (wave == 0)
    for (int i = c_end * 64 + lane; i < N; i += 64) kb[i] = 0;
}

template <int SLOTS>
static int launch_sweep_lds(const unsigned long long* mask, const int* nvalid, unsigned char* keep, int B, int N, int col_blocks, int max_keep,
                            hipStream_t stream) {
  const size_t smem = (size_t)3 * 64 * col_blocks * sizeof(unsigned long long);
  if (max_keep) return mq_launch<nms_sweep_lds_kernel<SLOTS, true>>(dim3(B), dim3(320), smem, stream, mask, nvalid, keep, N, col_blocks, max_keep);
  return mq_launch<nms_sweep_lds_kernel<SLOTS, false>>(dim3(B), dim3(320), smem, stream, mask, nvalid, keep, N, col_blocks, max_keep);
}

// mask, then the sweep the size allows.  max_keep >= 1: the sweep that stops (five waves from LDS only: col_blocks <= 104); 0: all of keep.
static int nms_run(const float* boxes, const int* labels, const int* nvalid, void* workspace, unsigned char* keep, int B, int N, float thr,
                   int max_keep, hipStream_t stream) {
  const int col_blocks = (N + 63) / 64;
  if (col_blocks > (max_keep ? 104 : 256)) return -1;
  unsigned long long* mask = (unsigned long long*)workspace;
  hipLaunchKernelGGL(nms_mask_kernel, dim3(col_blocks, col_blocks, B), dim3(64), 0, stream, boxes, labels, nvalid, mask, N, col_blocks, thr);
  MQ_CHECK_LAUNCH();
  if (col_blocks <= 64)                                    // three 64-row blocks of mask words fit the 160 KB LDS
    return launch_sweep_lds<1>(mask, nvalid, keep, B, N, col_blocks, max_keep, stream);
  else if (col_blocks <= 104)
    return launch_sweep_lds<2>(mask, nvalid, keep, B, N, col_blocks, max_keep, stream);
  else if (col_blocks <= 128)
    hipLaunchKernelGGL((nms_sweep_kernel<2>), dim3(B), dim3(64), 0, stream, mask, nvalid, keep, N, col_blocks);
  else
    hipLaunchKernelGGL((nms_sweep_kernel<4>), dim3(B), dim3(64), 0, stream, mask, nvalid, keep, N, col_blocks);
  MQ_CHECK_LAUNCH();
  return 0;
}

extern "C" long mq_ml_nms_workspace_bytes(int B, int N) {
  long col_blocks = (N + 63) / 64;
  return (long)B * N * col_blocks * 8;
}

// boxes [B,N,4] fp32 sorted by score (descending) per image, labels [B,N] int32, nvalid [B] int32, workspace of mq_ml_nms_workspace_bytes(B, N)
// bytes -> keep [B,N] uint8, all of it written.  N <= 256 * 64; larger inputs: -1.
extern "C" int mq_ml_nms(const float* boxes, const int* labels, const int* nvalid, void* workspace, unsigned char* keep,
                         int B, int N, float thr, void* stream) {
  if (B <= 0 || N <= 0) return 0;
  return nms_run(boxes, labels, nvalid, workspace, keep, B, N, thr, 0, (hipStream_t)stream);
}

// the same with the sweep of an image ending once max_keep >= 1 boxes are kept (keep = 0 from the stopping chunk on).
// N <= 104 * 64 = 6656 (the LDS sweep); larger inputs: -1 (use mq_ml_nms).
extern "C" int mq_ml_nms_topk(const float* boxes, const int* labels, const int* nvalid, void* workspace, unsigned char* keep,
                              int B, int N, float thr, int max_keep, void* stream) {
  if (B <= 0 || N <= 0) return 0;
  if (max_keep < 1) return -2;
  return nms_run(boxes, labels, nvalid, workspace, keep, B, N, thr, max_keep, (hipStream_t)stream);
}
#endif

MQ_NAMESPACE_END
