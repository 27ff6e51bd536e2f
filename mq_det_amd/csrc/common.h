// Shared device helpers for the MQ-Det gfx950 (CDNA4 / MI355X) kernels.
// Wavefront = 64 lanes.  MFMA tile used everywhere: v_mfma_f32_16x16x32_f16
//   A frag: lane l holds A[row = l&15][k = 8*(l>>4) .. +7]      (8 halfs = 16 B, K-contiguous)
//   B frag: lane l holds B[k = 8*(l>>4) .. +7][col = l&15]      (same bytes as a row of B^T)
//   C/D   : lane l holds C[row = 4*(l>>4) + r][col = l&15], r = 0..3
// so every contraction here is written in "NT" form: both operands K-contiguous in memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <type_traits>

// Element type of the 16-bit operands.  Every kernel source is compiled TWICE (mq_det_amd/build.py): as is -- half_t = fp16, the
// entry points of include/mqdet_hip.h -- and with -DMQ_BF16 -- half_t = bf16 (v_mfma_f32_16x16x32_bf16), entry points with the
// suffix _bf16, everything inside namespace mq_bf16 (BASELINE.json configs[3]: "MQ-GLIP-L ... bf16 MFMA").  Without the macro
// MQ_SYM / MQ_NAMESPACE_* expand to nothing: the fp16 objects are token-for-token what they were before the switch existed.
#if defined(MQ_F32)
// fp32-OPERAND build (the "precise mode", MODEL.COMPUTE_DTYPE = "float32"; entry points *_f32, namespace mq_f32): every 16-bit operand of
// the kernel sources is a float and one 16x16x32 MFMA is THREE fp16 MFMAs on the split operands hi + lo (mfma16 below; round 5: eight
// v_mfma_f32_16x16x4_f32, still there under -DMQ_F32_EXACT).  What is left between such a run and the fp32 reference is summation order and
// 2^-22 per operand, not fp16 operand rounding: the north-star's 1e-3 end to end.
typedef float half_t;
typedef float half8 __attribute__((ext_vector_type(8)));
typedef float half4 __attribute__((ext_vector_type(4)));
typedef float half2_ __attribute__((ext_vector_type(2)));
#define MQ_SYM(name) name##_f32
#define MQ_NAMESPACE_BEGIN namespace mq_f32 {
#define MQ_NAMESPACE_END }
#elif defined(MQ_BF16)
typedef __bf16 half_t;
typedef __bf16 half8 __attribute__((ext_vector_type(8)));
typedef __bf16 half4 __attribute__((ext_vector_type(4)));
typedef __bf16 half2_ __attribute__((ext_vector_type(2)));
#define MQ_SYM(name) name##_bf16
#define MQ_NAMESPACE_BEGIN namespace mq_bf16 {
#define MQ_NAMESPACE_END }
#else
typedef _Float16 half_t;
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef _Float16 half2_ __attribute__((ext_vector_type(2)));
#define MQ_SYM(name) name
#define MQ_NAMESPACE_BEGIN
#define MQ_NAMESPACE_END
#endif
// code that sees no 16-bit data (NMS, selection, size queries) exists once, in the fp16 translation unit
#if !defined(MQ_BF16) && !defined(MQ_F32)
#define MQ_PRIMARY_UNIT 1
#endif
#if defined(MQ_F32)
// the precise mode also drops the hardware approximations of exp / reciprocal the 16-bit builds use beside their MFMAs (v_exp_f32 on a
// pre-multiplied argument: a relative error of ~|x| 2^-24 per softmax term; v_rcp_f32: 1 ulp): library exp / exp2 and IEEE division
#define __expf(x) expf(x)
#define __builtin_amdgcn_exp2f(x) exp2f(x)
#define __builtin_amdgcn_rcpf(x) (1.0f / (x))
#endif
typedef float float4_ __attribute__((ext_vector_type(4)));
typedef float float2_ __attribute__((ext_vector_type(2)));

#define MQ_NEG_BIG (-1.0e30f)

// 1: the split-precise build -- fp32 operands carried through the fp16 matrix cores as (hi, lo) pairs (below); 0: the 16-bit builds (and -DMQ_F32_EXACT)
#if defined(MQ_F32) && !defined(MQ_F32_EXACT)
#define MQ_SPLIT_OPERANDS 1
#else
#define MQ_SPLIT_OPERANDS 0
#endif

#if MQ_SPLIT_OPERANDS
// The SPLIT-PRECISE contraction (round 6; VERDICT r5 #1b).  An fp32 operand x is carried through the fp16 matrix cores as x = hi + lo / 2^11:
//   hi = fp16(x)                      (11 significant bits, round to nearest even)
//   lo = fp16((x - hi) * 2^11)        (x - hi is exact in fp32; the power-of-two pre-scale keeps lo a NORMAL fp16 number wherever hi is one)
// and a . b ~ hi_a hi_b + (hi_a lo_b + lo_a hi_b) / 2^11: three v_mfma_f32_16x16x32_f16 with fp32 accumulation on the SAME fragments and the
// same accumulator layout.  Every fp16 x fp16 product is exact in fp32 (22 bits); what is dropped is lo_a lo_b (2^-22 relative) and the
// rounding of lo (2^-22 relative): operands to ~22 bits instead of fp16's 11 -- at 3/16 of the fp16 matrix rate instead of the 1/16 of eight
// v_mfma_f32_16x16x4_f32 (kept under -DMQ_F32_EXACT).  Range = fp16's (|x| <= 65504), like the 16-bit builds of the same kernels.
typedef _Float16 mq_h16x8 __attribute__((ext_vector_type(8)));
struct mq_split8 { mq_h16x8 hi, lo; };
__device__ __forceinline__ mq_split8 mq_split(half8 x) {
  mq_split8 s;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const _Float16 h = (_Float16)x[i];
    s.hi[i] = h;
    s.lo[i] = (_Float16)(__builtin_fmaf((float)h, -1.0f, x[i]) * 2048.0f);
  }
  return s;
}
__device__ __forceinline__ float4_ mfma16_split(const mq_split8& a, const mq_split8& b, float4_ c) {
#if defined(MQ_SIMT_EMULATION)
  return simt_mfma_16x16x32_split_frag(a.hi, a.lo, b.hi, b.lo, c);   // tests/simt: the three products below in one lane exchange
#else
  float4_ t = {0.f, 0.f, 0.f, 0.f};
  c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.hi, b.hi, c, 0, 0, 0);
  t = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.hi, b.lo, t, 0, 0, 0);
  t = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.lo, b.hi, t, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r) c[r] = __builtin_fmaf(t[r], 1.0f / 2048.0f, c[r]);
  return c;
#endif
}
// the same split for 4 elements (a 16-byte chunk of fp32 operands on its way into a planar hi / lo LDS tile: dcn_fused.hip, vlfuse_attn.hip)
typedef _Float16 mq_h16x4 __attribute__((ext_vector_type(4)));
typedef float mq_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void mq_split4(mq_f32x4 x, mq_h16x4& hi, mq_h16x4& lo) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const _Float16 h = (_Float16)x[i];
    hi[i] = h;
    lo[i] = (_Float16)(__builtin_fmaf((float)h, -1.0f, x[i]) * 2048.0f);
  }
}
#endif

__device__ __forceinline__ float4_ mfma16(half8 a, half8 b, float4_ c) {
#if MQ_SPLIT_OPERANDS
#if defined(MQ_SIMT_EMULATION)
  return simt_mfma_16x16x32_split(a, b, c);         // tests/simt: the same split and the same three products, one lane exchange instead of three
#else
  return mfma16_split(mq_split(a), mq_split(b), c); // the splits of a fragment that feeds several MFMAs are common subexpressions: computed once
#endif
#elif defined(MQ_F32)
  // v_mfma_f32_16x16x4_f32: lane l holds A[l & 15][k = l >> 4] and B[k = l >> 4][l & 15]; step j contracts the k values 8 g + j (g = l >> 4)
  // of the 16x16x32 fragments, so the eight steps together are the same 32-deep contraction with exact fp32 products
#if defined(MQ_SIMT_EMULATION)
  return simt_mfma_16x16x32_f32_8x4(a, b, c);       // tests/simt: the same eight steps in the same order, one lane exchange instead of eight
#else
#pragma unroll
  for (int j = 0; j < 8; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], c, 0, 0, 0);
  return c;
#endif
#elif defined(MQ_BF16)
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
#else
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
#endif
}

// An MFMA operand fragment as the kernels keep it when it feeds SEVERAL MFMAs: the split-precise build splits it once (mq_to_frag) into (hi, lo)
// and contracts the pairs; in the other builds it is the half8 itself.
#if MQ_SPLIT_OPERANDS
typedef mq_split8 mq_frag;
__device__ __forceinline__ mq_frag mq_to_frag(half8 x) { return mq_split(x); }
__device__ __forceinline__ float4_ mq_frag_mfma(const mq_frag& a, const mq_frag& b, float4_ c) { return mfma16_split(a, b, c); }
#else
typedef half8 mq_frag;
__device__ __forceinline__ mq_frag mq_to_frag(half8 x) { return x; }
__device__ __forceinline__ float4_ mq_frag_mfma(mq_frag a, mq_frag b, float4_ c) { return mfma16(a, b, c); }
#endif

// compile-time loop: f(std::integral_constant<int, 0>{}) ... f(std::integral_constant<int, N - 1>{})
template <int I, int N, class F>
__device__ __forceinline__ void mq_static_for_impl(F& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    mq_static_for_impl<I + 1, N>(f);
  }
}
template <int N, class F>
__device__ __forceinline__ void mq_static_for(F f) { mq_static_for_impl<0, N>(f); }

__device__ __forceinline__ half8 zero8() {
  half8 z;
#pragma unroll
  for (int i = 0; i < 8; ++i) z[i] = (half_t)0.f;
  return z;
}

// 4 x 16 block of operand elements, row-major in LDS (row pitch free), read column-wise: within a 16-lane group lane i passes the address of
// the 4 contiguous elements (row i / 4, columns 4 (i % 4) .. + 3) and receives (rows 0 .. 3, column i).  16-bit builds: ds_read_b64_tr_b16;
// fp32-operand build: the same exchange for 4-byte elements -- the addresses cross the lanes by shuffle, four scalar LDS reads.
typedef __fp16 mq_fp16x4_t __attribute__((__vector_size__(8)));
__device__ __forceinline__ half4 lds_read_tr16(const half_t* p) {
#if defined(MQ_F32)
  const int l = __lane_id(), base = l & ~15, i = l & 15;
  half4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const half_t* src = (const half_t*)__shfl((unsigned long long)p, base + 4 * j + (i >> 2));
    o[j] = src[i & 3];
  }
  return o;
#else
  mq_fp16x4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) mq_fp16x4_t*)p);
  half4 o;
  __builtin_memcpy(&o, &v, 8);
  return o;
#endif
}

// the same transposed read on an fp16 plane, in EVERY build (the planar hi / lo tiles of the split-precise kernels are fp16 whatever half_t is)
typedef _Float16 mq_h16x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ mq_h16x4_t lds_read_tr16_h(const _Float16* p) {
  mq_fp16x4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) mq_fp16x4_t*)p);
  mq_h16x4_t o;
  __builtin_memcpy(&o, &v, 8);
  return o;
}

// One 8-element operand fragment per lane, global -> LDS: lane l's fragment `src_lane` lands at dst_base + 8 l (dst_base wave-uniform).
// 16-bit builds: LDS-DMA (global_load_lds_dwordx4: no VGPRs, asynchronous -- the caller waits with vmcnt before its barrier);
// fp32-operand build: a 32-byte copy through registers that is complete when the call returns (a legal refinement of the asynchronous copy).
__device__ __forceinline__ void lds_stage_frag8(const half_t* src_lane, half_t* dst_base, int lane) {
#if defined(MQ_F32)
  *(half8*)(dst_base + lane * 8) = *(const half8*)src_lane;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#else
  (void)lane;
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src_lane, (__attribute__((address_space(3))) void*)dst_base, 16, 0, 0);
#endif
}

// The same copy with the source as (raw buffer over the array, wave-uniform element offset `eoff`, lane-linear fragments): the 16-bit builds issue
// the MUBUF form `buffer_load_dwordx4 ... lds`.  Why not global_load_lds: hipcc's wait-count pass books that FLAT-encoded instruction as a flat
// access that may touch LDS AND memory ("pending flat" -- vmcnt and lgkmcnt no longer count in order for it) and from then on every s_waitcnt of
// the loop is vmcnt(0) / lgkmcnt(0): a register ring of fragment reads "six deep" waits for its NEWEST read at every MFMA (round 6: the ISA of the
// Swin MLP loop had no other wait than lgkmcnt(0)).  The MUBUF form is a vector-memory load to it; counted waits stay counted.
typedef __amdgpu_buffer_rsrc_t mq_rsrc;
__device__ __forceinline__ mq_rsrc mq_raw_buffer(const void* base) { return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 0x7fffffff, 0x00020000); }
// lane l's fragment = base[eoff + leoff .. + 8), eoff wave-uniform (scalar offset), leoff per lane (vector offset; lane-linear sources: 8 l)
__device__ __forceinline__ void lds_stage_frag8_buf(mq_rsrc r, const half_t* base, int eoff, int leoff, half_t* dst_base, int lane) {
#if defined(MQ_F32)
  (void)r;
  lds_stage_frag8(base + eoff + leoff, dst_base, lane);
#else
  (void)base; (void)lane;
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)dst_base, 16, leoff * (int)sizeof(half_t), eoff * (int)sizeof(half_t), 0, 0);
#endif
}
// 16 raw bytes per lane (lane-linear destination as above), every build
__device__ __forceinline__ void lds_stage_16b_buf(mq_rsrc r, int boff, int lboff, void* dst_base) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)dst_base, 16, lboff, boff, 0, 0);
}

// reduce across the 16 lanes that share (lane >> 4): lanes differ in their low 4 bits
__device__ __forceinline__ float group16_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 1));
  v = fmaxf(v, __shfl_xor(v, 2));
  v = fmaxf(v, __shfl_xor(v, 4));
  v = fmaxf(v, __shfl_xor(v, 8));
  return v;
}
__device__ __forceinline__ float group16_sum(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// Make this wave's earlier LDS writes visible to its own later LDS reads (other lanes of the SAME wave).
// LDS ops of one wave retire in order; the explicit wait + scheduling barrier keeps the compiler honest.
__device__ __forceinline__ void wave_lds_fence() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// The CU count is a per-DEVICE property: a process that drives several GPUs (one host thread each) reads it once per device.
static inline int mq_device_cus() {
  static std::atomic<int> cus[32] = {};
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 32) return 256;
  if (!(n = cus[dev].load(std::memory_order_relaxed))) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

#define MQ_CHECK_LAUNCH()                                   \
  do {                                                      \
    hipError_t e__ = hipGetLastError();                     \
    if (e__ != hipSuccess) return (int)e__;                 \
  } while (0)

// Every launch with dynamic LDS: raise the kernel's limit (hipFuncSetAttribute, needed above 64 KB) where this device has not seen that
// many bytes for THIS kernel yet, launch, return the launch's error code.  The largest size set so far is kept per device in a static of
// the function template -- one per kernel instantiation, nothing to list.  A failed attribute call is returned without a launch and without
// a mark (the next call tries again); with an unknown device index the attribute is set on every call.
template <auto Kernel, class... A>
static int mq_launch(dim3 grid, dim3 block, size_t smem, hipStream_t stream, const A&... args) {
  if (smem) {
    static std::atomic<size_t> max_[32] = {};
    int dev = -1;
    const bool known = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 32;
    if (!known || smem > max_[dev].load(std::memory_order_relaxed)) {
      hipError_t e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
      if (e != hipSuccess) return (int)e;
      if (known) max_[dev].store(smem, std::memory_order_relaxed);
    }
  }
  hipLaunchKernelGGL(Kernel, grid, block, smem, stream, args...);
  return (int)hipGetLastError();
}
