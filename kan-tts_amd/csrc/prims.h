// The small primitives every kernel file needs: vector typedefs, bf16 pack / unpack, 16-float rows, the LDS-only barrier,
// the XCD tile order, the device seed word, and the host-side alignment test and dynamic-LDS limit.  Included by common.h;
// new kernels take these from here instead of declaring a file-local copy.
#pragma once

#include <atomic>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
// operand of the transposing LDS read (ds_read_b64_tr_b16)
typedef __attribute__((address_space(3))) bf16x4 kantts_lds_bf16x4;

// ---------------------------------------------------------------------------------------------
// Two floats rounded to bf16 (nearest even), a in the low half of the word.  Two spellings of one value: the compiler
// schedules and allocates registers around them differently, and each kernel keeps the one it was tuned and measured with.
// kantts_pack2: enc_attn.hip, upsample.hip, norm.hip.  kantts_pack2_of4 (through a 4-vector with two zero lanes):
// cconv.hip, ffn_pair.hip, gemm_bf16.hip, pnca_block.hip.  New kernels use kantts_pack2.
__device__ __forceinline__ unsigned kantts_pack2(float a, float b) {
  bf16x2 t = {(__bf16)a, (__bf16)b};
  return (unsigned&)t;
}
__device__ __forceinline__ unsigned kantts_pack2_of4(float a, float b) {
  bf16x4 t = {(__bf16)a, (__bf16)b, (__bf16)0.f, (__bf16)0.f};
  return ((u32x2&)t).x;
}
__device__ __forceinline__ float kantts_bf16_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float kantts_bf16_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }

// ---------------------------------------------------------------------------------------------
// Rows of 16 floats (one attention head), 16-byte aligned: global or LDS to registers and back, dot products.
__device__ __forceinline__ void kantts_load16(const float* p, float* r) {
  const float4* p4 = reinterpret_cast<const float4*>(p);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float4 t = p4[e];
    r[4 * e + 0] = t.x;
    r[4 * e + 1] = t.y;
    r[4 * e + 2] = t.z;
    r[4 * e + 3] = t.w;
  }
}
__device__ __forceinline__ void kantts_store16(float* p, const float* r) {
  float4* p4 = reinterpret_cast<float4*>(p);
#pragma unroll
  for (int e = 0; e < 4; ++e) p4[e] = make_float4(r[4 * e], r[4 * e + 1], r[4 * e + 2], r[4 * e + 3]);
}
__device__ __forceinline__ float kantts_dot16(const float* a, const float* b) {
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < 16; ++d) s = fmaf(a[d], b[d], s);
  return s;
}
__device__ __forceinline__ void kantts_lds16(const float* p, float* r) { kantts_load16(p, r); }
__device__ __forceinline__ float kantts_dot16l(const float* a, const float* lrow) {
  float b[16];
  kantts_lds16(lrow, b);
  return kantts_dot16(a, b);
}

// ---------------------------------------------------------------------------------------------
// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains the vector-memory counter, i.e. it waits
// until the step's global STORES (saved gates / cell state / outputs: pure outputs, never re-read by this kernel) have
// been acknowledged by L2 -- two or three such round trips on the critical path of every time step.  The host build of the
// kernel sources (tests/hipemu) has no such counters: there it is the plain barrier.
__device__ __forceinline__ void kantts_lds_barrier() {
#ifdef KANTTS_HOSTSIM
  __syncthreads();
#else
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#endif
}

// XCD-aware tile order.  The dispatcher deals workgroup L of a launch to XCD L % 8, each with its own L2; this gives
// XCD k a contiguous band of the `total` tiles instead (slot k*q + min(k, r) + j for L = 8*j + k, total = 8*q + r), so
// neighbouring tiles share one L2.  Callers apply it from 64 workgroups up (eight per XCD), decompose the slot into their
// own tile coordinates and keep their own switch.  (`total` comes first on purpose: the compiler orders the operands of
// k * q by the position of the parameters they derive from, and only this order reproduces the hand-written form.)
__device__ __forceinline__ int kantts_xcd_slot(int total, int linear_id) {
  const int k = linear_id & 7, j = linear_id >> 3;
  const int q = total >> 3, r = total & 7;
  return k * q + (k < r ? k : r) + j;
}

// The device word added to every dropout / noise seed of a launch (a captured step advances it on the device); NULL = 0.
__device__ __forceinline__ uint64_t kantts_seed_offset(const uint64_t* seed_dev) { return seed_dev ? *seed_dev : 0ull; }

// ---------------------------------------------------------------------------------------------
// Host side.
static inline bool kantts_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// Raises the dynamic-LDS limit of KERNEL to `bytes` on the current device; returns the HIP error code (0 = done).  The
// attribute belongs to the device, so what is remembered is a mask of device ordinals per kernel (one instantiation of
// this template each): the first launch on every device sets it, later ones only read the mask.  An ordinal that does
// not fit the mask sets the attribute on every call.
#if defined(KANTTS_HOSTSIM) && !defined(HIPEMU_HAS_DEVICES)
// a host stand-in for the HIP runtime that knows no devices (tests/hipemu before it had them): everything is device 0
static inline hipError_t hipGetDevice(int* ordinal) { *ordinal = 0; return hipSuccess; }
#endif
template <auto KERNEL>
static int kantts_allow_dynamic_lds(int bytes) {
  static std::atomic<uint64_t> done{0};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return (int)e;
  const uint64_t bit = (dev >= 0 && dev < 64) ? (1ull << dev) : 0ull;
  if (done.load(std::memory_order_acquire) & bit) return 0;
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) return (int)e;
  done.fetch_or(bit, std::memory_order_release);
  return 0;
}
