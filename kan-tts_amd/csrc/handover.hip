// The hand-over between the two streaming halves: final post-net rows of every acoustic slot (channels-last, the `y` buffer
// of AcousticSlots) become the step input of the chunked vocoder (channels-first), in ONE launch per step and without a
// trip to the host.  Per slot s, with start_s = clamp(start[s], 0, T) and n_s = clamp(rows[s], 0, min(Tc, T - start_s)):
//     out[s][c][t] = t < n_s ? f_c(src[s][start_s + t][c]) : 0.0f                       c < C, t < Tc
// Nothing outside rows [start_s, start_s + n_s) of a slot is read; every element of out is written.  start and rows live on
// the device and are not read back: an out-of-range value acts as its clamp.
//
// f_c is the identity, except with nsf != 0 for the last two channels, which an NSF acoustic model predicts behind the mel
// bins (infer_sambert.denorm_f0; reference kantts/bin/infer_sambert.py:26-56):
//     c == C - 2 (f0):      fmaxf(v * scale + offset, f0_floor)       Hz, floored
//     c == C - 1 (voicing): v < uv_threshold ? 0.0f : 1.0f
// The product and the sum round SEPARATELY (contraction is switched off for that expression), so the result has the bits of
// numpy's fp32 `mel * scale + offset`; a fused multiply-add would differ in the last place for some values.
//
// Form: a transpose through LDS.  A workgroup owns a tile of 32 frames x 64 channels of one slot; it reads the tile with the
// channel fastest (one 16-byte load per lane when C % 4 == 0 and src is 16-byte aligned, 4-byte loads otherwise -- C = 82
// of the NSF voices), parks it in LDS at a row stride of 65 floats, and writes it with the frame fastest: a 32-lane half of
// a wave reads one LDS column (banks (t * 65 + c) % 32 = (t + c) % 32: all different) and stores 32 consecutive floats of
// one channel row of out.  The 16-byte form's four LDS writes per lane land two lanes on a bank (stride 4 over 16 lanes);
// at tens of kilobytes per launch that is not worth a swizzle.  A tile wholly at or after n_s is zero-filled without a load.
#include "common.h"

#define HO_TT 32        // frames per tile
#define HO_TC 64        // channels per tile
#define HO_LD 65        // LDS row stride in floats (odd: a column read touches 32 different banks)
#define HO_THREADS 256

// fp32 v * scale + offset with two roundings, whatever the compiler's contraction default
__device__ __forceinline__ float ho_scale_offset(float v, float scale, float offset) {
#pragma clang fp contract(off)
  const float p = v * scale;
  return p + offset;
}

template <int VEC>
__global__ __launch_bounds__(HO_THREADS) void mel_handover_kernel(const float* __restrict__ src,
                                                                  const int* __restrict__ start,
                                                                  const int* __restrict__ rows, float* __restrict__ out,
                                                                  int T, int C, int Tc, int nsf, float scale, float offset,
                                                                  float f0_floor, float uv_threshold) {
  __shared__ float tile[HO_TT * HO_LD];
  const int s = blockIdx.z;
  const int t0 = blockIdx.x * HO_TT, c0 = blockIdx.y * HO_TC;
  const int tid = threadIdx.x;
  const int a = min(max(start[s], 0), T);
  const int n = min(min(max(rows[s], 0), Tc), T - a);
  const int live = min(max(n - t0, 0), HO_TT);  // live frames of this tile: workgroup-uniform
  if (live > 0) {
    const float* sp = src + ((long long)s * T + a + t0) * C + c0;
    constexpr int LANES = HO_TC / VEC;           // lanes along the channels
    constexpr int ROWS = HO_THREADS / LANES;     // frames per pass
    const int cl = (tid % LANES) * VEC, tr = tid / LANES;
#pragma unroll
    for (int t = tr; t < HO_TT; t += ROWS) {
      if (t < live && c0 + cl < C) {             // C % VEC == 0: a lane's VEC channels exist together
        if (VEC == 4) {
          const float4 v = *reinterpret_cast<const float4*>(sp + (long long)t * C + cl);
          float* d = tile + t * HO_LD + cl;
          d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
        } else {
          tile[t * HO_LD + cl] = sp[(long long)t * C + cl];
        }
      }
    }
    __syncthreads();
  }
  const int tl = tid % HO_TT, t = t0 + tl;
  if (t >= Tc) return;
  for (int c = tid / HO_TT; c < HO_TC && c0 + c < C; c += HO_THREADS / HO_TT) {
    const int cg = c0 + c;
    float v = 0.f;
    if (tl < live) {
      v = tile[tl * HO_LD + c];
      if (nsf && cg >= C - 2)
        v = cg == C - 2 ? fmaxf(ho_scale_offset(v, scale, offset), f0_floor) : (v < uv_threshold ? 0.f : 1.f);
    }
    out[((long long)s * C + cg) * Tc + t] = v;
  }
}

extern "C" int kantts_mel_handover_rows(const float* src, const int32_t* start, const int32_t* rows, float* out, int S, int T,
                                        int C, int Tc, int nsf, float scale, float offset, float f0_floor,
                                        float uv_threshold, void* stream) {
  if (!src || !start || !rows || !out || S < 0 || Tc < 0 || T < 1 || C < 1 || (nsf && C < 3)) return KANTTS_E_BADARG;
  if (S == 0 || Tc == 0) return KANTTS_OK;
  if (S > 65535 || kantts_cdiv(C, HO_TC) > 65535) return KANTTS_E_UNSUPPORTED;
  const dim3 grid((unsigned)kantts_cdiv(Tc, HO_TT), (unsigned)kantts_cdiv(C, HO_TC), (unsigned)S);
  const int* st = reinterpret_cast<const int*>(start);
  const int* rw = reinterpret_cast<const int*>(rows);
  if (C % 4 == 0 && reinterpret_cast<uintptr_t>(src) % 16 == 0)
    hipLaunchKernelGGL((mel_handover_kernel<4>), grid, dim3(HO_THREADS), 0, (hipStream_t)stream, src, st, rw, out, T, C, Tc,
                       nsf, scale, offset, f0_floor, uv_threshold);
  else
    hipLaunchKernelGGL((mel_handover_kernel<1>), grid, dim3(HO_THREADS), 0, (hipStream_t)stream, src, st, rw, out, T, C, Tc,
                       nsf, scale, offset, f0_floor, uv_threshold);
  KANTTS_CHECK_LAUNCH();
}
