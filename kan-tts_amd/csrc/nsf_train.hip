// The NSF excitation in TRAINING: what a captured GAN step needs beside kantts_nsf_source_rows (csrc/nsf_source.hip), which
// is the forward as it stands (S = batch, Tc = frames of the batch, rows = NULL, the drawn words as state_in).
//
// kantts_nsf_draw_states -- the device twin of kantts.models.hifigan.chunked_nsf.initial_state.  The host function derives a
//   slot's starting words from (seed, key); here {seed, counter} live in DEVICE memory and item s of draw number `counter`
//   plays utterance key (counter << 20) | s:
//     key64     = mix(mix(seed, 0x4E5346), (counter << 20) | s)                      (slot_key)
//     phase0[h] = (float)(((mix(key64, 2^63 + h) >> 40) / 2^24 * 2 - 1) * pi)       h in [1, H1); fp64, ONE rounding
//     words     = {phase[16] = 0, phase0[0] = 0, phase0[1 .. H1), 0 ..., cursor = 0, key64}
//   and the launch leaves counter + 1 behind, so the replay of a captured launch draws new numbers.  One workgroup: every
//   thread reads both words, a barrier, then thread 0 stores the new counter -- no thread can read the counter it wrote.
//   A thread owns (item, word) pairs with the word fastest: plain coalesced 32-bit vector stores, the KANTTS_NSF_STATE_WORDS
//   words of every item and nothing between items.
//
// kantts_nsf_source_wgrad -- the backward of the projection e = tanh(bias + sum_h w[h] * x_h):
//     dpre[s, n] = de[s, n] * (1 - e[s, n]^2)         evaluated as de * ((1 - e) * (1 + e)): 1 - e is exact for e >= 1/2, so
//                                                     a saturated tanh costs no cancellation
//     dw[h]      = sum_{s, n} dpre[s, n] * x_h[s, n],     dbias = sum_{s, n} dpre[s, n]
//   x_h is NOT stored by the forward ((S, T, H1) floats that only this kernel would read): it is recomputed from the same
//   f0 / uv / state_in / noise through nsf_harmonic of nsf_source_body.inc, the function the forward calls -- same bits.
//   Two launches, no atomics, the same bits from run to run:
//     1. one workgroup per (item, frame), the grid of the forward: a thread adds its samples' H1 + 1 products into its own
//        LDS column, a fixed binary tree over the 256 columns, H1 + 1 partial sums to ws[(s * Tc + k) * (H1 + 1) + c];
//     2. one workgroup per c: thread t adds partials t, t + 256, ... in this order, the same tree, dw[c] (c < H1) / dbias.
//   The second launch starts behind the first on the stream: no workgroup waits for another inside a launch.
#include "nsf_source_body.inc"

#define NSF_DRAW_MAX_S (1 << 20)

__global__ __launch_bounds__(NSF_THREADS) void nsf_draw_kernel(uint64_t* words, int S, int H1, int32_t* state_out,
                                                               long long state_ss) {
  const uint64_t seed = words[0], counter = words[1];
  __syncthreads();  // every thread holds both words before the counter moves
  if (threadIdx.x == 0) words[1] = counter + 1;
  const uint64_t base = kantts_rng_mix(seed, 0x4E5346ull);
  const int total = S * KANTTS_NSF_STATE_WORDS;  // < 2^20 * 36
  for (int i = threadIdx.x; i < total; i += NSF_THREADS) {
    const int s = i / KANTTS_NSF_STATE_WORDS, w = i - s * KANTTS_NSF_STATE_WORDS;
    int32_t v = 0;
    const int h = w - NSF_MAXH1;
    if ((h >= 1 && h < H1) || w >= 2 * NSF_MAXH1 + 2) {
      const uint64_t key = kantts_rng_mix(base, (counter << 20) | (uint64_t)s);
      if (w >= 2 * NSF_MAXH1 + 2) {
        v = (int32_t)(uint32_t)(w == 2 * NSF_MAXH1 + 2 ? key : key >> 32);
      } else {
        const uint64_t r = kantts_rng_mix(key, (1ull << 63) + (uint64_t)h);
        const double p = ((double)(r >> 40) / 16777216.0 * 2.0 - 1.0) * 3.141592653589793;
        v = __float_as_int((float)p);
      }
    }
    state_out[(long long)s * state_ss + w] = v;
  }
}

extern "C" int kantts_nsf_draw_states(uint64_t* seed_counter, int S, int H1, int32_t* state_out, long long state_ss,
                                      void* stream) {
  if (!seed_counter || !state_out || ((uintptr_t)seed_counter & 7) || ((uintptr_t)state_out & 7)) return KANTTS_E_BADARG;
  if (H1 < 1 || (state_ss & 1) || (S > 1 && state_ss < KANTTS_NSF_STATE_WORDS)) return KANTTS_E_BADARG;
  if (S < 1 || S >= NSF_DRAW_MAX_S || H1 > NSF_MAXH1) return KANTTS_E_UNSUPPORTED;
  hipLaunchKernelGGL(nsf_draw_kernel, dim3(1), dim3(NSF_THREADS), 0, (hipStream_t)stream, seed_counter, S, H1, state_out,
                     state_ss);
  KANTTS_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------
// s_acc[c][t]: column t is thread t's; sums every column c < n into s_acc[c][0] (256 -> 1 by halves, the same order always)
__device__ __forceinline__ void nsf_tree_sum(float (*s_acc)[NSF_THREADS], int n) {
  const int tid = threadIdx.x;
  for (int half = NSF_THREADS / 2; half > 0; half >>= 1) {
    __syncthreads();
    if (tid < half)
      for (int c = 0; c < n; ++c) s_acc[c][tid] += s_acc[c][tid + half];
  }
  __syncthreads();
}

__global__ __launch_bounds__(NSF_THREADS) void nsf_wgrad_frame_kernel(const kantts_nsf_source_args g, const float* de,
                                                                      float* ws) {
  __shared__ nsf_source_lds lds;
  __shared__ float s_acc[NSF_MAXH1 + 1][NSF_THREADS];
  const int H1 = g.H1, hop = g.hop;
  const int tid = threadIdx.x;
  const int s = blockIdx.x / g.Tc, k = blockIdx.x - s * g.Tc;
  const nsf_state* si = reinterpret_cast<const nsf_state*>(g.state_in + (long long)s * g.state_ss);
  nsf_frame_phases(g, s, k, lds);
  for (int c = 0; c <= H1; ++c) s_acc[c][tid] = 0.f;
  __syncthreads();
  const float uv = g.uv[(long long)s * g.Tc + k];
  const float unv = g.alpha / 3.f / g.sigma;
  const uint64_t key = si->key;
  const uint64_t n0 = si->cursor + (uint64_t)k * (uint64_t)hop;
  for (int j = tid; j < hop; j += NSF_THREADS) {
    const long long o = ((long long)s * g.Tc + k) * hop + j;
    const float ev = g.e[o];
    const float dpre = de[o] * ((1.f - ev) * (1.f + ev));
    float z1 = 0.f;
    for (int h = 0; h < H1; ++h) {
      const float x = nsf_harmonic(g, lds, h, j, o, key, n0 + (uint64_t)j, uv, unv, z1);
      s_acc[h][tid] += dpre * x;
    }
    s_acc[H1][tid] += dpre;
  }
  nsf_tree_sum(s_acc, H1 + 1);
  if (tid <= H1) ws[(long long)blockIdx.x * (H1 + 1) + tid] = s_acc[tid][0];
}

__global__ __launch_bounds__(NSF_THREADS) void nsf_wgrad_sum_kernel(const float* ws, int parts, int H1, float* dw,
                                                                    float* dbias) {
  __shared__ float s_acc[1][NSF_THREADS];
  const int c = blockIdx.x, tid = threadIdx.x;
  float acc = 0.f;
  for (int i = tid; i < parts; i += NSF_THREADS) acc += ws[(long long)i * (H1 + 1) + c];
  s_acc[0][tid] = acc;
  nsf_tree_sum(s_acc, 1);
  if (tid == 0) {
    if (c < H1)
      dw[c] = s_acc[0][0];
    else if (dbias)
      dbias[0] = s_acc[0][0];
  }
}

extern "C" int kantts_nsf_source_wgrad(const kantts_nsf_wgrad_args* a, void* stream) {
  if (!a) return KANTTS_E_BADARG;
  if (!a->f0 || !a->uv || !a->state_in || !a->e || !a->de || !a->dw || !a->ws) return KANTTS_E_BADARG;
  if (a->S < 1 || a->Tc < 1 || a->hop < 1 || a->H1 < 1 || !(a->sr > 0.f) || !(a->sigma > 0.f)) return KANTTS_E_BADARG;
  if (a->S > 1 && a->state_ss < KANTTS_NSF_STATE_WORDS) return KANTTS_E_BADARG;
  if (a->H1 > NSF_MAXH1) return KANTTS_E_UNSUPPORTED;
  if (((uintptr_t)a->state_in & 7) || (a->state_ss & 1) || a->state_ss < 0) return KANTTS_E_UNSUPPORTED;
  const long long parts = (long long)a->S * a->Tc;
  if (parts > 0x7fffffffLL || parts * a->hop > 0x7fffffffLL) return KANTTS_E_UNSUPPORTED;
  if (a->ws_floats < parts * (a->H1 + 1)) return KANTTS_E_BADARG;
  kantts_nsf_source_args g = {};  // what nsf_frame_phases / nsf_harmonic read of the forward's argument
  g.f0 = a->f0, g.uv = a->uv, g.noise = a->noise, g.state_in = a->state_in, g.e = const_cast<float*>(a->e);
  g.state_ss = a->state_ss, g.S = a->S, g.Tc = a->Tc, g.hop = a->hop, g.H1 = a->H1;
  g.sr = a->sr, g.alpha = a->alpha, g.sigma = a->sigma;
  hipLaunchKernelGGL(nsf_wgrad_frame_kernel, dim3((unsigned)parts), dim3(NSF_THREADS), 0, (hipStream_t)stream, g, a->de, a->ws);
  hipLaunchKernelGGL(nsf_wgrad_sum_kernel, dim3((unsigned)(a->H1 + 1)), dim3(NSF_THREADS), 0, (hipStream_t)stream,
                     (const float*)a->ws, (int)parts, a->H1, a->dw, a->dbias);
  KANTTS_CHECK_LAUNCH();
}
