// The NSF excitation of chunked HiFi-GAN inference: a sine source that can be cut at any frame boundary, and the strided
// one-channel convolutions that bring it down to every upsampling stage's rate.  Two launches per step, both per slot and
// driven by the same device `rows` buffer as kantts_sconv_rows_launch (slot s has n_s = clamp(rows[s], 0, Tc) live frames;
// nothing at or after frame n_s of its inputs is read, nothing at or after it is written; n_s == 0 carries the state over
// bit for bit; rows == NULL: every slot advances by Tc).  Plain VALU / LDS kernels, fp32 in both precision modes.
//
// kantts_nsf_source_rows -- SourceModule.forward_cl (reference kantts/models/hifigan/layers.py:229-290) in one launch:
//   frame k of slot s has f0_k (Hz) and uv_k; sample j of that frame (absolute index n = cursor + k * hop + j) and
//   harmonic h (frequency (h + 1) * f0_k):
//     theta   = 2 pi * frac( sum over all samples up to and including this one of (h + 1) * f0 / sr )
//     x_h     = uv_k * (alpha * sin(theta + phase0[h]) + z) + (1 - uv_k) * (alpha / (3 sigma)) * z
//     e[s, n] = tanh(bias + sum_h w[h] * x_h)
//   z: noise[s, k * hop + j, h] as given, or sigma * N(0, 1) generated from (key, h, n).
//
// Running phase.  The reference sums f0 / sr in fp32 over the whole utterance and takes `% 1`.  Here the phase of every
// harmonic is a 32-bit FIXED-POINT accumulator in cycles (2^32 = one cycle): wrap-around is the `% 1`, and integer addition
// is exact and associative, so the result cannot depend on where the chunks are cut.  f0 is constant inside a frame, so
// with inc_k[h] = round(frac((h + 1) * f0_k / sr) * 2^32) (computed in fp64: H + 1 values per frame, where the rounding of an
// fp32 product would accumulate over the utterance) sample j of frame k has phase P_k + (j + 1) * inc_k, and
// P_{k+1} = P_k + hop * inc_k.  The only serial part is that sum over the frames of the chunk (tens of terms, walked by
// H + 1 threads of each workgroup); every sample is then independent.  The accumulator is read as a SIGNED fraction
// ([-1/2, 1/2) cycles) before it becomes a float, so the argument of the sine stays inside [-2 pi, 2 pi).
//
// Frame indexing is exact: sample n belongs to frame n / hop.  The reference upsamples with
// torch.nn.functional.interpolate(scale_factor=hop, mode="nearest"), whose float scale can pick the NEIGHBOURING frame at a
// frame boundary when hop is not a power of two; that rounding is not reproduced here.
//
// Generated noise.  One kantts_rng_mix hash serves the two harmonics 2i and 2i + 1 of a sample: Box-Muller on its two
// 32-bit halves (u1 in (0, 1] from the high half, u2 in [0, 1) from the low half) gives r cos(2 pi u2) and r sin(2 pi u2).
// The hash is keyed by the slot's 64-bit key and the block 8 * n + i, n the ABSOLUTE sample index of the utterance: the same
// utterance gets the same noise whatever the chunking, the slot or its batch-mates.
//
// State (KANTTS_NSF_STATE_WORDS 32-bit words per slot, ping-pong like the history of sconv.hip: state_in is read by every
// workgroup, state_out is written by S extra workgroups of the same launch): phase[16] (uint32), phase0[16] (float),
// the sample cursor (uint64), the noise key (uint64).
//
// kantts_nsf_downs_rows -- every source_downs convolution of the generator (reference hifigan.py:119-143) in one launch:
//   d_i[s, q, c] = bias_i[c] + sum_j w_i[j][c] * E[s, q * u_i - (K_i - 1) + j],   q < n_s * hop / u_i
//   E = [history ; e], the history being the last Hh = max_i (K_i - 1) excitation samples of the slot (2 * u_0 - 1 for the
//   generator's stages: kernel 2 u, stride u, left pad 2 u - 1; the last stage, u = 1, is the 1x1 convolution).  A zero history
//   is the reference's zero left pad.  It is updated like hist_out of the sconv rule and copied when n_s == 0.
// One workgroup owns a tile of output rows of one stage and one slot: its window of E goes to LDS once, a thread owns
// (row, channel) elements with the channel fastest, so weight loads (tap-major (K, C)) and output stores are coalesced and
// the LDS reads are broadcasts.
#include "common.h"

#define NSF_THREADS 256
#define NSF_MAXH1 16
#define NSF_MAXSTAGES 8
#define NSF_WINDOW 8192  // floats of LDS for a tile's window of E

struct nsf_state {
  uint32_t phase[NSF_MAXH1];
  float phase0[NSF_MAXH1];
  uint64_t cursor;
  uint64_t key;
};
static_assert(sizeof(nsf_state) == 4 * KANTTS_NSF_STATE_WORDS, "the state layout of include/kantts_hip.h");

__device__ __forceinline__ int nsf_live(const int32_t* rows, int s, int Tc) {
  return rows ? min(max(rows[s], 0), Tc) : Tc;
}

// round(frac((h + 1) * f0 / sr) * 2^32) as a wrapping 32-bit count of cycles
__device__ __forceinline__ uint32_t nsf_inc(float f0, int h, double inv_sr) {
  double c = (double)f0 * (double)(h + 1) * inv_sr;
  c -= floor(c);
  return (uint32_t)(unsigned long long)llrint(c * 4294967296.0);
}

__global__ __launch_bounds__(NSF_THREADS) void nsf_source_kernel(const kantts_nsf_source_args g) {
  __shared__ uint32_t s_phase[NSF_MAXH1], s_inc[NSF_MAXH1];
  __shared__ float s_phase0[NSF_MAXH1], s_w[NSF_MAXH1];
  const int H1 = g.H1, hop = g.hop;
  const double inv_sr = 1.0 / (double)g.sr;
  int bid = blockIdx.x;
  const int tid = threadIdx.x;
  if (bid < g.S) {
    // ---- state of slot bid: the phase after its n live frames, the cursor behind them; phase0 and the key are carried
    const int s = bid;
    const int n = nsf_live(g.rows, s, g.Tc);
    const nsf_state* si = reinterpret_cast<const nsf_state*>(g.state_in + (long long)s * g.state_ss);
    nsf_state* so = reinterpret_cast<nsf_state*>(g.state_out + (long long)s * g.state_ss);
    if (tid < NSF_MAXH1) {
      uint32_t p = si->phase[tid];
      if (tid < H1)
        for (int k = 0; k < n; ++k) p += (uint32_t)hop * nsf_inc(g.f0[(long long)s * g.Tc + k], tid, inv_sr);
      so->phase[tid] = p;
      so->phase0[tid] = si->phase0[tid];
    } else if (tid == NSF_MAXH1) {
      so->cursor = si->cursor + (uint64_t)n * (uint64_t)hop;
      so->key = si->key;
    }
    return;
  }
  bid -= g.S;
  const int s = bid / g.Tc, k = bid - s * g.Tc;
  if (k >= nsf_live(g.rows, s, g.Tc)) return;  // a dead frame: workgroup-uniform, before any load of f0 / uv / noise
  const nsf_state* si = reinterpret_cast<const nsf_state*>(g.state_in + (long long)s * g.state_ss);
  const float* f0p = g.f0 + (long long)s * g.Tc;
  if (tid < H1) {
    uint32_t p = si->phase[tid];
    for (int kk = 0; kk < k; ++kk) p += (uint32_t)hop * nsf_inc(f0p[kk], tid, inv_sr);
    s_phase[tid] = p;
    s_inc[tid] = nsf_inc(f0p[k], tid, inv_sr);
    s_phase0[tid] = si->phase0[tid];
    s_w[tid] = g.w[tid];
  }
  __syncthreads();
  const float uv = g.uv[(long long)s * g.Tc + k];
  const float b = g.bias ? g.bias[0] : 0.f;
  const float unv = g.alpha / 3.f / g.sigma;
  const uint64_t key = si->key;
  const uint64_t n0 = si->cursor + (uint64_t)k * (uint64_t)hop;  // absolute index of the frame's first sample
  const float cyc = 6.283185307179586f / 4294967296.f;
  for (int j = tid; j < hop; j += NSF_THREADS) {
    const long long o = ((long long)s * g.Tc + k) * hop + j;  // sample of this call
    float acc = b;
    float z1 = 0.f;  // the second Gaussian of a Box-Muller pair, for the odd harmonic
    for (int h = 0; h < H1; ++h) {
      float z;
      if (g.noise) {
        z = g.noise[o * H1 + h];
      } else if ((h & 1) == 0) {
        const uint64_t r = kantts_rng_mix(key, (n0 + (uint64_t)j) * 8ull + (uint64_t)(h >> 1));
        const float u1 = (float)((uint32_t)(r >> 40) + 1u) * (1.f / 16777216.f);  // (0, 1]
        const float u2 = (float)((uint32_t)r >> 8) * (1.f / 16777216.f);          // [0, 1)
        const float rad = g.sigma * sqrtf(-2.f * logf(u1));
        z = rad * cosf(6.283185307179586f * u2);
        z1 = rad * sinf(6.283185307179586f * u2);
      } else {
        z = z1;
      }
      const uint32_t ph = s_phase[h] + (uint32_t)(j + 1) * s_inc[h];
      const float theta = (float)(int32_t)ph * cyc;  // [-pi, pi)
      const float voiced = g.alpha * sinf(theta + s_phase0[h]) + z;
      const float x = voiced * uv + (unv * z) * (1.f - uv);
      if (g.harm) g.harm[o * H1 + h] = x;
      acc += s_w[h] * x;
    }
    g.e[o] = tanhf(acc);
  }
}

extern "C" int kantts_nsf_source_rows(const kantts_nsf_source_args* a, void* stream) {
  if (!a || !a->f0 || !a->uv || !a->w || !a->state_in || !a->state_out || !a->e || a->state_in == a->state_out)
    return KANTTS_E_BADARG;
  if (a->Tc < 1 || a->hop < 1 || a->H1 < 1 || !(a->sr > 0.f) || !(a->sigma > 0.f)) return KANTTS_E_BADARG;
  if (a->S > 1 && a->state_ss < KANTTS_NSF_STATE_WORDS) return KANTTS_E_BADARG;
  if (a->H1 > NSF_MAXH1) return KANTTS_E_UNSUPPORTED;
  if (((uintptr_t)a->state_in & 7) || ((uintptr_t)a->state_out & 7) || (a->state_ss & 1) || a->state_ss < 0)
    return KANTTS_E_UNSUPPORTED;
  if (a->S <= 0) return KANTTS_OK;
  const long long blocks = (long long)a->S * a->Tc + a->S;
  if (blocks > 0x7fffffffLL || (long long)a->S * a->Tc * a->hop > 0x7fffffffLL) return KANTTS_E_UNSUPPORTED;
  hipLaunchKernelGGL(nsf_source_kernel, dim3((unsigned)blocks), dim3(NSF_THREADS), 0, (hipStream_t)stream, *a);
  KANTTS_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------
// what the launcher derives from kantts_nsf_downs_args: tile rows and the first block of every stage
struct nsf_downs_plan {
  int rq[NSF_MAXSTAGES];     // output rows per tile
  int nt[NSF_MAXSTAGES];     // tiles per slot
  int first[NSF_MAXSTAGES];  // first block of the stage (behind the S state workgroups)
  int Hh;                    // history samples
};

// sample t (>= -Hh) of slot s of E = [hist_in ; e]
__device__ __forceinline__ float nsf_E(const kantts_nsf_downs_args& g, int s, int t, int Hh) {
  return t < 0 ? g.hist_in[(long long)s * g.hist_ss + Hh + t] : g.e[(long long)s * g.Tc * g.hop + t];
}

__global__ __launch_bounds__(NSF_THREADS) void nsf_downs_kernel(const kantts_nsf_downs_args g, const nsf_downs_plan p) {
  __shared__ float s_E[NSF_WINDOW];
  int bid = blockIdx.x;
  const int tid = threadIdx.x;
  const int Hh = p.Hh;
  if (bid < g.S) {
    // ---- hist_out[s] = the last Hh samples of [hist_in[s] ; e[s, 0 : n_s * hop]]
    const int n = nsf_live(g.rows, bid, g.Tc) * g.hop;
    for (int i = tid; i < Hh; i += NSF_THREADS) g.hist_out[(long long)bid * g.hist_ss + i] = nsf_E(g, bid, n - Hh + i, Hh);
    return;
  }
  bid -= g.S;
  int i = 0;
  while (i + 1 < g.nstages && bid >= p.first[i + 1]) ++i;
  bid -= p.first[i];
  const int s = bid / p.nt[i], tile = bid - s * p.nt[i];
  const int u = g.u[i], K = g.k[i], C = g.C[i];
  const int per = g.hop / u;                                 // rows of this stage per frame
  const int live = nsf_live(g.rows, s, g.Tc) * per;          // live rows of the slot at this stage
  const int q0 = tile * p.rq[i];
  if (q0 >= live) return;                                    // a dead tile: before any load and any barrier
  const int nq = min(p.rq[i], live - q0);
  const int W = (nq - 1) * u + K;                            // window: E[q0 * u - (K - 1) .. (q0 + nq - 1) * u]
  const int t0 = q0 * u - (K - 1);
  for (int x = tid; x < W; x += NSF_THREADS) s_E[x] = nsf_E(g, s, t0 + x, Hh);
  __syncthreads();
  const float* w = g.w[i];
  const float* bias = g.bias[i];
  float* out = g.out[i] + ((long long)s * g.Tc * per + q0) * C;
  for (int x = tid; x < nq * C; x += NSF_THREADS) {
    const int q = x / C, c = x - q * C;
    float acc = bias ? bias[c] : 0.f;
    const float* ep = s_E + q * u;
    for (int j = 0; j < K; ++j) acc += w[(long long)j * C + c] * ep[j];
    out[x] = acc;
  }
}

extern "C" int kantts_nsf_downs_rows(const kantts_nsf_downs_args* a, void* stream) {
  if (!a || !a->e || a->Tc < 1 || a->hop < 1 || a->nstages < 1) return KANTTS_E_BADARG;
  if (a->nstages > NSF_MAXSTAGES) return KANTTS_E_UNSUPPORTED;
  nsf_downs_plan p;
  p.Hh = 0;
  long long blocks = 0;
  for (int i = 0; i < a->nstages; ++i) {
    if (!a->w[i] || !a->out[i] || a->u[i] < 1 || a->k[i] < 1 || a->C[i] < 1) return KANTTS_E_BADARG;
    if (a->hop % a->u[i] != 0) return KANTTS_E_UNSUPPORTED;
    p.Hh = max(p.Hh, a->k[i] - 1);
    int rq = min(max(2048 / a->C[i], 1), 64);
    rq = min(rq, max(4096 / a->u[i], 1));
    while (rq > 1 && (long long)(rq - 1) * a->u[i] + a->k[i] > NSF_WINDOW) rq >>= 1;
    if (a->k[i] > NSF_WINDOW) return KANTTS_E_UNSUPPORTED;  // the window of a one-row tile
    p.rq[i] = rq;
    p.nt[i] = kantts_cdiv((long long)a->Tc * (a->hop / a->u[i]), rq);
    p.first[i] = (int)blocks;
    blocks += (long long)(a->S > 0 ? a->S : 0) * p.nt[i];
    if (blocks > 0x7fffff00LL || (long long)a->S * a->Tc * (a->hop / a->u[i]) * a->C[i] > 0x7fffffffLL)
      return KANTTS_E_UNSUPPORTED;
  }
  for (int i = a->nstages; i < NSF_MAXSTAGES; ++i) p.rq[i] = p.nt[i] = 1, p.first[i] = 0x7fffffff;
  if (p.Hh > 0 && (!a->hist_in || !a->hist_out || a->hist_in == a->hist_out)) return KANTTS_E_BADARG;
  if (a->S > 1 && a->hist_ss < p.Hh) return KANTTS_E_BADARG;
  if (a->S <= 0) return KANTTS_OK;
  blocks += a->S;
  hipLaunchKernelGGL(nsf_downs_kernel, dim3((unsigned)blocks), dim3(NSF_THREADS), 0, (hipStream_t)stream, *a, p);
  KANTTS_CHECK_LAUNCH();
}
