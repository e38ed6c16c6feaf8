// The device code that csrc/nsf_source.hip (causal generators) and csrc/nsf_source_sym.hip (non-causal generators) share:
// one body each for the sine source and for the excitation down-convolutions, so that the two files' entry points run the
// SAME arithmetic in the same order -- kantts_nsf_source_end_rows gives the bits of kantts_nsf_source_rows on its live
// frames, kantts_nsf_downs_sym_rows with lag = k - 1 the bits of kantts_nsf_downs_rows.  The kernels own the LDS buffers
// and say how many frames of a slot are live; the rules are written out in the two files and in include/kantts_hip.h.
#pragma once
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

// what a frame's workgroup keeps in LDS
struct nsf_source_lds {
  uint32_t phase[NSF_MAXH1], inc[NSF_MAXH1];
  float phase0[NSF_MAXH1], w[NSF_MAXH1];
};

__device__ __forceinline__ int nsf_live(const int32_t* rows, int s, int Tc) {
  return rows ? min(max(rows[s], 0), Tc) : Tc;
}

// round(frac((h + 1) * f0 / sr) * 2^32) as a wrapping 32-bit count of cycles
__device__ __forceinline__ uint32_t nsf_inc(float f0, int h, double inv_sr) {
  double c = (double)f0 * (double)(h + 1) * inv_sr;
  c -= floor(c);
  return (uint32_t)(unsigned long long)llrint(c * 4294967296.0);
}

// ---- state of slot s behind its n live frames: the phase after them, the cursor behind them; phase0 and the key are carried
__device__ __forceinline__ void nsf_source_state(const kantts_nsf_source_args& g, int s, int n) {
  const int tid = threadIdx.x;
  const double inv_sr = 1.0 / (double)g.sr;
  const nsf_state* si = reinterpret_cast<const nsf_state*>(g.state_in + (long long)s * g.state_ss);
  nsf_state* so = reinterpret_cast<nsf_state*>(g.state_out + (long long)s * g.state_ss);
  if (tid < NSF_MAXH1) {
    uint32_t p = si->phase[tid];
    if (tid < g.H1)
      for (int k = 0; k < n; ++k) p += (uint32_t)g.hop * nsf_inc(g.f0[(long long)s * g.Tc + k], tid, inv_sr);
    so->phase[tid] = p;
    so->phase0[tid] = si->phase0[tid];
  } else if (tid == NSF_MAXH1) {
    so->cursor = si->cursor + (uint64_t)n * (uint64_t)g.hop;
    so->key = si->key;
  }
}

// ---- what LIVE frame k of slot s starts from: the phase in front of it, its increment and the initial phases, H1 cells each
// (threads below H1; the caller puts the barrier behind it)
__device__ __forceinline__ void nsf_frame_phases(const kantts_nsf_source_args& g, int s, int k, nsf_source_lds& lds) {
  const int tid = threadIdx.x;
  const double inv_sr = 1.0 / (double)g.sr;
  const nsf_state* si = reinterpret_cast<const nsf_state*>(g.state_in + (long long)s * g.state_ss);
  const float* f0p = g.f0 + (long long)s * g.Tc;
  if (tid < g.H1) {
    uint32_t p = si->phase[tid];
    for (int kk = 0; kk < k; ++kk) p += (uint32_t)g.hop * nsf_inc(f0p[kk], tid, inv_sr);
    lds.phase[tid] = p;
    lds.inc[tid] = nsf_inc(f0p[k], tid, inv_sr);
    lds.phase0[tid] = si->phase0[tid];
  }
}

// ---- x_h of ONE sample: sample j of its frame, element o of the call, absolute sample n of the utterance.  THE definition
// of the excitation before its projection: the forward (nsf_source_frame) and the weight gradient of csrc/nsf_train.hip both
// call it, for h = 0, 1, ... H1 - 1 in this order, so both see the same bits.  An even h forms the Box-Muller pair of
// harmonics h and h + 1 from one hash and leaves the second Gaussian in z1, where h + 1 finds it (an odd H1: the last
// harmonic forms a pair and uses its first half).
__device__ __forceinline__ float nsf_harmonic(const kantts_nsf_source_args& g, const nsf_source_lds& lds, int h, int j,
                                              long long o, uint64_t key, uint64_t n, float uv, float unv, float& z1) {
  const float cyc = 6.283185307179586f / 4294967296.f;
  float z;
  if (g.noise) {
    z = g.noise[o * g.H1 + h];
  } else if ((h & 1) == 0) {
    const uint64_t r = kantts_rng_mix(key, n * 8ull + (uint64_t)(h >> 1));
    const float u1 = (float)((uint32_t)(r >> 40) + 1u) * (1.f / 16777216.f);  // (0, 1]
    const float u2 = (float)((uint32_t)r >> 8) * (1.f / 16777216.f);          // [0, 1)
    const float rad = g.sigma * sqrtf(-2.f * logf(u1));
    z = rad * cosf(6.283185307179586f * u2);
    z1 = rad * sinf(6.283185307179586f * u2);
  } else {
    z = z1;
  }
  const uint32_t ph = lds.phase[h] + (uint32_t)(j + 1) * lds.inc[h];
  const float theta = (float)(int32_t)ph * cyc;  // [-pi, pi)
  const float voiced = g.alpha * sinf(theta + lds.phase0[h]) + z;
  return voiced * uv + (unv * z) * (1.f - uv);
}

// ---- the hop samples of LIVE frame k of slot s (the caller has returned for a dead frame, before any load)
__device__ __forceinline__ void nsf_source_frame(const kantts_nsf_source_args& g, int s, int k, nsf_source_lds& lds) {
  const int H1 = g.H1, hop = g.hop;
  const int tid = threadIdx.x;
  const nsf_state* si = reinterpret_cast<const nsf_state*>(g.state_in + (long long)s * g.state_ss);
  nsf_frame_phases(g, s, k, lds);
  if (tid < H1) lds.w[tid] = g.w[tid];
  __syncthreads();
  const float uv = g.uv[(long long)s * g.Tc + k];
  const float b = g.bias ? g.bias[0] : 0.f;
  const float unv = g.alpha / 3.f / g.sigma;
  const uint64_t key = si->key;
  const uint64_t n0 = si->cursor + (uint64_t)k * (uint64_t)hop;  // absolute index of the frame's first sample
  for (int j = tid; j < hop; j += NSF_THREADS) {
    const long long o = ((long long)s * g.Tc + k) * hop + j;  // sample of this call
    float acc = b;
    float z1 = 0.f;  // the second Gaussian of a Box-Muller pair, for the odd harmonic
    for (int h = 0; h < H1; ++h) {
      const float x = nsf_harmonic(g, lds, h, j, o, key, n0 + (uint64_t)j, uv, unv, z1);
      if (g.harm) g.harm[o * H1 + h] = x;
      acc += lds.w[h] * x;
    }
    g.e[o] = tanhf(acc);
  }
}

// what both launchers check of kantts_nsf_source_args, and the grid: S state workgroups, then one per (slot, frame)
static inline int nsf_source_check(const kantts_nsf_source_args* a, long long* blocks) {
  if (!a->f0 || !a->uv || !a->w || !a->state_in || !a->state_out || !a->e || a->state_in == a->state_out)
    return KANTTS_E_BADARG;
  if (a->Tc < 1 || a->hop < 1 || a->H1 < 1 || !(a->sr > 0.f) || !(a->sigma > 0.f)) return KANTTS_E_BADARG;
  if (a->S > 1 && a->state_ss < KANTTS_NSF_STATE_WORDS) return KANTTS_E_BADARG;
  if (a->H1 > NSF_MAXH1) return KANTTS_E_UNSUPPORTED;
  if (((uintptr_t)a->state_in & 7) || ((uintptr_t)a->state_out & 7) || (a->state_ss & 1) || a->state_ss < 0)
    return KANTTS_E_UNSUPPORTED;
  *blocks = a->S <= 0 ? 0 : (long long)a->S * a->Tc + a->S;
  if (*blocks > 0x7fffffffLL || (long long)a->S * a->Tc * a->hop > 0x7fffffffLL) return KANTTS_E_UNSUPPORTED;
  return KANTTS_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// what the launchers derive from kantts_nsf_downs_args: tile rows and the first block of every stage
struct nsf_downs_plan {
  int rq[NSF_MAXSTAGES];     // output rows per tile
  int nt[NSF_MAXSTAGES];     // tiles per slot
  int first[NSF_MAXSTAGES];  // first block of the stage (behind the S state workgroups)
  int Hh;                    // history samples
};

// sample t (>= -Hh) of slot s of E = [hist_in ; e]; samples at or beyond lim (<= n_s * hop) are 0.0f and are not loaded
__device__ __forceinline__ float nsf_E(const kantts_nsf_downs_args& g, int s, int t, int Hh, int lim) {
  return t < 0 ? g.hist_in[(long long)s * g.hist_ss + Hh + t] : t < lim ? g.e[(long long)s * g.Tc * g.hop + t] : 0.f;
}

// ---- hist_out[s] = the last Hh samples of E[s, -Hh : n], n = n_s * hop
__device__ __forceinline__ void nsf_downs_hist(const kantts_nsf_downs_args& g, int s, int Hh, int n, int lim) {
  for (int i = threadIdx.x; i < Hh; i += NSF_THREADS) g.hist_out[(long long)s * g.hist_ss + i] = nsf_E(g, s, n - Hh + i, Hh, lim);
}

// ---- tile block `bid` (counted behind the state workgroups): rows of one stage and one slot whose tap j reads
// E[q * u - lag + j].  The window E[q0 * u - lag .. (q0 + nq - 1) * u - lag + K - 1] goes to LDS once (the lag moves its
// base, it does not widen it); a thread owns (row, channel) elements with the channel fastest.  lag[] and lim[] are the
// caller's: lag[i] of stage i, lim(s, live frames) the first sample of e that counts as zero.
template <class Lag, class Lim>
__device__ __forceinline__ void nsf_downs_tile(const kantts_nsf_downs_args& g, const nsf_downs_plan& p, float* s_E, int bid,
                                               Lag lag_of, Lim lim_of) {
  const int tid = threadIdx.x;
  int i = 0;
  while (i + 1 < g.nstages && bid >= p.first[i + 1]) ++i;
  bid -= p.first[i];
  const int s = bid / p.nt[i], tile = bid - s * p.nt[i];
  const int u = g.u[i], K = g.k[i], C = g.C[i];
  const int per = g.hop / u;                                 // rows of this stage per frame
  const int frames = nsf_live(g.rows, s, g.Tc);
  const int live = frames * per;                             // live rows of the slot at this stage
  const int q0 = tile * p.rq[i];
  if (q0 >= live) return;                                    // a dead tile: before any load and any barrier
  const int nq = min(p.rq[i], live - q0);
  const int W = (nq - 1) * u + K;
  const int t0 = q0 * u - lag_of(i);
  const int lim = lim_of(s, frames);
  for (int x = tid; x < W; x += NSF_THREADS) s_E[x] = nsf_E(g, s, t0 + x, p.Hh, lim);
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

// the tiling of both launchers (it depends on u, k and C alone, never on a lag): fills p.rq / nt / first and *blocks (the
// tile blocks; the caller adds the S state workgroups).  p.Hh is the caller's.
static inline int nsf_downs_make_plan(const kantts_nsf_downs_args* a, nsf_downs_plan* p, long long* nblocks) {
  if (!a->e || a->Tc < 1 || a->hop < 1 || a->nstages < 1) return KANTTS_E_BADARG;
  if (a->nstages > NSF_MAXSTAGES) return KANTTS_E_UNSUPPORTED;
  long long blocks = 0;
  for (int i = 0; i < a->nstages; ++i) {
    if (!a->w[i] || !a->out[i] || a->u[i] < 1 || a->k[i] < 1 || a->C[i] < 1) return KANTTS_E_BADARG;
    if (a->hop % a->u[i] != 0) return KANTTS_E_UNSUPPORTED;
    int rq = min(max(2048 / a->C[i], 1), 64);
    rq = min(rq, max(4096 / a->u[i], 1));
    while (rq > 1 && (long long)(rq - 1) * a->u[i] + a->k[i] > NSF_WINDOW) rq >>= 1;
    if (a->k[i] > NSF_WINDOW) return KANTTS_E_UNSUPPORTED;  // the window of a one-row tile
    p->rq[i] = rq;
    p->nt[i] = kantts_cdiv((long long)a->Tc * (a->hop / a->u[i]), rq);
    p->first[i] = (int)blocks;
    blocks += (long long)(a->S > 0 ? a->S : 0) * p->nt[i];
    if (blocks > 0x7fffff00LL || (long long)a->S * a->Tc * (a->hop / a->u[i]) * a->C[i] > 0x7fffffffLL)
      return KANTTS_E_UNSUPPORTED;
  }
  for (int i = a->nstages; i < NSF_MAXSTAGES; ++i) p->rq[i] = p->nt[i] = 1, p->first[i] = 0x7fffffff;
  *nblocks = blocks;
  return KANTTS_OK;
}
