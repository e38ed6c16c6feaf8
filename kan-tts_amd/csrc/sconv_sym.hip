// The layer of chunked inference for SYMMETRIC (non-causal) networks: kantts_sconv_sym_rows_launch.
//
// A symmetric convolution of padding p is the causal convolution with the same taps whose output stream is p rows late,
// so a non-causal network is a causal one whose tensors carry integer delays -- provided every layer's output is zero
// outside the utterance (the reference pads every layer at the utterance's edges) and the end is flushed.  This file is
// the rule of csrc/sconv.hip's per-slot kernel (same tiles, same MFMA path in both precisions, same chunk-major,
// tap-inner summation order) with what that needs:
//   lag        tap j of output row q reads X[q - lag - j*step]; the state is the last Hs = H + lag rows.  The lag moves
//              the base of the LDS window, it does not widen it (the window is still rows + H rows).
//   residual   row q - res_lag of [res_hist ; res]: res_hist is the state another layer keeps anyway (read only).
//   window     an output sample whose true index (64-bit) lies outside [0, end * row_mul * sub) is stored as 0.0f; a tile
//              wholly outside stores zeros before its first load.
//   input end  rows of `in` at or beyond end * row_mul (flush rows) are not loaded and count as zero, in the LDS window
//              and in the state copy.
//   pos        frames consumed so far, per slot, read from pos_in by every launch; the state workgroup of the launch
//              that passes pos_out writes pos_in + n_s / row_mul there.
// include/kantts_hip.h has the token rule.  Reference: Conv1d / ConvTranspose1d, kantts/models/hifigan/layers.py:15-121.
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

#define SS_THREADS 256
#define SS_MAXK 11
#define SS_MAXSTEP 7
#define SS_OPEN 0x7fffffffffffffffLL

__device__ __forceinline__ float ss_leaky(float v, int act, float slope) { return (act && !(v > 0.f)) ? v * slope : v; }

// row t (>= -Hs) of slot s of X = [hist_in ; in]
__device__ __forceinline__ const float* ss_row(const kantts_sconv_sym_args& g, int s, int t, int Hs) {
  return t < 0 ? g.hist_in + (long long)s * g.hist_ss + (long long)(Hs + t) * g.Cin
               : g.in + ((long long)s * g.Tc + t) * g.Cin;
}

// what a workgroup knows about its slot: one uniform load each of rows, pos and end
struct ss_slot {
  int nlive;        // live rows of this call
  int in_lim;       // rows t >= in_lim of `in` are flush rows (== nlive without an input end)
  long long obase;  // true index of sample 0 of output row 0
  long long oend;   // first true index behind the utterance (SS_OPEN: open)
  int pos;
};

__device__ __forceinline__ ss_slot ss_slot_of(const kantts_sconv_sym_args& g, int s, int cap) {
  ss_slot k;
  k.nlive = min(max(g.rows[s], 0), cap) * g.row_mul;
  k.pos = g.pos_in[(long long)s * g.pos_ss];
  const int e = g.end[s];
  const long long p0 = (long long)k.pos * g.row_mul;  // stream position of row 0
  k.in_lim = k.nlive;
  if (g.in_end && e >= 0) k.in_lim = (int)min(max((long long)e * g.row_mul - p0, 0LL), (long long)k.nlive);
  k.obase = p0 * g.sub - g.delay;
  k.oend = e < 0 ? SS_OPEN : (long long)e * g.row_mul * g.sub;
  return k;
}

// hist_out[s] = the last Hs rows of [hist_in[s] ; in[s, 0:n]] with flush rows as zeros; pos_out -- one workgroup per slot
__device__ __forceinline__ void ss_copy_state(const kantts_sconv_sym_args& g, int s, int cap) {
  const ss_slot k = ss_slot_of(g, s, cap);
  const int Hs = (g.K - 1) * g.step + g.lag;
  const int c4n = g.Cin >> 2;
  float* dst = g.hist_out + (long long)s * g.hist_ss;
  for (int i = threadIdx.x; i < Hs * c4n; i += SS_THREADS) {
    const int h = i / c4n, c = (i - h * c4n) * 4;
    const int t = k.nlive - Hs + h;
    *reinterpret_cast<float4*>(dst + (long long)h * g.Cin + c) =
        t >= k.in_lim ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(ss_row(g, s, t, Hs) + c);
  }
  if (g.pos_out && threadIdx.x == 0) g.pos_out[(long long)s * g.pos_ss] = k.pos + k.nlive / g.row_mul;
}

template <bool BF16>
struct ss_bfrag;
template <>
struct ss_bfrag<true> {
  bf16x8 v;
};
template <>
struct ss_bfrag<false> {
  float4 lo, hi;
};

template <bool BF16, int WM, int MREP, int NFR>
__global__ __launch_bounds__(SS_THREADS) void sconv_sym_kernel(const kantts_sconv_sym_args g, const int ntm, const int ntn,
                                                               const int row_cap, const int cps) {
  constexpr int WN = 4 / WM;
  constexpr int BQ = WM * MREP * 16;
  constexpr int BN = WN * NFR * 16;
  constexpr int CKS = BF16 ? 128 : 64;           // channels per window slab
  constexpr int LDW = BF16 ? CKS + 8 : CKS + 4;  // row pitch in elements: 16 consecutive rows hit distinct bank groups
  constexpr int PF = (BF16 ? 16 : 4) / NFR;      // (chunk, tap) iterations of weight fragments in flight ahead of the MFMAs
  extern __shared__ __attribute__((aligned(16))) unsigned char ss_lds_raw[];

  int bid = blockIdx.x;
  if (bid < g.S) {
    ss_copy_state(g, bid, row_cap);
    return;
  }
  bid -= g.S;
  const int tn = bid % ntn;
  const int tm = (bid / ntn) % ntm;
  const int s = bid / (ntn * ntm);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM;
  const int H = (g.K - 1) * g.step;
  const int Hs = H + g.lag;
  const int q0 = tm * BQ;
  const ss_slot sl = ss_slot_of(g, s, row_cap);
  if (q0 >= sl.nlive) return;              // a dead tile: workgroup-uniform, before any load and any barrier
  const int rows = min(BQ, sl.nlive - q0);  // live output rows of this tile (>= 1)
  const int W = rows + H;                  // window rows
  const int t0 = q0 - g.lag - H;           // row of X in window row 0 (>= -Hs)
  const int ncol0 = tn * BN + wn * (NFR * 16);
  const bool wave_live = ncol0 < g.N && wm * (MREP * 16) < rows;  // wave-uniform

  // a tile wholly outside the utterance (before the delay has passed, or flushed out): zeros, nothing is loaded
  const long long glo = sl.obase + (long long)q0 * g.sub, ghi = sl.obase + (long long)(q0 + rows) * g.sub;
  if (ghi <= 0 || glo >= sl.oend) {
    const int ncols = min(BN, g.N - tn * BN);
    for (int i = tid; i < rows * ncols; i += SS_THREADS) {
      const int m = i / ncols, n = tn * BN + (i - m * ncols);
      g.out[((long long)s * g.Tc + q0 + m) * g.N + n] = 0.f;
    }
    return;
  }

  // window row of fragment f's MFMA row for tap 0 (rows past the tile's end are clamped: computed, never stored)
  int arow0[MREP];
#pragma unroll
  for (int f = 0; f < MREP; ++f) arow0[f] = min(wm * (MREP * 16) + f * 16 + (lane & 15), rows - 1) + H;

  f32x4 acc[MREP][NFR];
#pragma unroll
  for (int f = 0; f < MREP; ++f)
#pragma unroll
    for (int j = 0; j < NFR; ++j) acc[f][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nch = (g.Cin + 31) >> 5;  // 32-channel MFMA chunks
  const int total = nch * g.K;        // (chunk, tap) iterations, chunk-major
  const int kg8 = (lane >> 4) * 8;    // this lane's 8 channels inside a chunk

  // Weight fragments, PF (chunk, tap) iterations ahead; out-of-range lanes read a CLAMPED, valid address (csrc/sconv.hip)
  ss_bfrag<BF16> bcur[PF][NFR], bnext[PF][NFR];
  int fch = 0, fj = 0;  // fetch cursor (chunk, tap); runs up to PF iterations past the end, clamped
  long long ncl[NFR];
#pragma unroll
  for (int nf = 0; nf < NFR; ++nf) ncl[nf] = (long long)min(ncol0 + nf * 16 + (lane & 15), g.N - 1) * g.Cin;
  auto fetch_b = [&](ss_bfrag<BF16> (&dst)[PF][NFR]) {
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      if (wave_live) {
        const long long o0 = (long long)fj * g.N * g.Cin + min(fch * 32 + kg8, g.Cin - 8);
#pragma unroll
        for (int nf = 0; nf < NFR; ++nf) {
          if constexpr (BF16) {
            dst[u][nf].v = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const __bf16*>(g.w) + o0 + ncl[nf]);
          } else {
            const float* wp = reinterpret_cast<const float*>(g.w) + o0 + ncl[nf];
            dst[u][nf].lo = *reinterpret_cast<const float4*>(wp);
            dst[u][nf].hi = *reinterpret_cast<const float4*>(wp + 4);
          }
        }
      }
      if (++fj == g.K) fj = 0, ++fch;
    }
  };

  int ch = 0, j = -1;  // compute cursor
  fetch_b(bnext);
  for (int it0 = 0; it0 < total; it0 += PF) {
#pragma unroll
    for (int u = 0; u < PF; ++u)
#pragma unroll
      for (int nf = 0; nf < NFR; ++nf) bcur[u][nf] = bnext[u][nf];
    fetch_b(bnext);
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      if (it0 + u >= total) continue;  // workgroup-uniform
      if (++j == g.K) j = 0, ++ch;
      const int cl = (ch * 32) % CKS;  // chunk's first column inside the slab
      if (j == 0 && cl == 0) {
        // ---- stage the slab: W rows x ncols channels of X, activated and rounded, 4 float4 in flight per thread
        const int cbase = ch * 32;
        const int ncols = min(CKS, ((g.Cin - cbase + 31) >> 5) << 5);  // multiple of 32; columns >= Cin are zeros
        const int c4n = ncols >> 2;
        const int nvec = W * c4n;
        __syncthreads();  // every wave is done with the previous slab
        for (int i0 = tid; i0 < nvec; i0 += SS_THREADS * 4) {
          float4 xv[4];
          int row[4], col[4];
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int i = i0 + v * SS_THREADS;
            row[v] = i / c4n;
            col[v] = (i - row[v] * c4n) * 4;
            const bool ok = i < nvec && cbase + col[v] < g.Cin && t0 + row[v] < sl.in_lim;  // flush rows: zeros
            xv[v] = ok ? *reinterpret_cast<const float4*>(ss_row(g, s, t0 + row[v], Hs) + cbase + col[v])
                       : make_float4(0.f, 0.f, 0.f, 0.f);
          }
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            if (i0 + v * SS_THREADS >= nvec) continue;
            const float v0 = ss_leaky(xv[v].x, g.in_act, g.in_slope), v1 = ss_leaky(xv[v].y, g.in_act, g.in_slope);
            const float v2 = ss_leaky(xv[v].z, g.in_act, g.in_slope), v3 = ss_leaky(xv[v].w, g.in_act, g.in_slope);
            const int o = row[v] * LDW + col[v];
            if constexpr (BF16) {
              bf16x4 p = {(__bf16)v0, (__bf16)v1, (__bf16)v2, (__bf16)v3};
              *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(ss_lds_raw) + o) = p;
            } else {
              *reinterpret_cast<float4*>(reinterpret_cast<float*>(ss_lds_raw) + o) = make_float4(v0, v1, v2, v3);
            }
          }
        }
        __syncthreads();
      }
      if (!wave_live) continue;
      const int back = j * g.step;
      if constexpr (BF16) {
        const __bf16* Wh = reinterpret_cast<const __bf16*>(ss_lds_raw);
        bf16x8 af[MREP];
#pragma unroll
        for (int f = 0; f < MREP; ++f)
          af[f] = *reinterpret_cast<const bf16x8*>(&Wh[(arow0[f] - back) * LDW + cl + kg8]);
#pragma unroll
        for (int f = 0; f < MREP; ++f)
#pragma unroll
          for (int nf = 0; nf < NFR; ++nf)
            acc[f][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[f], bcur[u][nf].v,
                                                                 acc[f][nf], 0, 0, 0);
      } else {
        const float* Wf = reinterpret_cast<const float*>(ss_lds_raw);
        float a8[MREP][8];
#pragma unroll
        for (int f = 0; f < MREP; ++f) {
          const float* ap = &Wf[(arow0[f] - back) * LDW + cl + kg8];
          const float4 lo = *reinterpret_cast<const float4*>(ap), hi = *reinterpret_cast<const float4*>(ap + 4);
          a8[f][0] = lo.x, a8[f][1] = lo.y, a8[f][2] = lo.z, a8[f][3] = lo.w;
          a8[f][4] = hi.x, a8[f][5] = hi.y, a8[f][6] = hi.z, a8[f][7] = hi.w;
        }
        // k-step e contracts channel kg8 + e of every lane group: A and B agree, so the order inside a chunk is free
#pragma unroll
        for (int e = 0; e < 8; ++e)
#pragma unroll
          for (int nf = 0; nf < NFR; ++nf) {
            const ss_bfrag<false>& b = bcur[u][nf];
            const float bv = e == 0 ? b.lo.x : e == 1 ? b.lo.y : e == 2 ? b.lo.z : e == 3 ? b.lo.w
                           : e == 4 ? b.hi.x : e == 5 ? b.hi.y : e == 6 ? b.hi.z : b.hi.w;
#pragma unroll
            for (int f = 0; f < MREP; ++f)
              acc[f][nf] = __builtin_amdgcn_mfma_f32_16x16x4f32(a8[f][e], bv, acc[f][nf], 0, 0, 0);
          }
      }
    }
  }
  if (!wave_live) return;

  // ---- epilogue from the accumulator layout: lane holds rows 4 * (lane / 16) .. + 3 of column lane % 16
  const float* rh = g.res_hist ? g.res_hist + (long long)s * g.res_hist_ss : nullptr;
#pragma unroll
  for (int nf = 0; nf < NFR; ++nf) {
    const int n = ncol0 + nf * 16 + (lane & 15);
    if (n >= g.N) continue;
    const float bv = g.bias ? g.bias[n] : 0.f;
    const int ph = g.sub > 1 ? n / cps : 0;  // sample of the row this column belongs to
#pragma unroll
    for (int f = 0; f < MREP; ++f)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = wm * (MREP * 16) + f * 16 + (lane >> 4) * 4 + r;
        if (m >= rows) continue;
        const long long o = ((long long)s * g.Tc + q0 + m) * g.N + n;
        const long long gi = sl.obase + (long long)(q0 + m) * g.sub + ph;
        float v = 0.f;
        if (gi >= 0 && gi < sl.oend) {
          v = ss_leaky(acc[f][nf][r] + bv, g.out_act, g.out_slope);
          if (g.res) {
            const int rq = q0 + m - g.res_lag;
            v += rq >= 0 ? g.res[((long long)s * g.Tc + rq) * g.N + n] : rh[(long long)(g.res_hist_rows + rq) * g.N + n];
          }
        }
        g.out[o] = v;
      }
  }
}

// N == 1 (conv_post): one thread per output row, a K x Cin fp32 dot product, the same rule
__global__ __launch_bounds__(SS_THREADS) void sconv_sym_n1_kernel(const kantts_sconv_sym_args g, const int row_cap) {
  int bid = blockIdx.x;
  if (bid < g.S) {
    ss_copy_state(g, bid, row_cap);
    return;
  }
  bid -= g.S;
  const long long e = (long long)bid * SS_THREADS + threadIdx.x;
  if (e >= (long long)g.S * g.Tc) return;
  const int s = (int)(e / g.Tc), q = (int)(e - (long long)s * g.Tc);
  const ss_slot sl = ss_slot_of(g, s, row_cap);
  if (q >= sl.nlive) {
    if (g.zero_tail) g.out[e] = 0.f;
    return;
  }
  const long long gi = sl.obase + q;  // N == 1: sub == 1
  if (gi < 0 || gi >= sl.oend) {
    g.out[e] = 0.f;
    return;
  }
  const int Hs = (g.K - 1) * g.step + g.lag;
  const float* w = reinterpret_cast<const float*>(g.w);
  float acc = 0.f;
  for (int j = 0; j < g.K; ++j) {
    const int t = q - g.lag - j * g.step;
    if (t >= sl.in_lim) continue;  // a flush row: zero
    const float* x = ss_row(g, s, t, Hs);
    const float* wr = w + (long long)j * g.Cin;
    for (int c = 0; c < g.Cin; c += 4) {
      const float4 xv = *reinterpret_cast<const float4*>(x + c), wv = *reinterpret_cast<const float4*>(wr + c);
      acc += ss_leaky(xv.x, g.in_act, g.in_slope) * wv.x;
      acc += ss_leaky(xv.y, g.in_act, g.in_slope) * wv.y;
      acc += ss_leaky(xv.z, g.in_act, g.in_slope) * wv.z;
      acc += ss_leaky(xv.w, g.in_act, g.in_slope) * wv.w;
    }
  }
  if (g.bias) acc += g.bias[0];
  acc = ss_leaky(acc, g.out_act, g.out_slope);
  if (g.res) {
    const int rq = q - g.res_lag;
    acc += rq >= 0 ? g.res[(long long)s * g.Tc + rq] : g.res_hist[(long long)s * g.res_hist_ss + g.res_hist_rows + rq];
  }
  g.out[e] = acc;
}

template <bool BF16, int WM, int MREP, int NFR>
static int ss_launch(const kantts_sconv_sym_args& g, int cap, hipStream_t st) {
  constexpr int BQ = WM * MREP * 16;
  constexpr int BN = (4 / WM) * NFR * 16;
  constexpr int LDW = BF16 ? 128 + 8 : 64 + 4;
  const int H = (g.K - 1) * g.step;
  const int ntm = kantts_cdiv(g.Tc, BQ), ntn = kantts_cdiv(g.N, BN);
  const long long blocks = (long long)g.S * ntm * ntn + g.S;
  if (blocks > 0x7fffffffLL) return KANTTS_E_UNSUPPORTED;
  const size_t lds = (size_t)(BQ + H) * LDW * (BF16 ? 2 : 4);  // <= (128 + 70) * 272 B = 52.6 KB, whatever the lag
  hipLaunchKernelGGL((sconv_sym_kernel<BF16, WM, MREP, NFR>), dim3((unsigned)blocks), dim3(SS_THREADS), lds, st, g, ntm, ntn,
                     cap, g.N / g.sub);
  KANTTS_CHECK_LAUNCH();
}

// the tile choice of csrc/sconv.hip (from Tc, S and N alone): the same tiles as the causal layer of the same shape
template <bool BF16, int WM, int MREP>
static int ss_pick_n(const kantts_sconv_sym_args& g, int cap, hipStream_t st) {
  constexpr int BQ = WM * MREP * 16, WN = 4 / WM;
  const long long mt = (long long)g.S * kantts_cdiv(g.Tc, BQ);
  auto blocks = [&](int nfr) { return mt * kantts_cdiv(g.N, WN * nfr * 16); };
  if (g.N > WN * 32 && blocks(4) >= 384) return ss_launch<BF16, WM, MREP, 4>(g, cap, st);
  if (g.N > WN * 16 && blocks(2) >= 384) return ss_launch<BF16, WM, MREP, 2>(g, cap, st);
  return ss_launch<BF16, WM, MREP, 1>(g, cap, st);
}

template <bool BF16>
static int ss_dispatch(const kantts_sconv_sym_args& g, int cap, hipStream_t st) {
  if (g.Tc <= 16) return ss_pick_n<BF16, 1, 1>(g, cap, st);
  if (g.Tc <= 64) return ss_pick_n<BF16, 4, 1>(g, cap, st);
  return ss_pick_n<BF16, 4, 2>(g, cap, st);
}

extern "C" int kantts_sconv_sym_rows_launch(const kantts_sconv_sym_args* a, void* stream) {
  if (!a) return KANTTS_E_BADARG;
  kantts_sconv_sym_args g = *a;
  if (!g.in || !g.w || !g.out || !g.rows || !g.end || !g.pos_in) return KANTTS_E_BADARG;
  if (g.K < 1 || g.step < 1 || g.Cin < 1 || g.N < 1 || (g.precision != 0 && g.precision != 1)) return KANTTS_E_BADARG;
  if (g.row_mul < 1 || g.lag < 0 || g.res_lag < 0 || g.delay < 0 || g.sub < 1 || g.N % g.sub != 0 || g.pos_ss < 0)
    return KANTTS_E_BADARG;
  if (g.res_hist && !g.res) return KANTTS_E_BADARG;
  if (g.res_lag > 0 && (!g.res || !g.res_hist || g.res_lag > g.res_hist_rows || g.res_hist_ss < 0)) return KANTTS_E_BADARG;
  const long long Hs = (long long)(g.K - 1) * g.step + g.lag;
  if (Hs > 0 && (!g.hist_in || !g.hist_out || g.hist_in == g.hist_out)) return KANTTS_E_BADARG;
  if (g.pos_out == g.pos_in) return KANTTS_E_BADARG;
  if (g.K > SS_MAXK || g.step > SS_MAXSTEP || (g.Cin & 7) || g.Cin < 16 || g.Cin > 512 ||
      !(g.N == 1 || (g.N >= 16 && g.N <= 4096)) || Hs > 0x3fffffff)
    return KANTTS_E_UNSUPPORTED;
  if (((uintptr_t)g.in & 15) || ((uintptr_t)g.w & 15) || ((uintptr_t)g.hist_in & 15) || ((uintptr_t)g.hist_out & 15) ||
      (g.hist_ss & 3) || g.hist_ss < 0)
    return KANTTS_E_UNSUPPORTED;
  if (g.zero_tail && g.N != 1) return KANTTS_E_UNSUPPORTED;  // the zero tail exists in the N == 1 kernel only
  g.S = g.S > 0 ? g.S : 0;
  g.Tc = g.Tc > 0 ? g.Tc : 0;
  if (g.Tc % g.row_mul != 0) return KANTTS_E_BADARG;
  if (g.S == 0 || g.Tc == 0) return KANTTS_OK;
  if (Hs > 0 && g.hist_ss < Hs * g.Cin && g.S > 1) return KANTTS_E_BADARG;
  const int cap = g.Tc / g.row_mul;
  hipStream_t st = (hipStream_t)stream;
  if (g.N == 1) {
    const long long blocks = ((long long)g.S * g.Tc + SS_THREADS - 1) / SS_THREADS + g.S;
    if (blocks > 0x7fffffffLL) return KANTTS_E_UNSUPPORTED;
    hipLaunchKernelGGL(sconv_sym_n1_kernel, dim3((unsigned)blocks), dim3(SS_THREADS), 0, st, g, cap);
    KANTTS_CHECK_LAUNCH();
  }
  return g.precision == 1 ? ss_dispatch<true>(g, cap, st) : ss_dispatch<false>(g, cap, st);
}
