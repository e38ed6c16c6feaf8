// Causal, stride-1, dilated, channels-last convolution WITH HISTORY: the layer of chunked HiFi-GAN inference.
//
// S independent slots advance together by Tc rows per call.  Every slot carries the last H = (K - 1) * step input rows
// of the previous call in a state buffer, so the concatenation of the chunk outputs equals the convolution of the whole
// left-zero-padded sequence (zero state == the zero pad):
//   out[s, q, n]      = post( bias[n] + sum_j sum_c pre( X[s, q - j*step, c] ) w[j][n][c] ),   q in [0, Tc)
//   X[s, t, c]        = in[s, t, c] (t >= 0),  hist_in[s, H + t, c] (-H <= t < 0)
//   hist_out[s, h, c] = X[s, Tc - H + h, c]
// The polyphase causal transposed convolution and the generator's fused dual-path stage are the same rule with step = 1,
// K = J taps and N = u * Cout (include/kantts_hip.h).
//
// Geometry.  One workgroup (4 waves) owns BQ = 16 * WM * MREP output rows of ONE slot and BN = 16 * (4 / WM) * NFR output
// channels.  Its window -- the rows q0 - H .. q0 + BQ - 1 of X, i.e. the tail of hist_in followed by rows of in -- is read
// from global memory once per CKS-channel slab (128 channels in bf16 mode, 64 in fp32 mode), activated, rounded to the
// operand type and stored in LDS; the K taps are row offsets into that window (tap j of output row m reads window row
// m + H - j*step), so no row is fetched once per tap.  Weights (K, N, Cin) are small and L2 resident: every lane loads
// its B fragment (8 consecutive channels of one output channel) straight from global memory, register-prefetched PF taps
// ahead of the MFMAs that consume it; the tap loop has no barrier.  The accumulators are written from their MFMA layout
// (16 lanes = 64 contiguous bytes of one output row) with bias, LeakyReLU and the residual fused.
//
// State.  The first S workgroups of the grid do no arithmetic: workgroup s copies the last H rows of [hist_in ; in] of
// slot s to hist_out (a different buffer: nobody reads what they write).  The state therefore travels in the SAME launch
// as the convolution: carrying it costs a chunk step no launch of its own.
//
// Per-slot row counts (kantts_sconv_rows_launch; the ROWS = true instantiations).  Slot s advances by
//   n_s = clamp(rows[s], 0, Tc / row_mul) * row_mul
// rows instead of Tc (rows: device memory, so that a captured launch stays valid while the counts change).  The grid is
// still sized by Tc.  A compute workgroup reads rows[s] once (a uniform load), returns before its first load and its
// first barrier when its tile starts at or after n_s, and bounds a partly live tile by n_s where the plain kernel bounds
// it by Tc: no row >= n_s of in / res is loaded, no row >= n_s of out is written.  The state workgroup copies the last
// H rows of [hist_in ; in[0:n_s]] -- for n_s == 0 that is hist_in itself.  The ROWS = false instantiations are the
// kernels of kantts_sconv_launch, instruction for instruction.
//
// Reference: CausalConv1d / CausalConvTranspose1d, kantts/models/hifigan/layers.py:52-165 (their left zero pad is the
// zero state of a fresh slot).
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

#define SC_THREADS 256
#define SC_MAXK 11
#define SC_MAXSTEP 7

__device__ __forceinline__ float sc_leaky(float v, int act, float slope) { return (act && !(v > 0.f)) ? v * slope : v; }

// row t (>= -H) of slot s of X = [hist_in ; in]
__device__ __forceinline__ const float* sc_row(const kantts_sconv_args& g, int s, int t, int H) {
  return t < 0 ? g.hist_in + (long long)s * g.hist_ss + (long long)(H + t) * g.Cin
               : g.in + ((long long)s * g.Tc + t) * g.Cin;
}

// live rows of slot s: the count is clamped from BOTH sides (cap = Tc / row_mul, computed by the host)
__device__ __forceinline__ int sc_live(const int32_t* rowsp, int s, int cap, int row_mul) {
  return min(max(rowsp[s], 0), cap) * row_mul;
}

// hist_out[s] = the last H rows of [hist_in[s] ; in[s, 0:n]], n = Tc or (ROWS) the slot's live rows -- one workgroup per
// slot, a plain float4 copy
template <bool ROWS>
__device__ __forceinline__ void sc_copy_state(const kantts_sconv_args& g, int s, const int32_t* rowsp, int cap, int row_mul) {
  int n = 0;
  if constexpr (ROWS) n = sc_live(rowsp, s, cap, row_mul);
  const int H = (g.K - 1) * g.step;
  const int c4n = g.Cin >> 2;
  float* dst = g.hist_out + (long long)s * g.hist_ss;
  for (int i = threadIdx.x; i < H * c4n; i += SC_THREADS) {
    const int h = i / c4n, c = (i - h * c4n) * 4;
    *reinterpret_cast<float4*>(dst + (long long)h * g.Cin + c) =
        *reinterpret_cast<const float4*>(sc_row(g, s, (ROWS ? n : g.Tc) - H + h, H) + c);
  }
}

template <bool BF16>
struct sc_bfrag;
template <>
struct sc_bfrag<true> {
  bf16x8 v;
};
template <>
struct sc_bfrag<false> {
  float4 lo, hi;
};

template <bool BF16, int WM, int MREP, int NFR, bool ROWS>
__global__ __launch_bounds__(SC_THREADS) void sconv_kernel(const kantts_sconv_args g, const int ntm, const int ntn,
                                                           const int32_t* rowsp, const int row_cap, const int row_mul) {
  constexpr int WN = 4 / WM;
  constexpr int BQ = WM * MREP * 16;
  constexpr int BN = WN * NFR * 16;
  constexpr int CKS = BF16 ? 128 : 64;  // channels per window slab
  constexpr int LDW = BF16 ? CKS + 8 : CKS + 4;  // row pitch in elements: 16 consecutive rows hit distinct bank groups
  constexpr int PF = (BF16 ? 16 : 4) / NFR;  // (chunk, tap) iterations of weight fragments in flight ahead of the MFMAs
  extern __shared__ __attribute__((aligned(16))) unsigned char sc_lds_raw[];

  int bid = blockIdx.x;
  if (bid < g.S) {
    if (g.K > 1) sc_copy_state<ROWS>(g, bid, rowsp, row_cap, row_mul);
    return;
  }
  bid -= g.S;
  const int tn = bid % ntn;
  const int tm = (bid / ntn) % ntm;
  const int s = bid / (ntn * ntm);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM;
  const int H = (g.K - 1) * g.step;
  const int q0 = tm * BQ;
  int nlive = g.Tc;  // rows of this slot that exist in this call
  if constexpr (ROWS) {
    nlive = sc_live(rowsp, s, row_cap, row_mul);  // one uniform load per workgroup
    if (q0 >= nlive) return;                      // a dead tile: workgroup-uniform, before any load and any barrier
  }
  const int rows = min(BQ, nlive - q0);  // live output rows of this tile (>= 1)
  const int W = rows + H;               // window rows
  const int ncol0 = tn * BN + wn * (NFR * 16);
  const bool wave_live = ncol0 < g.N && wm * (MREP * 16) < rows;  // wave-uniform

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

  // Weight fragments, PF (chunk, tap) iterations ahead.  No lane-dependent select follows a load (it would make the wave
  // wait for the load where it is issued): out-of-range lanes read a CLAMPED, valid address instead -- a column n >= N is
  // never stored, and channels >= Cin meet the zeros the window holds there (weights are finite).
  sc_bfrag<BF16> bcur[PF][NFR], bnext[PF][NFR];
  int fch = 0, fj = 0;  // fetch cursor (chunk, tap); runs up to PF iterations past the end, clamped
  long long ncl[NFR];
#pragma unroll
  for (int nf = 0; nf < NFR; ++nf) ncl[nf] = (long long)min(ncol0 + nf * 16 + (lane & 15), g.N - 1) * g.Cin;
  auto fetch_b = [&](sc_bfrag<BF16> (&dst)[PF][NFR]) {
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
        for (int i0 = tid; i0 < nvec; i0 += SC_THREADS * 4) {
          float4 xv[4];
          int row[4], col[4];
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int i = i0 + v * SC_THREADS;
            row[v] = i / c4n;
            col[v] = (i - row[v] * c4n) * 4;
            const bool ok = i < nvec && cbase + col[v] < g.Cin;
            xv[v] = ok ? *reinterpret_cast<const float4*>(sc_row(g, s, q0 - H + row[v], H) + cbase + col[v])
                       : make_float4(0.f, 0.f, 0.f, 0.f);
          }
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            if (i0 + v * SC_THREADS >= nvec) continue;
            const float v0 = sc_leaky(xv[v].x, g.in_act, g.in_slope), v1 = sc_leaky(xv[v].y, g.in_act, g.in_slope);
            const float v2 = sc_leaky(xv[v].z, g.in_act, g.in_slope), v3 = sc_leaky(xv[v].w, g.in_act, g.in_slope);
            const int o = row[v] * LDW + col[v];
            if constexpr (BF16) {
              bf16x4 p = {(__bf16)v0, (__bf16)v1, (__bf16)v2, (__bf16)v3};
              *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(sc_lds_raw) + o) = p;
            } else {
              *reinterpret_cast<float4*>(reinterpret_cast<float*>(sc_lds_raw) + o) = make_float4(v0, v1, v2, v3);
            }
          }
        }
        __syncthreads();
      }
      if (!wave_live) continue;
      const int back = j * g.step;
      if constexpr (BF16) {
        const __bf16* Wh = reinterpret_cast<const __bf16*>(sc_lds_raw);
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
        const float* Wf = reinterpret_cast<const float*>(sc_lds_raw);
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
            const sc_bfrag<false>& b = bcur[u][nf];
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
#pragma unroll
  for (int nf = 0; nf < NFR; ++nf) {
    const int n = ncol0 + nf * 16 + (lane & 15);
    if (n >= g.N) continue;
    const float bv = g.bias ? g.bias[n] : 0.f;
#pragma unroll
    for (int f = 0; f < MREP; ++f)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = wm * (MREP * 16) + f * 16 + (lane >> 4) * 4 + r;
        if (m >= rows) continue;
        const long long o = ((long long)s * g.Tc + q0 + m) * g.N + n;
        float v = sc_leaky(acc[f][nf][r] + bv, g.out_act, g.out_slope);
        if (g.res) v += g.res[o];
        g.out[o] = v;
      }
  }
}

// N == 1 (conv_post): one thread per output row, a K x Cin fp32 dot product over rows its neighbours share through L1.
// ROWS: a dead row (q >= n_s) loads nothing; it is left alone, or written as 0 with zero_tail.
template <bool ROWS>
__global__ __launch_bounds__(SC_THREADS) void sconv_n1_kernel(const kantts_sconv_args g, const int32_t* rowsp,
                                                              const int row_cap, const int row_mul, const int zero_tail) {
  int bid = blockIdx.x;
  if (bid < g.S) {
    if (g.K > 1) sc_copy_state<ROWS>(g, bid, rowsp, row_cap, row_mul);
    return;
  }
  bid -= g.S;
  const long long e = (long long)bid * SC_THREADS + threadIdx.x;
  if (e >= (long long)g.S * g.Tc) return;
  const int s = (int)(e / g.Tc), q = (int)(e - (long long)s * g.Tc);
  if constexpr (ROWS) {
    if (q >= sc_live(rowsp, s, row_cap, row_mul)) {
      if (zero_tail) g.out[e] = 0.f;
      return;
    }
  }
  const int H = (g.K - 1) * g.step;
  const float* w = reinterpret_cast<const float*>(g.w);
  float acc = 0.f;
  for (int j = 0; j < g.K; ++j) {
    const float* x = sc_row(g, s, q - j * g.step, H);
    const float* wr = w + (long long)j * g.Cin;
    for (int c = 0; c < g.Cin; c += 4) {
      const float4 xv = *reinterpret_cast<const float4*>(x + c), wv = *reinterpret_cast<const float4*>(wr + c);
      acc += sc_leaky(xv.x, g.in_act, g.in_slope) * wv.x;
      acc += sc_leaky(xv.y, g.in_act, g.in_slope) * wv.y;
      acc += sc_leaky(xv.z, g.in_act, g.in_slope) * wv.z;
      acc += sc_leaky(xv.w, g.in_act, g.in_slope) * wv.w;
    }
  }
  if (g.bias) acc += g.bias[0];
  acc = sc_leaky(acc, g.out_act, g.out_slope);
  if (g.res) acc += g.res[e];
  g.out[e] = acc;
}

// the per-slot counts of kantts_sconv_rows_launch as the kernels take them (all unused by the ROWS = false instantiations)
struct sc_rows {
  const int32_t* p;
  int cap, mul, zero_tail;
};

template <bool BF16, int WM, int MREP, int NFR, bool ROWS>
static int sc_launch(const kantts_sconv_args& g, const sc_rows& r, hipStream_t st) {
  constexpr int BQ = WM * MREP * 16;
  constexpr int BN = (4 / WM) * NFR * 16;
  constexpr int LDW = BF16 ? 128 + 8 : 64 + 4;
  const int H = (g.K - 1) * g.step;
  const int ntm = kantts_cdiv(g.Tc, BQ), ntn = kantts_cdiv(g.N, BN);
  const long long blocks = (long long)g.S * ntm * ntn + g.S;
  if (blocks > 0x7fffffffLL) return KANTTS_E_UNSUPPORTED;
  const size_t lds = (size_t)(BQ + H) * LDW * (BF16 ? 2 : 4);  // <= (128 + 70) * 272 B = 52.6 KB
  hipLaunchKernelGGL((sconv_kernel<BF16, WM, MREP, NFR, ROWS>), dim3((unsigned)blocks), dim3(SC_THREADS), lds, st, g, ntm, ntn,
                     r.p, r.cap, r.mul);
  KANTTS_CHECK_LAUNCH();
}

// Tile choice.  Rows: one 16-row tile with the four waves side by side over the channels for the few-row early stages of a
// short chunk, 64 or 128 rows with the waves stacked over the rows otherwise.  Channels per wave (NFR fragments of 16): a
// chunk-sized problem is bound by the latency of streaming its weights (K * N * Cin elements that no cache level holds
// across the 78 layers of a step), so the narrowest tile is taken until the grid has a workgroup or two per CU -- every
// workgroup then streams a 1/ntn slice of the weights with 16 (bf16) iterations of fragments in flight per wave.
// With per-slot counts the choice is still made from Tc (the counts are not known on the host): the same tiles, and
// therefore the same bits, as the plain launch of the same Tc.
template <bool BF16, int WM, int MREP, bool ROWS>
static int sc_pick_n(const kantts_sconv_args& g, const sc_rows& r, hipStream_t st) {
  constexpr int BQ = WM * MREP * 16, WN = 4 / WM;
  const long long mt = (long long)g.S * kantts_cdiv(g.Tc, BQ);
  auto blocks = [&](int nfr) { return mt * kantts_cdiv(g.N, WN * nfr * 16); };
  if (g.N > WN * 32 && blocks(4) >= 384) return sc_launch<BF16, WM, MREP, 4, ROWS>(g, r, st);
  if (g.N > WN * 16 && blocks(2) >= 384) return sc_launch<BF16, WM, MREP, 2, ROWS>(g, r, st);
  return sc_launch<BF16, WM, MREP, 1, ROWS>(g, r, st);
}

template <bool BF16, bool ROWS>
static int sc_dispatch(const kantts_sconv_args& g, const sc_rows& r, hipStream_t st) {
  if (g.Tc <= 16) return sc_pick_n<BF16, 1, 1, ROWS>(g, r, st);
  if (g.Tc <= 64) return sc_pick_n<BF16, 4, 1, ROWS>(g, r, st);
  return sc_pick_n<BF16, 4, 2, ROWS>(g, r, st);
}

// argument checks, clamping and launch of both entry points
template <bool ROWS>
static int sc_run(kantts_sconv_args g, const sc_rows& r, void* stream) {
  if (!g.in || !g.w || !g.out) return KANTTS_E_BADARG;
  if (g.K < 1 || g.step < 1 || g.Cin < 1 || g.N < 1 || (g.precision != 0 && g.precision != 1)) return KANTTS_E_BADARG;
  if (g.K > 1 && (!g.hist_in || !g.hist_out || g.hist_in == g.hist_out)) return KANTTS_E_BADARG;
  if (g.K > SC_MAXK || g.step > SC_MAXSTEP || (g.Cin & 7) || g.Cin < 16 || g.Cin > 512 ||
      !(g.N == 1 || (g.N >= 16 && g.N <= 4096)))
    return KANTTS_E_UNSUPPORTED;
  if (((uintptr_t)g.in & 15) || ((uintptr_t)g.w & 15) || ((uintptr_t)g.hist_in & 15) || ((uintptr_t)g.hist_out & 15) ||
      (g.hist_ss & 3) || g.hist_ss < 0)
    return KANTTS_E_UNSUPPORTED;
  g.S = g.S > 0 ? g.S : 0;
  g.Tc = g.Tc > 0 ? g.Tc : 0;
  if (g.S == 0 || g.Tc == 0) return KANTTS_OK;
  if (g.K > 1 && g.hist_ss < (long long)(g.K - 1) * g.step * g.Cin && g.S > 1) return KANTTS_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (g.N == 1) {
    const long long blocks = ((long long)g.S * g.Tc + SC_THREADS - 1) / SC_THREADS + g.S;
    if (blocks > 0x7fffffffLL) return KANTTS_E_UNSUPPORTED;
    hipLaunchKernelGGL(sconv_n1_kernel<ROWS>, dim3((unsigned)blocks), dim3(SC_THREADS), 0, st, g, r.p, r.cap, r.mul,
                       r.zero_tail);
    KANTTS_CHECK_LAUNCH();
  }
  return g.precision == 1 ? sc_dispatch<true, ROWS>(g, r, st) : sc_dispatch<false, ROWS>(g, r, st);
}

extern "C" int kantts_sconv_launch(const kantts_sconv_args* a, void* stream) {
  if (!a) return KANTTS_E_BADARG;
  return sc_run<false>(*a, sc_rows{nullptr, 0, 1, 0}, stream);
}

extern "C" int kantts_sconv_rows_launch(const kantts_sconv_rows_args* a, void* stream) {
  if (!a || !a->rows || a->row_mul < 1) return KANTTS_E_BADARG;
  kantts_sconv_args g;
  g.in = a->in, g.hist_in = a->hist_in, g.hist_out = a->hist_out, g.w = a->w, g.bias = a->bias, g.res = a->res;
  g.out = a->out, g.hist_ss = a->hist_ss;
  g.S = a->S, g.Tc = a->Tc, g.Cin = a->Cin, g.N = a->N, g.K = a->K, g.step = a->step;
  g.in_slope = a->in_slope, g.in_act = a->in_act, g.out_slope = a->out_slope, g.out_act = a->out_act;
  g.precision = a->precision;
  const int Tc = g.Tc > 0 ? g.Tc : 0;
  if (Tc % a->row_mul != 0) return KANTTS_E_BADARG;
  if (a->zero_tail && g.N != 1) return KANTTS_E_UNSUPPORTED;  // the zero tail exists in the N == 1 kernel only
  return sc_run<true>(g, sc_rows{a->rows, Tc / a->row_mul, a->row_mul, a->zero_tail != 0}, stream);
}
