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
// Shared with csrc/sconv_sym.hip, the layer of symmetric networks: the tile loop between a kernel's prologue and its
// epilogue (csrc/sconv_body.inc), and the host side from the argument checks to the tile choice (csrc/sconv_common.inc).
//
// Reference: CausalConv1d / CausalConvTranspose1d, kantts/models/hifigan/layers.py:52-165 (their left zero pad is the
// zero state of a fresh slot).
#include "sconv_common.inc"

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
  for (int i = threadIdx.x; i < H * c4n; i += SCONV_THREADS) {
    const int h = i / c4n, c = (i - h * c4n) * 4;
    *reinterpret_cast<float4*>(dst + (long long)h * g.Cin + c) =
        *reinterpret_cast<const float4*>(sconv_row(g, s, (ROWS ? n : g.Tc) - H + h, H) + c);
  }
}

template <bool BF16, int WM, int MREP, int NFR, bool ROWS>
__global__ __launch_bounds__(SCONV_THREADS) void sconv_kernel(const kantts_sconv_args g, const int ntm, const int ntn,
                                                              const int32_t* rowsp, const int row_cap, const int row_mul) {
  constexpr int WN = 4 / WM;
  constexpr int BQ = WM * MREP * 16;
  constexpr int BN = WN * NFR * 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char sconv_lds_raw[];

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

#define SCONV_WINDOW_ROW(r) sconv_row(g, s, q0 - H + (r), H)  // window row r is row q0 - H + r of X
#define SCONV_ROW_LOADED(r) true                              // every window row exists
#include "sconv_body.inc"

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
        float v = sconv_leaky(acc[f][nf][r] + bv, g.out_act, g.out_slope);
        if (g.res) v += g.res[o];
        g.out[o] = v;
      }
  }
}

// N == 1 (conv_post): one thread per output row, a K x Cin fp32 dot product over rows its neighbours share through L1.
// ROWS: a dead row (q >= n_s) loads nothing; it is left alone, or written as 0 with zero_tail.
template <bool ROWS>
__global__ __launch_bounds__(SCONV_THREADS) void sconv_n1_kernel(const kantts_sconv_args g, const int32_t* rowsp,
                                                              const int row_cap, const int row_mul, const int zero_tail) {
  int bid = blockIdx.x;
  if (bid < g.S) {
    if (g.K > 1) sc_copy_state<ROWS>(g, bid, rowsp, row_cap, row_mul);
    return;
  }
  bid -= g.S;
  const long long e = (long long)bid * SCONV_THREADS + threadIdx.x;
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
    const float* x = sconv_row(g, s, q - j * g.step, H);
    const float* wr = w + (long long)j * g.Cin;
    for (int c = 0; c < g.Cin; c += 4) {
      const float4 xv = *reinterpret_cast<const float4*>(x + c), wv = *reinterpret_cast<const float4*>(wr + c);
      acc += sconv_leaky(xv.x, g.in_act, g.in_slope) * wv.x;
      acc += sconv_leaky(xv.y, g.in_act, g.in_slope) * wv.y;
      acc += sconv_leaky(xv.z, g.in_act, g.in_slope) * wv.z;
      acc += sconv_leaky(xv.w, g.in_act, g.in_slope) * wv.w;
    }
  }
  if (g.bias) acc += g.bias[0];
  acc = sconv_leaky(acc, g.out_act, g.out_slope);
  if (g.res) acc += g.res[e];
  g.out[e] = acc;
}

// the per-slot counts of kantts_sconv_rows_launch as the kernels take them (all unused by the ROWS = false instantiations)
struct sc_rows {
  const int32_t* p;
  int cap, mul, zero_tail;
};

// both entry points: the common procedure (sconv_run: argument checks, clamping, tile choice) with this file's kernels
template <bool ROWS>
static int sc_run(kantts_sconv_args g, const sc_rows& r, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  auto launch_n1 = [&](unsigned blocks) -> int {
    hipLaunchKernelGGL(sconv_n1_kernel<ROWS>, dim3(blocks), dim3(SCONV_THREADS), 0, st, g, r.p, r.cap, r.mul, r.zero_tail);
    KANTTS_CHECK_LAUNCH();
  };
  auto launch_tile = [&](auto t, unsigned blocks, size_t lds, int ntm, int ntn) -> int {
    using T = decltype(t);
    hipLaunchKernelGGL((sconv_kernel<T::BF16, T::WM, T::MREP, T::NFR, ROWS>), dim3(blocks), dim3(SCONV_THREADS), lds, st, g,
                       ntm, ntn, r.p, r.cap, r.mul);
    KANTTS_CHECK_LAUNCH();
  };
  return sconv_run(g, /*lag*/ 0, /*row_mul*/ 1, /*own_bad*/ false, /*own_unsupported*/ false, launch_n1, launch_tile);
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
