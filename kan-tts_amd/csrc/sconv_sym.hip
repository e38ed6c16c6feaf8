// The layer of chunked inference for SYMMETRIC (non-causal) networks: kantts_sconv_sym_rows_launch.
//
// A symmetric convolution of padding p is the causal convolution with the same taps whose output stream is p rows late,
// so a non-causal network is a causal one whose tensors carry integer delays -- provided every layer's output is zero
// outside the utterance (the reference pads every layer at the utterance's edges) and the end is flushed.  This file is
// the rule of csrc/sconv.hip's per-slot kernel (same tiles: the tile choice of csrc/sconv_common.inc; same MFMA path in both
// precisions, same chunk-major, tap-inner summation order: the tile loop of csrc/sconv_body.inc) with what that needs:
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
#include "sconv_common.inc"

#define SS_OPEN 0x7fffffffffffffffLL

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
  for (int i = threadIdx.x; i < Hs * c4n; i += SCONV_THREADS) {
    const int h = i / c4n, c = (i - h * c4n) * 4;
    const int t = k.nlive - Hs + h;
    *reinterpret_cast<float4*>(dst + (long long)h * g.Cin + c) =
        t >= k.in_lim ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(sconv_row(g, s, t, Hs) + c);
  }
  if (g.pos_out && threadIdx.x == 0) g.pos_out[(long long)s * g.pos_ss] = k.pos + k.nlive / g.row_mul;
}

template <bool BF16, int WM, int MREP, int NFR>
__global__ __launch_bounds__(SCONV_THREADS) void sconv_sym_kernel(const kantts_sconv_sym_args g, const int ntm, const int ntn,
                                                               const int row_cap, const int cps) {
  constexpr int WN = 4 / WM;
  constexpr int BQ = WM * MREP * 16;
  constexpr int BN = WN * NFR * 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char sconv_lds_raw[];

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
    for (int i = tid; i < rows * ncols; i += SCONV_THREADS) {
      const int m = i / ncols, n = tn * BN + (i - m * ncols);
      g.out[((long long)s * g.Tc + q0 + m) * g.N + n] = 0.f;
    }
    return;
  }

#define SCONV_WINDOW_ROW(r) sconv_row(g, s, t0 + (r), Hs)  // window row r is row t0 + r of X
#define SCONV_ROW_LOADED(r) (t0 + (r) < sl.in_lim)         // a flush row is not loaded: zeros
#include "sconv_body.inc"

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
          v = sconv_leaky(acc[f][nf][r] + bv, g.out_act, g.out_slope);
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
__global__ __launch_bounds__(SCONV_THREADS) void sconv_sym_n1_kernel(const kantts_sconv_sym_args g, const int row_cap) {
  int bid = blockIdx.x;
  if (bid < g.S) {
    ss_copy_state(g, bid, row_cap);
    return;
  }
  bid -= g.S;
  const long long e = (long long)bid * SCONV_THREADS + threadIdx.x;
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
    const float* x = sconv_row(g, s, t, Hs);
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
  if (g.res) {
    const int rq = q - g.res_lag;
    acc += rq >= 0 ? g.res[(long long)s * g.Tc + rq] : g.res_hist[(long long)s * g.res_hist_ss + g.res_hist_rows + rq];
  }
  g.out[e] = acc;
}

extern "C" int kantts_sconv_sym_rows_launch(const kantts_sconv_sym_args* a, void* stream) {
  if (!a) return KANTTS_E_BADARG;
  kantts_sconv_sym_args g = *a;
  const bool own_bad =
      !g.rows || !g.end || !g.pos_in || g.pos_out == g.pos_in || g.row_mul < 1 || g.lag < 0 || g.res_lag < 0 || g.delay < 0 ||
      g.sub < 1 || g.N % g.sub != 0 || g.pos_ss < 0 || (g.res_hist && !g.res) ||
      (g.res_lag > 0 && (!g.res || !g.res_hist || g.res_lag > g.res_hist_rows || g.res_hist_ss < 0));
  const bool own_unsupported = g.zero_tail && g.N != 1;  // the zero tail exists in the N == 1 kernel only
  hipStream_t st = (hipStream_t)stream;
  // the lambdas run behind the checks, with S and Tc clamped: row_cap = Tc / row_mul
  auto launch_n1 = [&](unsigned blocks) -> int {
    hipLaunchKernelGGL(sconv_sym_n1_kernel, dim3(blocks), dim3(SCONV_THREADS), 0, st, g, g.Tc / g.row_mul);
    KANTTS_CHECK_LAUNCH();
  };
  // the tile of the causal layer of the same shape (chosen from Tc, S and N alone); cps = N / sub columns per sample
  auto launch_tile = [&](auto t, unsigned blocks, size_t lds, int ntm, int ntn) -> int {
    using T = decltype(t);
    hipLaunchKernelGGL((sconv_sym_kernel<T::BF16, T::WM, T::MREP, T::NFR>), dim3(blocks), dim3(SCONV_THREADS), lds, st, g, ntm,
                       ntn, g.Tc / g.row_mul, g.N / g.sub);
    KANTTS_CHECK_LAUNCH();
  };
  return sconv_run(g, g.lag, g.row_mul, own_bad, own_unsupported, launch_n1, launch_tile);
}
