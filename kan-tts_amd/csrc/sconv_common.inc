// What csrc/sconv.hip (causal layers) and csrc/sconv_sym.hip (symmetric layers) share besides the tile loop of
// sconv_body.inc: the limits and fragment types of that loop, and on the host the ONE tile choice, grid / LDS formula and
// common argument contract of kantts_sconv_launch, kantts_sconv_rows_launch and kantts_sconv_sym_rows_launch.
#pragma once
#include "common.h"

#define SCONV_THREADS 256
#define SCONV_MAXK 11
#define SCONV_MAXSTEP 7

__device__ __forceinline__ float sconv_leaky(float v, int act, float slope) { return (act && !(v > 0.f)) ? v * slope : v; }

// row t (>= -Hs) of slot s of X = [hist_in ; in], Hs = the rows of the state (A, here and below: either args struct)
template <class A>
__device__ __forceinline__ const float* sconv_row(const A& g, int s, int t, int Hs) {
  return t < 0 ? g.hist_in + (long long)s * g.hist_ss + (long long)(Hs + t) * g.Cin
               : g.in + ((long long)s * g.Tc + t) * g.Cin;
}

// a lane's B fragment of one (chunk, tap) iteration: 8 consecutive channels of one output channel
template <bool BF16>
struct sconv_bfrag;
template <>
struct sconv_bfrag<true> {
  bf16x8 v;
};
template <>
struct sconv_bfrag<false> {
  float4 lo, hi;
};

// ---- host side.  A tile as a value: what the tile choice hands to the file's own launch
template <bool BF16_, int WM_, int MREP_, int NFR_>
struct sconv_tile {
  static constexpr bool BF16 = BF16_;
  static constexpr int WM = WM_, MREP = MREP_, NFR = NFR_;
};

// Tile choice.  Rows: one 16-row tile with the four waves side by side over the channels for the few-row early stages of a
// short chunk, 64 or 128 rows with the waves stacked over the rows otherwise.  Channels per wave (NFR fragments of 16): a
// chunk-sized problem is bound by the latency of streaming its weights (K * N * Cin elements that no cache level holds
// across the 78 layers of a step), so the narrowest tile is taken until the grid has a workgroup or two per CU -- every
// workgroup then streams a 1/ntn slice of the weights with 16 (bf16) iterations of fragments in flight per wave.
// With per-slot counts the choice is still made from Tc (the counts are not known on the host): the same tiles, and
// therefore the same bits, as the plain launch of the same Tc -- and the same tiles in both files, whatever the lag.
// launch_tile(tile, blocks, lds_bytes, ntm, ntn) is the file's hipLaunchKernelGGL of its kernel for that tile.
template <bool BF16, int WM, int MREP, class A, class L>
static int sconv_pick_n(const A& g, L& launch_tile) {
  constexpr int BQ = WM * MREP * 16, WN = 4 / WM, LDW = BF16 ? 128 + 8 : 64 + 4;
  const int ntm = kantts_cdiv(g.Tc, BQ), H = (g.K - 1) * g.step;
  auto ntn = [&](int nfr) { return kantts_cdiv(g.N, WN * nfr * 16); };
  auto blocks = [&](int nfr) { return (long long)g.S * ntm * ntn(nfr); };
  auto launch = [&](auto tile) -> int {
    const long long grid = blocks(tile.NFR) + g.S;  // the first S workgroups carry the state
    if (grid > 0x7fffffffLL) return KANTTS_E_UNSUPPORTED;
    const size_t lds = (size_t)(BQ + H) * LDW * (BF16 ? 2 : 4);  // <= (128 + 70) * 272 B = 52.6 KB
    return launch_tile(tile, (unsigned)grid, lds, ntm, ntn(tile.NFR));
  };
  if (g.N > WN * 32 && blocks(4) >= 384) return launch(sconv_tile<BF16, WM, MREP, 4>{});
  if (g.N > WN * 16 && blocks(2) >= 384) return launch(sconv_tile<BF16, WM, MREP, 2>{});
  return launch(sconv_tile<BF16, WM, MREP, 1>{});
}

template <bool BF16, class A, class L>
static int sconv_pick_m(const A& g, L& launch_tile) {
  if (g.Tc <= 16) return sconv_pick_n<BF16, 1, 1>(g, launch_tile);
  if (g.Tc <= 64) return sconv_pick_n<BF16, 4, 1>(g, launch_tile);
  return sconv_pick_n<BF16, 4, 2>(g, launch_tile);
}

// The one procedure of the three entry points, from the argument checks to the launch.  Every KANTTS_E_BADARG condition
// (the common ones and own_bad, the entry point's own) ranks before every KANTTS_E_UNSUPPORTED one (the common ones and
// own_unsupported); then S and Tc are clamped IN g.  The state has Hs = (K - 1) * step + lag rows.  launch_n1(blocks) is the
// file's hipLaunchKernelGGL of its N == 1 kernel.
template <class A, class L1, class L>
static int sconv_run(A& g, int lag, int row_mul, bool own_bad, bool own_unsupported, L1 launch_n1, L launch_tile) {
  if (!g.in || !g.w || !g.out || own_bad) return KANTTS_E_BADARG;
  if (g.K < 1 || g.step < 1 || g.Cin < 1 || g.N < 1 || (g.precision != 0 && g.precision != 1)) return KANTTS_E_BADARG;
  const long long Hs = (long long)(g.K - 1) * g.step + lag;
  if (Hs > 0 && (!g.hist_in || !g.hist_out || g.hist_in == g.hist_out)) return KANTTS_E_BADARG;
  if (g.K > SCONV_MAXK || g.step > SCONV_MAXSTEP || (g.Cin & 7) || g.Cin < 16 || g.Cin > 512 ||
      !(g.N == 1 || (g.N >= 16 && g.N <= 4096)) || Hs > 0x3fffffff || own_unsupported)
    return KANTTS_E_UNSUPPORTED;
  if (((uintptr_t)g.in & 15) || ((uintptr_t)g.w & 15) || ((uintptr_t)g.hist_in & 15) || ((uintptr_t)g.hist_out & 15) ||
      (g.hist_ss & 3) || g.hist_ss < 0)
    return KANTTS_E_UNSUPPORTED;
  g.S = g.S > 0 ? g.S : 0;
  g.Tc = g.Tc > 0 ? g.Tc : 0;
  if (g.Tc % row_mul != 0) return KANTTS_E_BADARG;
  if (g.S == 0 || g.Tc == 0) return KANTTS_OK;
  if (Hs > 0 && g.hist_ss < Hs * g.Cin && g.S > 1) return KANTTS_E_BADARG;  // the states of two slots would overlap
  if (g.N == 1) {
    const long long blocks = ((long long)g.S * g.Tc + SCONV_THREADS - 1) / SCONV_THREADS + g.S;
    if (blocks > 0x7fffffffLL) return KANTTS_E_UNSUPPORTED;
    return launch_n1((unsigned)blocks);
  }
  return g.precision == 1 ? sconv_pick_m<true>(g, launch_tile) : sconv_pick_m<false>(g, launch_tile);
}

