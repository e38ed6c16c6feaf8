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
#include "nsf_source_body.inc"  // the bodies of both kernels, shared with csrc/nsf_source_sym.hip

__global__ __launch_bounds__(NSF_THREADS) void nsf_source_kernel(const kantts_nsf_source_args g) {
  __shared__ nsf_source_lds lds;
  int bid = blockIdx.x;
  if (bid < g.S) {
    nsf_source_state(g, bid, nsf_live(g.rows, bid, g.Tc));
    return;
  }
  bid -= g.S;
  const int s = bid / g.Tc, k = bid - s * g.Tc;
  if (k >= nsf_live(g.rows, s, g.Tc)) return;  // a dead frame: workgroup-uniform, before any load of f0 / uv / noise
  nsf_source_frame(g, s, k, lds);
}

extern "C" int kantts_nsf_source_rows(const kantts_nsf_source_args* a, void* stream) {
  if (!a) return KANTTS_E_BADARG;
  long long blocks;
  const int rc = nsf_source_check(a, &blocks);
  if (rc != KANTTS_OK || blocks == 0) return rc;
  hipLaunchKernelGGL(nsf_source_kernel, dim3((unsigned)blocks), dim3(NSF_THREADS), 0, (hipStream_t)stream, *a);
  KANTTS_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NSF_THREADS) void nsf_downs_kernel(const kantts_nsf_downs_args g, const nsf_downs_plan p) {
  __shared__ float s_E[NSF_WINDOW];
  const int bid = blockIdx.x;
  if (bid < g.S) {
    const int n = nsf_live(g.rows, bid, g.Tc) * g.hop;
    nsf_downs_hist(g, bid, p.Hh, n, n);
    return;
  }
  // left pad k - 1: tap j of row q reads E[q * u - (k - 1) + j]; every sample of the live frames counts
  nsf_downs_tile(g, p, s_E, bid - g.S, [&](int i) { return g.k[i] - 1; }, [&](int, int frames) { return frames * g.hop; });
}

extern "C" int kantts_nsf_downs_rows(const kantts_nsf_downs_args* a, void* stream) {
  if (!a) return KANTTS_E_BADARG;
  nsf_downs_plan p;
  long long blocks;
  const int rc = nsf_downs_make_plan(a, &p, &blocks);
  if (rc != KANTTS_OK) return rc;
  p.Hh = 0;
  for (int i = 0; i < a->nstages; ++i) p.Hh = max(p.Hh, a->k[i] - 1);
  if (p.Hh > 0 && (!a->hist_in || !a->hist_out || a->hist_in == a->hist_out)) return KANTTS_E_BADARG;
  if (a->S > 1 && a->hist_ss < p.Hh) return KANTTS_E_BADARG;
  if (a->S <= 0) return KANTTS_OK;
  blocks += a->S;
  hipLaunchKernelGGL(nsf_downs_kernel, dim3((unsigned)blocks), dim3(NSF_THREADS), 0, (hipStream_t)stream, *a, p);
  KANTTS_CHECK_LAUNCH();
}
