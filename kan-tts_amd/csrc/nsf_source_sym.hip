// The NSF excitation of chunked inference for NON-CAUSAL generators: the sine source of csrc/nsf_source.hip stopped at the
// utterance's end, and the symmetric source_downs convolutions (kernel 2 u, stride u, padding u / 2) read with the lag
// that lines them up with the delayed output of every stage's polyphase up-layer (csrc/sconv_sym.hip).  Two launches per
// step, both per slot, fp32 VALU / LDS in both precision modes, driven by the device buffers the rest of a
// ChunkedNCVocoder step reads:
//   rows[s]            n_s = clamp(rows[s], 0, Tc) frames of slot s in this call, flush frames included
//   end[s]             frames of the slot's utterance, < 0 while it is open (end == NULL: every slot is open)
//   pos_in[s * pos_ss] frames the slot consumed before this call: the arena word of sconv_sym.hip, NOT the source's own
//                      cursor, which stops at the end
// The arithmetic is csrc/nsf_source_body.inc, the bodies csrc/nsf_source.hip runs too.
//
// kantts_nsf_source_end_rows -- kantts_nsf_source_rows on the first l_s frames of every slot,
//   l_s = n_s when end_s < 0, else clamp(end_s - pos_s, 0, n_s):
// the same bits of e, harm and state_out as that entry gives for n_s = l_s.  Frames at or beyond l_s (flush frames) are not
// loaded, samples at or beyond l_s * hop are not written, l_s == 0 copies the state bit for bit: phase, cursor and noise
// position stop where the utterance does.
//
// kantts_nsf_downs_sym_rows -- every source_downs convolution in one launch, stage i with the lag lag[i]:
//   d_i[s, q, c] = bias_i[c] + sum_{j < k_i} w_i[j][c] * E[s, q * u_i - lag_i + j],    q < n_s * hop / u_i
//   E[s, t] = e[s, t] for 0 <= t < n_s * hop inside the utterance (end_s < 0 or pos_s * hop + t < end_s * hop), 0.0f and
//   NOT loaded behind it (the reference's right pad), hist_in[s, Hh + t] for -Hh <= t < 0 (a zero history: its left pad).
// The symmetric convolution's true row m reads e[m u - p + j], and the up-layer's stream row q is true row q - D, so
// lag = D u + p; lag >= k - u keeps every tap inside what the slot has seen.  The history is the last Hh >= max lag samples
// of E, written by S extra workgroups of the same launch.  A tile's LDS window is (rows - 1) u + k samples whatever the lag:
// the lag moves the window's base.  lag = k - 1 without an end is kantts_nsf_downs_rows, bit for bit (same tiles, same
// summation order).
#include "nsf_source_body.inc"

// live frames of slot s: the frames of this call that lie inside the utterance
__device__ __forceinline__ int nsf_inside(const int32_t* end, const int32_t* pos_in, long long pos_ss, int s, int n) {
  if (!end) return n;
  const int e = end[s];
  if (e < 0) return n;
  return (int)min(max((long long)e - (long long)pos_in[(long long)s * pos_ss], 0LL), (long long)n);
}

__global__ __launch_bounds__(NSF_THREADS) void nsf_source_end_kernel(const kantts_nsf_source_end_args a) {
  __shared__ nsf_source_lds lds;
  const kantts_nsf_source_args& g = a.src;
  int bid = blockIdx.x;
  if (bid < g.S) {
    nsf_source_state(g, bid, nsf_inside(a.end, a.pos_in, a.pos_ss, bid, nsf_live(g.rows, bid, g.Tc)));
    return;
  }
  bid -= g.S;
  const int s = bid / g.Tc, k = bid - s * g.Tc;
  // a dead or a flush frame: workgroup-uniform, before any load of f0 / uv / noise
  if (k >= nsf_inside(a.end, a.pos_in, a.pos_ss, s, nsf_live(g.rows, s, g.Tc))) return;
  nsf_source_frame(g, s, k, lds);
}

extern "C" int kantts_nsf_source_end_rows(const kantts_nsf_source_end_args* a, void* stream) {
  if (!a) return KANTTS_E_BADARG;
  if ((a->end && !a->pos_in) || a->pos_ss < 0) return KANTTS_E_BADARG;
  long long blocks;
  const int rc = nsf_source_check(&a->src, &blocks);
  if (rc != KANTTS_OK || blocks == 0) return rc;
  hipLaunchKernelGGL(nsf_source_end_kernel, dim3((unsigned)blocks), dim3(NSF_THREADS), 0, (hipStream_t)stream, *a);
  KANTTS_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NSF_THREADS) void nsf_downs_sym_kernel(const kantts_nsf_downs_sym_args a, const nsf_downs_plan p) {
  __shared__ float s_E[NSF_WINDOW];
  const kantts_nsf_downs_args& g = a.d;
  // the first sample of e[s] behind the utterance (frames * hop while it is open): from there on E is zero
  auto lim_of = [&](int s, int frames) { return nsf_inside(a.end, a.pos_in, a.pos_ss, s, frames) * g.hop; };
  const int bid = blockIdx.x;
  if (bid < g.S) {
    const int frames = nsf_live(g.rows, bid, g.Tc);
    nsf_downs_hist(g, bid, p.Hh, frames * g.hop, lim_of(bid, frames));
    return;
  }
  nsf_downs_tile(g, p, s_E, bid - g.S, [&](int i) { return a.lag[i]; }, lim_of);
}

extern "C" int kantts_nsf_downs_sym_rows(const kantts_nsf_downs_sym_args* a, void* stream) {
  if (!a) return KANTTS_E_BADARG;
  if ((a->end && !a->pos_in) || a->pos_ss < 0 || a->Hh < 0) return KANTTS_E_BADARG;
  const kantts_nsf_downs_args* d = &a->d;
  nsf_downs_plan p;
  long long blocks;
  const int rc = nsf_downs_make_plan(d, &p, &blocks);
  if (rc != KANTTS_OK) return rc;
  p.Hh = a->Hh;
  for (int i = 0; i < d->nstages; ++i)  // a tap in the future of the slot, or behind the history it keeps
    if (a->lag[i] < d->k[i] - d->u[i] || a->lag[i] > a->Hh) return KANTTS_E_BADARG;
  if (p.Hh > 0 && (!d->hist_in || !d->hist_out || d->hist_in == d->hist_out)) return KANTTS_E_BADARG;
  if (d->S > 1 && d->hist_ss < p.Hh) return KANTTS_E_BADARG;
  if (d->S <= 0) return KANTTS_OK;
  blocks += d->S;
  hipLaunchKernelGGL(nsf_downs_sym_kernel, dim3((unsigned)blocks), dim3(NSF_THREADS), 0, (hipStream_t)stream, *a, p);
  KANTTS_CHECK_LAUNCH();
}
