// The tail of a multi-band generator in chunked inference, one launch: conv_post (causal, K taps, step 1, Cin -> B sub-bands,
// LeakyReLU on its input, bias), tanh, and a PQMF synthesis that can be cut at any chunk boundary.  Per slot and driven by the
// same device `rows` buffer and row_mul as kantts_sconv_rows_launch, plus a device `last` flag per slot.  Plain VALU / LDS
// kernel, fp32 in both precision modes (conv_post with one output channel is fp32 for the same reason: the last layer sets
// the noise floor of the waveform, and its K * Cin * B multiply-adds per row are nothing beside the stack in front of it).
//
// The synthesis bank is symmetric: low-rate output row q needs the sub-band rows q - D .. q + D,
//   out[q * B + r] = sum_{d = -D .. D} sum_k W[r, k, d + D] * z[q + d, k],       z = 0 outside the utterance,
// so it looks AHEAD by D rows and nothing causal can carry that as history.  Instead a slot holds back the rows whose future
// it has not seen: state = the last 2 D rows of z (zero at the start) and pending = min(rows of z seen so far, D).  A call
// with n new rows emits max(0, n + pending - D) rows (all n + pending with `last`: the future is zeros), the next rows of
// the utterance in order.  With Z = [state ; new z ; zeros], emitted row i is centred on Z[2 D - pending + i].
//
// Bits.  An utterance's samples must not depend on the chunking, the slot, its batch-mates or the tile:
//   * a z row is computed by ONE function (mb_zrow), explicit fmaf, tap-major and channel-inner, whether a tile, a
//     neighbouring tile's halo or the state workgroup needs it;
//   * an output sample is one fmaf chain, d ascending and k inner (zero rows take part: fmaf(w, 0, acc) == acc);
//   * rows taken from the state are used as stored.
//
// Grid: S state workgroups (state_out, hist_out, emitted -- different buffers from state_in / hist_in, so nobody reads what
// they write), then per slot cdiv(Tq + D, TR) tiles of TR = 256 - 2 D output rows.  A tile builds its window of TR + 2 D = 256
// rows of Z in LDS, one row per thread (rows of the state copied, new rows computed from [hist_in ; in], rows behind the
// slot's count zero: no row >= n_s of `in` is loaded), so the halo recompute is 2 D rows per tile; the weights of conv_post
// are addressed by loop counters only and come through the scalar cache.  Then a thread owns an output row and its B phases.
#include "common.h"

#define MB_THREADS 256
#define MB_MAXB 8
#define MB_MAXD 16
#define MB_MAXK 11

__device__ __forceinline__ float mb_leaky(float v, int act, float slope) { return (act && v < 0.f) ? v * slope : v; }

// raw row t (>= -(K - 1)) of slot s of X = [hist_in ; in]
__device__ __forceinline__ const float* mb_xrow(const kantts_mb_tail_args& g, int s, int t) {
  return t < 0 ? g.hist_in + (long long)s * g.hist_ss + (long long)(g.K - 1 + t) * g.Cin
               : g.in + ((long long)s * g.Tq + t) * g.Cin;
}

// z[0 .. B) = row t (0 <= t < n_s) of the slot's new sub-band rows: tanh(conv_post), or `in` itself in the pass-through form.
// THE definition of a z row: every caller gets the same bits.
template <int B>
__device__ __forceinline__ void mb_zrow(const kantts_mb_tail_args& g, int s, int t, float* z) {
  if (!g.w) {
    const float* x = g.in + ((long long)s * g.Tq + t) * B;
#pragma unroll
    for (int k = 0; k < B; ++k) z[k] = x[k];
    return;
  }
  float acc[B];
#pragma unroll
  for (int k = 0; k < B; ++k) acc[k] = 0.f;
  for (int j = 0; j < g.K; ++j) {
    const float* x = mb_xrow(g, s, t - j);
    const float* wj = g.w + (long long)j * B * g.Cin;
    for (int c = 0; c < g.Cin; c += 4) {
      float4 xv = *reinterpret_cast<const float4*>(x + c);
      xv.x = mb_leaky(xv.x, g.in_act, g.in_slope);
      xv.y = mb_leaky(xv.y, g.in_act, g.in_slope);
      xv.z = mb_leaky(xv.z, g.in_act, g.in_slope);
      xv.w = mb_leaky(xv.w, g.in_act, g.in_slope);
#pragma unroll
      for (int k = 0; k < B; ++k) {
        const float4 wv = *reinterpret_cast<const float4*>(wj + (long long)k * g.Cin + c);
        acc[k] = fmaf(xv.x, wv.x, acc[k]);
        acc[k] = fmaf(xv.y, wv.y, acc[k]);
        acc[k] = fmaf(xv.z, wv.z, acc[k]);
        acc[k] = fmaf(xv.w, wv.w, acc[k]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < B; ++k) z[k] = tanhf(acc[k] + (g.bias ? g.bias[k] : 0.f));
}

// what every workgroup of a slot derives from the device buffers
struct mb_slot {
  int n;     // live new rows
  int p;     // rows held back by the calls before
  int E;     // low-rate rows this call emits
  int last;
};

template <int B>
__device__ __forceinline__ mb_slot mb_plan(const kantts_mb_tail_args& g, int s) {
  mb_slot m;
  m.n = g.rows ? min(max(g.rows[s], 0), g.Tq / g.row_mul) * g.row_mul : g.Tq;
  const int32_t* si = reinterpret_cast<const int32_t*>(g.state_in + (long long)s * g.state_ss);
  m.p = min(max(si[2 * g.D * B], 0), g.D);
  m.last = g.last ? (g.last[s] != 0) : 0;
  m.E = m.last ? m.n + m.p : max(0, m.n + m.p - g.D);
  return m;
}

// z[0 .. B) = row j of Z = [state (2 D rows) ; new z (n rows) ; zeros]
template <int B>
__device__ __forceinline__ void mb_Zrow(const kantts_mb_tail_args& g, int s, int n, int j, float* z) {
  if (j < 2 * g.D) {
    const float* st = g.state_in + (long long)s * g.state_ss + (long long)j * B;
#pragma unroll
    for (int k = 0; k < B; ++k) z[k] = st[k];
  } else if (j < 2 * g.D + n) {
    mb_zrow<B>(g, s, j - 2 * g.D, z);
  } else {
#pragma unroll
    for (int k = 0; k < B; ++k) z[k] = 0.f;
  }
}

template <int B>
__global__ __launch_bounds__(MB_THREADS) void mb_tail_kernel(const kantts_mb_tail_args g, const int nt) {
  __shared__ float s_z[MB_THREADS * B];
  __shared__ float s_poly[(2 * MB_MAXD + 1) * B * B];
  int bid = blockIdx.x;
  const int tid = threadIdx.x;
  const int D = g.D;
  if (bid < g.S) {
    // ---- the state of slot bid after this call
    const int s = bid;
    const mb_slot m = mb_plan<B>(g, s);
    float* so = g.state_out + (long long)s * g.state_ss;
    if (tid < 2 * D) {  // the last 2 D rows of Z[0 : 2 D + n]; after `last` the slot is as after a reset
      float z[B];
      if (m.last) {
#pragma unroll
        for (int k = 0; k < B; ++k) z[k] = 0.f;
      } else {
        mb_Zrow<B>(g, s, m.n, m.n + tid, z);
      }
#pragma unroll
      for (int k = 0; k < B; ++k) so[(long long)tid * B + k] = z[k];
    }
    if (tid == 0) {
      reinterpret_cast<int32_t*>(so)[2 * D * B] = m.last ? 0 : min(m.n + m.p, D);
      if (g.emitted) g.emitted[s] = m.E * B;
    }
    if (g.w && g.K > 1) {  // hist_out: the last K - 1 raw rows of [hist_in ; in[0 : n]] (a copy when n == 0), zeros after `last`
      const int H = g.K - 1;
      float* ho = g.hist_out + (long long)s * g.hist_ss;
      for (int i = tid; i < H * g.Cin; i += MB_THREADS) {
        const int h = i / g.Cin, c = i - h * g.Cin;
        ho[i] = m.last ? 0.f : mb_xrow(g, s, m.n - H + h)[c];
      }
    }
    return;
  }
  bid -= g.S;
  const int s = bid / nt, tile = bid - s * nt;
  const int TR = MB_THREADS - 2 * D;
  const int total = g.Tq + D;  // low-rate rows of the slot's output buffer
  const int i0 = tile * TR;
  const mb_slot m = mb_plan<B>(g, s);
  const int live = min(TR, m.E - i0);
  float* out = g.out + ((long long)s * total + i0) * B;
  if (live <= 0) {  // a dead tile: zeros, before any load of `in` and any barrier (workgroup-uniform)
    if (tid < TR && i0 + tid < total) {
#pragma unroll
      for (int r = 0; r < B; ++r) out[(long long)tid * B + r] = 0.f;
    }
    return;
  }
  // poly (B, B, 2 D + 1) -> s_poly[d][k][r]: the B phases of one (d, k) side by side
  for (int x = tid; x < (2 * D + 1) * B * B; x += MB_THREADS) {
    const int d = x / (B * B), k = (x / B) % B, r = x % B;
    s_poly[x] = g.poly[(r * B + k) * (2 * D + 1) + d];
  }
  // the window: emitted row i0 + i is centred on Z[2 D - p + i0 + i], so window row w is Z[D - p + i0 + w]
  if (tid < live + 2 * D) {
    float z[B];
    mb_Zrow<B>(g, s, m.n, D - m.p + i0 + tid, z);
#pragma unroll
    for (int k = 0; k < B; ++k) s_z[tid * B + k] = z[k];
  }
  __syncthreads();
  if (tid >= TR || i0 + tid >= total) return;
  float acc[B];
#pragma unroll
  for (int r = 0; r < B; ++r) acc[r] = 0.f;
  if (tid < live) {
    for (int d = 0; d <= 2 * D; ++d) {
      const float* zr = s_z + (tid + d) * B;
      const float* pw = s_poly + d * B * B;
#pragma unroll
      for (int k = 0; k < B; ++k) {
        const float zv = zr[k];
#pragma unroll
        for (int r = 0; r < B; ++r) acc[r] = fmaf(pw[k * B + r], zv, acc[r]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < B; ++r) out[(long long)tid * B + r] = acc[r];  // rows behind the emitted count: 0.0f
}

template <int B>
static int mb_launch(const kantts_mb_tail_args& g, hipStream_t st) {
  const int nt = kantts_cdiv((long long)g.Tq + g.D, MB_THREADS - 2 * g.D);
  const long long blocks = (long long)g.S * nt + g.S;
  if (blocks > 0x7fffffffLL) return KANTTS_E_UNSUPPORTED;
  hipLaunchKernelGGL(mb_tail_kernel<B>, dim3((unsigned)blocks), dim3(MB_THREADS), 0, st, g, nt);
  KANTTS_CHECK_LAUNCH();
}

extern "C" int kantts_mb_tail_rows(const kantts_mb_tail_args* a, void* stream) {
  if (!a || !a->in || !a->poly || !a->out || !a->state_in || !a->state_out || a->state_in == a->state_out)
    return KANTTS_E_BADARG;
  if (a->row_mul < 1) return KANTTS_E_BADARG;
  const int Tq = a->Tq > 0 ? a->Tq : 0, S = a->S > 0 ? a->S : 0;
  if (Tq % a->row_mul != 0) return KANTTS_E_BADARG;
  if (a->w && a->K > 1 && (!a->hist_in || !a->hist_out || a->hist_in == a->hist_out)) return KANTTS_E_BADARG;
  if (a->B < 2 || a->B > MB_MAXB || a->D < 1 || a->D > MB_MAXD || a->K < 1 || a->K > MB_MAXK || (a->Cin & 3) || a->Cin < 4 ||
      a->Cin > 512 || (!a->w && a->Cin != a->B))
    return KANTTS_E_UNSUPPORTED;
  if (((uintptr_t)a->in & 15) || ((uintptr_t)a->w & 15) || ((uintptr_t)a->hist_in & 15) || ((uintptr_t)a->hist_out & 15) ||
      ((uintptr_t)a->poly & 15) || ((uintptr_t)a->state_in & 15) || ((uintptr_t)a->state_out & 15) || ((uintptr_t)a->out & 15) ||
      (a->hist_ss & 3) || a->hist_ss < 0 || a->state_ss < 0 || Tq > 0x3fffffff)
    return KANTTS_E_UNSUPPORTED;
  if (S == 0 || Tq == 0) return KANTTS_OK;
  if (S > 1 && (a->state_ss < KANTTS_MB_STATE_WORDS(a->D, a->B) ||
                (a->w && a->K > 1 && a->hist_ss < (long long)(a->K - 1) * a->Cin)))
    return KANTTS_E_BADARG;
  kantts_mb_tail_args g = *a;
  g.S = S, g.Tq = Tq;
  hipStream_t st = (hipStream_t)stream;
  switch (g.B) {
    case 2: return mb_launch<2>(g, st);
    case 3: return mb_launch<3>(g, st);
    case 4: return mb_launch<4>(g, st);
    case 5: return mb_launch<5>(g, st);
    case 6: return mb_launch<6>(g, st);
    case 7: return mb_launch<7>(g, st);
    default: return mb_launch<8>(g, st);
  }
}
