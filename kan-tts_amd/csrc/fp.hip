// Filled-pause voices (FP: True, sambert_fp_8k.yaml): the tail of FP_Predictor, the insertion of the "en" / "a" / "e"
// filler rows into the text encoder's output, and FpCELoss.  The reference (kantts_sambert.py:766-860) walks B x T tokens
// in Python, reads one device scalar per token and rebuilds the sequence with a torch.cat per insertion; here the whole
// feature is three launches forward (head, plan, insert) and two backward, with one host read (T', the output width;
// a second plan and read when ties inflate T' past the 4 T columns the host side starts with).
//
// Contract (include/kantts_hip.h has the full text).  Per sequence b, with label[b][p] in {0, 1, 2, 3} for p < T:
//   stream_b = for p = 0, 1, 2, ...: [the 3 rows of F[label[b][p]] if p < T and label[b][p] > 0], text_hid[b, p mod T]
//   out[b]   = the first T' rows of stream_b,     T' = T + max_b(len_b + 3 fp_number_b) - max_b(len_b)
// With E(p) / I(p) the exclusive / inclusive count of labels > 0 in front of / up to p and N = I(T - 1):
//   filler row k of token p at q = p + 3 E(p) + k, token p at q = p + 3 I(p), and q >= T + 3 N holds token (q - 3 N) mod T.
// kantts_fp_plan forms that map once (src, and its inverse pos / nins for the backward); insert_fwd / insert_bwd are
// gathers through it, so no atomics and equal bits on every run.
// kantts_fp_plan_given forms the same map from GIVEN labels at a GIVEN width (teacher forcing, where T' is the width of the
// duration targets): no host read at all, so a training step with it can be captured.
//
// Everything is fp32 with plain vector loads and stores; C % 4 == 0 (one float4 per lane along the channels).
#include "common.h"

#include <limits.h>

#define FP_THREADS 256
#define FP_WAVES (FP_THREADS / KANTTS_WAVE)
#define FP_MAX_C 1024  // C / 4 column lanes of one row fit a workgroup; the head keeps its (4, C) weight in 16 KB of LDS

__device__ __forceinline__ int fp_wave_sum_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ int fp_wave_max_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ int fp_wave_or_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v |= __shfl_xor(v, off, 64);
  return v;
}
// integer block sum (exact, so the order does not matter); red: FP_WAVES ints of LDS; valid in all threads
__device__ __forceinline__ int fp_block_sum_i(int v, int* red) {
  v = fp_wave_sum_i(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int i = 0; i < FP_WAVES; ++i) t += red[i];
  return t;
}

// softmax of four logits; the arithmetic every kernel of this file shares
__device__ __forceinline__ void fp_softmax4(const float z[4], float p[4], float* log_sum, float* zmax) {
  const float m = fmaxf(fmaxf(z[0], z[1]), fmaxf(z[2], z[3]));
  float e[4], s = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    e[k] = expf(z[k] - m);
    s += e[k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) p[k] = e[k] / s;
  if (log_sum) *log_sum = logf(s);
  if (zmax) *zmax = m;
}

// ---------------------------------------------------------------------------------------------------------------------
// Head: fc (C -> 4), softmax and the insertion decision.  One workgroup per sequence, one thread per token.
__global__ __launch_bounds__(FP_THREADS) void fp_head_kernel(const float* __restrict__ rows, const float* __restrict__ w,
                                                             const float* __restrict__ bias, const int* __restrict__ lens,
                                                             const int* __restrict__ fp_label, float* __restrict__ probs,
                                                             int* __restrict__ label, int* __restrict__ fp_number, int T,
                                                             int C) {
  __shared__ __attribute__((aligned(16))) float sw[4 * FP_MAX_C];
  __shared__ int red[FP_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < 4 * C; i += FP_THREADS) sw[i] = w[i];
  __syncthreads();
  const int len = lens[b];
  const int C4 = C >> 2;
  int count = 0;
  for (int j = tid; j < T; j += FP_THREADS) {
    const long long r = (long long)b * T + j;
    const float4* x = reinterpret_cast<const float4*>(rows + r * C);
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < C4; ++c) {
      const float4 v = x[c];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float4 u = *reinterpret_cast<const float4*>(sw + k * C + 4 * c);
        z[k] = fmaf(v.x, u.x, z[k]);
        z[k] = fmaf(v.y, u.y, z[k]);
        z[k] = fmaf(v.z, u.z, z[k]);
        z[k] = fmaf(v.w, u.w, z[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) z[k] += bias[k];
    float p[4];
    fp_softmax4(z, p, nullptr, nullptr);
    *reinterpret_cast<float4*>(probs + r * 4) = make_float4(p[0], p[1], p[2], p[3]);
    int lab = 0;
    if (fp_label) {  // teacher forcing: the labels as given, padded tokens included (reference :793, :846-859)
      lab = fp_label[r];
      count += lab > 0;
    } else if (j < len) {  // (p == max p) for the classes 1..3: ties count severally, the smallest class is inserted
      const float pm = fmaxf(fmaxf(p[0], p[1]), fmaxf(p[2], p[3]));
      const int m1 = p[1] == pm, m2 = p[2] == pm, m3 = p[3] == pm;
      count += m1 + m2 + m3;
      lab = m1 ? 1 : (m2 ? 2 : (m3 ? 3 : 0));
    }
    label[r] = lab;
  }
  count = fp_block_sum_i(count, red);
  if (tid == 0) fp_number[b] = count;
}

// d_z[k] of one row from its probabilities and their cotangent
__device__ __forceinline__ void fp_dz4(const float* __restrict__ probs, const float* __restrict__ d_probs, long long r,
                                       float dz[4]) {
  const float4 p = *reinterpret_cast<const float4*>(probs + r * 4);
  const float4 g = *reinterpret_cast<const float4*>(d_probs + r * 4);
  const float s = p.x * g.x + p.y * g.y + p.z * g.z + p.w * g.w;
  dz[0] = p.x * (g.x - s), dz[1] = p.y * (g.y - s), dz[2] = p.z * (g.z - s), dz[3] = p.w * (g.w - s);
}

// Head backward.  Workgroups [0, nb): d_rows, a thread per (row, float4 of channels).  Workgroups nb + k, k < 4: row k of
// d_weight and d_bias[k]; G = FP_THREADS / (C / 4) row groups walk the rows r = g, g + G, ... in order and are then added
// in the order g = 0, 1, ... -- fixed, no atomics.
__global__ __launch_bounds__(FP_THREADS) void fp_head_bwd_kernel(const float* __restrict__ rows, const float* __restrict__ w,
                                                                 const float* __restrict__ probs,
                                                                 const float* __restrict__ d_probs, float* __restrict__ d_rows,
                                                                 float* __restrict__ d_weight, float* __restrict__ d_bias,
                                                                 long long N, int C, int nb) {
  __shared__ __attribute__((aligned(16))) float red[FP_THREADS * 4];
  __shared__ float redb[FP_THREADS];
  const int C4 = C >> 2, tid = threadIdx.x;
  if ((int)blockIdx.x < nb) {
    const long long i = (long long)blockIdx.x * FP_THREADS + tid;
    if (i >= N * C4) return;
    const long long r = i / C4;
    const int c = (int)(i % C4);
    float dz[4];
    fp_dz4(probs, d_probs, r, dz);
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float4 u = *reinterpret_cast<const float4*>(w + (long long)k * C + 4 * c);
      a.x = fmaf(dz[k], u.x, a.x), a.y = fmaf(dz[k], u.y, a.y), a.z = fmaf(dz[k], u.z, a.z), a.w = fmaf(dz[k], u.w, a.w);
    }
    *reinterpret_cast<float4*>(d_rows + r * C + 4 * c) = a;
    return;
  }
  const int k = (int)blockIdx.x - nb;
  const int G = FP_THREADS / C4, g = tid / C4, c = tid % C4;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  float ab = 0.f;
  if (g < G) {
    for (long long r = g; r < N; r += G) {
      float dz[4];
      fp_dz4(probs, d_probs, r, dz);
      const float4 x = *reinterpret_cast<const float4*>(rows + r * C + 4 * c);
      a.x = fmaf(dz[k], x.x, a.x), a.y = fmaf(dz[k], x.y, a.y), a.z = fmaf(dz[k], x.z, a.z), a.w = fmaf(dz[k], x.w, a.w);
      ab += dz[k];
    }
  }
  *reinterpret_cast<float4*>(red + 4 * tid) = a;
  redb[tid] = ab;
  __syncthreads();
  if (g == 0) {
    for (int i = 1; i < G; ++i) {
      const float4 o = *reinterpret_cast<const float4*>(red + 4 * (i * C4 + c));
      a.x += o.x, a.y += o.y, a.z += o.z, a.w += o.w;
      ab += redb[i * C4 + c];
    }
    *reinterpret_cast<float4*>(d_weight + (long long)k * C + 4 * c) = a;
    if (c == 0) d_bias[k] = ab;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Plan.  One workgroup per sequence.  Every workgroup derives T' from the B lengths and counts (a few hundred bytes), then
// scans its own labels in tiles of FP_THREADS tokens: a 64-lane shuffle scan inside each wave, the wave totals through LDS,
// the tile total carried to the next tile.  Nothing is written at or past min(T', cap).
#define FP_ERR_CAP 1      // cap < T'
#define FP_ERR_LENGTH 2   // a length outside [0, T] or a negative count
#define FP_ERR_LABEL 4    // a label outside [0, 3] (taken as 0)
#define FP_ERR_WIDTH 8    // kantts_fp_plan_given: the T' of the labels is not the width the caller planned at

// The tile scan both plans share: the labels of one row, FP_THREADS tokens at a time, into the map (columns < Tw only) and
// its inverse.  Returns N, the labels > 0 of the row, in every thread.  s_tot: FP_WAVES ints of LDS.
__device__ __forceinline__ int fp_scan_row(const int* __restrict__ lrow, int T, int Tw, int* __restrict__ srow,
                                           int* __restrict__ prow, int* s_tot, int* flags) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int carry = 0;
  for (int base = 0; base < T; base += FP_THREADS) {
    const int p = base + tid;
    int lab = p < T ? lrow[p] : 0;
    if (lab < 0 || lab > 3) *flags |= FP_ERR_LABEL, lab = 0;
    const int f = lab > 0;
    int inc = f;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(inc, d, 64);
      if (lane >= d) inc += v;
    }
    __syncthreads();  // s_tot of the previous tile has been read by everyone
    if (lane == 63) s_tot[wv] = inc;
    __syncthreads();
    int woff = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < FP_WAVES; ++i) {
      woff += i < wv ? s_tot[i] : 0;
      tot += s_tot[i];
    }
    const int incl = carry + woff + inc, excl = incl - f;
    if (p < T) {
      const int q0 = p + 3 * excl, qt = p + 3 * incl;
      if (f) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
          if (q0 + k < Tw) srow[q0 + k] = -(1 + 3 * (lab - 1) + k);
      }
      if (qt < Tw) srow[qt] = p;
      prow[p] = qt;
    }
    carry += tot;
  }
  return carry;
}

// the wrapped tail of the map (columns [T + 3 N, Tw)) and the extended ids of columns [0, Tw); row b of (B, cap) tensors
__device__ __forceinline__ void fp_tail_and_ids(int* __restrict__ srow, const long long* __restrict__ emo,
                                                const long long* __restrict__ spk, long long* __restrict__ emo_out,
                                                long long* __restrict__ spk_out, int b, int T, int N, int Tw, int cap) {
  const int tid = threadIdx.x;
  for (int q = T + 3 * N + tid; q < Tw; q += FP_THREADS) srow[q] = (q - 3 * N) % T;
  for (int q = tid; q < Tw; q += FP_THREADS) {  // the ids are NOT shifted by the insertions (reference :805-828)
    if (emo) emo_out[(long long)b * cap + q] = emo[(long long)b * T + q % T];
    if (spk) spk_out[(long long)b * cap + q] = spk[(long long)b * T + q % T];
  }
}

// OR of the threads' status bits; the result is valid in thread 0.  red: FP_WAVES ints of LDS
__device__ __forceinline__ int fp_block_or_i(int flags, int* red) {
  flags = fp_wave_or_i(flags);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = flags;
  __syncthreads();
  flags = 0;
#pragma unroll
  for (int i = 0; i < FP_WAVES; ++i) flags |= red[i];
  return flags;
}

__global__ __launch_bounds__(FP_THREADS) void fp_plan_kernel(const int* __restrict__ label, const int* __restrict__ lens,
                                                             const int* __restrict__ fp_number,
                                                             const long long* __restrict__ emo,
                                                             const long long* __restrict__ spk, int* __restrict__ inter_len,
                                                             int* __restrict__ meta, int* __restrict__ src,
                                                             int* __restrict__ pos, int* __restrict__ nins,
                                                             long long* __restrict__ emo_out, long long* __restrict__ spk_out,
                                                             int B, int T, int cap) {
  __shared__ int s_a[FP_WAVES], s_b[FP_WAVES], s_c[FP_WAVES], s_tot[FP_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int flags = 0;
  // T' = T + max(len + 3 number) - max(len)
  int mi = 0, ml = 0;
  for (int i = tid; i < B; i += FP_THREADS) {
    int l = lens[i], f = fp_number[i];
    l = min(max(l, 0), T), f = min(max(f, 0), 3 * T);
    mi = max(mi, l + 3 * f), ml = max(ml, l);
  }
  mi = fp_wave_max_i(mi), ml = fp_wave_max_i(ml);
  if (lane == 0) s_a[wv] = mi, s_b[wv] = ml;
  __syncthreads();
  mi = ml = 0;
#pragma unroll
  for (int i = 0; i < FP_WAVES; ++i) mi = max(mi, s_a[i]), ml = max(ml, s_b[i]);
  const int Tp = T + mi - ml;
  const int Tw = min(Tp, cap);  // rows this launch may write
  if (Tp > cap) flags |= FP_ERR_CAP;
  {
    const int l = lens[b], f = fp_number[b];
    if (l < 0 || l > T || f < 0 || f > 3 * T) flags |= FP_ERR_LENGTH;
    if (tid == 0) inter_len[b] = min(max(l, 0), T) + 3 * min(max(f, 0), 3 * T);
  }
  int* srow = src + (long long)b * cap;
  const int N = fp_scan_row(label + (long long)b * T, T, Tw, srow, pos + (long long)b * T, s_tot, &flags);
  fp_tail_and_ids(srow, emo, spk, emo_out, spk_out, b, T, N, Tw, cap);
  flags = fp_block_or_i(flags, s_c);
  if (tid == 0) {
    nins[b] = N;
    meta[1 + b] = flags;
    if (b == 0) meta[0] = Tp;
  }
}

// Plan from GIVEN labels at a GIVEN width W (teacher forcing: nothing of the insertion depends on the network, and the
// caller knows T' = the width of its duration targets on the host).  Same map as above, but all of columns [0, W) of the
// stream is written whatever T' is, nothing behind them, and the counts come from the labels: every workgroup counts the
// labels > 0 of all B rows (a wave per row; B T ints), so T' needs no second launch.  T' != W sets FP_ERR_WIDTH.
__global__ __launch_bounds__(FP_THREADS) void fp_plan_given_kernel(const int* __restrict__ label, const int* __restrict__ lens,
                                                                   const long long* __restrict__ emo,
                                                                   const long long* __restrict__ spk,
                                                                   int* __restrict__ inter_len, int* __restrict__ meta,
                                                                   int* __restrict__ src, int* __restrict__ pos,
                                                                   int* __restrict__ nins, long long* __restrict__ emo_out,
                                                                   long long* __restrict__ spk_out, int* __restrict__ fp_number,
                                                                   int B, int T, int W) {
  __shared__ int s_a[FP_WAVES], s_b[FP_WAVES], s_c[FP_WAVES], s_tot[FP_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int flags = 0;
  int mi = 0, ml = 0;
  for (int i = wv; i < B; i += FP_WAVES) {
    int c = 0;
    for (int p = lane; p < T; p += 64) {
      const int lab = label[(long long)i * T + p];
      c += lab >= 1 && lab <= 3;
    }
    c = fp_wave_sum_i(c);
    const int l = min(max(lens[i], 0), T);
    mi = max(mi, l + 3 * c), ml = max(ml, l);
  }
  if (lane == 0) s_a[wv] = mi, s_b[wv] = ml;
  __syncthreads();
  mi = ml = 0;
#pragma unroll
  for (int i = 0; i < FP_WAVES; ++i) mi = max(mi, s_a[i]), ml = max(ml, s_b[i]);
  const int Tp = T + mi - ml;
  if (Tp != W) flags |= FP_ERR_WIDTH;
  const int l = lens[b];
  if (l < 0 || l > T) flags |= FP_ERR_LENGTH;
  int* srow = src + (long long)b * W;
  const int N = fp_scan_row(label + (long long)b * T, T, W, srow, pos + (long long)b * T, s_tot, &flags);
  fp_tail_and_ids(srow, emo, spk, emo_out, spk_out, b, T, N, W, W);
  flags = fp_block_or_i(flags, s_c);
  if (tid == 0) {
    nins[b] = N;
    fp_number[b] = N;
    inter_len[b] = min(max(l, 0), T) + 3 * N;
    meta[1 + b] = flags;
    if (b == 0) meta[0] = Tp;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Insert forward: out[b, q, :] = src >= 0 ? text_hid[b, src] : F[-src - 1]; a float4 per lane.  A map entry outside
// [-9, T) (a map this library did not write) gives a zero row instead of a stray load.
__global__ __launch_bounds__(FP_THREADS) void fp_insert_fwd_kernel(const float* __restrict__ text_hid,
                                                                   const float* __restrict__ fill, const int* __restrict__ src,
                                                                   float* __restrict__ out, long long total, int T, int Tp,
                                                                   int cap, int C4) {
  const long long i = (long long)blockIdx.x * FP_THREADS + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C4);
  const long long row = i / C4;
  const int q = (int)(row % Tp);
  const long long b = row / Tp;
  const int s = src[b * cap + q];
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (s >= 0 && s < T)
    v = reinterpret_cast<const float4*>(text_hid)[(b * T + s) * C4 + c];
  else if (s < 0 && s >= -9)
    v = reinterpret_cast<const float4*>(fill)[(long long)(-s - 1) * C4 + c];
  reinterpret_cast<float4*>(out)[row * C4 + c] = v;
}

// Insert backward, the gather form.  Workgroups [0, nb): d_text_hid[b, j] = d_out[b, pos[b, j]] (if that place is inside
// T') + d_out[b, j + 3 N + m T], m = 1, 2, ... (the wrapped copies), in ascending place.  Workgroups nb + r, r < 9: filler
// row r; G row groups walk the B T' places i = g, g + G, ... in order, take those whose map entry is -(r + 1), and are then
// added in the order g = 0, 1, ...
__global__ __launch_bounds__(FP_THREADS) void fp_insert_bwd_kernel(const float* __restrict__ d_out, const int* __restrict__ src,
                                                                   const int* __restrict__ pos, const int* __restrict__ nins,
                                                                   float* __restrict__ d_text, float* __restrict__ d_fill,
                                                                   int B, int T, int Tp, int cap, int C4, int nb) {
  __shared__ __attribute__((aligned(16))) float red[FP_THREADS * 4];
  const int tid = threadIdx.x;
  const float4* g4 = reinterpret_cast<const float4*>(d_out);
  if ((int)blockIdx.x < nb) {
    const long long i = (long long)blockIdx.x * FP_THREADS + tid;
    if (i >= (long long)B * T * C4) return;
    const int c = (int)(i % C4);
    const long long row = i / C4;
    const int j = (int)(row % T);
    const long long b = row / T;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    const int q0 = pos[row];
    if (q0 >= 0 && q0 < Tp) a = g4[(b * Tp + q0) * C4 + c];
    const int N = min(max(nins[b], 0), T);
    for (long long q = (long long)j + 3 * N + T; q < Tp; q += T) {
      const float4 o = g4[(b * Tp + q) * C4 + c];
      a.x += o.x, a.y += o.y, a.z += o.z, a.w += o.w;
    }
    reinterpret_cast<float4*>(d_text)[row * C4 + c] = a;
    return;
  }
  const int want = -((int)blockIdx.x - nb + 1);
  const int G = FP_THREADS / C4, g = tid / C4, c = tid % C4;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  if (g < G) {
    const long long n = (long long)B * Tp;
    for (long long i = g; i < n; i += G) {
      const long long b = i / Tp;
      const int q = (int)(i % Tp);
      if (src[b * cap + q] == want) {
        const float4 o = g4[i * C4 + c];
        a.x += o.x, a.y += o.y, a.z += o.z, a.w += o.w;
      }
    }
  }
  *reinterpret_cast<float4*>(red + 4 * tid) = a;
  __syncthreads();
  if (g == 0) {
    for (int i = 1; i < G; ++i) {
      const float4 o = *reinterpret_cast<const float4*>(red + 4 * (i * C4 + c));
      a.x += o.x, a.y += o.y, a.z += o.z, a.w += o.w;
    }
    reinterpret_cast<float4*>(d_fill)[(long long)((int)blockIdx.x - nb) * C4 + c] = a;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// FpCELoss: CrossEntropyLoss(weight, reduction none) on the PROBABILITIES taken as logits (a second softmax), masked to
// j < len_b, summed, divided by the unweighted number of valid tokens; and its gradient with respect to the probabilities.
// One workgroup: a thread adds its tokens i = tid, tid + 256, ... in order, then the fixed tree of kantts_block_sum.
// A label outside [0, 3] on a valid token makes the loss NaN (the reference raises).
__global__ __launch_bounds__(FP_THREADS) void fp_ce_kernel(const float* __restrict__ probs, const int* __restrict__ label,
                                                           const int* __restrict__ lens, const float* __restrict__ weight,
                                                           float* __restrict__ loss, float* __restrict__ d_probs, int B,
                                                           int T) {
  __shared__ int redi[FP_WAVES];
  __shared__ float redf[FP_WAVES];
  const int tid = threadIdx.x;
  int cnt = 0;
  for (int i = tid; i < B; i += FP_THREADS) cnt += min(max(lens[i], 0), T);
  cnt = fp_block_sum_i(cnt, redi);
  const float inv = 1.f / (float)cnt;  // no valid token: 0 / 0 below, as in the reference
  const float wk[4] = {weight[0], weight[1], weight[2], weight[3]};
  float acc = 0.f;
  const long long n = (long long)B * T;
  for (long long i = tid; i < n; i += FP_THREADS) {
    const int b = (int)(i / T), j = (int)(i % T);
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < lens[b]) {
      const float4 p = *reinterpret_cast<const float4*>(probs + i * 4);
      const float z[4] = {p.x, p.y, p.z, p.w};
      float sm[4], ls, zm;
      fp_softmax4(z, sm, &ls, &zm);
      const int y = label[i];
      if (y >= 0 && y <= 3) {
        const float wy = wk[y];
        acc += wy * (ls - (z[y] - zm));
        const float s = wy * inv;
        g = make_float4(s * (sm[0] - (y == 0)), s * (sm[1] - (y == 1)), s * (sm[2] - (y == 2)), s * (sm[3] - (y == 3)));
      } else {
        acc += __int_as_float(0x7fc00000);
      }
    }
    if (d_probs) *reinterpret_cast<float4*>(d_probs + i * 4) = g;
  }
  acc = kantts_block_sum(acc, redf);
  if (tid == 0) loss[0] = cnt > 0 ? acc * inv : __int_as_float(0x7fc00000);
}

// ---------------------------------------------------------------------------------------------------------------------
static inline bool fp_al16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

extern "C" int kantts_fp_head(const float* rows, const float* weight, const float* bias, const int32_t* lens,
                              const int32_t* fp_label, float* probs, int32_t* label, int32_t* fp_number, int B, int T, int C,
                              void* stream) {
  if (!rows || !weight || !bias || !lens || !probs || !label || !fp_number || B < 0 || T < 0 || C < 1) return KANTTS_E_BADARG;
  if (C % 4 || C > FP_MAX_C || B > 65535 || !fp_al16(rows) || !fp_al16(weight) || !fp_al16(probs)) return KANTTS_E_UNSUPPORTED;
  if (B == 0) return KANTTS_OK;
  hipLaunchKernelGGL(fp_head_kernel, dim3(B), dim3(FP_THREADS), 0, (hipStream_t)stream, rows, weight, bias,
                     reinterpret_cast<const int*>(lens), reinterpret_cast<const int*>(fp_label), probs,
                     reinterpret_cast<int*>(label), reinterpret_cast<int*>(fp_number), T, C);
  KANTTS_CHECK_LAUNCH();
}

extern "C" int kantts_fp_head_bwd(const float* rows, const float* weight, const float* probs, const float* d_probs,
                                  float* d_rows, float* d_weight, float* d_bias, long long N, int C, void* stream) {
  if (!rows || !weight || !probs || !d_probs || !d_rows || !d_weight || !d_bias || N < 0 || C < 1) return KANTTS_E_BADARG;
  if (C % 4 || C > FP_MAX_C || !fp_al16(rows) || !fp_al16(weight) || !fp_al16(probs) || !fp_al16(d_probs) || !fp_al16(d_rows) ||
      !fp_al16(d_weight))
    return KANTTS_E_UNSUPPORTED;
  const long long nbl = (N * (C / 4) + FP_THREADS - 1) / FP_THREADS;
  if (nbl > 0x7fffff00ll) return KANTTS_E_UNSUPPORTED;
  const int nb = (int)nbl;
  hipLaunchKernelGGL(fp_head_bwd_kernel, dim3(nb + 4), dim3(FP_THREADS), 0, (hipStream_t)stream, rows, weight, probs, d_probs,
                     d_rows, d_weight, d_bias, N, C, nb);
  KANTTS_CHECK_LAUNCH();
}

extern "C" int kantts_fp_plan(const int32_t* label, const int32_t* lens, const int32_t* fp_number, const int64_t* emo,
                              const int64_t* spk, int32_t* inter_len, int32_t* meta, int32_t* src, int32_t* pos,
                              int32_t* nins, int64_t* emo_out, int64_t* spk_out, int B, int T, int cap, void* stream) {
  if (!label || !lens || !fp_number || !inter_len || !meta || !src || !pos || !nins || B < 1 || T < 1 || cap < 1 ||
      (emo && !emo_out) || (spk && !spk_out))
    return KANTTS_E_BADARG;
  if (B > 65535 || T > (1 << 24)) return KANTTS_E_UNSUPPORTED;
  hipLaunchKernelGGL(fp_plan_kernel, dim3(B), dim3(FP_THREADS), 0, (hipStream_t)stream, reinterpret_cast<const int*>(label),
                     reinterpret_cast<const int*>(lens), reinterpret_cast<const int*>(fp_number),
                     reinterpret_cast<const long long*>(emo), reinterpret_cast<const long long*>(spk),
                     reinterpret_cast<int*>(inter_len), reinterpret_cast<int*>(meta), reinterpret_cast<int*>(src),
                     reinterpret_cast<int*>(pos), reinterpret_cast<int*>(nins), reinterpret_cast<long long*>(emo_out),
                     reinterpret_cast<long long*>(spk_out), B, T, cap);
  KANTTS_CHECK_LAUNCH();
}

extern "C" int kantts_fp_plan_given(const int32_t* label, const int32_t* lens, const int64_t* emo, const int64_t* spk,
                                    int32_t* inter_len, int32_t* meta, int32_t* src, int32_t* pos, int32_t* nins,
                                    int64_t* emo_out, int64_t* spk_out, int32_t* fp_number, int B, int T, int W, void* stream) {
  if (!label || !lens || !inter_len || !meta || !src || !pos || !nins || !fp_number || B < 1 || T < 1 || W < 1 ||
      (emo && !emo_out) || (spk && !spk_out))
    return KANTTS_E_BADARG;
  if (B > 65535 || T > (1 << 24) || W > (1 << 26)) return KANTTS_E_UNSUPPORTED;
  hipLaunchKernelGGL(fp_plan_given_kernel, dim3(B), dim3(FP_THREADS), 0, (hipStream_t)stream,
                     reinterpret_cast<const int*>(label), reinterpret_cast<const int*>(lens),
                     reinterpret_cast<const long long*>(emo), reinterpret_cast<const long long*>(spk),
                     reinterpret_cast<int*>(inter_len), reinterpret_cast<int*>(meta), reinterpret_cast<int*>(src),
                     reinterpret_cast<int*>(pos), reinterpret_cast<int*>(nins), reinterpret_cast<long long*>(emo_out),
                     reinterpret_cast<long long*>(spk_out), reinterpret_cast<int*>(fp_number), B, T, W);
  KANTTS_CHECK_LAUNCH();
}

extern "C" int kantts_fp_insert_fwd(const float* text_hid, const float* fill, const int32_t* src, float* out, int B, int T,
                                    int Tp, int cap, int C, void* stream) {
  if (!text_hid || !fill || !src || !out || B < 0 || T < 1 || Tp < 0 || C < 1) return KANTTS_E_BADARG;
  if (Tp > cap) return KANTTS_E_BADARG;  // the map has no entry for such a row
  if (C % 4 || !fp_al16(text_hid) || !fp_al16(fill) || !fp_al16(out)) return KANTTS_E_UNSUPPORTED;
  const long long total = (long long)B * Tp * (C / 4);
  if (total == 0) return KANTTS_OK;
  const long long nb = (total + FP_THREADS - 1) / FP_THREADS;
  if (nb > 0x7fffffffll) return KANTTS_E_UNSUPPORTED;
  hipLaunchKernelGGL(fp_insert_fwd_kernel, dim3((unsigned)nb), dim3(FP_THREADS), 0, (hipStream_t)stream, text_hid, fill,
                     reinterpret_cast<const int*>(src), out, total, T, Tp, cap, C / 4);
  KANTTS_CHECK_LAUNCH();
}

extern "C" int kantts_fp_insert_bwd(const float* d_out, const int32_t* src, const int32_t* pos, const int32_t* nins,
                                    float* d_text_hid, float* d_fill, int B, int T, int Tp, int cap, int C, void* stream) {
  if (!d_out || !src || !pos || !nins || !d_text_hid || !d_fill || B < 1 || T < 1 || Tp < 1 || C < 1) return KANTTS_E_BADARG;
  if (Tp > cap) return KANTTS_E_BADARG;
  if (C % 4 || C > FP_MAX_C || !fp_al16(d_out) || !fp_al16(d_text_hid) || !fp_al16(d_fill)) return KANTTS_E_UNSUPPORTED;
  const long long nbl = ((long long)B * T * (C / 4) + FP_THREADS - 1) / FP_THREADS;
  if (nbl > 0x7fffff00ll) return KANTTS_E_UNSUPPORTED;
  const int nb = (int)nbl;
  hipLaunchKernelGGL(fp_insert_bwd_kernel, dim3(nb + 9), dim3(FP_THREADS), 0, (hipStream_t)stream, d_out,
                     reinterpret_cast<const int*>(src), reinterpret_cast<const int*>(pos), reinterpret_cast<const int*>(nins),
                     d_text_hid, d_fill, B, T, Tp, cap, C / 4, nb);
  KANTTS_CHECK_LAUNCH();
}

extern "C" int kantts_fp_ce(const float* probs, const int32_t* label, const int32_t* lens, const float* weight, float* loss,
                            float* d_probs, int B, int T, void* stream) {
  if (!probs || !label || !lens || !weight || !loss || B < 1 || T < 1) return KANTTS_E_BADARG;
  if (!fp_al16(probs) || (d_probs && !fp_al16(d_probs))) return KANTTS_E_UNSUPPORTED;
  hipLaunchKernelGGL(fp_ce_kernel, dim3(1), dim3(FP_THREADS), 0, (hipStream_t)stream, probs,
                     reinterpret_cast<const int*>(label), reinterpret_cast<const int*>(lens), weight, loss, d_probs, B, T);
  KANTTS_CHECK_LAUNCH();
}
