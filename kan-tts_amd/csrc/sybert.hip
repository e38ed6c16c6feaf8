// sy-BERT pre-training: the BERT masking of a padded batch and the masked-LM head (include/kantts_hip.h has the contracts).
//
// kantts_bert_mask_rows -- the device twin of kantts.datasets.bert_masking.draw.  ONE workgroup of 16 waves, a wave per
//   sequence: {seed, counter} is read by every thread, a barrier, thread 0 stores counter + 1 (as nsf_draw_kernel does; a
//   workgroup per sequence could not: one that starts late would read the advanced counter).  A wave walks its sequence 64
//   positions at a time.  Pass 1 counts the masked positions (a ballot per 64).  Pass 2, for each block of 64 positions of
//   its own: every lane ranks its position against all masked positions, which come by 64 as well -- their rank keys go
//   through a 512-byte cell row of the wave in LDS and are read back as broadcasts, only the set bits of the ballot.  The
//   hashes are recomputed, never stored: (T / 64)^2 * 2 hashes per lane, 8 at the shipped lengths (T <= 128).
//
// kantts_mlm_head_fwd / _bwd -- logits = hid W^T + bias 16 rows at a time on v_mfma_f32_16x16x4_f32 (an exact fp32 fmaf
//   chain), never stored.  Operands go from global memory straight to registers: a lane loads ONE float4 of its row per 16
//   channels (lane (li, kg): row li, channels 16 q + 4 kg ... + 3) and the 4 MFMAs of that step take element e of both
//   float4s, i.e. MFMA e contracts channels {16 q + 4 kg + e : kg}, the same set for both operands.  A wave holds two logit
//   tiles (32 symbols) at a time: two independent accumulator chains, one load of the rows.
//     forward   : workgroup = 16 rows, its 4 waves share the symbol tiles; per (lane, row) an online softmax state (max,
//                 sum, arg-max, target logit), merged over the 16 lanes of a row by xor-shuffles and over the waves through
//                 LDS in wave order; three partial sums per workgroup, a one-workgroup launch adds them in a fixed order.
//     backward 1: the same walk; dlogits to the zero-padded workspace.
//     backward 2: d_W tiles (contraction over rows, 8 waves on interleaved row blocks, added in wave order; d_bias beside
//                 the first channel tile) and d_hid row blocks (contraction over symbols), one launch, the role by blockIdx.
#include "common.h"

#define SYB_TAG 0x53594245ull
#define SYB_MASK_THREADS 1024
#define SYB_MASK_WAVES (SYB_MASK_THREADS / 64)
#define SYB_MAX_T 4096
#define SYB_MAX_B (1 << 20)

__global__ __launch_bounds__(SYB_MASK_THREADS) void bert_mask_kernel(uint64_t* words, const int64_t* targets,
                                                                     long long tgt_ts, const int32_t* lens, int64_t* lings,
                                                                     long long ling_ts, float* masks, int64_t* targets_out,
                                                                     int B, int T, int thr, int mask_id, int nsym) {
  __shared__ uint64_t s_key[SYB_MASK_WAVES][64];
  const uint64_t seed = words[0], counter = words[1];
  __syncthreads();  // every thread holds both words before the counter moves
  if (threadIdx.x == 0) words[1] = counter + 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t base = kantts_rng_mix(seed, SYB_TAG);
  for (int b = wave; b < B; b += SYB_MASK_WAVES) {  // (wave-uniform)
    const uint64_t key = kantts_rng_mix(base, (counter << 20) | (uint64_t)b);
    const int L = min(max(lens[b], 0), T);
    const int E = max(L - 1, 0);          // eligible positions [0, E)
    const int nblk = (E + 63) >> 6;       // blocks of 64 that hold one
    int n = 0;
    for (int c = 0; c < nblk; ++c) {
      const int i = c * 64 + lane;
      n += __popcll(__ballot(i < E && (int)(kantts_rng_mix(key, (uint64_t)i) >> 40) < thr));
    }
    const int n2 = (int)((4ll * n) / 5), n3 = n / 10;
    const int64_t rnd = (int64_t)(((kantts_rng_mix(key, 1ull << 33) >> 32) * (uint64_t)nsym) >> 32);
    for (int cj = 0; cj < (T + 63) >> 6; ++cj) {
      const int j = cj * 64 + lane;
      const bool mine = j < E && (int)(kantts_rng_mix(key, (uint64_t)j) >> 40) < thr;
      const uint64_t kj = kantts_rng_mix(key, (1ull << 32) + (uint64_t)j);
      int rank = 0;
      if (cj < nblk) {  // (wave-uniform) a block past the eligible positions holds no masked one: nothing to rank
        for (int ci = 0; ci < nblk; ++ci) {
          const int i = ci * 64 + lane;
          const bool m = i < E && (int)(kantts_rng_mix(key, (uint64_t)i) >> 40) < thr;
          unsigned long long bits = __ballot(m);  // also: every lane is done with the cells of the block before
          s_key[wave][lane] = kantts_rng_mix(key, (1ull << 32) + (uint64_t)i);
          KANTTS_WAVE_ORDERED();
          while (bits) {
            const int k = __ffsll(bits) - 1;
            bits &= bits - 1;
            const uint64_t ki = s_key[wave][k];
            rank += (ki < kj || (ki == kj && ci * 64 + k < j)) ? 1 : 0;
          }
        }
      }
      if (j < T) {
        const int64_t t = targets[((long long)b * T + j) * tgt_ts];  // (may be the cell of lings written below)
        const int64_t id = !mine ? t : (rank < n2 ? (int64_t)mask_id : (rank < n2 + n3 ? rnd : t));
        lings[((long long)b * T + j) * ling_ts] = id;
        masks[(long long)b * T + j] = mine ? 1.f : 0.f;
        if (targets_out) targets_out[(long long)b * T + j] = t;
      }
    }
  }
}

extern "C" int kantts_bert_mask_rows(uint64_t* seed_counter, const int64_t* targets, long long tgt_ts, const int32_t* lens,
                                     int64_t* input_lings, long long ling_ts, float* bert_masks, int64_t* targets_out, int B,
                                     int T, int thr, int mask_id, int nsym, void* stream) {
  if (!seed_counter || !targets || !lens || !input_lings || !bert_masks) return KANTTS_E_BADARG;
  if (((uintptr_t)seed_counter & 7) || ((uintptr_t)targets & 7) || ((uintptr_t)input_lings & 7)) return KANTTS_E_BADARG;
  if (((uintptr_t)lens & 3) || ((uintptr_t)bert_masks & 3) || ((uintptr_t)targets_out & 7)) return KANTTS_E_BADARG;
  if (B < 1 || T < 1 || ling_ts < 1 || tgt_ts < 1 || thr < 0 || thr > (1 << 24)) return KANTTS_E_BADARG;
  if (T > SYB_MAX_T || B >= SYB_MAX_B || nsym < 1) return KANTTS_E_UNSUPPORTED;
  hipLaunchKernelGGL(bert_mask_kernel, dim3(1), dim3(SYB_MASK_THREADS), 0, (hipStream_t)stream, seed_counter, targets, tgt_ts,
                     lens, input_lings, ling_ts, bert_masks, targets_out, B, T, thr, mask_id, nsym);
  KANTTS_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------
#define MLM_ROWS 16
#define MLM_FWD_THREADS 256
#define MLM_FWD_WAVES (MLM_FWD_THREADS / 64)
#define MLM_BWD_THREADS 512
#define MLM_BWD_WAVES (MLM_BWD_THREADS / 64)

// acc0 / acc1 += rows [r0, r0 + 16) of hid times symbols [v0, v0 + 16) / [v0 + 16, v0 + 32) of W, transposed: lane
// (li, kg) gets logits[r0 + 4 kg + e][v0 (+ 16) + li] in element e.  Rows past M and symbols past V are read from the last
// valid row (their results are never used).
__device__ __forceinline__ void mlm_logit_tiles(const float* hid, const float* W, int M, int C, int V, int r0, int v0,
                                                f32x4& acc0, f32x4& acc1) {
  const int lane = threadIdx.x & 63, li = lane & 15, kg = lane >> 4;
  const float* pa = hid + (long long)min(r0 + li, M - 1) * C + 4 * kg;
  const float* pb0 = W + (long long)min(v0 + li, V - 1) * C + 4 * kg;
  const float* pb1 = W + (long long)min(v0 + 16 + li, V - 1) * C + 4 * kg;
  for (int k = 0; k < C; k += 16) {
    const float4 a = *reinterpret_cast<const float4*>(pa + k);
    const float4 b0 = *reinterpret_cast<const float4*>(pb0 + k);
    const float4 b1 = *reinterpret_cast<const float4*>(pb1 + k);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b0.x, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b1.x, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b0.y, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b1.y, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b0.z, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b1.z, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b0.w, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b1.w, acc1, 0, 0, 0);
  }
}

struct mlm_row_state {
  float m, s, tl;  // maximum, sum of exp(x - m), the target's logit (0 while unseen)
  int am, hit;     // arg-max (lowest index among equal maxima), 1 once the target's logit was seen
};

__device__ __forceinline__ void mlm_merge(mlm_row_state& a, const mlm_row_state& b) {
  const float mx = fmaxf(a.m, b.m);
  const float sa = a.m == -INFINITY ? 0.f : a.s * expf(a.m - mx), sb = b.m == -INFINITY ? 0.f : b.s * expf(b.m - mx);
  if (b.m > a.m || (b.m == a.m && b.am < a.am)) a.am = b.am;
  a.s = (a.s != a.s || b.s != b.s) ? NAN : sa + sb;  // a NaN logit: the row's sum is NaN whatever the maxima are
  a.m = mx;
  a.tl += b.tl;
  a.hit |= b.hit;
}

__global__ __launch_bounds__(MLM_FWD_THREADS) void mlm_fwd_kernel(const float* hid, const float* W, const float* bias,
                                                                  const int64_t* targets, const float* mask, float* lse,
                                                                  float* part, int M, int C, int V) {
  __shared__ mlm_row_state s_st[MLM_FWD_WAVES][MLM_ROWS];
  __shared__ float s_sum[3][MLM_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kg = lane >> 4;
  const int r0 = blockIdx.x * MLM_ROWS;
  mlm_row_state st[4];
  long long tg[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    st[e].m = -INFINITY, st[e].s = 0.f, st[e].tl = 0.f, st[e].am = 0x7fffffff, st[e].hit = 0;
    tg[e] = targets[min(r0 + 4 * kg + e, M - 1)];
  }
  for (int v0 = wave * 32; v0 < V; v0 += MLM_FWD_WAVES * 32) {  // (wave-uniform)
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    mlm_logit_tiles(hid, W, M, C, V, r0, v0, acc[0], acc[1]);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int v = v0 + 16 * h + li;
      if (v < V) {
        const float bv = bias ? bias[v] : 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float x = acc[h][e] + bv;
          if (x > st[e].m) {
            st[e].s = (st[e].m == -INFINITY ? 0.f : st[e].s * expf(st[e].m - x)) + 1.f;
            st[e].m = x, st[e].am = v;
          } else {
            st[e].s += x == -INFINITY ? 0.f : expf(x - st[e].m);  // (x NaN: the sum becomes NaN)
          }
          if ((long long)v == tg[e]) st[e].tl = x, st[e].hit = 1;
        }
      }
    }
  }
  // over the 16 lanes (symbols) of a row: every lane computes the same merge in the same order
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      mlm_row_state o;
      o.m = __shfl_xor(st[e].m, off, 64), o.s = __shfl_xor(st[e].s, off, 64), o.tl = __shfl_xor(st[e].tl, off, 64);
      o.am = __shfl_xor(st[e].am, off, 64), o.hit = __shfl_xor(st[e].hit, off, 64);
      if (li & off) {  // the lower lane's state first, in both partners: the same bits on both sides
        mlm_row_state t = o;
        mlm_merge(t, st[e]);
        st[e] = t;
      } else {
        mlm_merge(st[e], o);
      }
    }
  }
  if (li == 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) s_st[wave][4 * kg + e] = st[e];
  }
  __syncthreads();
  if (tid < MLM_ROWS) {
    mlm_row_state t = s_st[0][tid];
    for (int w = 1; w < MLM_FWD_WAVES; ++w) mlm_merge(t, s_st[w][tid]);
    const int r = r0 + tid;
    float lo = 0.f, er = 0.f, ms = 0.f;
    if (r < M) {
      const float l = t.m + logf(t.s);
      lse[r] = l;
      const float mk = mask[r];
      if (mk != 0.f) {
        lo = t.hit ? mk * (l - t.tl) : NAN;
        er = (long long)t.am != targets[r] ? mk : 0.f;
        ms = mk;
      }
    }
    s_sum[0][tid] = lo, s_sum[1][tid] = er, s_sum[2][tid] = ms;
  }
  __syncthreads();
  if (tid < 3) {
    float a = 0.f;
    for (int i = 0; i < MLM_ROWS; ++i) a += s_sum[tid][i];
    part[(long long)blockIdx.x * 3 + tid] = a;
  }
}

// out[0] = sum loss / sum mask, out[1] = sum err / sum mask, out[2] = sum mask: thread t adds partials t, t + 256, ... in
// this order, then a fixed binary tree over the 256 threads
__global__ __launch_bounds__(256) void mlm_fwd_sum_kernel(const float* part, int parts, float* out) {
  __shared__ float s_acc[3][256];
  const int tid = threadIdx.x;
  float a[3] = {0.f, 0.f, 0.f};
  for (int i = tid; i < parts; i += 256)
    for (int c = 0; c < 3; ++c) a[c] += part[(long long)i * 3 + c];
  for (int c = 0; c < 3; ++c) s_acc[c][tid] = a[c];
  for (int half = 128; half > 0; half >>= 1) {
    __syncthreads();
    if (tid < half)
      for (int c = 0; c < 3; ++c) s_acc[c][tid] += s_acc[c][tid + half];
  }
  __syncthreads();
  if (tid == 0) {
    const float ms = s_acc[2][0];
    out[0] = s_acc[0][0] / ms, out[1] = s_acc[1][0] / ms, out[2] = ms;
  }
}

static int mlm_check(const void* hid, const void* W, int M, int C, int V) {
  if (!hid || !W || M < 1) return KANTTS_E_BADARG;
  if (((uintptr_t)hid & 15) || ((uintptr_t)W & 15)) return KANTTS_E_BADARG;
  if (C < 16 || C > 512 || (C & 15) || V < 1 || V > 4096 || M > (1 << 24)) return KANTTS_E_UNSUPPORTED;
  return KANTTS_OK;
}

extern "C" int kantts_mlm_head_fwd(const float* hid, const float* W, const float* bias, const int64_t* targets,
                                   const float* mask, float* out, float* lse, float* ws, long long ws_floats, int M, int C,
                                   int V, void* stream) {
  if (!targets || !mask || !out || !lse || !ws) return KANTTS_E_BADARG;
  const int rc = mlm_check(hid, W, M, C, V);
  if (rc != KANTTS_OK) return rc;
  const int parts = kantts_cdiv(M, MLM_ROWS);
  if (ws_floats < 3ll * parts) return KANTTS_E_WORKSPACE;
  hipLaunchKernelGGL(mlm_fwd_kernel, dim3(parts), dim3(MLM_FWD_THREADS), 0, (hipStream_t)stream, hid, W, bias, targets, mask,
                     lse, ws, M, C, V);
  hipLaunchKernelGGL(mlm_fwd_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)ws, parts, out);
  KANTTS_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------
// backward 1: dlog (Mp, Vp), every cell written
__global__ __launch_bounds__(MLM_FWD_THREADS) void mlm_dlogits_kernel(const float* hid, const float* W, const float* bias,
                                                                      const int64_t* targets, const float* mask,
                                                                      const float* lse, const float* out, const float* dloss,
                                                                      float gscale, float* dlog, int M, int C, int V, int Vp) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kg = lane >> 4;
  const int r0 = blockIdx.x * MLM_ROWS;
  const float msum = out[2], up = gscale * dloss[0];
  float g[4], ls[4];
  long long tg[4];
  bool live[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int r = r0 + 4 * kg + e, rr = min(r, M - 1);
    const float mk = mask[rr];
    tg[e] = targets[rr], ls[e] = lse[rr];
    live[e] = r < M && (mk != 0.f || !(msum != 0.f));  // no masked row at all: NaN everywhere, the reference's 0 / 0
    g[e] = (tg[e] < 0 || tg[e] >= V) ? NAN : up * mk / msum;
  }
  for (int v0 = wave * 32; v0 < Vp; v0 += MLM_FWD_WAVES * 32) {  // (wave-uniform)
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    if (v0 < V) mlm_logit_tiles(hid, W, M, C, V, r0, v0, acc[0], acc[1]);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int v = v0 + 16 * h + li;
      if (v < Vp) {
        const float bv = (bias && v < V) ? bias[v] : 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float p = expf(acc[h][e] + bv - ls[e]);
          const float d = g[e] * (p - ((long long)v == tg[e] ? 1.f : 0.f));
          dlog[(long long)(r0 + 4 * kg + e) * Vp + v] = (live[e] && v < V) ? d : 0.f;
        }
      }
    }
  }
}

// backward 2.  blockIdx < wtiles: the 16 x 16 tile (vt, ct) of d_W, and d_bias[16 vt ...] where ct == 0; else 16 rows of d_hid.
__global__ __launch_bounds__(MLM_BWD_THREADS) void mlm_grads_kernel(const float* hid, const float* W, const float* dlog,
                                                                    float* d_hid, float* d_W, float* d_bias, int M, int C,
                                                                    int V, int Vp, int wtiles) {
  __shared__ float s_tile[MLM_BWD_WAVES][256];
  __shared__ float s_bias[MLM_BWD_WAVES][16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kg = lane >> 4;
  const int ctiles = C >> 4;
  if ((int)blockIdx.x < wtiles) {
    const int vt = blockIdx.x / ctiles, ct = blockIdx.x - vt * ctiles;
    const int rblocks = (M + 15) >> 4;
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    float bsum = 0.f;
    // A[v][k = row] = dlog[row][16 vt + v], B[c][k = row] = hid[row][16 ct + c]; MFMA e of a block contracts rows 4 kg + e
    for (int rb = wave; rb < rblocks; rb += 2 * MLM_BWD_WAVES) {  // (wave-uniform) two row blocks, two chains
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int rbh = rb + h * MLM_BWD_WAVES;
        if (rbh < rblocks) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = rbh * 16 + 4 * kg + e;
            const float a = dlog[(long long)r * Vp + vt * 16 + li];
            const float b = r < M ? hid[(long long)r * C + ct * 16 + li] : 0.f;
            bsum += a;
            acc[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[h], 0, 0, 0);
          }
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) s_tile[wave][(4 * kg + e) * 16 + li] = acc[0][e] + acc[1][e];
    bsum += __shfl_xor(bsum, 16, 64);
    bsum += __shfl_xor(bsum, 32, 64);
    if (kg == 0) s_bias[wave][li] = bsum;
    __syncthreads();
    if (tid < 256) {
      float a = s_tile[0][tid];
      for (int w = 1; w < MLM_BWD_WAVES; ++w) a += s_tile[w][tid];
      const int v = vt * 16 + (tid >> 4);
      if (v < V) d_W[(long long)v * C + ct * 16 + (tid & 15)] = a;
    } else if (tid < 272 && ct == 0 && d_bias) {
      const int i = tid - 256;
      float a = s_bias[0][i];
      for (int w = 1; w < MLM_BWD_WAVES; ++w) a += s_bias[w][i];
      if (vt * 16 + i < V) d_bias[vt * 16 + i] = a;
    }
    return;
  }
  // d_hid rows [r0, r0 + 16): A[row][k = v] = dlog[r0 + row][v] (one float4 of 4 symbols per lane), B[c][k = v] = W[v][c]
  const int r0 = ((int)blockIdx.x - wtiles) * MLM_ROWS;
  const float* pa = dlog + (long long)(r0 + li) * Vp + 4 * kg;
  for (int ct = wave; ct < ctiles; ct += MLM_BWD_WAVES) {  // (wave-uniform)
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int v0 = 0; v0 < Vp; v0 += 16) {
      const float4 a = *reinterpret_cast<const float4*>(pa + v0);
      const float* pw = W + ct * 16 + li;
      const int v = v0 + 4 * kg;
      const float b0 = v + 0 < V ? pw[(long long)(v + 0) * C] : 0.f, b1 = v + 1 < V ? pw[(long long)(v + 1) * C] : 0.f;
      const float b2 = v + 2 < V ? pw[(long long)(v + 2) * C] : 0.f, b3 = v + 3 < V ? pw[(long long)(v + 3) * C] : 0.f;
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b0, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b1, acc[1], 0, 0, 0);
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b2, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b3, acc[1], 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = r0 + 4 * kg + e;
      if (r < M) d_hid[(long long)r * C + ct * 16 + li] = acc[0][e] + acc[1][e];
    }
  }
}

extern "C" int kantts_mlm_head_bwd(const float* hid, const float* W, const float* bias, const int64_t* targets,
                                   const float* mask, const float* lse, const float* out, const float* dloss, float gscale,
                                   float* d_hid, float* d_W, float* d_bias, float* ws, long long ws_floats, int M, int C, int V,
                                   void* stream) {
  if (!targets || !mask || !lse || !out || !dloss || !d_hid || !d_W || !ws) return KANTTS_E_BADARG;
  if (((uintptr_t)d_hid & 15) || ((uintptr_t)d_W & 15) || ((uintptr_t)ws & 15)) return KANTTS_E_BADARG;
  const int rc = mlm_check(hid, W, M, C, V);
  if (rc != KANTTS_OK) return rc;
  const int rblocks = kantts_cdiv(M, MLM_ROWS), Vp = kantts_cdiv(V, 16) * 16;
  if (ws_floats < (long long)rblocks * MLM_ROWS * Vp) return KANTTS_E_WORKSPACE;
  const int wtiles = (Vp >> 4) * (C >> 4);
  hipLaunchKernelGGL(mlm_dlogits_kernel, dim3(rblocks), dim3(MLM_FWD_THREADS), 0, (hipStream_t)stream, hid, W, bias, targets,
                     mask, lse, out, dloss, gscale, ws, M, C, V, Vp);
  hipLaunchKernelGGL(mlm_grads_kernel, dim3(wtiles + rblocks), dim3(MLM_BWD_THREADS), 0, (hipStream_t)stream, hid, W,
                     (const float*)ws, d_hid, d_W, d_bias, M, C, V, Vp, wtiles);
  KANTTS_CHECK_LAUNCH();
}
