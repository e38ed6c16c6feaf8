// The two batch fields a device-resident corpus of duration-free (MAS) and speaker-embedding (SE) voices still took from
// the host (kantts/datasets/device_batching.py; the C ABI and the formula are written out in include/kantts_hip.h):
//   * kantts_attn_prior_rows: the zero-padded beta-binomial alignment prior of a whole batch (reference
//     kantts/datasets/dataset.py:20-31 evaluates scipy.stats.betabinom row by row per utterance, :798-827 pads it) -- a pure
//     function of two integers per utterance, so nothing of it has to exist on the host;
//   * kantts_broadcast_rows_f32: an utterance's speaker embedding repeated over its symbols and padded (:757-762).
// Both are store-bound fills of a (B, rows, width) fp32 tensor: a workgroup owns a run of whole rows of one item, its
// threads walk the run in 16-byte groups (aligned to the ADDRESS, so any 4-byte aligned output takes the vector stores; the
// cells of a group that lie outside the run are the neighbour's and are left to it: scalar head and tail).
//
// The prior in log space, with lf[n] = log n! (every gamma argument is a positive integer):
//   log pmf(i, k) = [lf[P] - lf[P + M] + lf[M]]  +  [-lf[i] - lf[M - 1 - i]]  +  [-lf[k] - lf[P - k]]  +  g(i + k)
//                    item                           row                          column
//   g(s) = lf[s] + lf[P + M - 1 - s]: the one term that couples row and column depends on i + k only.
// A workgroup stages its rows' term (item term folded in), the column term and g over its window of s in LDS: a cell is two
// LDS reads, two fp64 adds and one fp64 exp, rounded once to fp32.  (No recurrence from pmf(0): that underflows fp64 for
// the last rows of a long utterance; no fp32 log space: the terms reach several thousand.)  Inputs whose window does not
// fit the 64 KB a launch may ask for (2 (rows + Tin) doubles: Tin > 4095, where a workgroup has one row) read the table
// through L1 / L2 instead -- same sums in the same order, same results.
#include "common.h"

#define PRIOR_THREADS 256
#define PRIOR_MAX_ROWS 64            // rows of one workgroup at most
#define PRIOR_CELLS 4096             // cells of one workgroup, about (the rows follow from it; 1024 ... 8192 measured:
                                     // profiles/mas_device_corpus_tile_sweep.txt)
#define PRIOR_LDS_BYTES (64 * 1024)  // dynamic LDS a launch may ask for without an attribute

extern __shared__ double kantts_prior_lds[];

// span: the first cell of a run of whole rows of ``W`` cells, ``n`` cells in all (n + 3 < 2^32); span[r * W + k] =
// cell(r, k).  Called by every thread of the workgroup.
template <typename F>
__device__ __forceinline__ void prior_store_rows(float* __restrict__ span, unsigned n, unsigned W, F cell) {
  const unsigned head = (unsigned)((reinterpret_cast<uintptr_t>(span) >> 2) & 3);  // cells of the first group before span
  float* const grp = span - head;                                                 // 16-byte aligned
  for (unsigned u = threadIdx.x * 4u; u < n + head; u += blockDim.x * 4u) {
    const unsigned first = u < head ? 0u : u - head;  // the first cell of this group inside the run
    unsigned r = first / W, k = first - r * W;
    float v[4];
    bool in[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      in[j] = u + j >= head && u + j - head < n;
      v[j] = 0.f;
      if (in[j]) {
        v[j] = cell((int)r, (int)k);
        if (++k == W) {
          k = 0;
          ++r;
        }
      }
    }
    if (in[0] && in[3]) {
      *reinterpret_cast<float4*>(grp + u) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (in[j]) grp[u + j] = v[j];
    }
  }
}

template <bool STAGE>
__global__ __launch_bounds__(PRIOR_THREADS) void attn_prior_kernel(const double* __restrict__ lfact, int n_lfact,
                                                                   const int* __restrict__ n_sym,
                                                                   const int* __restrict__ n_mel, float* __restrict__ out,
                                                                   int Tout, int Tin, int rows_per_wg) {
  const int b = blockIdx.y;
  const int i0 = blockIdx.x * rows_per_wg;  // < Tout (the grid is cdiv(Tout, rows_per_wg))
  const int rows = min(rows_per_wg, Tout - i0);
  int P = min(n_sym[b], Tin), M = min(n_mel[b], Tout);
  if (P < 1 || M < 1) P = M = 0;
  const bool covered = (long long)P + M < n_lfact;  // the largest index read is P + M
  const int live = max(0, min(rows, M - i0));       // this workgroup's rows with live cells
  float* const span = out + ((long long)b * Tout + i0) * Tin;
  const unsigned n = (unsigned)rows * (unsigned)Tin;  // <= Tout * Tin < 2^31
  if (live == 0 || !covered) {
    const float dead = __builtin_nanf("");
    prior_store_rows(span, n, (unsigned)Tin, [&](int r, int k) { return (r < live && k < P) ? dead : 0.f; });
    return;
  }
  // from here on: 1 <= P <= Tin, 1 <= M <= Tout, P + M < n_lfact, i0 < M; every index below is in [0, P + M]
  const double item = lfact[P] - lfact[P + M] + lfact[M];
  if (STAGE) {
    double* const rowc = kantts_prior_lds;       // [live]          item - lf[i] - lf[M - 1 - i],  i = i0 + r
    double* const colc = rowc + rows_per_wg;     // [P]             -lf[k] - lf[P - k]
    double* const g = colc + Tin;                // [live + P - 1]  lf[s] + lf[P + M - 1 - s],     s = i0 + r + k
    for (int r = threadIdx.x; r < live; r += blockDim.x) rowc[r] = item - lfact[i0 + r] - lfact[M - 1 - i0 - r];
    for (int k = threadIdx.x; k < P; k += blockDim.x) colc[k] = -lfact[k] - lfact[P - k];
    for (int s = threadIdx.x; s < live + P - 1; s += blockDim.x) g[s] = lfact[i0 + s] + lfact[P + M - 1 - i0 - s];
    __syncthreads();
    prior_store_rows(span, n, (unsigned)Tin, [&](int r, int k) {
      return (r < live && k < P) ? (float)exp(rowc[r] + colc[k] + g[r + k]) : 0.f;
    });
  } else {
    prior_store_rows(span, n, (unsigned)Tin, [&](int r, int k) {
      if (r >= live || k >= P) return 0.f;
      const int i = i0 + r;
      const double rc = item - lfact[i] - lfact[M - 1 - i], cc = -lfact[k] - lfact[P - k];
      return (float)exp(rc + cc + (lfact[i + k] + lfact[P + M - 1 - i - k]));
    });
  }
}

extern "C" int kantts_attn_prior_rows(const double* lfact, int n_lfact, const int32_t* n_sym, const int32_t* n_mel, float* out,
                                      int B, int Tout, int Tin, void* stream) {
  if (!lfact || !n_sym || !n_mel || !out || B < 1 || Tout < 1 || Tin < 1 || n_lfact < 2) return KANTTS_E_BADARG;
  if (B > 65535 || (long long)Tout * Tin >= (1ll << 31)) return KANTTS_E_UNSUPPORTED;
  const int rows_per_wg = max(1, min(min(PRIOR_MAX_ROWS, Tout), PRIOR_CELLS / Tin));
  const size_t lds = sizeof(double) * (2 * ((size_t)rows_per_wg + (size_t)Tin));
  dim3 grid((unsigned)kantts_cdiv(Tout, rows_per_wg), B);
  if (lds <= PRIOR_LDS_BYTES)
    hipLaunchKernelGGL((attn_prior_kernel<true>), grid, dim3(PRIOR_THREADS), lds, (hipStream_t)stream, lfact, n_lfact, n_sym,
                       n_mel, out, Tout, Tin, rows_per_wg);
  else
    hipLaunchKernelGGL((attn_prior_kernel<false>), grid, dim3(PRIOR_THREADS), 0, (hipStream_t)stream, lfact, n_lfact, n_sym,
                       n_mel, out, Tout, Tin, rows_per_wg);
  KANTTS_CHECK_LAUNCH();
}

// out[b][t][:] = t < len[b] ? table[item[b]][:] : 0 -- the same walk over runs of whole rows; a bit-exact copy.
__global__ __launch_bounds__(PRIOR_THREADS) void broadcast_rows_kernel(const float* __restrict__ table, int n_items,
                                                                       const long long* __restrict__ item,
                                                                       const int* __restrict__ len, float* __restrict__ out,
                                                                       int Tmax, int D, int rows_per_wg) {
  const int b = blockIdx.y;
  const int t0 = blockIdx.x * rows_per_wg;
  const int rows = min(rows_per_wg, Tmax - t0);
  const long long it = item[b];
  const int live = (it < 0 || it >= n_items) ? 0 : max(0, min(rows, len[b] - t0));
  const float* const src = table + (live ? it : 0) * D;
  float* const span = out + ((long long)b * Tmax + t0) * D;
  prior_store_rows(span, (unsigned)rows * (unsigned)D, (unsigned)D, [&](int r, int c) { return r < live ? src[c] : 0.f; });
}

extern "C" int kantts_broadcast_rows_f32(const float* table, int n, const int64_t* item, const int32_t* len, float* out, int B,
                                         int Tmax, int D, void* stream) {
  if (!table || !item || !len || !out || B < 1 || Tmax < 1 || D < 1 || n < 1) return KANTTS_E_BADARG;
  if (B > 65535 || (long long)Tmax * D >= (1ll << 31)) return KANTTS_E_UNSUPPORTED;
  const int rows_per_wg = max(1, min(Tmax, PRIOR_CELLS / D));
  dim3 grid((unsigned)kantts_cdiv(Tmax, rows_per_wg), B);
  hipLaunchKernelGGL(broadcast_rows_kernel, grid, dim3(PRIOR_THREADS), 0, (hipStream_t)stream, table, n,
                     reinterpret_cast<const long long*>(item), len, out, Tmax, D, rows_per_wg);
  KANTTS_CHECK_LAUNCH();
}
