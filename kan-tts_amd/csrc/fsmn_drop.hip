// FSMN memory block of a TRAINING step (K == 41): the FIR, the block's own dropout, the encoder's dropout on the block
// output and the residual add as one launch each way (kantts_fsmn_memory_drop_fwd / _bwd).
//
// Before, a layer ran fsmn_fir41_kernel (seq.hip) and dropout2_add_kernel (elementwise.hip) one after the other: forward the
// FIR wrote m and the dropout pass read it back (100 MB per postnet layer where c, x and y are 60), backward the masked dy
// made the same round trip.  The FIR thread owned one channel x 16 frames and fetched a 56-frame window per 16 output frames
// with 4-byte loads, its 41 taps from global memory at a 164-byte stride.
//
// Here a workgroup owns FD_TT = 64 frames x FD_CB = 64 channels of one sequence:
//   * the (64 + 40) x 64 input tile is staged in LDS ONCE (16-byte loads, whole 256-byte row segments), with everything that
//     belongs to the input applied on the way in: the length mask, and in backward the two dropout masks (one hash per
//     staged float4 and dropout: 1.6 x the element quads, where 16-frame tiles would hash 3.5 x);
//   * the taps of the 64 channels are read as one contiguous run and kept in LDS, transposed (and flipped in backward);
//   * a thread owns FOUR consecutive channels x FD_NF = 4 frames, so that a dropout mask -- one 64-bit hash per four
//     consecutive channels -- is evaluated once per output float4, exactly as dropout2_add_kernel does;
//   * per tap a thread reads one float4 of taps and one new float4 row from LDS (a rolling window of 4 rows in registers)
//     for 16 multiply-adds; the centre tap and, in backward, the masked dy the filter gradient needs come from the same tile.
// Tile sizes, timed alone at the postnet's 32 x 612 x 256 (forward / backward, us; the pair: 36.1 / 35.9): 64 frames x 4
// per thread 19.1 / 22.8, 64 x 8 23.1 / 27.0, 32 x 4 22.5 / 29.6, 32 x 8 28.0 / 36.9 -- four waves per workgroup, sixteen
// per CU (LDS: four workgroups of 37 KB) hide the phases of a workgroup (loads, staging, FIR, stores) behind each other.
// The arithmetic of an output is that of the pair, operation for operation: acc = centre, fmaf(w[k], x[o + k], acc) for
// k = 0..40, the length mask, * keep1, * keep2, + res -- the last three as separate roundings, which is what
// dropout2_add_kernel compiles to (its multiplies and its add are in different basic blocks), so results are the same bits.
#include "common.h"

#define FD_K 41
#define FD_TT 64
#define FD_CB 64
#define FD_NF 4
#define FD_Q (FD_CB / 4)                     // channel quads of a tile
#define FD_THREADS (FD_Q * (FD_TT / FD_NF))  // 256
#define FD_ROWS (FD_TT + FD_K - 1)           // 104 staged rows
#define FD_WQ (FD_Q + 1)                     // tap row pitch in float4: 68 floats, so the transposing writes spread over banks
static_assert((FD_TT * FD_Q) % FD_THREADS == 0, "the padded-tile loop has no remainder");

// The operands of one problem: the single launch passes one block, the pair launch (two memory blocks of one shape over the
// same lengths: the pitch and the energy predictor's) two, picked by blockIdx.y.
struct FdProblem {
  const float* x;
  const float* w;
  const float* res;
  float* y;
  float* dym;
  float p1, p2;
  uint64_t seed1, seed2;
};
struct FdPairArgs {
  FdProblem p[2];
};

// BWD = false: x = c (the projection's output), y = keep1 * keep2 * len-masked(FIR(c) + c) (+ res); dym unused.
// BWD = true:  x = dy, dym = len-masked(keep1 * keep2 * dy) (the tile's own rows), y = dx = len-masked(FIRflip(dym) + dym).
template <bool BWD>
__device__ __forceinline__ void fsmn_drop41_body(const float* __restrict__ x, const float* __restrict__ w,
                                                 const float* __restrict__ res, const int64_t* __restrict__ lens,
                                                 float* __restrict__ y, float* __restrict__ dym, int B, int T, int C, int lp,
                                                 float p1, uint64_t seed1, float p2, uint64_t seed2,
                                                 const uint64_t* __restrict__ seed_dev) {
  __shared__ float4 sx[FD_ROWS * FD_Q];
  __shared__ float4 sw[FD_K * FD_WQ];
  // XCD-aware order (see fsmn_fir41_kernel): consecutive workgroup ids are dealt to the 8 XCDs in turn, each with its own L2,
  // and neighbouring time tiles share 40 halo rows -- XCD k owns a contiguous band of (sequence, time tile, channel block).
  const int ncb = (C + FD_CB - 1) / FD_CB, nt = (T + FD_TT - 1) / FD_TT;
  int vid = blockIdx.x;
  {
    const int total = gridDim.x;
    if (total >= 64) vid = kantts_xcd_slot(total, vid);
  }
  const int cb = vid % ncb, bt = vid / ncb;
  const int b = bt / nt, t0 = (bt - b * nt) * FD_TT, c0 = cb * FD_CB;
  const int tid = threadIdx.x;
  const int len = lens ? (int)min((long long)lens[b], (long long)T) : T;
  const long long row0 = (long long)b * T;
  const uint64_t off = kantts_seed_offset(seed_dev);
  const uint64_t s1 = seed1 + off, s2 = seed2 + off;

  if (t0 >= len) {  // a tile of padding: the masked FIR is zero, so y = 0 * keep1 * keep2 + res; dx = dym = 0
#pragma unroll
    for (int it = 0; it < FD_TT * FD_Q / FD_THREADS; ++it) {
      const int idx = it * FD_THREADS + tid, t = t0 + idx / FD_Q, c = c0 + (idx % FD_Q) * 4;
      if (t < T && c < C) {
        const long long o = (row0 + t) * C + c;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!BWD && res) {
          const float4 r = *reinterpret_cast<const float4*>(res + o);
          v = make_float4(0.f + r.x, 0.f + r.y, 0.f + r.z, 0.f + r.w);
        }
        *reinterpret_cast<float4*>(y + o) = v;
        if (BWD) *reinterpret_cast<float4*>(dym + o) = v;
      }
    }
    return;
  }

  // ---- every global load of the workgroup is issued before the first of them is used: the taps (w[c0 .. c0 + 64) is one
  // contiguous run of 64 * 41 floats), then the input tile -- one round trip to memory where a loop over the taps followed
  // by the tile made five or six dependent ones (26 us for a lone workgroup on the first device run)
  const int lpe = BWD ? (FD_K - 1 - lp) : lp;
  {
    constexpr int NW = (FD_CB * FD_K + FD_THREADS - 1) / FD_THREADS, NL = (FD_ROWS * FD_Q + FD_THREADS - 1) / FD_THREADS;
    const int nw = min(FD_CB, C - c0) * FD_K;
    const float* wb = w + (long long)c0 * FD_K;
    float wv[NW];
    float4 v[NL];
#pragma unroll
    for (int it = 0; it < NW; ++it) {
      const int i = it * FD_THREADS + tid;
      wv[it] = wb[i < nw ? i : 0];
    }
#pragma unroll
    for (int it = 0; it < NL; ++it) {
      const int idx = it * FD_THREADS + tid, ts = t0 + idx / FD_Q - lpe, c = c0 + (idx % FD_Q) * 4;
      const bool ok = idx < FD_ROWS * FD_Q && ts >= 0 && ts < len && c < C;
      v[it] = *reinterpret_cast<const float4*>(x + (ok ? (row0 + ts) * C + c : 0));
    }
    // tap k of channel cl goes to row k (backward: 40 - k) of the transposed image
    float* swf = reinterpret_cast<float*>(sw);
#pragma unroll
    for (int it = 0; it < NW; ++it) {
      const int i = it * FD_THREADS + tid, cl = i / FD_K, k = i - cl * FD_K;
      if (i < nw) swf[(BWD ? (FD_K - 1 - k) : k) * (FD_WQ * 4) + cl] = wv[it];
    }
    // the input tile: row n is frame t0 + n - lpe; zero outside [0, len) and beyond C
#pragma unroll
    for (int it = 0; it < NL; ++it) {
      const int idx = it * FD_THREADS + tid, n = idx / FD_Q, ts = t0 + n - lpe, c = c0 + (idx % FD_Q) * 4;
      if (idx >= FD_ROWS * FD_Q) break;
      const bool ok = ts >= 0 && ts < len && c < C;
      float o[4] = {0.f, 0.f, 0.f, 0.f};
      if (ok) {
        o[0] = v[it].x, o[1] = v[it].y, o[2] = v[it].z, o[3] = v[it].w;
        if (BWD) {
          const uint64_t base = (uint64_t)((row0 + ts) * C + c);
          kantts_dropout_scale4(p1, s1, base, o);
          kantts_dropout_scale4(p2, s2, base, o);
        }
      }
      const float4 m = make_float4(o[0], o[1], o[2], o[3]);
      sx[idx] = m;
      if (BWD && n >= lpe && n < lpe + FD_TT && ts < T && c < C)  // the tile's own rows (ts >= t0 >= 0)
        *reinterpret_cast<float4*>(dym + (row0 + ts) * C + c) = m;
    }
  }
  const int q = tid % FD_Q, g = tid / FD_Q, c = c0 + q * 4, tf = t0 + g * FD_NF;
  const bool cok = c < C;
  float4 rs[FD_NF];
  if (!BWD && res && cok) {  // the residual rows travel while the FIR runs
#pragma unroll
    for (int j = 0; j < FD_NF; ++j)
      rs[j] = *reinterpret_cast<const float4*>(res + (row0 + min(tf + j, T - 1)) * C + c);
  }
  __syncthreads();
  if (!cok || tf >= T) return;  // (no barrier below)

  float4 acc[FD_NF], win[FD_NF];
#pragma unroll
  for (int j = 0; j < FD_NF; ++j) {
    acc[j] = sx[(g * FD_NF + j + lpe) * FD_Q + q];  // the centre tap: x[t] itself
    win[j] = sx[(g * FD_NF + j) * FD_Q + q];
  }
  // taps in groups of FD_NF, the groups as a real loop: fully unrolled, the compiler hoists every LDS read of the 41 taps to
  // the top and spills (660 bytes of scratch per lane with 8 frames per thread); within a group the window's slots are
  // compile-time registers
  static_assert((FD_K - 1) % FD_NF == 0, "41 taps = whole groups of FD_NF and the last one");
#pragma unroll 1
  for (int kk = 0; kk < FD_K - 1; kk += FD_NF) {
#pragma unroll
    for (int ki = 0; ki < FD_NF; ++ki) {
      const int k = kk + ki;
      const float4 w4 = sw[k * FD_WQ + q];
#pragma unroll
      for (int j = 0; j < FD_NF; ++j) {
        const float4 xv = win[(j + ki) % FD_NF];  // row g * FD_NF + j + k
        acc[j].x = fmaf(w4.x, xv.x, acc[j].x);
        acc[j].y = fmaf(w4.y, xv.y, acc[j].y);
        acc[j].z = fmaf(w4.z, xv.z, acc[j].z);
        acc[j].w = fmaf(w4.w, xv.w, acc[j].w);
      }
      win[ki] = sx[(g * FD_NF + k + FD_NF) * FD_Q + q];  // row k is done with; row k + FD_NF takes its place
    }
  }
  {
    const float4 w4 = sw[(FD_K - 1) * FD_WQ + q];
#pragma unroll
    for (int j = 0; j < FD_NF; ++j) {
      const float4 xv = win[j];
      acc[j].x = fmaf(w4.x, xv.x, acc[j].x);
      acc[j].y = fmaf(w4.y, xv.y, acc[j].y);
      acc[j].z = fmaf(w4.z, xv.z, acc[j].z);
      acc[j].w = fmaf(w4.w, xv.w, acc[j].w);
    }
  }
#pragma unroll
  for (int j = 0; j < FD_NF; ++j) {
    const int t = tf + j;
    if (t >= T) break;
    const long long oidx = (row0 + t) * C + c;
    const bool in = t < len;
    float o[4] = {in ? acc[j].x : 0.f, in ? acc[j].y : 0.f, in ? acc[j].z : 0.f, in ? acc[j].w : 0.f};
    if (!BWD) {
      kantts_dropout_scale4(p1, s1, (uint64_t)oidx, o);
      kantts_dropout_scale4(p2, s2, (uint64_t)oidx, o);
      if (res) {
        // one rounding of its own, as in dropout2_add_kernel: not contracted with the multiply by keep2
#pragma clang fp contract(off)
        o[0] = o[0] + rs[j].x;
        o[1] = o[1] + rs[j].y;
        o[2] = o[2] + rs[j].z;
        o[3] = o[3] + rs[j].w;
      }
    }
    *reinterpret_cast<float4*>(y + oidx) = make_float4(o[0], o[1], o[2], o[3]);
  }
}

template <bool BWD>
__global__ __launch_bounds__(FD_THREADS) void fsmn_drop41_kernel(const FdProblem a, const int64_t* __restrict__ lens, int B,
                                                                 int T, int C, int lp,
                                                                 const uint64_t* __restrict__ seed_dev) {
  fsmn_drop41_body<BWD>(a.x, a.w, a.res, lens, a.y, a.dym, B, T, C, lp, a.p1, a.seed1, a.p2, a.seed2, seed_dev);
}

// grid (tiles of one problem, 2): the XCD-aware order of the body runs over gridDim.x, i.e. per problem
template <bool BWD>
__global__ __launch_bounds__(FD_THREADS) void fsmn_drop41_pair_kernel(const FdPairArgs pa, const int64_t* __restrict__ lens,
                                                                      int B, int T, int C, int lp,
                                                                      const uint64_t* __restrict__ seed_dev) {
  const FdProblem& a = pa.p[blockIdx.y];
  fsmn_drop41_body<BWD>(a.x, a.w, a.res, lens, a.y, a.dym, B, T, C, lp, a.p1, a.seed1, a.p2, a.seed2, seed_dev);
}

static int fd_check(const void* a, const void* w, const void* o, int B, int T, int C, int K, int left_pad, float p1, float p2,
                    long long* blocks) {
  if (!a || !w || !o || B < 0 || T < 0 || C < 1 || K < 1 || left_pad < 0 || left_pad >= K || p1 < 0.f || p1 >= 1.f ||
      p2 < 0.f || p2 >= 1.f)
    return KANTTS_E_BADARG;
  if (K != FD_K || (C & 3)) return KANTTS_E_UNSUPPORTED;
  *blocks = (long long)B * kantts_cdiv(T, FD_TT) * kantts_cdiv(C, FD_CB);
  if (*blocks > 0x7fffffffLL) return KANTTS_E_UNSUPPORTED;
  return KANTTS_OK;
}

// one problem's checks: the forward form (c, res, y) or the backward form (dy, dx, dym)
static int fd_check_fwd(const float* c, const float* w, const float* res, float* y, int B, int T, int C, int K, int left_pad,
                        float p1, float p2, long long* blocks) {
  const int rc = fd_check(c, w, y, B, T, C, K, left_pad, p1, p2, blocks);
  if (rc != KANTTS_OK) return rc;
  if (!kantts_aligned16(c) || !kantts_aligned16(res) || !kantts_aligned16(y)) return KANTTS_E_UNSUPPORTED;
  return KANTTS_OK;
}
static int fd_check_bwd(const float* dy, const float* w, float* dx, float* dym, int B, int T, int C, int K, int left_pad,
                        float p1, float p2, long long* blocks) {
  const int rc = fd_check(dy, w, dx, B, T, C, K, left_pad, p1, p2, blocks);
  if (rc != KANTTS_OK) return rc;
  if (!dym) return KANTTS_E_BADARG;
  if (!kantts_aligned16(dy) || !kantts_aligned16(dx) || !kantts_aligned16(dym)) return KANTTS_E_UNSUPPORTED;
  return KANTTS_OK;
}

extern "C" int kantts_fsmn_memory_drop_fwd(const float* c, const float* w, const float* res, const int64_t* lens, float* y,
                                           int B, int T, int C, int K, int left_pad, float p1, uint64_t seed1, float p2,
                                           uint64_t seed2, const uint64_t* seed_dev, void* stream) {
  long long blocks = 0;
  const int rc = fd_check_fwd(c, w, res, y, B, T, C, K, left_pad, p1, p2, &blocks);
  if (rc != KANTTS_OK) return rc;
  if (blocks == 0) return KANTTS_OK;
  const FdProblem a = {c, w, res, y, nullptr, p1, p2, seed1, seed2};
  hipLaunchKernelGGL(fsmn_drop41_kernel<false>, dim3((unsigned)blocks), dim3(FD_THREADS), 0, (hipStream_t)stream, a, lens, B,
                     T, C, left_pad, seed_dev);
  KANTTS_CHECK_LAUNCH();
}

extern "C" int kantts_fsmn_memory_drop_bwd(const float* dy, const float* w, const int64_t* lens, float* dx, float* dym, int B,
                                           int T, int C, int K, int left_pad, float p1, uint64_t seed1, float p2,
                                           uint64_t seed2, const uint64_t* seed_dev, void* stream) {
  long long blocks = 0;
  const int rc = fd_check_bwd(dy, w, dx, dym, B, T, C, K, left_pad, p1, p2, &blocks);
  if (rc != KANTTS_OK) return rc;
  if (blocks == 0) return KANTTS_OK;
  const FdProblem a = {dy, w, nullptr, dx, dym, p1, p2, seed1, seed2};
  hipLaunchKernelGGL(fsmn_drop41_kernel<true>, dim3((unsigned)blocks), dim3(FD_THREADS), 0, (hipStream_t)stream, a, lens, B, T,
                     C, left_pad, seed_dev);
  KANTTS_CHECK_LAUNCH();
}

// Two memory blocks of one shape (B, T, C, K, left_pad) over the same lengths in one launch each way; every problem keeps its
// own operands, dropout probabilities and seeds, and gets the bits of its own single call.
extern "C" int kantts_fsmn_memory_drop_fwd_pair(const kantts_fsmn_drop_args* a, const kantts_fsmn_drop_args* b,
                                                const int64_t* lens, int B, int T, int C, int K, int left_pad,
                                                const uint64_t* seed_dev, void* stream) {
  if (!a || !b) return KANTTS_E_BADARG;
  long long blocks = 0;
  FdPairArgs pa;
  const kantts_fsmn_drop_args* both[2] = {a, b};
  for (int i = 0; i < 2; ++i) {
    const kantts_fsmn_drop_args& g = *both[i];
    const int rc = fd_check_fwd(g.x, g.w, g.res, g.y, B, T, C, K, left_pad, g.p1, g.p2, &blocks);
    if (rc != KANTTS_OK) return rc;
    pa.p[i] = {g.x, g.w, g.res, g.y, nullptr, g.p1, g.p2, g.seed1, g.seed2};
  }
  if (blocks == 0) return KANTTS_OK;
  hipLaunchKernelGGL(fsmn_drop41_pair_kernel<false>, dim3((unsigned)blocks, 2), dim3(FD_THREADS), 0, (hipStream_t)stream, pa,
                     lens, B, T, C, left_pad, seed_dev);
  KANTTS_CHECK_LAUNCH();
}

extern "C" int kantts_fsmn_memory_drop_bwd_pair(const kantts_fsmn_drop_args* a, const kantts_fsmn_drop_args* b,
                                                const int64_t* lens, int B, int T, int C, int K, int left_pad,
                                                const uint64_t* seed_dev, void* stream) {
  if (!a || !b) return KANTTS_E_BADARG;
  long long blocks = 0;
  FdPairArgs pa;
  const kantts_fsmn_drop_args* both[2] = {a, b};
  for (int i = 0; i < 2; ++i) {
    const kantts_fsmn_drop_args& g = *both[i];
    const int rc = fd_check_bwd(g.x, g.w, g.y, g.dym, B, T, C, K, left_pad, g.p1, g.p2, &blocks);
    if (rc != KANTTS_OK) return rc;
    pa.p[i] = {g.x, g.w, nullptr, g.y, g.dym, g.p1, g.p2, g.seed1, g.seed2};
  }
  if (blocks == 0) return KANTTS_OK;
  hipLaunchKernelGGL(fsmn_drop41_pair_kernel<true>, dim3((unsigned)blocks, 2), dim3(FD_THREADS), 0, (hipStream_t)stream, pa,
                     lens, B, T, C, left_pad, seed_dev);
  KANTTS_CHECK_LAUNCH();
}
