// Body of the feed-forward pair kernel of ffn_pair.hip (ffn_pair_kernel<BWD, KT2, K1, N, F, BM, MAXKT>).  Expects: BWD, KT2
// and the geometry K1 (input width), N (output width), F (hidden width), BM (token tile height), MAXKT (most taps of phase
// 1; 1 = no tap halo, KT is the constant 1) as compile-time constants, and `g` (kantts_ffn_args).  [round 4] the variant
// that ended in the LayerNorm backward (ffn_pair_lnb_kernel) was timed on the device at 35.1 us against 23.0 us for the
// two launches it replaced and was removed.
  constexpr int NB = BM / 16;              // 16-token MFMA B blocks of the tile
  constexpr int XP = K1 + 16;              // X tile pitch in elements: 32 B mod 64 (conflict-free 16-byte fragment reads)
  constexpr int XROWS = BM + MAXKT - 1;    // tile + tap halo (up to 4 rows either side at MAXKT = 9)
  constexpr int TP = F + 16;               // T tile pitch in elements
  constexpr int KQ = K1 / 128;             // weight units per tap and chunk of phase 1 (a unit: 32 rows x 128 k per wave)
  constexpr bool HALVES = N == 128;        // phase 2: 4 x 32 output rows, the reduction split over two groups of waves;
                                           // N = 256: 8 x 32 output rows, every wave owns its whole reduction
  constexpr int U2 = HALVES ? F / 256 : F / 128;  // weight units per tap of phase 2
  constexpr int NA = HALVES ? 1 : 2;       // 16-row output blocks a wave stores
  // MAXKT == 1: the unit sequence (S1 of phase 1, then S2 of phase 2) is known at compile time and is walked fully unrolled,
  // with D units in flight ahead of the one being consumed.  A wave spends BM / 32 times as many MFMAs on a unit as at
  // BM = 32, so fewer units in flight hide the same latency: at BM = 80 the ten accumulators, five B fragments and the
  // epilogue operands leave room for three ring sets, not four (four: 404 bytes of scratch per lane).
  constexpr bool SEQ = MAXKT == 1;
  constexpr int S1 = (F / 256) * KQ, S2 = U2;
  constexpr int D = S1 + S2 < 4 ? S1 + S2 : (BM > 32 ? FP_DEPTH_TALL : 4);
  static_assert(BM % 16 == 0 && K1 % 128 == 0 && F % 256 == 0 && (N == 128 || N == 256), "ffn_pair geometry");
  static_assert((BM * (F / 8)) % FP_THREADS == 0, "gate staging: whole passes");
  static_assert(SEQ ? KT2 == 1 : (S1 % 4 == 0 && U2 == 4), "ring");
  __shared__ __attribute__((aligned(16))) __bf16 Xs[XROWS * XP];
  __shared__ __attribute__((aligned(16))) __bf16 Ts[BM * TP];
  __shared__ __attribute__((aligned(16))) float B1s[F];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kg = lane >> 4;
  // phase-2 tap t reads tile row (output slot + HL + s2_first + t*s2_step)
  constexpr int OUT = BM - (KT2 - 1);
  const int s2_lo = KT2 == 1 ? 0 : min(g.s2_first, g.s2_first + (KT2 - 1) * g.s2_step);
  const int HL = KT2 == 1 ? 0 : -s2_lo;                 // halo rows in front of the first output row
  const int mo0 = blockIdx.x * OUT;                     // first output row of this workgroup
  const int m0 = mo0 - HL;                              // global row of tile row 0 (may be negative)
  const int M = g.M, KT = MAXKT == 1 ? 1 : g.KT, pad = MAXKT == 1 ? 0 : g.pad, T = g.T;
  const uint64_t seed_off = kantts_seed_offset(g.seed_dev);
  const __bf16* __restrict__ w1 = reinterpret_cast<const __bf16*>(g.w1);
  const __bf16* __restrict__ w2 = reinterpret_cast<const __bf16*>(g.w2);

  // ---- weight stream: units of 8 fragment loads (8 KB per wave; at K1 = 128 contiguous in the fragment-major images)
  //   phase 1, step s = (chunk c, tap, k quarter kq): rows tap*F + c*256 + wave*32 + {0, 16}, k-blocks kq*4 + {0..3}
  //   phase 2, unit u = (tap, uu): N = 128: rows (wave & 3)*32 + {0, 16}, k-blocks (wave >> 2)*(F/64) + uu*4 + {0..3}
  //                                N = 256: rows wave*32 + {0, 16},       k-blocks uu*4 + {0..3}
  const int upc = KT * KQ;                // units per chunk
  const int steps = (F >> 8) * upc;       // a multiple of 4 (SEQ: S1, any)
  u32x4 ring[4][8];
  auto load1 = [&](u32x4* w, int s) {
    const int c = s / upc, r = s - c * upc, tap = r / KQ, kq = r - tap * KQ;
    if constexpr (KQ == 1) {  // the two row blocks are adjacent in the image: 8 KB contiguous
      const __bf16* p = w1 + ((long long)(tap * (F >> 4) + c * 16 + wave * 2) * 4) * 512 + lane * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) w[j] = *reinterpret_cast<const u32x4*>(p + j * 512);
    } else {
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const __bf16* p = w1 + ((long long)(tap * (F >> 4) + c * 16 + wave * 2 + a) * (K1 >> 5) + kq * 4) * 512 + lane * 8;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) w[a * 4 + kk] = *reinterpret_cast<const u32x4*>(p + kk * 512);
      }
    }
  };
  const int nq = HALVES ? (wave & 3) : wave, kh = HALVES ? (wave >> 2) : 0;
  auto load2 = [&](u32x4* w, int u) {
    const int tap = u / U2, uu = u - tap * U2;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const __bf16* p = w2 + ((long long)(tap * (N >> 4) + nq * 2 + a) * (F >> 5) + kh * (F >> 6) + uu * 4) * 512 + lane * 8;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) w[a * 4 + kk] = *reinterpret_cast<const u32x4*>(p + kk * 512);
    }
  };
  auto fetch = [&](int t) {  // SEQ: unit t of the whole sequence into its ring set
    if (t < S1)
      load1(ring[t & 3], t);
    else
      load2(ring[t & 3], t - S1);
  };
  if constexpr (SEQ) {
#pragma unroll
    for (int t = 0; t < D; ++t) fetch(t);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) load1(ring[j], j);
  }

  // SEQ: the bias is requested with the X tile (unconditionally; a dummy address when absent)
  float4 bv1 = {0.f, 0.f, 0.f, 0.f};
  if constexpr (SEQ && !BWD) {
    const bool has = g.bias1 && tid < F / 4;
    bv1 = *reinterpret_cast<const float4*>(has ? g.bias1 + tid * 4 : reinterpret_cast<const float*>(g.w1));
    if (!has) bv1 = (float4){0.f, 0.f, 0.f, 0.f};
  }
  // ---- X tile: LDS row j <-> global row m0 - pad + j
  if constexpr (MAXKT == 1) {
    // no halo, no regenerated dropout, no row mask (the host entry declines them at these shapes): every load of the tile
    // is issued before the first conversion, none inside a branch (rows past M read a clamped row and store zeros)
    constexpr int XV = K1 / 8, XIT = BM * XV / FP_THREADS;
    static_assert((BM * XV) % FP_THREADS == 0, "X tile: whole passes");
    if (g.x_f32) {
      float4 xa[XIT], xb[XIT];
#pragma unroll
      for (int it = 0; it < XIT; ++it) {
        const int id = tid + FP_THREADS * it;
        const long long row = max(0ll, min((long long)m0 + id / XV, (long long)M - 1));
        const float* p = reinterpret_cast<const float*>(g.x) + row * g.ldx + (id % XV) * 8;
        xa[it] = *reinterpret_cast<const float4*>(p);
        xb[it] = *reinterpret_cast<const float4*>(p + 4);
      }
#pragma unroll
      for (int it = 0; it < XIT; ++it) {
        const int id = tid + FP_THREADS * it, j = id / XV;
        u32x4 v = {kantts_pack2_of4(xa[it].x, xa[it].y), kantts_pack2_of4(xa[it].z, xa[it].w), kantts_pack2_of4(xb[it].x, xb[it].y),
                   kantts_pack2_of4(xb[it].z, xb[it].w)};
        if (m0 + j >= M) v = (u32x4){0u, 0u, 0u, 0u};
        *reinterpret_cast<u32x4*>(&Xs[j * XP + (id % XV) * 8]) = v;
      }
    } else {
      u32x4 xv[XIT];
#pragma unroll
      for (int it = 0; it < XIT; ++it) {
        const int id = tid + FP_THREADS * it;
        const long long row = max(0ll, min((long long)m0 + id / XV, (long long)M - 1));
        xv[it] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const __bf16*>(g.x) + row * g.ldx + (id % XV) * 8);
      }
#pragma unroll
      for (int it = 0; it < XIT; ++it) {
        const int id = tid + FP_THREADS * it, j = id / XV;
        u32x4 v = xv[it];
        if (m0 + j >= M) v = (u32x4){0u, 0u, 0u, 0u};
        *reinterpret_cast<u32x4*>(&Xs[j * XP + (id % XV) * 8]) = v;
      }
    }
  } else {
    const int rows = BM + KT - 1;
    for (int id = tid; id < rows * (K1 / 8); id += FP_THREADS) {
      const int j = id / (K1 / 8), ch = id % (K1 / 8);
      const long long src = (long long)m0 - pad + j;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (src >= 0 && src < M && !(g.xrowmask && g.xrowmask[src])) {
        if (g.x_f32) {
          const float* p = reinterpret_cast<const float*>(g.x) + src * g.ldx + ch * 8;
          float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
          if (g.xdrop_p > 0.f) {
            const uint64_t base = (uint64_t)src * (uint64_t)K1 + (uint64_t)(ch * 8);
            const uint64_t sd = g.xdrop_seed + seed_off;
            float lo4[4] = {a.x, a.y, a.z, a.w}, hi4[4] = {b.x, b.y, b.z, b.w};
            kantts_dropout_scale4(g.xdrop_p, sd, base, lo4);
            kantts_dropout_scale4(g.xdrop_p, sd, base + 4, hi4);
            a = make_float4(lo4[0], lo4[1], lo4[2], lo4[3]);
            b = make_float4(hi4[0], hi4[1], hi4[2], hi4[3]);
          }
          v.x = kantts_pack2_of4(a.x, a.y);
          v.y = kantts_pack2_of4(a.z, a.w);
          v.z = kantts_pack2_of4(b.x, b.y);
          v.w = kantts_pack2_of4(b.z, b.w);
        } else {
          v = *reinterpret_cast<const u32x4*>(reinterpret_cast<const __bf16*>(g.x) + src * g.ldx + ch * 8);
        }
      }
      *reinterpret_cast<u32x4*>(&Xs[j * XP + ch * 8]) = v;
    }
  }

  // Everything the chunk epilogues need from global memory is fetched NOW: the vector-memory counter retires in order,
  // so a load issued inside the weight stream could only be waited for by draining the whole 4-deep ring.
  if (!BWD && tid < F / 4) {
    float4 bv = bv1;
    if constexpr (!SEQ) {
      if (g.bias1) bv = *reinterpret_cast<const float4*>(g.bias1 + tid * 4);
    }
    *reinterpret_cast<float4*>(&B1s[tid * 4]) = bv;
  }
  // position of this lane's tokens inside their sequences (tap validity at sequence boundaries), their row masks
  int tpos[NB];
  bool rz1[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const long long m = (long long)m0 + b * 16 + li;
    tpos[b] = ((KT > 1 || KT2 > 1) && T > 0) ? (int)(((m % T) + T) % T) : 0;
    rz1[b] = !BWD && g.rowmask1 && m >= 0 && m < M && g.rowmask1[m] != 0;
  }

  // wave-local coordinates of the T tile copy-out: the wave owns 32 columns (64 bytes) of a chunk: 4 lanes x 16 bytes
  // per row, 16 rows per pass
  const int crow = lane >> 2, ccol = (lane & 3) * 8;
  // backward: the gate (saved hidden activation, BM x F bf16) goes into the cells of the T tile that the gradient will
  // overwrite -- all of it now, next to the X tile (one exposed load latency for both; see the note on the counter above)
  if (BWD) {
    constexpr int GV = F / 8, GIT = BM * GV / FP_THREADS;
    const __bf16* gp = reinterpret_cast<const __bf16*>(g.gate);
    u32x4 gq[GIT];
#pragma unroll
    for (int it = 0; it < GIT; ++it) {
      const int id = tid + FP_THREADS * it;
      const long long row = max(0ll, min((long long)m0 + id / GV, (long long)M - 1));
      gq[it] = *reinterpret_cast<const u32x4*>(gp + row * F + (id % GV) * 8);
    }
#pragma unroll
    for (int it = 0; it < GIT; ++it) {
      const int id = tid + FP_THREADS * it;
      *reinterpret_cast<u32x4*>(&Ts[(id / GV) * TP + (id % GV) * 8]) = gq[it];
    }
  }
  __syncthreads();  // X tile complete

  f32x4 acc[2][NB];
  auto mfma1 = [&](const u32x4* w, int s) {
    const int c = s / upc, r = s - c * upc, tap = r / KQ, kq = r - tap * KQ;
    if (r == 0) {
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    bool ok[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int q = tpos[b] + tap - pad;
      ok[b] = (KT == 1) || (q >= 0 && q < T);
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      bf16x8 bf[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        u32x4 v = *reinterpret_cast<const u32x4*>(&Xs[(b * 16 + li + tap) * XP + kq * 128 + kk * 32 + kg * 8]);
        if (!ok[b]) v = (u32x4){0u, 0u, 0u, 0u};
        bf[b] = (bf16x8&)v;
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16((const bf16x8&)w[a * 4 + kk], bf[b], acc[a][b], 0, 0, 0);
    }
    if (r != upc - 1) return;
    // ---- epilogue of chunk c: four consecutive channels of one token per accumulator
    const uint64_t sd1 = g.drop1_seed + seed_off;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int f0 = c * 256 + wave * 32 + a * 16 + kg * 4;
      float4 bs = {0.f, 0.f, 0.f, 0.f};
      if (!BWD) bs = *reinterpret_cast<const float4*>(&B1s[f0]);
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int tok = b * 16 + li;
        const long long m = (long long)m0 + tok;
        float o[4] = {acc[a][b][0], acc[a][b][1], acc[a][b][2], acc[a][b][3]};
        if (BWD) {
          const u32x2 q = *reinterpret_cast<const u32x2*>(&Ts[tok * TP + f0]);
          const float gv[4] = {kantts_bf16_lo(q.x), kantts_bf16_hi(q.x), kantts_bf16_lo(q.y), kantts_bf16_hi(q.y)};
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4) o[r4] = (gv[r4] > 0.f) ? o[r4] * g.alpha1 : 0.f;
        } else {
          o[0] += bs.x; o[1] += bs.y; o[2] += bs.z; o[3] += bs.w;
          if (g.relu) {
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) o[r4] = fmaxf(o[r4], 0.f);
          }
          if (g.drop1_p > 0.f) {
            const uint64_t base = (uint64_t)m * (uint64_t)F + (uint64_t)f0;  // f0 % 4 == 0: one hash
            kantts_dropout_scale4(g.drop1_p, sd1, base, o);
          }
          if (rz1[b]) {
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) o[r4] = 0.f;
          }
        }
        const u32x2 pk = {kantts_pack2_of4(o[0], o[1]), kantts_pack2_of4(o[2], o[3])};
        *reinterpret_cast<u32x2*>(&Ts[tok * TP + f0]) = pk;
      }
    }
    // the wave's own 32 columns of T -> HBM (LDS operations of a wave execute in order: no barrier)
    KANTTS_WAVE_ORDERED();
    if (g.t_out) {
      __bf16* tp = reinterpret_cast<__bf16*>(g.t_out);
#pragma unroll
      for (int it = 0; it < NB; ++it) {
        const int i = crow + 16 * it;
        const u32x4 v = *reinterpret_cast<const u32x4*>(&Ts[i * TP + c * 256 + wave * 32 + ccol]);
        if (i >= HL && i < HL + OUT && m0 + i < M)  // rows this workgroup owns
          *reinterpret_cast<u32x4*>(tp + ((long long)m0 + i) * F + c * 256 + wave * 32 + ccol) = v;
      }
    }
  };

  // set j of the ring holds unit s = j (mod 4); it is refilled with unit s + 4 -- the tail of phase 1 pulls in the four
  // units of phase 2, which are therefore in flight across the barrier
  if constexpr (SEQ) {
#pragma unroll
    for (int s = 0; s < S1; ++s) {
      mfma1(ring[s & 3], s);
      if (s + D < S1 + S2) fetch(s + D);
    }
  } else {
    for (int s = 0; s < steps; s += 4) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        mfma1(ring[j], s + j);
        if (s + 4 < steps)
          load1(ring[j], s + 4 + j);
        else
          load2(ring[j], j);
      }
    }
  }
  __syncthreads();  // T tile complete

  // ---- phase 2: 32 output channels x BM tokens per wave, over half (N = 128) or all (N = 256) of the reduction
  // what the output epilogue needs from memory is requested before the contraction (it lands while the ring drains)
  int n0[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) n0[a] = HALVES ? nq * 32 + kh * 16 + kg * 4 : wave * 32 + a * 16 + kg * 4;
  // (unconditional loads -- a dummy address when an operand is absent: a load inside a branch makes hipcc drain the
  // counter where the branch re-joins)
  const float4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const float* dummy = reinterpret_cast<const float*>(g.w2);
  float4 bs2[NA], rv[NA][NB];
  const bool ln_epi = !BWD && KT2 == 1 && N == 128 && g.ln_out != nullptr;
  const float4 lg4 = *reinterpret_cast<const float4*>(ln_epi ? g.ln_gamma + n0[0] : dummy);
  const float4 lb4 = *reinterpret_cast<const float4*>(ln_epi ? g.ln_beta + n0[0] : dummy);
  bool rz2[NB];
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    bs2[a] = *reinterpret_cast<const float4*>(g.bias2 ? g.bias2 + n0[a] : dummy);
    if (!g.bias2) bs2[a] = zero4;
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const long long m = min((long long)mo0 + b * 16 + li, (long long)M - 1);
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      rv[a][b] = *reinterpret_cast<const float4*>(g.res ? g.res + m * g.ldr + n0[a] : dummy);
      if (!g.res) rv[a][b] = zero4;
    }
    const uint8_t q = *(g.rowmask2 ? g.rowmask2 + m : reinterpret_cast<const uint8_t*>(dummy));
    rz2[b] = g.rowmask2 && q != 0;
  }
  f32x4 acc2[2][NB];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc2[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
  int tpo[NB];  // position of the OUTPUT tokens inside their sequences
#pragma unroll
  for (int b = 0; b < NB; ++b) tpo[b] = (KT2 > 1 && T > 0) ? (mo0 + b * 16 + li) % T : 0;
  auto mfma2 = [&](const u32x4* w, int u) {
    const int tap = u / U2, uu = u - tap * U2;
    const int sh = KT2 == 1 ? 0 : g.s2_first + tap * g.s2_step;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      bf16x8 bf[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int row = min(b * 16 + li + HL + sh, BM - 1);  // slots beyond OUT read a clamped row (never stored)
        u32x4 v = *reinterpret_cast<const u32x4*>(&Ts[row * TP + (kh * (F >> 6) + uu * 4 + kk) * 32 + kg * 8]);
        if (KT2 > 1) {
          const int q = tpo[b] + sh;
          if (q < 0 || q >= T) v = (u32x4){0u, 0u, 0u, 0u};
        }
        bf[b] = (bf16x8&)v;
      }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b)
          acc2[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16((const bf16x8&)w[a * 4 + kk], bf[b], acc2[a][b], 0, 0, 0);
    }
  };
  if constexpr (SEQ) {
#pragma unroll
    for (int u = 0; u < S2; ++u) {
      mfma2(ring[(S1 + u) & 3], u);
      if (S1 + u + D < S1 + S2) fetch(S1 + u + D);
    }
  } else {
#pragma unroll
    for (int u0 = 0; u0 < 4 * KT2; u0 += 4) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        mfma2(ring[j], u0 + j);
        if (u0 + 4 + j < 4 * KT2) load2(ring[j], u0 + 4 + j);
      }
    }
  }
  if constexpr (HALVES) {
    // the two halves of the reduction meet through LDS (the T tile is dead): wave (nq, kh) finishes row block a = kh and
    // hands its partial sums of the other block to its partner
    __syncthreads();
    float* Ex = reinterpret_cast<float*>(Ts);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const f32x4 snd = kh ? acc2[0][b] : acc2[1][b];
      *reinterpret_cast<f32x4*>(&Ex[(((nq * 2 + (kh ^ 1)) * NB + b) * 64 + lane) * 4]) = snd;
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(&Ex[(((nq * 2 + kh) * NB + b) * 64 + lane) * 4]);
      acc2[0][b] = (kh ? acc2[1][b] : acc2[0][b]) + v;
    }
  }

  // ---- output: four consecutive channels of one token per accumulator -> 16-byte (fp32) / 8-byte (bf16) stores
  const uint64_t sd2 = g.drop2_seed + seed_off;
  float ov[NA][NB][4];
  bool live[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const long long m = (long long)mo0 + b * 16 + li;
    live[b] = m < M && b * 16 + li < OUT;
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      float* o = ov[a][b];
      o[0] = acc2[a][b][0] + bs2[a].x; o[1] = acc2[a][b][1] + bs2[a].y;
      o[2] = acc2[a][b][2] + bs2[a].z; o[3] = acc2[a][b][3] + bs2[a].w;
      if (g.drop2_p > 0.f) {
        const uint64_t base = (uint64_t)m * (uint64_t)N + (uint64_t)n0[a];
        kantts_dropout_scale4(g.drop2_p, sd2, base, o);
      }
      o[0] += rv[a][b].x; o[1] += rv[a][b].y; o[2] += rv[a][b].z; o[3] += rv[a][b].w;
      if (rz2[b]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = 0.f;
      }
      if (!live[b]) continue;
      if (g.y_bf16) {
        const u32x2 pk = {kantts_pack2_of4(o[0], o[1]), kantts_pack2_of4(o[2], o[3])};
        *reinterpret_cast<u32x2*>(reinterpret_cast<__bf16*>(g.y) + m * g.ldy + n0[a]) = pk;
      } else {
        const f32x4 v = {o[0], o[1], o[2], o[3]};
        *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(g.y) + m * g.ldy + n0[a]) = v;
      }
    }
  }
  if constexpr (N == 128) {
  if (ln_epi) {
    // LayerNorm(128) of the rows just formed (the pre-LN sub-layer that consumes y): a token's 128 channels sit in 4 lanes
    // (kg) of each of the 8 waves -> two-pass statistics through 2 x 8 x BM floats of LDS (the X tile is dead)
    float* St = reinterpret_cast<float*>(Xs);
    constexpr int SP = 8 * BM;  // one pass of partial sums: [wave][token]
    float mu[NB], rs[NB];
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      float ps[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        float t = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float d = pass ? ov[0][b][r] - mu[b] : ov[0][b][r];
          t += pass ? d * d : d;
        }
        t += __shfl_xor(t, 16, 64);
        t += __shfl_xor(t, 32, 64);
        ps[b] = t;
      }
      if (kg == 0) {
#pragma unroll
        for (int b = 0; b < NB; ++b) St[pass * SP + (wave * NB + b) * 16 + li] = ps[b];
      }
      __syncthreads();
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) t += St[pass * SP + (w * NB + b) * 16 + li];
        if (pass)
          rs[b] = 1.0f / sqrtf(t * (1.f / 128.f) + g.ln_eps);
        else
          mu[b] = t * (1.f / 128.f);
      }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const long long m = (long long)mo0 + b * 16 + li;
      if (!live[b]) continue;
      const float* o = ov[0][b];
      const float y0 = (o[0] - mu[b]) * rs[b] * lg4.x + lb4.x, y1 = (o[1] - mu[b]) * rs[b] * lg4.y + lb4.y;
      const float y2 = (o[2] - mu[b]) * rs[b] * lg4.z + lb4.z, y3 = (o[3] - mu[b]) * rs[b] * lg4.w + lb4.w;
      if (g.ln_out_bf16) {
        const u32x2 pk = {kantts_pack2_of4(y0, y1), kantts_pack2_of4(y2, y3)};
        *reinterpret_cast<u32x2*>(reinterpret_cast<__bf16*>(g.ln_out) + m * N + n0[0]) = pk;
      } else {
        const f32x4 v = {y0, y1, y2, y3};
        *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(g.ln_out) + m * N + n0[0]) = v;
      }
      if (wave == 0 && kg == 0) {
        g.ln_mean[m] = mu[b];
        g.ln_rstd[m] = rs[b];
      }
    }
  }
  }
