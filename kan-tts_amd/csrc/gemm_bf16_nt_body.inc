// Body of the NT kernels of gemm_bf16.hip, included once per kernel definition (textual inclusion, not a function:
// handing the kernel arguments to an inlined device function by reference changed the code of the existing kernels).
// Expects: template parameters / constants BM, A_F32, B_KN, LNB; `g` (kantts_bgemm_args); `lnb` (const kantts_lnbwd_args*,
// nullptr unless LNB).
  constexpr int A_BYTES = BM * BG_BK * 2;
  constexpr int B_BYTES = B_KN ? BG_BK * BG_LDKN * 2 : BG_BN * BG_BK * 2;
  constexpr int STAGE = A_BYTES + B_BYTES;
  constexpr int CLD = BG_BN + 4;
  constexpr int CS_BYTES = BM * CLD * 4;
  constexpr int LDS_BYTES = (2 * STAGE > CS_BYTES) ? 2 * STAGE : CS_BYTES;
  __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];
  constexpr int NA = BM * 8 / BG_THREADS;  // 16-byte chunks of the A tile per thread (4 / 2 / 1)
  constexpr int NB = 4;                    // B tile: 1024 chunks
  constexpr int WM = (BM >= 64) ? 2 : 1;   // waves along M
  constexpr int NREP = (BM >= 64) ? 4 : 2; // 16-column fragments per wave
  constexpr int MREP = BM / (WM * 16);     // 16-row fragments per wave (4 / 2 / 2)
  constexpr int WROWS = MREP * 16;         // rows per wave

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = (WM == 2) ? (wave >> 1) : 0, wc = (WM == 2) ? (wave & 1) : wave;
  const int li = lane & 15, kg = lane >> 4;
  int bx = blockIdx.x, by = blockIdx.y;
  bg_xcd_remap(bx, by);
  const int i0 = by * BM, j0 = bx * BG_BN;
  const uint64_t seed_off = kantts_seed_offset(g.seed_dev);

  f32x4 acc[MREP][NREP];
#pragma unroll
  for (int m = 0; m < MREP; ++m)
#pragma unroll
    for (int n = 0; n < NREP; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // ---- per-thread chunk coordinates (fixed over the reduction)
  int a_row[NA], a_ch[NA];
#pragma unroll
  for (int v = 0; v < NA; ++v) {
    const int id = tid + BG_THREADS * v;
    a_row[v] = id >> 3;
    a_ch[v] = id & 7;
  }
  int b_r[NB], b_c[NB];  // !B_KN: (n row, k chunk);  B_KN: (k row, n chunk)
#pragma unroll
  for (int v = 0; v < NB; ++v) {
    const int id = tid + BG_THREADS * v;
    if (B_KN) {
      b_r[v] = id >> 4;
      b_c[v] = id & 15;
    } else {
      b_r[v] = id >> 3;
      b_c[v] = id & 7;
    }
  }

  // two register sets: the global loads of TWO reduction tiles are in flight while a third is multiplied (the
  // contractions of this model are short chains of dependent L2 / HBM round trips: with one tile in flight a
  // 1024-deep reduction paid 16 load latencies back to back)
  BgRaw<A_F32> ra0[NA], ra1[NA];
  BgRaw<false> rb0[NB], rb1[NB];
  int seg = 0, k0 = 0;    // next tile to fetch
  int fs0 = 0, fk0 = 0, fs1 = 0, fk1 = 0;  // (segment, k offset) of the tile held by register set 0 / 1
  int ntile = 0;
  for (int s = 0; s < g.nseg; ++s) ntile += (g.seg[s].klen + BG_BK - 1) / BG_BK;
  int fetched = 0, fs_last = 0, fk_last = 0;

  // [round 5] fetch = loads only (bg_fetch8: unconditional, clamped addresses), finished -- predicate, dropout, rounding --
  // when the tile is committed one iteration later.  A fetch past the last tile repeats the last tile (never inside a branch).
  auto fetch = [&](BgRaw<A_F32>* ra, BgRaw<false>* rb, int& fs, int& fk) {
    if (fetched >= ntile) {  // repeat the last tile's addresses: (seg, k0) step back to it
      seg = fs_last;
      k0 = fk_last;
    }
    const kantts_bgemm_seg& s = g.seg[seg];
    fs = seg;
    fk = k0;
#pragma unroll
    for (int v = 0; v < NA; ++v) {
      const int row = i0 + a_row[v];
      const int kc = k0 + a_ch[v] * 8;
      bool ok = row < g.M && kc < s.klen;
      long long src = row;
      if (s.a_shift != 0) {
        const int t = row % g.T + s.a_shift;
        ok = ok && t >= 0 && t < g.T;
        src = (long long)row + s.a_shift;
      }
      ra[v] = bg_fetch8<A_F32>(s.a, src * s.lda + kc, ok);
    }
#pragma unroll
    for (int v = 0; v < NB; ++v) {
      if (B_KN) {
        const int kr = k0 + b_r[v], nc = j0 + b_c[v] * 8;
        const bool ok = kr < s.klen && nc < g.N;
        rb[v] = bg_fetch8<false>(s.b, (long long)kr * s.ldb + nc, ok);
      } else {
        const int n = j0 + b_r[v], kc = k0 + b_c[v] * 8;
        const bool ok = n < g.N && kc < s.klen;
        rb[v] = bg_fetch8<false>(s.b, (long long)n * s.ldb + kc, ok);
      }
    }
    fs_last = seg;
    fk_last = k0;
    ++fetched;
    k0 += BG_BK;
    if (k0 >= s.klen) {
      k0 = 0;
      ++seg;
    }
  };
  auto commit = [&](int buf, const BgRaw<A_F32>* ra, const BgRaw<false>* rb, int fs, int fk) {
    unsigned char* Ab = lds + buf * STAGE;
    unsigned char* Bb = Ab + A_BYTES;
    const kantts_bgemm_seg& s = g.seg[fs];
#pragma unroll
    for (int v = 0; v < NA; ++v) {
      const int r = a_row[v];
      const int row = i0 + r;
      const int kc = fk + a_ch[v] * 8;
      bool ok = row < g.M && kc < s.klen;
      long long src = row;
      if (s.a_shift != 0) {
        const int t = row % g.T + s.a_shift;
        ok = ok && t >= 0 && t < g.T;
        src = (long long)row + s.a_shift;
      }
      *reinterpret_cast<u32x4*>(Ab + r * 128 + ((a_ch[v] ^ ((r >> 1) & 7)) << 4)) =
          bg_finish8<A_F32>(ra[v], ok, A_F32 ? g.a_drop_p : 0.f, g.a_drop_seed + seed_off,
                            (uint64_t)src * (uint64_t)g.a_drop_ld + (uint64_t)kc);
    }
#pragma unroll
    for (int v = 0; v < NB; ++v) {
      if (B_KN) {
        const int kr = fk + b_r[v], nc = j0 + b_c[v] * 8;
        const bool ok = kr < s.klen && nc < g.N;
        *reinterpret_cast<u32x4*>(Bb + (b_r[v] * BG_LDKN + b_c[v] * 8) * 2) = bg_finish8<false>(rb[v], ok, 0.f, 0ull, 0ull);
      } else {
        const int r = b_r[v];
        const int n = j0 + r, kc = fk + b_c[v] * 8;
        const bool ok = n < g.N && kc < s.klen;
        *reinterpret_cast<u32x4*>(Bb + r * 128 + ((b_c[v] ^ ((r >> 1) & 7)) << 4)) = bg_finish8<false>(rb[v], ok, 0.f, 0ull, 0ull);
      }
    }
  };
  auto compute = [&](int buf) {
    const unsigned char* Ab = lds + buf * STAGE;
    const unsigned char* Bb = Ab + A_BYTES;
#pragma unroll
    for (int kk = 0; kk < BG_BK / 32; ++kk) {
      bf16x8 af[MREP], bf[NREP];
#pragma unroll
      for (int m = 0; m < MREP; ++m) {
        const int r = wr * WROWS + m * 16 + li;
        const int sw = (r >> 1) & 7;
        if (B_KN) {
          // permuted-k convention of the transpose reads: lane group kg holds k = kg*4..+3 and 16 + kg*4..+3
          const int c0 = kk * 4 + (kg >> 1), hb = (kg & 1) * 8;
          const bf16x4 lo = *reinterpret_cast<const bf16x4*>(Ab + r * 128 + ((c0 ^ sw) << 4) + hb);
          const bf16x4 hi = *reinterpret_cast<const bf16x4*>(Ab + r * 128 + (((c0 + 2) ^ sw) << 4) + hb);
          af[m] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        } else {
          af[m] = *reinterpret_cast<const bf16x8*>(Ab + r * 128 + (((kk * 4 + kg) ^ sw) << 4));
        }
      }
#pragma unroll
      for (int n = 0; n < NREP; ++n) {
        const int c = wc * (NREP * 16) + n * 16;
        if (B_KN) {
          const __bf16* p = reinterpret_cast<const __bf16*>(Bb) + (kk * 32 + kg * 4 + (li >> 2)) * BG_LDKN + c + (li & 3) * 4;
          const bf16x4 lo = bg_tr4(p), hi = bg_tr4(p + 16 * BG_LDKN);
          bf[n] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        } else {
          const int r = c + li;
          bf[n] = *reinterpret_cast<const bf16x8*>(Bb + r * 128 + (((kk * 4 + kg) ^ ((r >> 1) & 7)) << 4));
        }
      }
#pragma unroll
      for (int m = 0; m < MREP; ++m)
#pragma unroll
        for (int n = 0; n < NREP; ++n)
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[m], bf[n], acc[m][n], 0, 0, 0);
    }
  };

  // tile t lives in register set t & 1 and LDS buffer t & 1.  A wave that reaches commit(buf) for tile t + 2 has
  // passed the barrier in front of compute(t + 1), which every wave reaches only after compute(t): one barrier per tile.
  fetch(ra0, rb0, fs0, fk0);
  fetch(ra1, rb1, fs1, fk1);
  for (int t = 0; t < ntile; t += 2) {
    commit(0, ra0, rb0, fs0, fk0);
    __syncthreads();
    fetch(ra0, rb0, fs0, fk0);
    compute(0);
    if (t + 1 < ntile) {
      commit(1, ra1, rb1, fs1, fk1);
      __syncthreads();
      fetch(ra1, rb1, fs1, fk1);
      compute(1);
    }
  }
  __syncthreads();

  // ---- epilogue: accumulators through LDS so that 16 lanes write one 256 / 512-byte output row piece
  float* Cs = reinterpret_cast<float*>(lds);
#pragma unroll
  for (int m = 0; m < MREP; ++m)
#pragma unroll
    for (int n = 0; n < NREP; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        Cs[(wr * WROWS + m * 16 + kg * 4 + r) * CLD + wc * (NREP * 16) + n * 16 + li] = acc[m][n][r];
  __syncthreads();

  const int jc = (tid & 15) * 8;  // 8 output columns per thread
  const int j = j0 + jc;
  if (j >= g.N) return;
  float bs[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) bs[e] = 0.f;
  if (g.bias) {
    const float4 b0 = *reinterpret_cast<const float4*>(g.bias + j), b1 = *reinterpret_cast<const float4*>(g.bias + j + 4);
    bs[0] = b0.x; bs[1] = b0.y; bs[2] = b0.z; bs[3] = b0.w; bs[4] = b1.x; bs[5] = b1.y; bs[6] = b1.z; bs[7] = b1.w;
  }
  if (g.bias2) {
    const float4 b0 = *reinterpret_cast<const float4*>(g.bias2 + j), b1 = *reinterpret_cast<const float4*>(g.bias2 + j + 4);
    bs[0] += b0.x; bs[1] += b0.y; bs[2] += b0.z; bs[3] += b0.w; bs[4] += b1.x; bs[5] += b1.y; bs[6] += b1.z; bs[7] += b1.w;
  }
  float lg[8], lb[8];
  if (g.ln_out) {  // N == 128: the 16 lanes that share a row hold all of it
    const float4 g0 = *reinterpret_cast<const float4*>(g.ln_gamma + j), g1 = *reinterpret_cast<const float4*>(g.ln_gamma + j + 4);
    const float4 b0 = *reinterpret_cast<const float4*>(g.ln_beta + j), b1 = *reinterpret_cast<const float4*>(g.ln_beta + j + 4);
    lg[0] = g0.x; lg[1] = g0.y; lg[2] = g0.z; lg[3] = g0.w; lg[4] = g1.x; lg[5] = g1.y; lg[6] = g1.z; lg[7] = g1.w;
    lb[0] = b0.x; lb[1] = b0.y; lb[2] = b0.z; lb[3] = b0.w; lb[4] = b1.x; lb[5] = b1.y; lb[6] = b1.z; lb[7] = b1.w;
  }
  float pg[8], pb[8];  // LNB: this thread's share of dgamma / dbeta (its 8 columns, its rows)
  if constexpr (LNB) {
    const float4 g0 = *reinterpret_cast<const float4*>(lnb->gamma + j), g1 = *reinterpret_cast<const float4*>(lnb->gamma + j + 4);
    lg[0] = g0.x; lg[1] = g0.y; lg[2] = g0.z; lg[3] = g0.w; lg[4] = g1.x; lg[5] = g1.y; lg[6] = g1.z; lg[7] = g1.w;
#pragma unroll
    for (int e = 0; e < 8; ++e) pg[e] = pb[e] = 0.f;
  }
#pragma unroll
  for (int v = 0; v < BM / 16; ++v) {
    const int rl = (tid >> 4) + 16 * v;
    // LNB: rows past the end go through the arithmetic as a copy of the last row (every lane takes part in the 16-lane
    // sums and reaches the barrier below); they store nothing and add nothing
    const bool live = i0 + rl < g.M;
    if (!LNB && !live) continue;
    const int i = LNB ? (live ? i0 + rl : g.M - 1) : i0 + rl;
    const float4 c0 = *reinterpret_cast<const float4*>(&Cs[rl * CLD + jc]);
    const float4 c1 = *reinterpret_cast<const float4*>(&Cs[rl * CLD + jc + 4]);
    float o[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float val = (o[e] + bs[e]) * g.alpha;
      if (g.relu) val = fmaxf(val, 0.f);
      o[e] = val;
    }
    if (g.drop_p > 0.f) {
      const uint64_t base = (uint64_t)i * (uint64_t)g.N + (uint64_t)j;  // N % 8 == 0, j % 8 == 0
      kantts_dropout_scale4(g.drop_p, g.drop_seed + seed_off, base, o);
      kantts_dropout_scale4(g.drop_p, g.drop_seed + seed_off, base + 4, o + 4);
    }
    if (g.res) {
      const float* rp = g.res + (long long)i * g.ldr + j;
      const float4 r0 = *reinterpret_cast<const float4*>(rp), r1 = *reinterpret_cast<const float4*>(rp + 4);
      o[0] += r0.x; o[1] += r0.y; o[2] += r0.z; o[3] += r0.w; o[4] += r1.x; o[5] += r1.y; o[6] += r1.z; o[7] += r1.w;
    }
    if (g.gate) {
      float gv[8];
      if (g.gate_bf16) {
        const u32x4 q = *reinterpret_cast<const u32x4*>(reinterpret_cast<const __bf16*>(g.gate) + (long long)i * g.ldg + j);
        gv[0] = kantts_bf16_lo(q.x); gv[1] = kantts_bf16_hi(q.x); gv[2] = kantts_bf16_lo(q.y); gv[3] = kantts_bf16_hi(q.y);
        gv[4] = kantts_bf16_lo(q.z); gv[5] = kantts_bf16_hi(q.z); gv[6] = kantts_bf16_lo(q.w); gv[7] = kantts_bf16_hi(q.w);
      } else {
        const float* gp = reinterpret_cast<const float*>(g.gate) + (long long)i * g.ldg + j;
        const float4 q0 = *reinterpret_cast<const float4*>(gp), q1 = *reinterpret_cast<const float4*>(gp + 4);
        gv[0] = q0.x; gv[1] = q0.y; gv[2] = q0.z; gv[3] = q0.w; gv[4] = q1.x; gv[5] = q1.y; gv[6] = q1.z; gv[7] = q1.w;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (gv[e] > 0.f) ? o[e] : 0.f;
    }
    if (g.rowmask && g.rowmask[i]) {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = 0.f;
    }
    if (!LNB || (g.c && live)) {
      if (g.c_bf16) {
        u32x4 w = {kantts_pack2_of4(o[0], o[1]), kantts_pack2_of4(o[2], o[3]), kantts_pack2_of4(o[4], o[5]), kantts_pack2_of4(o[6], o[7])};
        *reinterpret_cast<u32x4*>(reinterpret_cast<__bf16*>(g.c) + (long long)i * g.ldc + j) = w;
      } else {
        float* cp = reinterpret_cast<float*>(g.c) + (long long)i * g.ldc + j;
        f32x4 w0 = {o[0], o[1], o[2], o[3]}, w1 = {o[4], o[5], o[6], o[7]};
        *reinterpret_cast<f32x4*>(cp) = w0;
        *reinterpret_cast<f32x4*>(cp + 4) = w1;
      }
    }
    if constexpr (LNB) {  // same arithmetic, in the same order, as ln128_bwd_kernel (csrc/norm.hip) on dy = o
      if (g.c_bf16) {     // ... as the two-launch form hands it over: rounded to bf16
        const u32x4 w = {kantts_pack2_of4(o[0], o[1]), kantts_pack2_of4(o[2], o[3]), kantts_pack2_of4(o[4], o[5]), kantts_pack2_of4(o[6], o[7])};
        o[0] = kantts_bf16_lo(w.x); o[1] = kantts_bf16_hi(w.x); o[2] = kantts_bf16_lo(w.y); o[3] = kantts_bf16_hi(w.y);
        o[4] = kantts_bf16_lo(w.z); o[5] = kantts_bf16_hi(w.z); o[6] = kantts_bf16_lo(w.w); o[7] = kantts_bf16_hi(w.w);
      }
      const long long off = (long long)i * 128 + j;
      const float4 xa = *reinterpret_cast<const float4*>(lnb->x + off), xb = *reinterpret_cast<const float4*>(lnb->x + off + 4);
      const float xv[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
      const float mu = lnb->mean[i], rs = lnb->rstd[i];
      float xh[8], gg[8], s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        xh[e] = (xv[e] - mu) * rs;
        gg[e] = o[e] * lg[e];
        s1 += gg[e];
        s2 += gg[e] * xh[e];
        if (live) {
          pg[e] += o[e] * xh[e];
          pb[e] += o[e];
        }
      }
      s1 = bg_sum16(s1) * (1.f / 128.f);
      s2 = bg_sum16(s2) * (1.f / 128.f);
      float dxv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) dxv[e] = rs * (gg[e] - s1 - xh[e] * s2);
      if (lnb->dres) {
        const float4 ra = *reinterpret_cast<const float4*>(lnb->dres + off), rb = *reinterpret_cast<const float4*>(lnb->dres + off + 4);
        dxv[0] += ra.x; dxv[1] += ra.y; dxv[2] += ra.z; dxv[3] += ra.w; dxv[4] += rb.x; dxv[5] += rb.y; dxv[6] += rb.z; dxv[7] += rb.w;
      }
      if (lnb->zero_rows && lnb->zero_rows[i]) {
#pragma unroll
        for (int e = 0; e < 8; ++e) dxv[e] = 0.f;
      }
      if (live) {
        f32x4 w0 = {dxv[0], dxv[1], dxv[2], dxv[3]}, w1 = {dxv[4], dxv[5], dxv[6], dxv[7]};
        *reinterpret_cast<f32x4*>(lnb->dx + off) = w0;
        *reinterpret_cast<f32x4*>(lnb->dx + off + 4) = w1;
      }
    }
    if (g.ln_out) {  // same arithmetic, in the same order, as ln128_fwd_kernel (csrc/norm.hip)
      float sm = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) sm += o[e];
      const float mu = bg_sum16(sm) * (1.f / 128.f);
      float qq = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = o[e] - mu;
        qq += d * d;
      }
      const float rs = 1.0f / sqrtf(bg_sum16(qq) * (1.f / 128.f) + g.ln_eps);
      float y[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) y[e] = (o[e] - mu) * rs * lg[e] + lb[e];
      if (g.ln_out_bf16) {
        u32x4 w = {kantts_pack2_of4(y[0], y[1]), kantts_pack2_of4(y[2], y[3]), kantts_pack2_of4(y[4], y[5]), kantts_pack2_of4(y[6], y[7])};
        *reinterpret_cast<u32x4*>(reinterpret_cast<__bf16*>(g.ln_out) + (long long)i * 128 + j) = w;
      } else {
        float* yp = reinterpret_cast<float*>(g.ln_out) + (long long)i * 128 + j;
        f32x4 w0 = {y[0], y[1], y[2], y[3]}, w1 = {y[4], y[5], y[6], y[7]};
        *reinterpret_cast<f32x4*>(yp) = w0;
        *reinterpret_cast<f32x4*>(yp + 4) = w1;
      }
      if ((tid & 15) == 0) {
        g.ln_mean[i] = mu;
        g.ln_rstd[i] = rs;
      }
    }
  }
  if constexpr (LNB) {  // N == 128 == BG_BN: nobody left above.  Partials of the 16 row groups through LDS (the C tile is
    __syncthreads();    // dead), then 256 atomics per workgroup, as ln128_bwd_kernel
    float* red = reinterpret_cast<float*>(lds);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      red[(tid >> 4) * 128 + jc + e] = pg[e];
      red[2048 + (tid >> 4) * 128 + jc + e] = pb[e];
    }
    __syncthreads();
    const int which = tid >> 7, c = tid & 127;
    float a = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) a += red[which * 2048 + w * 128 + c];
    if (lnb->part_rows)  // [round 5] this workgroup's row of [dgamma | dbeta] partial sums: the caller adds the rows
      lnb->part_rows[(long long)blockIdx.y * 256 + which * 128 + c] = a;
    else if (a != 0.f)
      atomicAdd(which ? &lnb->dbeta_accum[c] : &lnb->dgamma_accum[c], a);
  }
