// The MFMA tile loop of sconv_kernel (csrc/sconv.hip) and sconv_sym_kernel (csrc/sconv_sym.hip), included once inside each
// kernel definition behind its prologue: the two kernels run the SAME text -- same tiles, same MFMA path in both precisions,
// same chunk-major, tap-inner summation order.  Textual inclusion, not a function: handing the kernel arguments and the
// accumulators to an inlined device function changed the code of every instantiation (csrc/gemm_bf16_nt_body.inc), and so
// does another order of the declarations below, or declaring what the kernels declare (W, ncol0, wave_live) in here.
// Expects in scope: the template parameters BF16, WM, MREP, NFR; `g` with the fields w, N, Cin, K, step, in_act, in_slope;
// s, tid, lane, wm, H, W (= rows + H window rows), rows, ncol0, wave_live; sconv_lds_raw, the dynamic LDS array (W * LDW
// elements of the operand type); and two macros, which the end of this file undefines:
//   SCONV_WINDOW_ROW(r)  the pointer to window row r of slot s, a row of X = [hist ; in];
//   SCONV_ROW_LOADED(r)  whether window row r is loaded (otherwise it counts as zeros).
// Leaves, in the waves that have something to store (the others return), acc[MREP][NFR] in the MFMA layout: lane holds rows
// 4 * (lane / 16) .. + 3 of column lane % 16 of each fragment.
  constexpr int CKS = BF16 ? 128 : 64;           // channels per window slab
  constexpr int LDW = BF16 ? CKS + 8 : CKS + 4;  // row pitch in elements: 16 consecutive rows hit distinct bank groups
  constexpr int PF = (BF16 ? 16 : 4) / NFR;      // (chunk, tap) iterations of weight fragments in flight ahead of the MFMAs

  // window row of fragment f's MFMA row for tap 0 (rows past the tile's end are clamped: computed, never stored)
  int arow0[MREP];
#pragma unroll
  for (int f = 0; f < MREP; ++f) arow0[f] = min(wm * (MREP * 16) + f * 16 + (lane & 15), rows - 1) + H;

  f32x4 acc[MREP][NFR];
#pragma unroll
  for (int f = 0; f < MREP; ++f)
#pragma unroll
    for (int j = 0; j < NFR; ++j) acc[f][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nch = (g.Cin + 31) >> 5;  // 32-channel MFMA chunks
  const int total = nch * g.K;        // (chunk, tap) iterations, chunk-major
  const int kg8 = (lane >> 4) * 8;    // this lane's 8 channels inside a chunk

  // Weight fragments, PF (chunk, tap) iterations ahead.  No lane-dependent select follows a load (it would make the wave
  // wait for the load where it is issued): out-of-range lanes read a CLAMPED, valid address instead -- a column n >= N is
  // never stored, and channels >= Cin meet the zeros the window holds there (weights are finite).
  sconv_bfrag<BF16> bcur[PF][NFR], bnext[PF][NFR];
  int fch = 0, fj = 0;  // fetch cursor (chunk, tap); runs up to PF iterations past the end, clamped
  long long ncl[NFR];
#pragma unroll
  for (int nf = 0; nf < NFR; ++nf) ncl[nf] = (long long)min(ncol0 + nf * 16 + (lane & 15), g.N - 1) * g.Cin;
  auto fetch_b = [&](sconv_bfrag<BF16> (&dst)[PF][NFR]) {
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      if (wave_live) {
        const long long o0 = (long long)fj * g.N * g.Cin + min(fch * 32 + kg8, g.Cin - 8);
#pragma unroll
        for (int nf = 0; nf < NFR; ++nf) {
          if constexpr (BF16) {
            dst[u][nf].v = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const __bf16*>(g.w) + o0 + ncl[nf]);
          } else {
            const float* wp = reinterpret_cast<const float*>(g.w) + o0 + ncl[nf];
            dst[u][nf].lo = *reinterpret_cast<const float4*>(wp);
            dst[u][nf].hi = *reinterpret_cast<const float4*>(wp + 4);
          }
        }
      }
      if (++fj == g.K) fj = 0, ++fch;
    }
  };

  int ch = 0, j = -1;  // compute cursor
  fetch_b(bnext);
  for (int it0 = 0; it0 < total; it0 += PF) {
#pragma unroll
    for (int u = 0; u < PF; ++u)
#pragma unroll
      for (int nf = 0; nf < NFR; ++nf) bcur[u][nf] = bnext[u][nf];
    fetch_b(bnext);
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      if (it0 + u >= total) continue;  // workgroup-uniform
      if (++j == g.K) j = 0, ++ch;
      const int cl = (ch * 32) % CKS;  // chunk's first column inside the slab
      if (j == 0 && cl == 0) {
        // ---- stage the slab: W rows x ncols channels of X, activated and rounded, 4 float4 in flight per thread
        const int cbase = ch * 32;
        const int ncols = min(CKS, ((g.Cin - cbase + 31) >> 5) << 5);  // multiple of 32; columns >= Cin are zeros
        const int c4n = ncols >> 2;
        const int nvec = W * c4n;
        __syncthreads();  // every wave is done with the previous slab
        for (int i0 = tid; i0 < nvec; i0 += SCONV_THREADS * 4) {
          float4 xv[4];
          int row[4], col[4];
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int i = i0 + v * SCONV_THREADS;
            row[v] = i / c4n;
            col[v] = (i - row[v] * c4n) * 4;
            const bool ok = i < nvec && cbase + col[v] < g.Cin && SCONV_ROW_LOADED(row[v]);
            xv[v] = ok ? *reinterpret_cast<const float4*>(SCONV_WINDOW_ROW(row[v]) + cbase + col[v])
                       : make_float4(0.f, 0.f, 0.f, 0.f);
          }
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            if (i0 + v * SCONV_THREADS >= nvec) continue;
            const float v0 = sconv_leaky(xv[v].x, g.in_act, g.in_slope), v1 = sconv_leaky(xv[v].y, g.in_act, g.in_slope);
            const float v2 = sconv_leaky(xv[v].z, g.in_act, g.in_slope), v3 = sconv_leaky(xv[v].w, g.in_act, g.in_slope);
            const int o = row[v] * LDW + col[v];
            if constexpr (BF16) {
              bf16x4 p = {(__bf16)v0, (__bf16)v1, (__bf16)v2, (__bf16)v3};
              *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(sconv_lds_raw) + o) = p;
            } else {
              *reinterpret_cast<float4*>(reinterpret_cast<float*>(sconv_lds_raw) + o) = make_float4(v0, v1, v2, v3);
            }
          }
        }
        __syncthreads();
      }
      if (!wave_live) continue;
      const int back = j * g.step;
      if constexpr (BF16) {
        const __bf16* Wh = reinterpret_cast<const __bf16*>(sconv_lds_raw);
        bf16x8 af[MREP];
#pragma unroll
        for (int f = 0; f < MREP; ++f)
          af[f] = *reinterpret_cast<const bf16x8*>(&Wh[(arow0[f] - back) * LDW + cl + kg8]);
#pragma unroll
        for (int f = 0; f < MREP; ++f)
#pragma unroll
          for (int nf = 0; nf < NFR; ++nf)
            acc[f][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[f], bcur[u][nf].v,
                                                                 acc[f][nf], 0, 0, 0);
      } else {
        const float* Wf = reinterpret_cast<const float*>(sconv_lds_raw);
        float a8[MREP][8];
#pragma unroll
        for (int f = 0; f < MREP; ++f) {
          const float* ap = &Wf[(arow0[f] - back) * LDW + cl + kg8];
          const float4 lo = *reinterpret_cast<const float4*>(ap), hi = *reinterpret_cast<const float4*>(ap + 4);
          a8[f][0] = lo.x, a8[f][1] = lo.y, a8[f][2] = lo.z, a8[f][3] = lo.w;
          a8[f][4] = hi.x, a8[f][5] = hi.y, a8[f][6] = hi.z, a8[f][7] = hi.w;
        }
        // k-step e contracts channel kg8 + e of every lane group: A and B agree, so the order inside a chunk is free
#pragma unroll
        for (int e = 0; e < 8; ++e)
#pragma unroll
          for (int nf = 0; nf < NFR; ++nf) {
            const sconv_bfrag<false>& b = bcur[u][nf];
            const float bv = e == 0 ? b.lo.x : e == 1 ? b.lo.y : e == 2 ? b.lo.z : e == 3 ? b.lo.w
                           : e == 4 ? b.hi.x : e == 5 ? b.hi.y : e == 6 ? b.hi.z : b.hi.w;
#pragma unroll
            for (int f = 0; f < MREP; ++f)
              acc[f][nf] = __builtin_amdgcn_mfma_f32_16x16x4f32(a8[f][e], bv, acc[f][nf], 0, 0, 0);
          }
      }
    }
  }
  if (!wave_live) return;
#undef SCONV_WINDOW_ROW
#undef SCONV_ROW_LOADED
