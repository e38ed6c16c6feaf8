// Speaker-embedding extractor for SE voices: Kaldi fbank and the inference graph of the D-TDNN (CAM++ style dense TDNN with
// a 2-D ResNet head) over a RAGGED batch.  The reference (kantts/preprocess/se_processor) runs one wav at a time through
// 52 dense layers that each end in a torch.cat of the growing block; here a block owns one (B, C_end, T) buffer, a layer
// reads channels [0, C_i) and writes its growth_rate channels in place, and a layer is two launches:
//   (a) spk_conv1d_kernel: h = relu(bn2(W1 . relu(bn1(x)))) with the per-tile channel sums and per-segment maxima of h as
//       its epilogue (plain vector stores of per-workgroup partials -- no atomics, equal bits on every run);
//   (b) spk_cam_kernel: the consumer adds the partials up in ascending tile order, forms the gate of every 100-frame
//       segment it touches and multiplies it into the dilated k = 3 convolution, stored into the block buffer's slice.
// The same (a) kernel is the TDNN (k = 5, stride 2) and the transit layers (k = 1); the head is one generic 3 x 3 launch,
// the pooling + embedding one launch.  Every kernel takes the items' own lengths: a tap at or past an item's end is zero
// AFTER the folded BatchNorm + ReLU of the input, which is what the reference's zero padding means for a lone item.
//
// Everything is fp32 on the VALU (an embedding is compared by cosine distance; nobody has measured what bf16 does to it).
// Contract: include/kantts_hip.h.
#include "common.h"

#include <float.h>
#include <math.h>

#define SPK_THREADS 256
#define SPK_SEG 100  // frames per pooled segment (the reference's seg_len)
#define SPK_TN 64    // columns (frames) per workgroup tile of the 1-D kernels

// ---------------------------------------------------------------------------------------------------------------------
// Kaldi fbank.  One workgroup per (frame, item): 400 samples -> DC removal -> pre-emphasis -> window -> 512-point radix-2
// FFT in LDS -> power -> banded mel filters -> log.
#define FB_WIN 400
#define FB_HOP 160
#define FB_FFT 512

__device__ __forceinline__ int fb_frames(int n, int tmax) {
  const int t = n < FB_WIN ? 0 : 1 + (n - FB_WIN) / FB_HOP;
  return t < tmax ? t : tmax;
}

__global__ __launch_bounds__(SPK_THREADS) void spk_fbank_kernel(const float* __restrict__ wav, const int* __restrict__ nsamp,
                                                                const float* __restrict__ window,
                                                                const float* __restrict__ tw, const int* __restrict__ mel_lo,
                                                                const int* __restrict__ mel_n,
                                                                const float* __restrict__ mel_w, float* __restrict__ out,
                                                                int ld, int Tmax, int nmel, int wmax) {
  __shared__ float sx[FB_WIN];
  __shared__ float sre[FB_FFT], sim[FB_FFT];
  __shared__ float pw[FB_FFT / 2 + 1];
  __shared__ float red[SPK_THREADS / KANTTS_WAVE];
  const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int n = min(nsamp[b], ld);
  float* o = out + ((long long)b * Tmax + f) * nmel;
  if (f >= fb_frames(n, Tmax)) {  // uniform over the workgroup
    if (tid < nmel) o[tid] = 0.f;
    return;
  }
  const float* x = wav + (long long)b * ld + (long long)f * FB_HOP;  // f * 160 + 399 <= n - 1
  const float v0 = x[tid], v1 = tid + 256 < FB_WIN ? x[tid + 256] : 0.f;
  const float mean = kantts_block_sum(v0 + v1, red) * (1.0f / FB_WIN);
  sx[tid] = v0 - mean;
  if (tid + 256 < FB_WIN) sx[tid + 256] = v1 - mean;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int i = tid + 256 * r;
    float v = 0.f;
    if (i < FB_WIN) v = (sx[i] - 0.97f * sx[i > 0 ? i - 1 : 0]) * window[i];
    int rev = 0;
#pragma unroll
    for (int q = 0; q < 9; ++q) rev |= ((i >> q) & 1) << (8 - q);
    sre[rev] = v;
    sim[rev] = 0.f;
  }
  __syncthreads();
#pragma unroll 1
  for (int s = 1; s <= 9; ++s) {  // decimation in time; one butterfly per thread and stage
    const int half = 1 << (s - 1);
    const int j = tid & (half - 1);
    const int i0 = ((tid >> (s - 1)) << s) + j, i1 = i0 + half;
    const int k = j << (9 - s);
    const float c = tw[k], sn = -tw[256 + k];  // e^{-2 pi i k / 512}
    const float br = sre[i1], bi = sim[i1];
    const float tr = br * c - bi * sn, ti = br * sn + bi * c;
    const float ar = sre[i0], ai = sim[i0];
    sre[i0] = ar + tr;
    sim[i0] = ai + ti;
    sre[i1] = ar - tr;
    sim[i1] = ai - ti;
    __syncthreads();
  }
  pw[tid] = sre[tid] * sre[tid] + sim[tid] * sim[tid];
  if (tid == 0) pw[256] = sre[256] * sre[256] + sim[256] * sim[256];
  __syncthreads();
  if (tid < nmel) {
    const int lo = min(max(mel_lo[tid], 0), FB_FFT / 2), cnt = min(min(mel_n[tid], wmax), FB_FFT / 2 + 1 - lo);
    const float* wr = mel_w + (long long)tid * wmax;
    float s = 0.f;
    for (int j = 0; j < cnt; ++j) s = fmaf(wr[j], pw[lo + j], s);
    o[tid] = logf(fmaxf(s, FLT_EPSILON));
  }
}

// per-utterance mean subtraction: a workgroup per item, a thread per mel bin, the item's own frames in ascending order
__global__ __launch_bounds__(128) void spk_cmn_kernel(const int* __restrict__ nsamp, float* __restrict__ out, int ld, int Tmax,
                                                       int nmel) {
  const int b = blockIdx.x, m = threadIdx.x;
  if (m >= nmel) return;
  const int T = fb_frames(min(nsamp[b], ld), Tmax);
  if (T < 1) return;
  float* o = out + (long long)b * Tmax * nmel + m;
  float s = 0.f;
  for (int t = 0; t < T; ++t) s += o[(long long)t * nmel];
  const float mean = s / (float)T;
  for (int t = 0; t < T; ++t) o[(long long)t * nmel] -= mean;
}

// ---------------------------------------------------------------------------------------------------------------------
// Head: 3 x 3 convolution over (F, T), stride (sf, 1), folded BN, optional residual (identity or 1 x 1 strided shortcut),
// ReLU.  A workgroup owns (item, output row fo, 64 frames); a wave owns 8 output channels, a lane one frame, so the weights
// are wave-uniform and the three input rows (+ one frame of halo either side) are staged in LDS once for all channels.
#define C2_MAXCIN 32
#define C2_NCO 8
#define C2_W (SPK_TN + 2)

struct SpkConv2dArgs {
  const float *in, *w, *scale, *shift, *res, *sc_w, *sc_scale, *sc_shift;
  const int* lens;
  float* out;
  long long in_sb, in_sc, in_sf, in_st;
  int Cin, Cout, Fin, Fout, T, sf, Cres, Fres, rsf;
};

__global__ __launch_bounds__(SPK_THREADS) void spk_conv2d_kernel(const SpkConv2dArgs a) {
  __shared__ float sx[C2_MAXCIN * 3 * C2_W];
  const int t0 = blockIdx.x * SPK_TN, fo = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const int lane = tid & 63, co0 = __builtin_amdgcn_readfirstlane(tid >> 6) * C2_NCO;
  const int len = min(a.lens[b], a.T), t = t0 + lane;
  float* ob = a.out + (((long long)b * a.Cout + co0) * a.Fout + fo) * a.T;
  const long long ostep = (long long)a.Fout * a.T;
  if (t0 >= len) {  // uniform over the workgroup: the whole tile is padding
    if (t < a.T)
      for (int u = 0; u < C2_NCO; ++u) ob[u * ostep + t] = 0.f;
    return;
  }
  const float* ib = a.in + (long long)b * a.in_sb;
  for (int i = tid; i < a.Cin * 3 * C2_W; i += blockDim.x) {
    const int j = i % C2_W, r = (i / C2_W) % 3, ci = i / (3 * C2_W);
    const int fi = fo * a.sf - 1 + r, ti = t0 - 1 + j;
    float v = 0.f;
    if (fi >= 0 && fi < a.Fin && ti >= 0 && ti < len) v = ib[ci * a.in_sc + fi * a.in_sf + ti * a.in_st];
    sx[i] = v;
  }
  __syncthreads();
  float acc[C2_NCO];
#pragma unroll
  for (int u = 0; u < C2_NCO; ++u) acc[u] = 0.f;
  const float* wb = a.w + (long long)co0 * a.Cin * 9;
  for (int ci = 0; ci < a.Cin; ++ci) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float v = sx[(ci * 3 + r) * C2_W + lane + k];
#pragma unroll
        for (int u = 0; u < C2_NCO; ++u) acc[u] = fmaf(wb[(u * a.Cin + ci) * 9 + r * 3 + k], v, acc[u]);
      }
    }
  }
  if (t >= a.T) return;
  const bool valid = t < len;
#pragma unroll
  for (int u = 0; u < C2_NCO; ++u) {
    const int co = co0 + u;
    float y = acc[u] * a.scale[co] + a.shift[co];
    if (a.res && valid) {
      if (a.sc_w) {
        const float* rb = a.res + ((long long)b * a.Cres * a.Fres + (long long)fo * a.rsf) * a.T + t;
        float s = 0.f;
        for (int ci = 0; ci < a.Cres; ++ci) s = fmaf(a.sc_w[co * a.Cres + ci], rb[(long long)ci * a.Fres * a.T], s);
        y += s * a.sc_scale[co] + a.sc_shift[co];
      } else {
        y += a.res[(((long long)b * a.Cres + co) * a.Fres + fo) * a.T + t];
      }
    }
    ob[u * ostep + t] = valid ? fmaxf(y, 0.f) : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// 1-D convolution as a tiled GEMM: 64 output channels x 64 frames per workgroup, 4 x 4 per thread, the contraction index
// kk = ci * K + k walked in chunks of 16 through LDS.  Folded BN + ReLU on the way in (pre) and on the way out (post);
// the CAM epilogue (psum / pmax) reduces the tile's columns in a fixed order.
#define C1_BM 64
#define C1_BK 16

struct SpkConv1dArgs {
  const float *x, *w, *pre_scale, *pre_shift, *post_scale, *post_shift;
  const int* lens;
  float *y, *psum, *pmax;
  int Cin, CX, TX, Cout, CY, TY, co_off, K, stride, dil, NT;
};

__global__ __launch_bounds__(SPK_THREADS) void spk_conv1d_kernel(const SpkConv1dArgs a) {
  __shared__ float As[C1_BK][C1_BM + 4];
  __shared__ float Bs[C1_BK][SPK_TN + 4];
  __shared__ float rs[C1_BM][17], r0[C1_BM][17], r1[C1_BM][17];
  const int n0 = blockIdx.x * SPK_TN, m0 = blockIdx.y * C1_BM, b = blockIdx.z, tid = threadIdx.x;
  const int len_in = min(a.lens[b], a.TX);
  const int len_out = len_in < 1 ? 0 : min((len_in - 1) / a.stride + 1, a.TY);
  if (n0 >= len_out) return;  // uniform over the workgroup
  const int tx = tid & 15, ty = tid >> 4;
  const int Ktot = a.Cin * a.K, half = a.K / 2;
  const float* xb = a.x + (long long)b * a.CX * a.TX;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (int kk0 = 0; kk0 < Ktot; kk0 += C1_BK) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int idx = tid + r * SPK_THREADS;
      {  // weights: (m, kk), kk fastest (contiguous in memory)
        const int kk = idx & 15, m = idx >> 4;
        float v = 0.f;
        if (m0 + m < a.Cout && kk0 + kk < Ktot) v = a.w[(long long)(m0 + m) * Ktot + kk0 + kk];
        As[kk][m] = v;
      }
      {  // activations: (kk, n), n fastest
        const int nn = idx & 63, kk = idx >> 6;
        float v = 0.f;
        if (kk0 + kk < Ktot) {
          const int ci = (kk0 + kk) / a.K, k = (kk0 + kk) - ci * a.K;
          const int ti = (n0 + nn) * a.stride + (k - half) * a.dil;
          if (ti >= 0 && ti < len_in) {
            v = xb[(long long)ci * a.TX + ti];
            if (a.pre_scale) v = fmaxf(v * a.pre_scale[ci] + a.pre_shift[ci], 0.f);
          }
        }
        Bs[kk][nn] = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < C1_BK; ++kk) {
      float av[4], bv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) av[i] = As[kk][ty * 4 + i];
#pragma unroll
      for (int j = 0; j < 4; ++j) bv[j] = Bs[kk][tx * 4 + j];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
    }
    __syncthreads();
  }
  const int seg0 = n0 / SPK_SEG;
  float* yb = a.y + ((long long)b * a.CY + a.co_off) * a.TY;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int co = m0 + ty * 4 + i;
    float s = 0.f, mx0 = -FLT_MAX, mx1 = -FLT_MAX;
    if (co < a.Cout) {
      const float ps = a.post_scale ? a.post_scale[co] : 1.f, pb = a.post_scale ? a.post_shift[co] : 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int t = n0 + tx * 4 + j;
        float v = acc[i][j];
        if (a.post_scale) v = fmaxf(v * ps + pb, 0.f);
        if (t < len_out) {
          yb[(long long)co * a.TY + t] = v;
          s += v;
          if (t / SPK_SEG == seg0) mx0 = fmaxf(mx0, v);
          else mx1 = fmaxf(mx1, v);
        }
      }
    }
    rs[ty * 4 + i][tx] = s;
    r0[ty * 4 + i][tx] = mx0;
    r1[ty * 4 + i][tx] = mx1;
  }
  if (!a.psum) return;  // uniform
  __syncthreads();
  if (tid < C1_BM && m0 + tid < a.Cout) {
    float s = 0.f, mx0 = -FLT_MAX, mx1 = -FLT_MAX;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      s += rs[tid][q];
      mx0 = fmaxf(mx0, r0[tid][q]);
      mx1 = fmaxf(mx1, r1[tid][q]);
    }
    const long long tile = (long long)b * a.NT + blockIdx.x;
    a.psum[tile * a.Cout + m0 + tid] = s;
    a.pmax[(tile * 2 + 0) * a.Cout + m0 + tid] = mx0;
    a.pmax[(tile * 2 + 1) * a.Cout + m0 + tid] = mx1;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// CAM gate + dilated k = 3 convolution.  A workgroup owns (item, 64 frames): it stages the h tile (+ dil frames of halo),
// reduces the producer's partials for the one or two 100-frame segments the tile touches, runs the two tiny gate matrices
// and multiplies the gate into the convolution.  Wave w owns NCO = G / 4 output channels, a lane one frame.
#define CAM_MAXCB 128
#define CAM_MAXCH 64
#define CAM_MAXG 64
#define CAM_MAXDIL 4
#define CAM_W (SPK_TN + 2 * CAM_MAXDIL)

struct SpkCamArgs {
  const float *h, *psum, *pmax, *wa, *ba, *wb, *bb, *w;
  const int* lens;
  float* y;
  int Cb, TH, Ch, G, CY, TY, co_off, dil, NT;
};

template <int NCO>
__global__ __launch_bounds__(SPK_THREADS) void spk_cam_kernel(const SpkCamArgs a) {
  __shared__ float sh[CAM_MAXCB * CAM_W];
  __shared__ float ctx[2][CAM_MAXCB], hid[2][CAM_MAXCH], gate[2][CAM_MAXG];
  const int n0 = blockIdx.x * SPK_TN, b = blockIdx.y, tid = threadIdx.x;
  const int len = min(min(a.lens[b], a.TH), a.TY);
  if (n0 >= len) return;  // uniform over the workgroup
  const int lane = tid & 63, co0 = __builtin_amdgcn_readfirstlane(tid >> 6) * NCO;
  const int W = SPK_TN + 2 * a.dil;
  const float* hb = a.h + (long long)b * a.Cb * a.TH;
  for (int i = tid; i < a.Cb * W; i += SPK_THREADS) {
    const int c = i / W, j = i - c * W;
    const int ti = n0 - a.dil + j;
    sh[c * CAM_W + j] = (ti >= 0 && ti < len) ? hb[(long long)c * a.TH + ti] : 0.f;
  }
  const int seg0 = n0 / SPK_SEG, ntb = (len + SPK_TN - 1) / SPK_TN;
  for (int i = tid; i < 2 * a.Cb; i += SPK_THREADS) {
    const int slot = i / a.Cb, c = i - slot * a.Cb, seg = seg0 + slot;
    float s = 0.f, mx = -FLT_MAX;
    for (int q = 0; q < ntb; ++q) {  // ascending tile order: the same bits on every run and in every batch
      const long long tile = (long long)b * a.NT + q;
      s += a.psum[tile * a.Cb + c];
      const int sq = q * SPK_TN / SPK_SEG;
      if (sq == seg) mx = fmaxf(mx, a.pmax[(tile * 2 + 0) * a.Cb + c]);
      if (sq + 1 == seg) mx = fmaxf(mx, a.pmax[(tile * 2 + 1) * a.Cb + c]);
    }
    ctx[slot][c] = seg * SPK_SEG < len ? s / (float)len + mx : 0.f;
  }
  __syncthreads();
  for (int i = tid; i < 2 * a.Ch; i += SPK_THREADS) {
    const int slot = i / a.Ch, j = i - slot * a.Ch;
    const float* wr = a.wa + (long long)j * a.Cb;
    float s = a.ba[j];
    for (int c = 0; c < a.Cb; ++c) s = fmaf(wr[c], ctx[slot][c], s);
    hid[slot][j] = fmaxf(s, 0.f);
  }
  __syncthreads();
  for (int i = tid; i < 2 * a.G; i += SPK_THREADS) {
    const int slot = i / a.G, o = i - slot * a.G;
    const float* wr = a.wb + (long long)o * a.Ch;
    float s = a.bb[o];
    for (int j = 0; j < a.Ch; ++j) s = fmaf(wr[j], hid[slot][j], s);
    gate[slot][o] = 1.f / (1.f + expf(-s));
  }
  __syncthreads();
  float acc[NCO];
#pragma unroll
  for (int u = 0; u < NCO; ++u) acc[u] = 0.f;
  const float* wv = a.w + (long long)co0 * a.Cb * 3;
  for (int c = 0; c < a.Cb; ++c) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float v = sh[c * CAM_W + lane + k * a.dil];
#pragma unroll
      for (int u = 0; u < NCO; ++u) acc[u] = fmaf(wv[(u * a.Cb + c) * 3 + k], v, acc[u]);
    }
  }
  const int t = n0 + lane;
  if (t >= len) return;
  const int slot = t / SPK_SEG - seg0;
  float* yb = a.y + ((long long)b * a.CY + a.co_off + co0) * a.TY + t;
#pragma unroll
  for (int u = 0; u < NCO; ++u) yb[(long long)u * a.TY] = acc[u] * gate[slot][co0 + u];
}

// ---------------------------------------------------------------------------------------------------------------------
// Tail: folded BN + ReLU, mean and unbiased std over the item's frames, 1 x 1 dense, affine-free BN.  A workgroup per item;
// a wave per channel (lanes along the frames), then a wave per embedding dimension (lanes along the 2 C statistics).
#define TAIL_MAXC 1024

__global__ __launch_bounds__(SPK_THREADS) void spk_tail_kernel(const float* __restrict__ x, const int* __restrict__ lens,
                                                               const float* __restrict__ scale, const float* __restrict__ shift,
                                                               const float* __restrict__ w, const float* __restrict__ oscale,
                                                               const float* __restrict__ oshift, float* __restrict__ out, int C,
                                                               int CX, int TX, int E) {
  __shared__ float st[2 * TAIL_MAXC];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int len = min(lens[b], TX);
  const float* xb = x + (long long)b * CX * TX;
  for (int c = wv; c < C; c += SPK_THREADS / KANTTS_WAVE) {
    const float sc = scale[c], sf = shift[c];
    const float* xr = xb + (long long)c * TX;
    float s = 0.f;
    for (int t = lane; t < len; t += 64) s += fmaxf(xr[t] * sc + sf, 0.f);
    const float mean = kantts_wave_sum(s) / (float)len;
    float q = 0.f;
    for (int t = lane; t < len; t += 64) {
      const float d = fmaxf(xr[t] * sc + sf, 0.f) - mean;
      q = fmaf(d, d, q);
    }
    q = kantts_wave_sum(q);
    if (lane == 0) {
      st[c] = mean;
      st[C + c] = sqrtf(q / (float)(len - 1));
    }
  }
  __syncthreads();
  for (int e = wv; e < E; e += SPK_THREADS / KANTTS_WAVE) {
    const float* wr = w + (long long)e * 2 * C;
    float s = 0.f;
    for (int j = lane; j < 2 * C; j += 64) s = fmaf(wr[j], st[j], s);
    s = kantts_wave_sum(s);
    if (lane == 0) out[(long long)b * E + e] = s * oscale[e] + oshift[e];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
extern "C" int kantts_kaldi_fbank(const float* wav, const int32_t* nsamp, const float* window, const float* tw,
                                  const int32_t* mel_lo, const int32_t* mel_n, const float* mel_w, float* out, int B, int ld,
                                  int Tmax, int nmel, int wmax, int cmn, void* stream) {
  if (!wav || !nsamp || !window || !tw || !mel_lo || !mel_n || !mel_w || !out || B < 1 || ld < 1 || Tmax < 1 || nmel < 1 ||
      wmax < 1)
    return KANTTS_E_BADARG;
  if (nmel > 128 || B > 65535) return KANTTS_E_UNSUPPORTED;
  hipLaunchKernelGGL(spk_fbank_kernel, dim3(Tmax, B), dim3(SPK_THREADS), 0, (hipStream_t)stream, wav,
                     reinterpret_cast<const int*>(nsamp), window, tw, reinterpret_cast<const int*>(mel_lo),
                     reinterpret_cast<const int*>(mel_n), mel_w, out, ld, Tmax, nmel, wmax);
  if (cmn)
    hipLaunchKernelGGL(spk_cmn_kernel, dim3(B), dim3(128), 0, (hipStream_t)stream, reinterpret_cast<const int*>(nsamp), out, ld,
                       Tmax, nmel);
  KANTTS_CHECK_LAUNCH();
}

extern "C" int kantts_spk_conv2d(const float* in, long long in_sb, long long in_sc, long long in_sf, long long in_st,
                                 const float* w, const float* scale, const float* shift, const float* res, const float* sc_w,
                                 const float* sc_scale, const float* sc_shift, const int32_t* lens, float* out, int B, int Cin,
                                 int Cout, int Fin, int T, int sf, int Cres, int Fres, int rsf, void* stream) {
  if (!in || !w || !scale || !shift || !lens || !out || B < 1 || Cin < 1 || Cout < 1 || Fin < 1 || T < 1 || sf < 1)
    return KANTTS_E_BADARG;
  const int Fout = (Fin - 1) / sf + 1;
  if (res) {
    if (Cres < 1 || Fres < 1 || rsf < 1) return KANTTS_E_BADARG;
    if (sc_w ? (!sc_scale || !sc_shift || (long long)(Fout - 1) * rsf >= Fres) : (Cres != Cout || Fres != Fout))
      return KANTTS_E_BADARG;
  }
  if (Cin > C2_MAXCIN || Cout % C2_NCO || Cout > C2_NCO * (SPK_THREADS / 64) || B > 65535 || Fout > 65535)
    return KANTTS_E_UNSUPPORTED;
  SpkConv2dArgs a;
  a.in = in, a.w = w, a.scale = scale, a.shift = shift, a.res = res, a.sc_w = sc_w, a.sc_scale = sc_scale;
  a.sc_shift = sc_shift, a.lens = reinterpret_cast<const int*>(lens), a.out = out;
  a.in_sb = in_sb, a.in_sc = in_sc, a.in_sf = in_sf, a.in_st = in_st;
  a.Cin = Cin, a.Cout = Cout, a.Fin = Fin, a.Fout = Fout, a.T = T, a.sf = sf, a.Cres = Cres, a.Fres = Fres, a.rsf = rsf;
  hipLaunchKernelGGL(spk_conv2d_kernel, dim3(kantts_cdiv(T, SPK_TN), Fout, B), dim3(64 * (Cout / C2_NCO)), 0,
                     (hipStream_t)stream, a);
  KANTTS_CHECK_LAUNCH();
}

extern "C" int kantts_spk_conv1d(const float* x, const int32_t* lens, const float* w, const float* pre_scale,
                                 const float* pre_shift, const float* post_scale, const float* post_shift, float* y,
                                 float* psum, float* pmax, int B, int Cin, int CX, int TX, int Cout, int CY, int TY, int co_off,
                                 int K, int stride, int dil, int max_out, void* stream) {
  if (!x || !lens || !w || !y || B < 1 || Cin < 1 || CX < Cin || TX < 1 || Cout < 1 || co_off < 0 || CY < co_off + Cout ||
      TY < 1 || K < 1 || !(K & 1) || stride < 1 || dil < 1 || max_out < 1 || max_out > TY)
    return KANTTS_E_BADARG;
  if ((pre_scale && !pre_shift) || (post_scale && !post_shift) || (!psum != !pmax) || (psum && stride != 1))
    return KANTTS_E_BADARG;
  if (B > 65535 || kantts_cdiv(Cout, C1_BM) > 65535) return KANTTS_E_UNSUPPORTED;
  SpkConv1dArgs a;
  a.x = x, a.w = w, a.pre_scale = pre_scale, a.pre_shift = pre_shift, a.post_scale = post_scale, a.post_shift = post_shift;
  a.lens = reinterpret_cast<const int*>(lens), a.y = y, a.psum = psum, a.pmax = pmax;
  a.Cin = Cin, a.CX = CX, a.TX = TX, a.Cout = Cout, a.CY = CY, a.TY = TY, a.co_off = co_off, a.K = K, a.stride = stride;
  a.dil = dil, a.NT = kantts_cdiv(max_out, SPK_TN);
  hipLaunchKernelGGL(spk_conv1d_kernel, dim3(a.NT, kantts_cdiv(Cout, C1_BM), B), dim3(SPK_THREADS), 0, (hipStream_t)stream, a);
  KANTTS_CHECK_LAUNCH();
}

extern "C" int kantts_spk_cam_gate_conv(const float* h, const int32_t* lens, const float* psum, const float* pmax,
                                        const float* wa, const float* ba, const float* wb, const float* bb, const float* w,
                                        float* y, int B, int Cb, int TH, int Ch, int G, int CY, int TY, int co_off, int dil,
                                        int NT, int max_len, void* stream) {
  if (!h || !lens || !psum || !pmax || !wa || !ba || !wb || !bb || !w || !y || B < 1 || Cb < 1 || TH < 1 || Ch < 1 || G < 1 ||
      co_off < 0 || CY < co_off + G || TY < 1 || dil < 1 || max_len < 1 || max_len > TH || max_len > TY ||
      NT != kantts_cdiv(max_len, SPK_TN))
    return KANTTS_E_BADARG;
  if (Cb > CAM_MAXCB || Ch > CAM_MAXCH || dil > CAM_MAXDIL || B > 65535) return KANTTS_E_UNSUPPORTED;
  SpkCamArgs a;
  a.h = h, a.psum = psum, a.pmax = pmax, a.wa = wa, a.ba = ba, a.wb = wb, a.bb = bb, a.w = w;
  a.lens = reinterpret_cast<const int*>(lens), a.y = y;
  a.Cb = Cb, a.TH = TH, a.Ch = Ch, a.G = G, a.CY = CY, a.TY = TY, a.co_off = co_off, a.dil = dil, a.NT = NT;
  const dim3 grid(NT, B), block(SPK_THREADS);
  switch (G) {
    case 8: hipLaunchKernelGGL(spk_cam_kernel<2>, grid, block, 0, (hipStream_t)stream, a); break;
    case 16: hipLaunchKernelGGL(spk_cam_kernel<4>, grid, block, 0, (hipStream_t)stream, a); break;
    case 32: hipLaunchKernelGGL(spk_cam_kernel<8>, grid, block, 0, (hipStream_t)stream, a); break;
    case 64: hipLaunchKernelGGL(spk_cam_kernel<16>, grid, block, 0, (hipStream_t)stream, a); break;
    default: return KANTTS_E_UNSUPPORTED;
  }
  KANTTS_CHECK_LAUNCH();
}

extern "C" int kantts_spk_tail(const float* x, const int32_t* lens, const float* scale, const float* shift, const float* w,
                               const float* oscale, const float* oshift, float* out, int B, int C, int CX, int TX, int E,
                               void* stream) {
  if (!x || !lens || !scale || !shift || !w || !oscale || !oshift || !out || B < 1 || C < 1 || CX < C || TX < 1 || E < 1)
    return KANTTS_E_BADARG;
  if (C > TAIL_MAXC || B > 65535) return KANTTS_E_UNSUPPORTED;
  hipLaunchKernelGGL(spk_tail_kernel, dim3(B), dim3(SPK_THREADS), 0, (hipStream_t)stream, x,
                     reinterpret_cast<const int*>(lens), scale, shift, w, oscale, oshift, out, C, CX, TX, E);
  KANTTS_CHECK_LAUNCH();
}
