/* libkantts_hip.so -- C ABI of the MI355X (gfx950) kernels behind the KAN-TTS hot path.
 *
 * The reference (modelscope/KAN-TTS) has no FFI: every "kernel" is a stock ATen op called from
 * the kantts/models Python modules.  Each entry point below names the reference call sites (file:line under
 * /root/reference) whose arithmetic it replaces.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - plain C, no C++ types / exceptions cross this boundary; every function returns int:
 *     0 = KANTTS_OK, negative = KANTTS_E_* (bad arguments), positive = hipError_t.
 *   - every pointer is a DEVICE pointer unless the parameter name ends in _host; the caller
 *     (PyTorch's caching allocator in the Python host layer) owns all buffers incl. workspaces;
 *     the library never allocates device memory and keeps no references after returning.
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*); stateless and re-entrant.
 *   - tensors are contiguous row-major fp32 unless stated; lengths/indices are int32 or int64
 *     as stated; "tokens" are rows of a (B, T, C) channels-last activation, row = b*T + t.
 */
#ifndef KANTTS_HIP_H
#define KANTTS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KANTTS_OK 0
#define KANTTS_E_BADARG (-1)
#define KANTTS_E_UNSUPPORTED (-2)
#define KANTTS_E_WORKSPACE (-3)

/* Library/ABI version and target ISA string ("gfx950"). */
int kantts_abi_version(void);
const char* kantts_target_arch(void);

/* ------------------------------------------------------------------------------------------
 * Segmented GEMM:  C[i][j] (op)= epilogue( alpha * sum_seg sum_tap sum_kk A(i,kk) * B(j,kk) )
 *
 * One kernel covers every dense contraction of the path (channels-last activations):
 *   nn.Linear fwd / dgrad / wgrad      kantts/models/sambert/__init__.py:82,102,217,242,287,297
 *   Conv1d k=1 and k=3 (im2col-free: one segment with ntaps shifted row windows)
 *                                      kantts/models/sambert/__init__.py:115-127, fsmn.py:14-29
 *   concatenated inputs (torch.cat + Linear) as several segments
 *                                      kantts/models/sambert/kantts_sambert.py:173-174, adaptors.py:54
 *   sums of projections (fc_x + fc_h)  kantts/models/sambert/__init__.py:287-299
 *   HiFi-GAN dilated Conv1d / polyphase ConvTranspose1d (taps + strided C)
 *                                      kantts/models/hifigan/layers.py:82-88,153-161
 * A(i,kk) = a[i*a_is + kk*a_ks] and B(j,kk) = b[j*b_js + kk*b_ks + tap*b_tap]; a token shift
 * (conv tap) moves the index that is a token (row of a (B,T,C) tensor) by s = shift0+tap*step and
 * yields 0 when (tok % T) + s falls outside [0, T).  Arithmetic: precision 0 = fp32 MFMA
 * (v_mfma_f32_16x16x4_f32, exact f32 FMA chain), 1 = bf16 MFMA inputs with fp32 accumulate
 * (v_mfma_f32_16x16x32_bf16), 2 = scalar fp32 reference kernel (debug).
 */
#define KANTTS_GEMM_MAX_SEG 4
typedef struct kantts_gemm_seg {
  const float* a;      /* A operand */
  const float* a_gate; /* optional, same addressing as A: A(i,kk) is used only where gate > 0
                          (ReLU / zeroed-row backward)                                           */
  const float* b;      /* B operand */
  int64_t a_is, a_ks;  /* A strides over i and kk (elements) */
  int64_t b_js, b_ks;  /* B strides over j and kk */
  int64_t b_tap;       /* B element offset per tap */
  int32_t klen;        /* reduction length per tap */
  int32_t ntaps;       /* >= 1 */
  int32_t a_tok_axis;  /* 0: A has no token shift, 1: i is the token index, 2: kk is */
  int32_t a_shift0, a_shift_step;
  int32_t b_tok_axis;  /* 0: none, 2: kk is the token index of B */
  int32_t b_shift0, b_shift_step;
  float a_drop_p;      /* > 0: A(i,kk) *= dropout keep-scale regenerated from (a_drop_seed, element
                          offset of A) -- backward of an epilogue dropout, A = dY contiguous (M,N) */
  uint64_t a_drop_seed;
  /* Extended token map (strided / transposed / period-folded / nearest-upsampled convolutions of the
   * HiFi-GAN stack, kantts/models/hifigan/{layers,hifigan}.py).  All zero = the plain map above.
   * A token tok of a (B, Tq, inner) domain reads source row ((b*Tsrc) + t)*inner + pi with
   * t = q*mul + shift; when div > 1, t must be a multiple of div and t /= div; the element is 0
   * unless 0 <= t < Tsrc*up; finally t /= up (nearest-neighbour upsampling of the source). */
  int32_t a_inner, a_Tq, a_Tsrc, a_mul, a_div, a_up;
  int32_t b_inner, b_Tq, b_Tsrc, b_mul, b_div, b_up;
  float a_slope;       /* a_act = 1: A value x -> x > 0 ? x : a_slope * x (LeakyReLU fused on load) */
  int32_t a_act;
  float b_slope;
  int32_t b_act;
  float a_gate_slope;  /* where the gate is <= 0, A is multiplied by this (0: hard gate; LeakyReLU backward) */
  int32_t a_mode, b_mode; /* staging layout hints, see csrc/gemm.hip: 0 scalar/lanes along k, 1 scalar/lanes
                          along rows, 2 float4 along k (needs unit k stride, klen % 4 == 0, 16-byte aligned
                          rows, no token map on kk), 3 float4 along rows (unit row stride, extent % 4 == 0,
                          no token map on the row index; every float4 16-byte aligned as well: base, gate, k stride,
                          group stride, and b_tap when there are several taps).  0 is always valid.  With kmask set the launcher stages
                          every a_mode == 2 segment as a_mode 0 (the mask is per element of k, the float4 is not). */
} kantts_gemm_seg;

typedef struct kantts_gemm_args {
  kantts_gemm_seg seg[KANTTS_GEMM_MAX_SEG];
  int32_t nseg;
  int32_t M, N;        /* extent of i and j */
  int32_t T;           /* tokens per sequence for token shifts (ignored when no shift) */
  float* c;
  int64_t c_is, c_js;  /* C strides */
  const float* bias;   /* over j, optional: v = (acc + bias[j] + bias2[j]) * alpha */
  const float* bias2;  /* optional second bias (sum of two projections) */
  const float* res;    /* optional residual added after the activation */
  int64_t r_is, r_js;
  const uint8_t* rowmask; /* optional, over i: rows with mask != 0 are written as 0 */
  const uint8_t* kmask;   /* optional, over kk (same for all segments): kk with mask != 0 skipped */
  float* a_rowsum;     /* optional: a_rowsum[i] += sum_kk A(i,kk) of segment 0 (bias gradient) */
  float alpha;
  int32_t relu;        /* 1: v = max(v, 0) before residual */
  int32_t accumulate;  /* 0: C = v, 1: atomicAdd(C, v) (required when splitk > 1) */
  int32_t splitk;      /* >= 1: reduction tiles are dealt round-robin to gridDim.z slices */
  int32_t precision;   /* 0 fp32 MFMA, 1 bf16 MFMA, 2 scalar reference */
  float drop_p;        /* dropout applied to v after the activation, before the residual */
  uint64_t drop_seed;  /* mask element (i,j) = rng(drop_seed + *seed_dev, i*N + j) */
  const uint64_t* seed_dev; /* optional device word added to every dropout seed of this launch (lets a
                          captured hipGraph draw fresh masks on every replay) */
  /* grouped convolutions: gridDim.z = groups * splitk; group g offsets every operand */
  int32_t groups;      /* 0/1 = none */
  int64_t a_gs, b_gs, c_gs, bias_gs, r_gs; /* element offsets per group for A, B, C(+gate), bias, res */
  float out_slope;     /* out_act = 1: LeakyReLU(out_slope) on v instead of / after relu=0 */
  int32_t out_act;
  const float* gate;   /* optional, addressed like C: v *= (gate > 0 ? 1 : gate_slope)  (backward through
                          an input-side LeakyReLU) */
  float gate_slope;
  int32_t z_taps;      /* > 0: gridDim.z additionally enumerates z_taps taps of segment 0 (each z-slab handles one
                          tap and writes C + tap * c_tap): one launch for all taps of a conv weight gradient */
  int64_t c_tap;
} kantts_gemm_args;

int kantts_gemm_seg_launch(const kantts_gemm_args* args_host, void* stream);

/* What kantts_gemm_seg_launch would do with this descriptor, without launching (the launcher takes its choice from the same
   function, KANTTS_GEMM_* switches included).  Returns KANTTS_OK unless a pointer is NULL.
   out[0]: <0 the refusal code, 0 nothing to launch (M == 0 or N == 0), 1 generic MFMA kernel, 2 fast kernel,
           3 scalar reference kernel
   out[1]: BM (32/64)   out[2]: BIGK   out[3]: A_ROW   out[4]: B_ROW   out[5]: GATE   out[6]: coalesced epilogue (vec_out)
   out[7]: segments whose a_mode 2 was demoted to 0 because kmask is set
   (out points to eight words) */
int kantts_gemm_plan(const kantts_gemm_args* args_host, int32_t* out);

/* ------------------------------------------------------------------------------------------
 * LayerNorm (eps inside sqrt, biased variance).  Replaces nn.LayerNorm(eps=1e-6) at
 * kantts/models/sambert/__init__.py:63,130,198 and kantts/models/sambert/kantts_sambert.py:58,128.
 * x,y,dx,dy: (M,C); mean,rstd: (M) saved for backward; dgamma/dbeta are ACCUMULATED (atomicAdd). */
int kantts_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean,
                         float* rstd, int M, int C, float eps, void* stream);
int kantts_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean,
                         const float* rstd, float* dx, float* dgamma_accum, float* dbeta_accum, int M, int C,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * Range-limited multi-head attention, d_head = 16.  Replaces ScaledDotProductAttention and the mask
 * tensors (kantts/models/sambert/__init__.py:17-29,85-100; kantts_sambert.py:135-166).
 * q/k/v/o/d*: element (b,t,h,d) at ptr[(b*L+t)*ld + h*16 + d]; every ld is a multiple of 4 and every base pointer
 * 16-byte aligned (KANTTS_E_BADARG for an ld that is not; d_head != 16: KANTTS_E_UNSUPPORTED); nothing else of a row is
 * read or written.  lens (B) int32 = valid positions per sequence, 0 <= len <= L (NULL: len = L); bw_dev: optional device
 * scalar overriding bw.  bw >= 0; a host bw of L or more means the whole sequence (any int), a width read from device
 * memory (bw_dev, bw_seq of kantts_attn_decode) must be below 2^30.
 * Query i of sequence b attends to the keys j of the interval [lo, hi]:
 *   mode 0 (key padding, encoder):   [0, len-1] for EVERY i, padded query rows (i >= len) included
 *   mode 1 (PNCA x, causal band):    [max(0, i-bw), i]              if i < len, else [0, L-1]
 *   mode 2 (PNCA h, look-ahead band): [i, min(i+bw, L-1, len-1)]     if i < len, else [0, L-1]
 * s_j = 0.25 * q_i . k_j (= 1/sqrt(d_head)), p_j = softmax of s over [lo, hi], lse_i = log sum_j exp(s_j),
 * o_i = sum_j p_j * m_j * v_j with the dropout scale m_j = rng(seed + *seed_dev, ((h*B+b)*L+i)*L+j) in {0, 1/(1-drop_p)}
 * (1 when drop_p = 0; seed_dev: optional device word).  An empty interval (mode 0, len = 0): o_i = 0, lse_i = 0.
 * lse: (B,H,L) saved; probs: optional (H*B, L, L) post-dropout probabilities p_j * m_j (reference layout), 0 outside
 * [lo, hi].
 * Band modes: rows of padded queries (i >= len) are un-masked in the reference ([0, L-1] above) but zeroed by every
 * caller; they are computed only when probs is requested, otherwise their context and lse are 0, and they never
 * receive / produce gradients in the backward.  Mode 0 computes padded query rows like any other row, forward and backward.
 * Backward, from d_o and the o / lse of the forward: D_i = d_o_i . o_i, dp_j = m_j * (d_o_i . v_j),
 * ds_j = 0.25 * p_j * (dp_j - D_i); dq_i = sum_j ds_j k_j, dk_j = sum_i ds_j q_i, dv_j = sum_i p_j m_j d_o_i, the sums over i
 * running over the queries whose interval holds j (band modes: i < len only).  Writes dq (or adds to it when
 * accumulate_dq), dk, dv -- every row of all three, zeros where nothing contributes (dq of a padded query row in the
 * band modes: 0, or unchanged under accumulate_dq); dvec (B,H,L) is scratch. */
int kantts_attn_fwd(const float* q, const float* k, const float* v, int ldq, int ldk, int ldv, float* o, int ldo,
                    float* lse, float* probs, const int32_t* lens, const int32_t* bw_dev, int bw, int B, int H,
                    int L, int d_head, int mode, float drop_p, uint64_t seed, const uint64_t* seed_dev,
                    void* stream);
int kantts_attn_bwd(const float* q, const float* k, const float* v, int ldq, int ldk, int ldv, const float* o,
                    int ldo, const float* d_o, int lddo, const float* lse, float* dvec, float* dq, float* dk,
                    float* dv, int lddq, int lddk, int lddv, int accumulate_dq, const int32_t* lens,
                    const int32_t* bw_dev, int bw, int B, int H, int L, int d_head, int mode, float drop_p,
                    uint64_t seed, const uint64_t* seed_dev, void* stream);

/* Both attentions of a PNCA block (MultiHeadPNCAAttention.forward, kantts/models/sambert/__init__.py:256-306: the causal
 * band over x and the look-ahead band over the memory share the queries) as ONE launch forward and ONE backward.
 * qkv (B,L,3D) = fused x projection [q | k_x | v_x], hkv = memory projection [k_h | v_h] with row pitch ldh >= 2D (the
 * twelve blocks' projections are columns of one (B,L,12*2D) GEMM output), D = H*16;
 * ox / oh (B,L,D) contexts, lse_x / lse_h (B,H,L) saved.  Backward: dqkv (B,L,3D) = [dq | dk_x | dv_x] with dq the SUM of
 * both bands' query gradients, dhkv (B,L,2D) = [dk_h | dv_h]; every output is written, none accumulated.  For L > 256
 * (more queries than a workgroup has threads) the backward returns 1 instead of KANTTS_OK: dqkv's
 * first D columns then hold the x band's query gradient only, dqh (B,L,D, required in that case) the memory band's, and
 * the caller adds them.  Same masks, dropout streams (seed_x / seed_h) and padded-row rules as kantts_attn_fwd / _bwd with
 * mode 1 / mode 2.  KANTTS_E_UNSUPPORTED if a head's rows do not fit in LDS (L > ~390): use the per-band calls. */
int kantts_pnca_attn_fwd(const float* qkv, const float* hkv, int ldh, float* ox, float* oh, float* lse_x, float* lse_h,
                         const int32_t* lens, const int32_t* bw_dev, int bw_x, int bw_h, int B, int H, int L, int d_head,
                         float drop_p, uint64_t seed_x, uint64_t seed_h, const uint64_t* seed_dev, void* stream);
int kantts_pnca_attn_bwd(const float* qkv, const float* hkv, int ldh, const float* ox, const float* oh, const float* d_ox,
                         const float* d_oh, const float* lse_x, const float* lse_h, float* dqkv, float* dqh, float* dhkv,
                         const int32_t* lens, const int32_t* bw_dev, int bw_x, int bw_h, int B, int H, int L, int d_head,
                         float drop_p, uint64_t seed_x, uint64_t seed_h, const uint64_t* seed_dev, void* stream);

/* Which kernels the four entry points above use for sequences of L positions, without launching (host only; the launchers
 * take their choice from the same function, the per-process switches KANTTS_ATTN_NO_QUAD / KANTTS_ATTN_NO_DQ2 included).
 * pass: KANTTS_ATTN_PASS_*; mode as above (ignored for the PNCA passes).  Returns a KANTTS_ATTN_* path,
 * KANTTS_E_UNSUPPORTED where the entry point refuses (PNCA forward L >= 410, PNCA backward L >= 391), KANTTS_E_BADARG for
 * an unknown pass / mode or L < 0.  A head is LDS-staged while its row images fit 64 KB. */
#define KANTTS_ATTN_PASS_FWD 0
#define KANTTS_ATTN_PASS_BWD 1
#define KANTTS_ATTN_PASS_PNCA_FWD 2
#define KANTTS_ATTN_PASS_PNCA_BWD 3
#define KANTTS_ATTN_FWD_LDS_QUAD 1   /* mode 0, L <= 409: four lanes per query */
#define KANTTS_ATTN_FWD_LDS 2        /* band modes (mode 0 under KANTTS_ATTN_NO_QUAD), L <= 409 */
#define KANTTS_ATTN_FWD_DIRECT 3     /* L >= 410: keys and values from global memory */
#define KANTTS_ATTN_BWD_LDS_QUAD 4   /* mode 0, L <= 390 */
#define KANTTS_ATTN_BWD_LDS 5        /* band modes (mode 0 under KANTTS_ATTN_NO_QUAD), L <= 390 */
#define KANTTS_ATTN_BWD_DIRECT 6     /* L >= 391 */
#define KANTTS_ATTN_PNCA_FWD_LDS 7   /* L <= 409 */
#define KANTTS_ATTN_PNCA_BWD_DQ2 8   /* L <= 256: both bands' query gradients summed in one pass, returns 0 */
#define KANTTS_ATTN_PNCA_BWD_SPLIT 9 /* 257 <= L <= 390 (L <= 390 under KANTTS_ATTN_NO_DQ2): dqh written, returns 1 */
int kantts_attn_plan(int L, int mode, int pass);

/* ------------------------------------------------------------------------------------------
 * LSTM recurrence, H = 128 (time loop of torch.nn.LSTM: kantts/models/sambert/adaptors.py:44-57,
 * :109-134; kantts_sambert.py:637-646).  gx (B,T,ndir*4H) = x W_ih^T + b_ih (from the GEMM);
 * whh (ndir,4H,H), bhh (ndir,4H) or NULL; lens (B) int32 or NULL = pack_padded_sequence lengths;
 * a length is clamped into [0, T] by both entry points (negative = empty sequence, beyond T = T): out and dgates
 * are exactly zero at t >= len, the saved state is unspecified there;
 * out (B,T,ndir*H); gates_save (ndir*B*T*4H floats; private to the fwd / bwd pair: since round 6 a cell's four activations
 * side by side, (ndir,B,T,H,4)) and c_save (ndir,B,T,H) are kept for backward.
 * Backward returns dgates (ndir,B,T,4H) = gradient w.r.t. the pre-activation gates.
 * precision 0: fp32 recurrent products; 1: h / dgates and W_hh rounded to bf16 for the recurrent product only
 * (packed v_dot2c_f32_bf16, fp32 accumulate) -- gates, cell state, outputs stay fp32. */
int kantts_lstm_fwd(const float* gx, const float* whh, const float* bhh, const int32_t* lens, float* out,
                    float* gates_save, float* c_save, int B, int T, int H, int ndir, int reverse_first,
                    int precision, void* stream);
int kantts_lstm_bwd(const float* dout, const float* whh, const int32_t* lens, const float* gates_save,
                    const float* c_save, float* dgates, int B, int T, int H, int ndir, int reverse_first,
                    int precision, void* stream);
/* Streaming form of kantts_lstm_fwd: steps [t0, min(t1, len)) of ONE forward direction (ndir == 2 or reverse_first:
 * KANTTS_E_UNSUPPORTED) over the same full-length buffers, which persist between calls.  The state entering step t0 > 0 is
 * h = out[b, t0 - 1], c = c_save[b, t0 - 1] (precision 1: h rounded to bf16 exactly as the step that produced it published
 * it); it is zero at t0 == 0.  Only rows [t0, t1) of out / gates_save / c_save are written -- the zero tail of `out` for
 * rows [max(len, t0), t1) -- and no row of gx at or after t1 is read (they need not exist yet).  Consecutive ranges give
 * the bits of one kantts_lstm_fwd call.  t0 < 0, t1 > T or t0 > t1: KANTTS_E_BADARG; t0 == t1: no-op.  KANTTS_LSTM_PAIR=0
 * selects the quad kernel here as it does for kantts_lstm_fwd. */
int kantts_lstm_fwd_range(const float* gx, const float* whh, const float* bhh, const int32_t* lens, float* out,
                          float* gates_save, float* c_save, int B, int T, int H, int ndir, int reverse_first, int t0,
                          int t1, int precision, void* stream);
/* kantts_lstm_fwd_range (one forward direction) with a range per sequence: t0 / t1 are DEVICE int32[B], clamped by the
 * kernel to c0 = clamp(t0[b], 0, T), c1 = clamp(t1[b], c0, T) and never read back.  Sequence b runs steps
 * [c0, min(c1, len)) from out[b, c0 - 1] / c_save[b, c0 - 1] and writes the zero tail for rows [max(len, c0), c1): the bits
 * of kantts_lstm_fwd_range(..., c0, c1, ...) for that sequence; c0 == c1 reads and writes nothing.  KANTTS_LSTM_PAIR=0
 * selects the quad kernel as above.  t0 == NULL or t1 == NULL: KANTTS_E_BADARG. */
int kantts_lstm_fwd_slots(const float* gx, const float* whh, const float* bhh, const int32_t* lens, float* out,
                          float* gates_save, float* c_save, int B, int T, int H, const int32_t* t0, const int32_t* t1,
                          int precision, void* stream);
/* TWO bidirectional layers of one shape (B, T, H = 128) over the same lengths in ONE launch each way: the pitch and the energy
 * predictor's BiLSTMs (kantts/models/sambert/adaptors.py:109-134), which are independent and would otherwise run one after
 * the other.  Every problem is computed exactly as its own kantts_lstm_fwd / kantts_lstm_bwd call with ndir = 2,
 * reverse_first = 0 computes it (same bits in out, gates_save, c_save, dgates); tensors as documented there, except that the
 * recurrent weights and biases are given PER DIRECTION (whh[d]: (4H,H), bhh[d]: (4H) or NULL), so the caller stacks nothing.
 * precision must be 1 (the bf16 recurrent product): anything else, H != 128 or KANTTS_LSTM_PAIR=0 / KANTTS_LSTM_PAIR_BWD=0
 * (the quad kernels have no such form) is KANTTS_E_UNSUPPORTED.  fwd reads gx, whh, bhh and writes out, gates_save, c_save;
 * bwd reads dout, whh, gates_save, c_save and writes dgates; the other fields may be NULL. */
typedef struct kantts_bilstm_args {
  const float* gx;      /* (B,T,2*4H) */
  const float* whh[2];
  const float* bhh[2];
  float* out;           /* (B,T,2H) */
  float* gates_save;    /* (2,B,T,H,4) */
  float* c_save;        /* (2,B,T,H) */
  const float* dout;    /* (B,T,2H) */
  float* dgates;        /* (2,B,T,4H) */
} kantts_bilstm_args;
int kantts_bilstm_pair_fwd(const kantts_bilstm_args* a, const kantts_bilstm_args* b, const int32_t* lens, int B, int T,
                           int H, int precision, void* stream);
int kantts_bilstm_pair_bwd(const kantts_bilstm_args* a, const kantts_bilstm_args* b, const int32_t* lens, int B, int T,
                           int H, int precision, void* stream);

/* ------------------------------------------------------------------------------------------
 * Embedding gather-sum: out[row] = scale * sum_k table_k[ids[row,k]] (+ pos[row % T]);
 * scaled_out (optional) receives the value before the positional add.  tables_host is a HOST array
 * of ntab (<=4) device pointers.  kantts/models/sambert/kantts_sambert.py:308-329, :62-64.
 * Backward scatter-adds scale*dout into dtables (NULL entries skipped). */
int kantts_embed_sum_fwd(const float* const* tables_host, int ntab, const int64_t* ids, const float* pos,
                         float* out, float* scaled_out, int rows, int T, int D, float scale, void* stream);
int kantts_embed_sum_bwd(float* const* dtables_host, int ntab, const int64_t* ids, const float* dout, int rows,
                         int D, float scale, void* stream);
/* [round 5] The length- / target-only preparation of a teacher-forced SAM-BERT step in one launch (csrc/seq.hip;
 * kantts/models/utils.py:13-23, kantts_sambert.py:466-468, 556-559, 736-750, 981-985, positions.py:83-98):
 *   in / out / lfr: lengths clamped to N / T_mel / Tp/r as int64 and int32, and masks (uint8, 1 = padding) of shapes (B, N),
 *     (B, T_mel), (B, Tp/r) -- lfr lengths are ceil(out_lens / r);  valid[b] = min(out length, max_len);
 *   pos_enc (B, Tp, depth): sin (even channels) / cos (odd) of pos_masked / inv_ts[c], pos = kantts_lr_index's, masked to 0
 *     from frame min(out length, max_len) on;  prev (B, N) = log(dur[b, n-1] + 1) (0 for n = 0);
 *   bw_val = max over valid (b, n) of dur / r + 0.5 (fp32), bw_dev = its truncation (int32);
 *   dec_input (B, Tp/r, d_mel): row 0 zeros, row l = mel[b, l*r - 1]. */
typedef struct kantts_plan_args {
  const int64_t* in_lens;
  const int64_t* out_lens;
  const int64_t* dur;
  const float* mel;
  const float* pos;
  const float* inv_ts;
  int32_t B, N, T_mel, Tp, max_len, r, d_mel, depth;
  int64_t* in_l64;
  int32_t* in_l32;
  uint8_t* in_mask;
  int64_t* out_l64;
  int32_t* out_l32;
  uint8_t* out_mask;
  int64_t* lfr_l64;
  int32_t* lfr_l32;
  uint8_t* lfr_mask;
  int64_t* valid;
  float* pos_enc;
  float* prev;
  float* bw_val;
  int32_t* bw_dev;
  float* dec_input;
} kantts_plan_args;
int kantts_teacher_plan(const kantts_plan_args* args, void* stream);

/* ------------------------------------------------------------------------------------------
 * Length regulator (kantts/models/sambert/adaptors.py:15-36, positions.py:72-90) in index form.
 * kantts_lr_index: reps = trunc(dur + 0.5) (dur_int (B,N) int64 or dur_float (B,N) fp32);
 *   idx (B,Tp) int32 token per frame or -1; pos (B,Tp) 1-based position inside the token (t+1 when
 *   uncovered); cs (B,N+1) int32 exclusive prefix sums; lens (B) int64 totals.  Bit-exact.
 * kantts_lr_gather_fwd: out[b,t, off:off+C] = x[b, idx[b,t], :] (0 when idx<0 or t >= valid_lens[b]);
 *   out rows have stride ldo (lets three regulators write one concatenated buffer).
 * kantts_lr_gather_bwd: deterministic segment sum over [cs[n], min(cs[n+1], Tp, valid_lens[b])); accumulate != 0: dx += it.
 * valid_lens (B) int64, optional, any value >= 0: it is compared in 64 bits (2^31 or 2^32 + 3 mask nothing). */
int kantts_lr_index(const int64_t* dur_int, const float* dur_float, int32_t* idx, float* pos, int32_t* cs,
                    int64_t* lens, int B, int N, int Tp, void* stream);
int kantts_lr_gather_fwd(const float* x, const int32_t* idx, const int64_t* valid_lens, float* out, int B, int N,
                         int Tp, int C, int ldo, int out_col_offset, void* stream);
int kantts_lr_gather_bwd(const float* dout, const int32_t* cs, const int64_t* valid_lens, float* dx, int B, int N,
                         int Tp, int C, int ldo, int out_col_offset, int accumulate, void* stream);

/* The regulated hand-over to the decoder (kantts_sambert.py: three regulators, + pos_enc, LFR reshape, cat) as one launch
 * each way.  aug (B,N,d_t), spk (B,N,d_s), emo (B,N,d_e), pos_enc (B,Tp,d_t), idx / cs / valid_lens of kantts_lr_index and
 * kantts_lr_gather_* (valid_lens may be NULL), Tp % r == 0, L = Tp / r:
 *   memory (B, L, r*d_t + d_s + d_e), contiguous:
 *     memory[b, l, j*d_t + c]       = G(aug)[b, l*r + j, c] + pos_enc[b, l*r + j, c]
 *     memory[b, l, r*d_t + c]       = G(spk)[b, l*r, c]       memory[b, l, r*d_t + d_s + c] = G(emo)[b, l*r, c]
 *   with G = kantts_lr_gather_fwd's rule (0 when idx < 0 or t >= valid_lens[b]); the sum is one fp32 add of the gathered
 *   value (or 0) and pos_enc: bit-identical to the composition.  lr_text (B,Tp,d_t), lr_spk (B,Tp,d_s), lr_emo (B,Tp,d_e):
 *   optional (NULL = not written) frame-level results of the composition, G(aug) + pos_enc, G(spk), G(emo).
 * kantts_lr_memory_bwd: d_memory (B, L, .) with row pitch ldm floats (>= r*d_t + d_s + d_e; batch pitch L * ldm) ->
 *   d_aug (B,N,d_t), d_spk (B,N,d_s), d_emo (B,N,d_e): per token the sum over its frames
 *   [cs[n], min(cs[n+1], Tp, valid_lens[b])) in frame order, as kantts_lr_gather_bwd sums them (d_spk / d_emo: the frames
 *   with t % r == 0) -- bit-identical to the composition's backward.  Every element of the three outputs is written.
 * KANTTS_E_UNSUPPORTED: a width that is no multiple of 4, ldm % 4 != 0, or a tensor that is not 16-byte aligned. */
int kantts_lr_memory_fwd(const float* aug, const float* spk, const float* emo, const int32_t* idx,
                         const int64_t* valid_lens, const float* pos_enc, float* memory, float* lr_text, float* lr_spk,
                         float* lr_emo, int B, int N, int Tp, int r, int d_t, int d_s, int d_e, void* stream);
int kantts_lr_memory_bwd(const float* d_memory, long long ldm, const int32_t* cs, const int64_t* valid_lens, float* d_aug,
                         float* d_spk, float* d_emo, int B, int N, int Tp, int r, int d_t, int d_s, int d_e, void* stream);

/* ------------------------------------------------------------------------------------------
 * FSMN memory block (kantts/models/sambert/fsmn.py:43-72), channels-last (B,T,C), w (C,K):
 *   xm = x*keep; y = keep*(sum_k w[c,k]*xm[t+k-left_pad] + xm[t]) (+ res); keep[b,t] = t < lens[b].
 * Backward: dx (w.r.t. x) and dw_accum (atomicAdd); d(res) = dy.  dx or dw_accum may be NULL: only the other gradient is
 * computed (two calls on two streams: the filter gradient runs beside the backward pass's critical path). */
int kantts_fsmn_dwconv_fwd(const float* x, const float* w, const float* res, const int64_t* lens, float* y, int B,
                           int T, int C, int K, int left_pad, void* stream);
/* Rows [t0, t1) of y only (res is indexed like y), over the same full-length buffers: the x rows a result depends on are
 * [t0 - left_pad, t1 + (K - 1 - left_pad)) inside [0, min(len, T)); later rows need not hold data yet, no other row of y is
 * written, and a row equals the same row of kantts_fsmn_dwconv_fwd bit for bit.  t0 < 0, t1 > T or t0 > t1: KANTTS_E_BADARG;
 * t0 == t1: no-op. */
int kantts_fsmn_dwconv_fwd_rows(const float* x, const float* w, const float* res, const int64_t* lens, float* y, int B,
                                int T, int C, int K, int left_pad, int t0, int t1, void* stream);
/* kantts_fsmn_dwconv_fwd_rows with a window per sequence: t0 / t1 are DEVICE int32[B], clamped by the kernel to
 * c0 = clamp(t0[b], 0, T), c1 = min(clamp(t1[b], c0, T), c0 + max_rows) and never read back.  max_rows (host-known, >= 0)
 * sizes the grid; a tile that starts at or after c1 exits.  Rows [c0, c1) of y equal the same rows of
 * kantts_fsmn_dwconv_fwd_rows(..., c0, c1) bit for bit (41-tap and generic kernel), no other row is written.
 * t0 == NULL, t1 == NULL or max_rows < 0: KANTTS_E_BADARG. */
int kantts_fsmn_dwconv_fwd_slots(const float* x, const float* w, const float* res, const int64_t* lens, float* y, int B,
                                 int T, int C, int K, int left_pad, const int32_t* t0, const int32_t* t1, int max_rows,
                                 void* stream);
int kantts_fsmn_dwconv_bwd(const float* dy, const float* x, const float* w, const int64_t* lens, float* dx,
                           float* dw_accum, float* workspace, long long ws_floats, int B, int T, int C, int K,
                           int left_pad, void* stream);
/* floats of caller-owned workspace the backward needs: B * ceil(T / 128) * C * 41 weight-gradient partials for K = 41, 0 for
 * every other K.  A NULL workspace or ws_floats below that, with dw_accum given: KANTTS_E_WORKSPACE, nothing is launched;
 * nothing behind ws_floats is ever written. */
long long kantts_fsmn_dwconv_bwd_ws(int B, int T, int C, int K);
/* The 41-tap filter gradient of up to KANTTS_FIR_DW_MAX memory blocks in two launches for all of them (the filter gradient
 * is a leaf of the backward graph: the host records the problems of a step and issues them together).  Per problem:
 * dw_accum (C, 41) += the filter gradient of kantts_fsmn_dwconv_bwd(dy, x, lens, dx = NULL, ...) with K = 41, the same
 * workgroups, arithmetic and summation order, hence the same bits; workspace as for that call
 * (kantts_fsmn_dwconv_bwd_ws(B, T, C, 41) floats; nothing behind ws_floats is written); lens may be NULL.  Problems may
 * differ in every field; their dw_accum and workspace ranges must not overlap.  A problem with B == 0 or T == 0 is skipped;
 * nprob == 0 launches nothing.  KANTTS_E_BADARG: nprob outside [0, KANTTS_FIR_DW_MAX], a NULL dy / x / dw_accum, B < 0,
 * T < 0, C < 1; KANTTS_E_WORKSPACE: a NULL or short workspace; KANTTS_E_UNSUPPORTED: more than 2^31 - 1 workgroups.  On an
 * error nothing is launched. */
#define KANTTS_FIR_DW_MAX 16
typedef struct kantts_fir_dw_problem {
  const float* dy;
  const float* x;
  const int64_t* lens;
  float* dw_accum;
  float* workspace;
  long long ws_floats;
  int32_t B, T, C, left_pad;
} kantts_fir_dw_problem;
int kantts_fsmn_dw41_many(const kantts_fir_dw_problem* probs, int nprob, void* stream);
/* The memory block of a training step with the two dropouts stacked on it and the residual add, one launch each way
 * (K == 41; c, res, y, dy, dx, dym (B,T,C) fp32 contiguous, w (C,K), lens int64[B] or NULL):
 *   fwd: y = keep2 * (keep1 * m) (+ res),  m = kantts_fsmn_dwconv_fwd(c, w, res = NULL, lens)
 *   bwd: dym[b,t] = keep2 * (keep1 * dy) for t < lens[b], 0 for the other rows;  dx = kantts_fsmn_dwconv_bwd's dx of dym
 * with keep_i the masks of kantts_dropout2_add(p1, seed1, p2, seed2, seed_dev) over the flat element index
 * ((b*T + t)*C + c) (p_i == 0: no mask; seed_dev may be NULL).  Every product and the residual add round as in the two
 * calls they replace, so y, dx and dym (rows t < lens[b]) are bit-identical to that pair; dym is what the filter gradient
 * (kantts_fsmn_dwconv_bwd with dx = NULL) takes as dy.  c / dy rows at or after lens[b] are not used (they may hold
 * anything); res is read and y, dx, dym are written at every row t < T.  res may be NULL.
 * KANTTS_E_BADARG: a NULL tensor, left_pad outside [0, K), p outside [0, 1).  KANTTS_E_UNSUPPORTED (the caller runs the
 * pair): K != 41, C % 4 != 0, a tensor that is not 16-byte aligned, more than 2^31 - 1 tiles. */
int kantts_fsmn_memory_drop_fwd(const float* c, const float* w, const float* res, const int64_t* lens, float* y, int B,
                                int T, int C, int K, int left_pad, float p1, uint64_t seed1, float p2, uint64_t seed2,
                                const uint64_t* seed_dev, void* stream);
int kantts_fsmn_memory_drop_bwd(const float* dy, const float* w, const int64_t* lens, float* dx, float* dym, int B, int T,
                                int C, int K, int left_pad, float p1, uint64_t seed1, float p2, uint64_t seed2,
                                const uint64_t* seed_dev, void* stream);
/* TWO memory blocks of one shape (B, T, C, K, left_pad) over the same lengths in one launch each way (the pitch and the
 * energy predictor's): each problem has its own operands, dropout probabilities and seeds, is checked as the single call
 * checks it and gets that call's bits.  fwd: x = c, y = y, res optional, dym unused; bwd: x = dy, y = dx, dym required. */
typedef struct kantts_fsmn_drop_args {
  const float* x;
  const float* w;
  const float* res;
  float* y;
  float* dym;
  float p1, p2;
  uint64_t seed1, seed2;
} kantts_fsmn_drop_args;
int kantts_fsmn_memory_drop_fwd_pair(const kantts_fsmn_drop_args* a, const kantts_fsmn_drop_args* b, const int64_t* lens,
                                     int B, int T, int C, int K, int left_pad, const uint64_t* seed_dev, void* stream);
int kantts_fsmn_memory_drop_bwd_pair(const kantts_fsmn_drop_args* a, const kantts_fsmn_drop_args* b, const int64_t* lens,
                                     int B, int T, int C, int K, int left_pad, const uint64_t* seed_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * Masked L1 ("mae") reduction: loss_accum[0] += sum_{t<rows_b} |target-pred| / (sum_b(rows_b)*C);
 * grad (optional, (B,T,C)) = d loss / d pred: sign(pred-target) / (sum_b(rows_b)*C) on valid rows, 0 on the others.
 * Sequence b has rows_b = min(lens[b], T) valid rows, in the mask and in the denominator; lens[b] >= 0 (the kernels do not
 * agree on a negative length).  B*T*C == 0: KANTTS_OK, nothing is read or written.  A non-empty call whose lengths are all
 * 0 adds NaN (the reference's 0 / 0) and writes a gradient of zeros.
 * kantts/train/loss.py:18-37, :51-85. */
int kantts_masked_l1(const float* pred, const float* target, const int64_t* lens, float* loss_accum, float* grad,
                     int B, int T, int C, void* stream);

/* Mean-style element losses of the GAN step (kantts/train/loss.py:108-256,310): mode 0: loss_accum += scale*sum|a-b|,
 * grad = scale*sign(a-b); mode 1: loss_accum += scale*sum (a-target)^2, grad = 2*scale*(a-target).  grad optional. */
int kantts_elem_loss(const float* a, const float* b, float target, int mode, float scale, float* loss_accum,
                     float* grad, long long n, void* stream);

/* out_accum[0] += sum x^2 (global gradient norm, torch.nn.utils.clip_grad_norm_) */
int kantts_sumsq(const float* x, float* out_accum, long long n, void* stream);

/* torch.optim.Adam step on flat fp32 arenas with optional global-norm clipping read from device
 * memory (gnorm_sq = sum of squares of all gradients): kantts/train/trainer.py:997-1004. */
int kantts_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1,
                     float beta2, float eps, float weight_decay, float bias_corr1, float bias_corr2,
                     const float* gnorm_sq, float max_norm, const float* dyn_lr_step, void* stream);
/* dyn_lr_step (optional, device, 2 floats {lr, step}): when given, lr and the bias corrections
 * 1 - beta^step are taken from device memory (hipGraph replay with a changing schedule). */

/* ------------------------------------------------------------------------------------------
 * Fused framed STFT -> |.| -> sparse mel filterbank -> 20 log10 - 20 -> clamp(8(x+100)/100-4, +-4).
 * Replaces MelSpectrogram.forward (kantts/utils/audio_torch.py:155-186) and, with out_mag only,
 * stft() (:8-31).  wav (B,T); window (n_fft) = hann(win_length) centred in n_fft; twiddle (n_fft/2
 * complex pairs) = exp(-2 pi i t / n_fft); pad_mode 0 = zeros (MelSpectrogram), 1 = reflect (stft);
 * frames = 1 + T / hop.  The mel basis is passed in support form: filter m covers bins
 * [mel_start[m], mel_start[m]+mel_len[m]) with weights mel_w[mel_off[m] ...].
 * out_mel (B, n_mels, frames) and/or out_mag (B, frames, n_fft/2+1). */
int kantts_melspec_fwd(const float* wav, int B, int T, int n_fft, int hop, int frames, int pad_mode,
                       const float* window, const float* twiddle, float eps_power, const int32_t* mel_start,
                       const int32_t* mel_len, const int32_t* mel_off, const float* mel_w, int n_mels,
                       float eps_mel, float* out_mel, float* out_mag, void* stream);

/* The same pipeline with the dB normalisation as parameters: S = 20 log10(max(mel, 1e-5)) - ref_level_db;
 * symmetric: clip(2*max_norm*(S - min_level_db)/(-min_level_db) - max_norm, +-max_norm); else clip(max_norm*(S - min_level_db)
 * /(-min_level_db), 0, max_norm).  Serves the offline feature extractor melspectrogram()
 * (kantts/preprocess/audio_processor/core/dsp.py:165-201: eps_power = 0, eps_mel = 1e-5, ref 20, min -100, max_norm 1,
 * asymmetric); kantts_melspec_fwd is this function at (20, -100, 4, symmetric). */
int kantts_melspec_norm_fwd(const float* wav, int B, int T, int n_fft, int hop, int frames, int pad_mode,
                            const float* window, const float* twiddle, float eps_power, const int32_t* mel_start,
                            const int32_t* mel_len, const int32_t* mel_off, const float* mel_w, int n_mels,
                            float eps_mel, float ref_level_db, float min_level_db, float max_norm, int symmetric,
                            float* out_mel, float* out_mag, void* stream);

/* [round 4] The same two functions with the mel tensor FRAME-major when mel_frame_major != 0: out_mel / dmel are
 * (B, frames, n_mels) instead of (B, n_mels, frames) -- a frame's channels are one contiguous store (the channel-major
 * layout makes every store a partial sector: 3 x the algorithmic write traffic); the host layer hands the reference's
 * (B, n_mels, frames) shape out as a transposed view.  mel_frame_major == 0: identical to the functions above / below. */
int kantts_melspec_norm_fwd_fm(const float* wav, int B, int T, int n_fft, int hop, int frames, int pad_mode,
                               const float* window, const float* twiddle, float eps_power, const int32_t* mel_start,
                               const int32_t* mel_len, const int32_t* mel_off, const float* mel_w, int n_mels, float eps_mel,
                               float ref_level_db, float min_level_db, float max_norm, int symmetric, int mel_frame_major,
                               float* out_mel, float* out_mag, void* stream);
int kantts_melspec_bwd_fm(const float* wav, const float* dmel, int B, int T, int n_fft, int hop, int frames, int pad_mode,
                          const float* window, const float* twiddle, float eps_power, const int32_t* mel_start,
                          const int32_t* mel_len, const int32_t* mel_off, const float* mel_w, int n_mels, float eps_mel,
                          int mel_frame_major, float* dwav_accum, void* stream);

/* [round 5] Measurement aid, not part of the model: a launch that reads read_bytes from src and writes write_bytes to dst
 * once each (16-byte chunks, whole chip) -- the copy roof a kernel with those algorithmic bytes is judged against
 * (bench.py: upsampling.copy_roof_us). */
int kantts_copy_roof(const void* src, long long read_bytes, void* dst, long long write_bytes, void* stream);

/* [round 5] The two knobs of the mel-STFT launchers, explicit instead of environment variables read on every launch: grid_cap
 * > 0 caps the persistent grid of the register-resident n_fft 1024 kernel (0 = default, 768 workgroups) -- sweeps, and the
 * tests that must reach its several-pairs-per-wave loop with small inputs; generic_only != 0 routes every size to the radix-2
 * kernel (A/B, tests).  Process-global; the only state the library keeps. */
int kantts_melspec_tuning(int grid_cap, int generic_only);

/* Backward of the mel path of kantts_melspec_fwd (MelSpectrogramLoss on generated audio, kantts/train/loss.py:
 * 259-311): dwav_accum (B,T) += d loss / d wav given dmel (B, n_mels, frames).  The spectrum is recomputed. */
int kantts_melspec_bwd(const float* wav, const float* dmel, int B, int T, int n_fft, int hop, int frames,
                       int pad_mode, const float* window, const float* twiddle, float eps_power,
                       const int32_t* mel_start, const int32_t* mel_len, const int32_t* mel_off, const float* mel_w,
                       int n_mels, float eps_mel, float* dwav_accum, void* stream);

/* The five masked-L1 terms of a SAM-BERT training step (MelReconLoss on the decoder and postnet mels, ProsodyReconLoss on
 * log-duration / pitch / energy: kantts/train/loss.py:7-85) in ONE launch: term k over pred (B, T, C) against target
 * (float, or -- target_log1p -- int64 values v read as log(v + 1): the duration targets) on rows t < lens[b];
 * losses[k] += mean |target - pred|, losses[KANTTS_LOSS_MAX_TERMS] += the same (the step's total); grad[k] (optional) =
 * d term k / d pred as kantts_masked_l1 writes it.  losses must be zeroed by the caller.  Valid rows are
 * min(lens[b], T), lens[b] >= 0, as for kantts_masked_l1.  Every term must be non-empty (B*T*C > 0: an empty term adds NaN
 * to losses[k] and to the total).  A term whose lengths are all 0 adds NaN to losses[k] and to the total as well. */
#define KANTTS_LOSS_MAX_TERMS 5
typedef struct kantts_loss_term {
  const float* pred;
  const void* target;
  const int64_t* lens;
  float* grad;
  int32_t B, T, C, target_log1p;
} kantts_loss_term;
int kantts_masked_l1_many(const kantts_loss_term* terms, int nterms, float* losses, void* stream);
/* x_k *= *scale_dev for up to KANTTS_ELOSS_MAX_TERMS tensors in one launch (the backward of the call above and of
 * kantts_elem_loss_many: the upstream gradient of a loss sum is a device scalar). */
int kantts_scale_many(float* const* x, const long long* n, int count, const float* scale_dev, void* stream);

/* [round 4] The mean-reduced element losses of a GAN step in ONE launch per criterion (kantts/train/loss.py:108-256: the
 * feature-matching loss alone is ~48 l1_loss calls per step -- one per discriminator layer --, the adversarial criteria 8 /
 * 16 mse_loss calls; each was a zero-fill, a reduction launch and an addition).  Term k adds into losses[out]:
 *   mode 0: scale * sum |a - b|      grad (optional) = scale * sign(a - b)
 *   mode 1: scale * sum (a - target)^2      grad = 2 * scale * (a - target)
 * exactly as kantts_elem_loss does for one term.  terms: HOST array of nterms <= KANTTS_ELOSS_MAX_TERMS; losses: device
 * accumulators, zeroed by the caller. */
#define KANTTS_ELOSS_MAX_TERMS 64
typedef struct kantts_eloss_term {
  const float* a;
  const float* b;  /* mode 0 only */
  float* grad;     /* may be NULL */
  long long n;
  float target, scale;
  int32_t mode, out;
} kantts_eloss_term;
int kantts_elem_loss_many(const kantts_eloss_term* terms, int nterms, float* losses, void* stream);

/* ------------------------------------------------------------------------------------------
 * weight_norm reparametrisation w = g * v / ||v|| per output row (torch.nn.utils.weight_norm, dim=0):
 * kantts/models/hifigan/layers.py:29,67,105,139, hifigan.py:224,332.  v,w,dw,dv: (rows, cols); g,dg: (rows).
 * Backward: dg = sum(dw * v) / ||v||, dv = (g / ||v||) * (dw - v * dg / ||v||).  A row of v that is all zeros has
 * ||v|| = 0: every output of that row (w and its bf16 images, dg, dv) is NaN, as torch.nn.utils.weight_norm gives, and no
 * other row is affected.  This holds for all entry points of the family below. */
int kantts_weight_norm_fwd(const float* v, const float* g, float* w, int rows, int cols, void* stream);
int kantts_weight_norm_bwd(const float* dw, const float* v, const float* g, float* dv, float* dg, int rows,
                           int cols, void* stream);

/* The same reparametrisation writing / reading the weight through strides: element (row r, input channel ci, tap k) at
 * r*rs + ci*cs + k*ks (tap-major (K, Cout, Cin_g): rs = Cin_g, cs = 1, ks = Cout*Cin_g); v / dv are (rows, cin, K). */
int kantts_weight_norm_strided_fwd(const float* v, const float* g, float* w, int rows, int cin, int K, long long rs,
                                   long long cs, long long ks, void* stream);
int kantts_weight_norm_strided_bwd(const float* dw, const float* v, const float* g, float* dv, float* dg, int rows,
                                   int cin, int K, long long rs, long long cs, long long ks, void* stream);

/* Tap-major weight norm with the bf16 operand images of kantts_cconv_launch in the same pass (v (rows, cin, K)):
 * w (K, rows, cin) fp32; wf_bf16 (K, rows, cin) = bf16(w) (optional); wd_bf16 (K, groups, cin, rows / groups) = the
 * per-tap transpose inside each group, the weight of the input-gradient contraction (optional). */
int kantts_weight_norm_tap_images(const float* v, const float* g, float* w, void* wf_bf16, void* wd_bf16, int rows, int cin,
                                  int K, int groups, void* stream);

/* The same for EVERY weight-normed convolution of a network in ONE launch (the network's parameters live in one flat
 * fp32 arena; images are rebuilt once per optimizer step, not once per layer and forward pass).  Table entry (device
 * memory): v at flat + v_off (rows, cin, K), g at flat + g_off (rows); outputs at w + w_off (K, rows, cin) fp32,
 * wf_bf16 + wf_off (K, rows, cin) and wd_bf16 + wd_off (K, groups, cin, rows / groups) -- wf_off / wd_off < 0: that layer
 * has no bf16 images; row0 = number of 8-row TILES, ceil(rows / 8) each, of all earlier entries (the launch has one
 * workgroup per tile; entries are found by bisection over row0); total_tiles = their sum.  Offsets of the bf16 images must
 * be multiples of 8 elements.  kantts/models/hifigan/layers.py:29,67, hifigan.py:224,332. */
typedef struct kantts_wn_desc {
  int64_t v_off, g_off, w_off, wf_off, wd_off;
  int32_t rows, cin, K, groups, row0, pad_;
} kantts_wn_desc;
int kantts_weight_norm_table(const float* flat, float* w, void* wf_bf16, void* wd_bf16, const kantts_wn_desc* table_dev,
                             int ndesc, int total_tiles, void* stream);

/* Backward of the same reparametrisation for up to KANTTS_WN_BWD_MAX layers of one network in one launch: layer l of the
 * launch is table entry desc[l], its tap-major weight gradient (K, rows, cin) fp32 is dw[l]; dv (rows, cin, K) and dg
 * (rows) are written into the network's flat GRADIENT arena at the entry's v_off / g_off (the parameters' own offsets).
 * tile0[l] = 8-row tiles of the layers before l in THIS launch (tile0[nl] = their total = the grid). */
#define KANTTS_WN_BWD_MAX 64
typedef struct kantts_wn_bwd_args {
  const float* dw[KANTTS_WN_BWD_MAX];
  int32_t desc[KANTTS_WN_BWD_MAX];
  int32_t tile0[KANTTS_WN_BWD_MAX + 1];
  int32_t nl;
} kantts_wn_bwd_args;
int kantts_weight_norm_table_bwd(const float* flat, float* grad_flat, const kantts_wn_desc* table_dev,
                                 const kantts_wn_bwd_args* args, void* stream);

/* y = sin(x) + x and its backward dx = dy * (cos(x) + 1)  (kantts/models/hifigan/hifigan.py:157) */
int kantts_sinadd_fwd(const float* x, float* y, long long n, void* stream);
int kantts_sinadd_bwd(const float* dy, const float* x, float* dx, long long n, void* stream);

/* Channels-last 1-D convolution with an LDS-resident input window (csrc/conv_win.hip): the im2col-free
 * kernel behind Conv1d / CausalConv1d (kantts/models/hifigan/layers.py:15-91) and their input gradients.
 *   for phase in [0, phases), m in [0, ceil((Tdst - phase) / phases)):      d = m*phases + phase
 *     out[b,d,n] = post( bias[n] + sum_{k : u_k % in_div == 0} sum_c pre(in[b, m*in_mul + u_k/in_div, g*CR + c]) * w[k][n][c] )
 *     u_k = in_add + phase + k*in_kstep;  taps whose source token falls outside [0, Tsrc) contribute 0;
 *     g = n / NG is the group of output channel n (Ntot = groups*NG outputs, Cin_tot = groups*CR inputs).
 *   pre(v)  : LeakyReLU(in_slope) when in_act, then v *= (in_gate > 0 ? 1 : in_gate_slope) when in_gate
 *   post(v) : LeakyReLU(out_slope) when out_act, + res, then *= (out_gate > 0 ? 1 : out_gate_slope)
 * forward : in_mul = stride, in_add = -pad, in_kstep = dilation, in_div = 1, phases = 1
 * dgrad   : in = dy, in_mul = 1, in_add = pad, in_kstep = -dilation, in_div = phases = stride
 * w is tap-major (K, Ntot, CR) fp32.  CR % 4 != 0 (1/2-channel layers) runs a direct one-thread-per-output kernel;
 * otherwise KANTTS_E_UNSUPPORTED when pointers are not 16-byte aligned or K > 64 -- callers then use
 * kantts_gemm_seg_launch. */
typedef struct {
  const float* in;
  const float* in_gate;
  const float* w;
  float* out;
  const float* bias;
  const float* res;
  const float* out_gate;
  int B, Tsrc, Tdst, Cin_tot, Ntot, CR, NG, groups, K;
  int in_mul, in_add, in_kstep, in_div, phases;
  int inner; /* folded axis between time and channels (MPD period): in is (B, Tsrc, inner, Cin_tot), out (B, Tdst, inner, Ntot) */
  int up;    /* > 1: `in` is read through a nearest-neighbour upsampling: token u of the rule above is source token u / up */
  float in_slope;
  int in_act;
  float in_gate_slope;
  float out_slope;
  int out_act;
  float out_gate_slope;
  int precision; /* 0 fp32 MFMA, 1 bf16 MFMA (fp32 accumulate) */
} kantts_conv_args;
int kantts_conv_win_launch(const kantts_conv_args* args, void* stream);

/* Weight / bias gradient of the same convolutions (csrc/conv_wgrad.hip), accumulated (+=) with fp32 atomics:
 *   dw[k][n][c] += sum_{b,p,q} gate(dy[b,q,p,n]) * act(x[b, q*stride + k*dil - pad, p, g*CR + c]),   g = n / NG
 *   db[n]       += sum_{b,p,q} gate(dy[b,q,p,n])                                   (db may be NULL)
 * x is (B, Tsrc, inner, Cin_tot), dy / dy_gate are (B, Tdst, inner, Ntot), dw is tap-major (K, Ntot, CR).
 * gate(v) = v * (dy_gate > 0 ? 1 : dy_gate_slope) when dy_gate is given; act = LeakyReLU(x_slope) when x_act.
 * CR or NG not a multiple of 4 runs a direct kernel (up must be 1); otherwise KANTTS_E_UNSUPPORTED when a
 * pointer is not 16-byte aligned. */
typedef struct {
  const float* x;
  const float* dy;
  const float* dy_gate;
  float* dw;
  float* db;
  int B, Tsrc, Tdst, Cin_tot, Ntot, CR, NG, groups, K;
  int stride, dil, pad, inner;
  int up; /* > 1: x is read through a nearest-neighbour upsampling (virtual token u = source token u / up) */
  float x_slope;
  int x_act;
  float dy_gate_slope;
  int precision; /* 0 fp32 MFMA, 1 bf16 MFMA (fp32 accumulate) */
} kantts_convw_args;
int kantts_conv_wgrad_launch(const kantts_convw_args* args, void* stream);

/* Single-input-channel convolutions (first layer of the HiFi-GAN discriminators; csrc/conv_c1.hip), fp32 streaming kernels.
 * x / dx are (B, Tsrc, inner), y (= dy for the gradients) and gate are (B, Tdst, inner, Cout), w / dw are (Cout, K) row-major.
 *   mode 0  y[b,q,p,n]   = act( bias[n] + sum_k x[b, q*stride + k*dil - pad, p] * w[n][k] )      act = LeakyReLU(out_slope) when out_act
 *   mode 1  dx[b,t,p]   += sum_k sum_n gate(y[b,q,p,n]) * w[n][k]   at t = q*stride + k*dil - pad   (dx must start at zero)
 *   mode 2  dw[n][k]    += sum_{b,q,p} gate(y[b,q,p,n]) * x[b, q*stride + k*dil - pad, p];   db[n] += sum gate(y)   (db may be NULL)
 * gate(v) = v * (gate > 0 ? 1 : gate_slope) when gate is given.
 * KANTTS_E_UNSUPPORTED unless K <= 16, Cout % 4 == 0, Cout <= 256 and 256 % Cout == 0. */
typedef struct {
  const float* x;
  float* dx;
  float* y;
  const float* gate;
  const float* w;
  const float* bias;
  float* dw;
  float* db;
  int B, Tsrc, Tdst, Cout, K, stride, dil, pad, inner;
  float out_slope;
  int out_act;
  float gate_slope;
  void* y_bf16; /* [round 4] mode 0, optional: the bf16 image of y (after the output activation) for the convolution that
                   consumes it -- the second layer of every sub-discriminator otherwise starts with a cast pass over y */
} kantts_conv_c1_args;
int kantts_conv_c1_launch(const kantts_conv_c1_args* args, int mode, void* stream);

/* [round 4] Convolutions with ONE output channel (csrc/conv_n1.hip): the conv_post layers of the generator
 * (kantts/models/hifigan/hifigan.py:178-180: Conv1d(32 -> 1, k = 7) after leaky_relu(x, 0.01)), of the period discriminators
 * (:238-262, Conv2d(1024 -> 1, (3, 1))) and of the scale discriminators (:373-402).  A dot product per output position:
 *   mode 0  y[b,q,p] = bias + sum_k sum_c w[k][c] act(x[b, q*stride + k*dil - pad, p, c])
 *   mode 1  dx[b,t,p,c] = act'(x) sum_k w[k][c] dy[b, (t + pad - k*dil) / stride, p]   (y holds dy; dx fully written)
 *   mode 2  dw[k][c] += sum act(x) dy,  db[0] += sum dy   (y holds dy; dw / db zeroed or accumulating, caller's choice)
 * x (B, Tsrc, inner, Cin) fp32, y (B, Tdst, inner); the weight and its gradient are addressed as w[k * w_ks + c * w_cs]
 * (tap-major (K, 1, Cin): w_ks = Cin, w_cs = 1; parameter layout (1, Cin, K): w_ks = 1, w_cs = K).  act = LeakyReLU(in_slope)
 * when in_act.  KANTTS_E_UNSUPPORTED unless Cin is a power of two in [4, 1024], K <= 8 and (Cin / 4 / min(64, Cin / 4)) * K <= 16. */
typedef struct {
  const float* x;
  float* dx;
  float* y;
  const float* w;
  const float* bias;
  float* dw;
  float* db;
  int B, Tsrc, Tdst, Cin, K, stride, dil, pad, inner;
  int w_ks, w_cs;
  float in_slope;
  int in_act;
} kantts_conv_n1_args;
int kantts_conv_n1_launch(const kantts_conv_n1_args* args, int mode, void* stream);

/* Free-running inference steps.
 * kantts_attn_decode: one query per sequence (decoder position `step`) against rows [lo, hi] of a (B, L, .) K/V
 *   buffer; the interval is the training kernels' function of (mode, step, len, bw) (HybridAttentionDecoder.infer,
 *   kantts/models/sambert/kantts_sambert.py:208-253; K/V state sambert/__init__.py:212-258).  q / o hold B rows
 *   (row b at ptr[b*ld + h*16 + d]); no dropout, no lse.  Band modes: a sequence with step >= len gets context 0.
 *   0 <= step < L, else KANTTS_E_BADARG; an ld that is not a multiple of 4: KANTTS_E_BADARG; d_head != 16:
 *   KANTTS_E_UNSUPPORTED (the codes of the training entry points).
 *   bw_seq (optional, B entries) gives every sequence its own band width: the reference infers one utterance at a
 *   time with the band of THAT utterance, which a batch can only reproduce per sequence.
 * kantts_lstm_cell: gates (B, 4H) in PyTorch order [i|f|g|o] -> h, c (VarRnnARPredictor.infer, adaptors.py:67-83). */
int kantts_attn_decode(const float* q, const float* k, const float* v, int ldq, int ldk, int ldv, float* o, int ldo,
                       const int32_t* lens, const int32_t* bw_seq, int B, int H, int L, int d_head, int mode, int step,
                       int bw, void* stream);
int kantts_lstm_cell(const float* gates, const float* c_prev, float* h_out, float* c_out, int B, int H, void* stream);

/* Monotonic alignment search, width 1 (csrc/mas.hip): replaces the host round trip of binarize_attention_parallel
 * (kantts/models/sambert/kantts_sambert.py:752-764 -> numba b_mas, alignment.py:32-71).  attn / opt are (B, To_max, Ti_max)
 * (the reference's (B, 1, mel, text) with the singleton squeezed); opt receives the 0/1 hard alignment of the valid
 * (out_lens[b] x in_lens[b]) corner and zeros elsewhere; workspace: B*To_max*Ti_max*4 bytes (float logs, or byte
 * back-pointers on the wide-map fallback). */
int kantts_mas_width1(const float* attn, const int32_t* in_lens, const int32_t* out_lens, float* opt, void* workspace,
                      int B, int To_max, int Ti_max, void* stream);

/* Alignment attention of the MAS path (csrc/mas.hip): the part of ConvAttention.forward after the projections
 * (kantts/models/sambert/attention.py:103-125).  q (B,T1,C) mel-side / k (B,T2,C) text-side encodings, channels last;
 * prior (B,T1,T2) or NULL; in_lens[b] = unpadded text length (positions >= it are masked out of `soft`).
 * logprob = attn_logprob, soft = attn of the reference, both (B,T1,T2) (= (B,1,T1,T2)).  T2 <= 1024.
 * bwd: d_logprob / d_soft may be NULL; g_ws: B*T1*T2 floats of workspace; dq / dk are overwritten. */
int kantts_align_attn_fwd(const float* q, const float* k, const float* prior, const int32_t* in_lens, float* logprob,
                          float* soft, int B, int T1, int T2, int C, void* stream);
int kantts_align_attn_bwd(const float* q, const float* k, const float* prior, const float* logprob, const float* soft,
                          const float* d_logprob, const float* d_soft, float* g_ws, float* dq, float* dk, int B, int T1,
                          int T2, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Contractions with bf16 operands in HBM (round 2; csrc/gemm_bf16.hip).  Same reference call sites as the segmented
 * GEMM above (nn.Linear / Conv1d k=1,3 forward, input gradient, weight gradient:
 * kantts/models/sambert/__init__.py:82,102,115-127,217,242,287,297; fsmn.py:14-29; kantts_sambert.py:173-174),
 * used when the numerics mode is bf16: weights come from the parameter arena's bf16 shadow, activations that only feed
 * contractions are stored bf16 by their producers.  All extents / leading dimensions are multiples of 8 elements and
 * all base pointers 16-byte aligned (KANTTS_E_UNSUPPORTED otherwise: the caller falls back to the segmented GEMM).
 *
 * kantts_bgemm_nt:  C[i][j] = epilogue( sum_s sum_k A_s[tok(i) + a_shift_s][k] * B_s(j, k) )
 *   A_s: (M, klen_s) rows of bf16 (or fp32 when a_f32: rounded to bf16 once per tile), row stride lda.
 *   B_s: b_kn = 0: (N, klen_s) k-contiguous, row stride ldb (forward: the weight);
 *        b_kn = 1: (klen_s, N) n-contiguous, row stride ldb (input gradient through the same weight buffer).
 *   a_shift: conv tap -- row i reads token i + a_shift of its own sequence of T tokens, zero outside [0, T).  M need not be a
 *            multiple of T, but A then holds every row of the last sequence: rows up to ceil(M / T) * T - 1 may be read.
 *   epilogue: v = (acc + bias[j] + bias2[j]) * alpha; relu; dropout(drop_p; element i*N + j of drop_seed + *seed_dev);
 *             v += res[i][j] (fp32); v = gate[i][j] > 0 ? v : 0 (ReLU backward on a saved activation); rowmask[i] -> 0;
 *             stored as bf16 (c_bf16) or fp32.
 *   a_drop_p > 0 (a_f32 only): A is an incoming gradient through an epilogue dropout of the forward pass; element
 *             (i, k) is multiplied by the keep-scale regenerated from (a_drop_seed + *seed_dev, i * a_drop_ld + k); under a
 *             tap shift i is the row that is READ (i + a_shift), the index the forward pass gave that element.
 *   After the KANTTS_E_BADARG checks (nseg, negative M / N, c NULL) M == 0 or N == 0 returns KANTTS_OK before any other
 *   check and writes nothing.
 */
#define KANTTS_BGEMM_MAX_SEG 12
typedef struct kantts_bgemm_seg {
  const void* a;
  const void* b;
  int64_t lda, ldb;
  int32_t klen;
  int32_t a_shift;
} kantts_bgemm_seg;

typedef struct kantts_bgemm_args {
  kantts_bgemm_seg seg[KANTTS_BGEMM_MAX_SEG];
  int32_t nseg, M, N, T;
  int32_t a_f32, b_kn;
  void* c;
  int64_t ldc;
  int32_t c_bf16;
  int32_t relu;
  const float* bias;
  const float* bias2;
  float alpha;
  float drop_p;
  uint64_t drop_seed;
  const uint64_t* seed_dev;
  const float* res;
  int64_t ldr;
  const void* gate;
  int64_t ldg;
  int32_t gate_bf16;
  float a_drop_p;
  uint64_t a_drop_seed;
  int64_t a_drop_ld;
  const uint8_t* rowmask;
  /* optional: LayerNorm(128) of the output rows in the epilogue (N == 128, fp32 c): the pre-LN sub-layer that consumes c
   * (kantts/models/sambert/__init__.py:130-131, 198) then needs no launch of its own.  ln_out (M,128) bf16 / fp32,
   * ln_mean / ln_rstd (M) as kantts_ln128_fwd writes them (its backward is unchanged). */
  const float* ln_gamma;
  const float* ln_beta;
  void* ln_out;
  int32_t ln_out_bf16;
  float ln_eps;
  float* ln_mean;
  float* ln_rstd;
} kantts_bgemm_args;
int kantts_bgemm_nt(const kantts_bgemm_args* args, void* stream);
/* Two kantts_bgemm_nt problems in ONE launch (third grid dimension = problem): each is checked and computed exactly as its
 * own kantts_bgemm_nt call (same bits), with its own operands, epilogue options and dropout seed.  Both must have the same
 * M, N, A dtype (a_f32), b_kn and tile choice, else KANTTS_E_UNSUPPORTED (nothing is launched); so is KANTTS_BGEMM_BM=128. */
int kantts_bgemm_nt_pair(const kantts_bgemm_args* a, const kantts_bgemm_args* b, void* stream);

/* kantts_bgemm_nt with the BACKWARD of a LayerNorm(128) as its epilogue.  The contraction's result (N == 128, b_kn) is
 * the gradient dy of a LayerNorm's output -- the input gradient of the projection that consumes the normalised rows of a
 * pre-LN sub-layer (kantts/models/sambert/__init__.py:63-64, 89-91, 198-199) -- and what the launch writes is what
 * kantts_ln128_bwd_rows makes of it: dx (M,128) fp32 (+ dres; rows of zero_rows written as 0) and the dgamma / dbeta
 * accumulations.  dy is rounded to bf16 first when args->c_bf16 is set (the value the two-launch form passes through
 * memory) and is itself stored only if args->c is not NULL.  args->ln_out / gate / relu / drop_p must be unset. */
typedef struct kantts_lnbwd_args {
  const float* x;        /* (M,128) the LayerNorm's input */
  const float* gamma;    /* (128) */
  const float* mean;     /* (M) as kantts_ln128_fwd wrote them */
  const float* rstd;
  const float* dres;     /* optional (M,128): gradient of the residual branch that by-passes the normalisation */
  const uint8_t* zero_rows; /* optional (M) */
  float* dx;             /* (M,128) */
  float* dgamma_accum;   /* (128), += */
  float* dbeta_accum;
  float* part_rows;      /* [round 5] optional (ceil(M / 32), 256): when set, workgroup w writes its 128 dgamma + 128 dbeta sums
                          * to row w INSTEAD of adding them to the accumulators (256 atomics per workgroup on the same 256
                          * addresses serialise in L2); the caller adds the rows: kantts_rows_sum_accum */
} kantts_lnbwd_args;
int kantts_bgemm_nt_lnbwd(const kantts_bgemm_args* args, const kantts_lnbwd_args* ln, void* stream);

/* kantts_bgemm_tn:  c[n*c_ns + k*c_ks + tap*c_ts] += alpha * sum_m A[m][n] * B[tok(m) + shift0 + tap*shift_step][k]
 *                   db[n] += alpha * sum_m A[m][n]                                   (optional)
 * Weight / bias gradients: A = gradient of the layer output (M, N), B = layer input (M, K), tokens m are the reduction
 * axis; fp32 atomics into a pre-zeroed gradient that may already be in the parameter's own layout (strides c_*).
 * A / B are bf16 or fp32 (a_f32 / b_f32); a_drop_* as above with the logical index m*N + n.  slices = 0 lets the
 * library choose the token split.  Operands given as fp32 are rounded to bf16 (ties to even) when staged, A after its
 * keep-scale; db is the sum of that rounded, dropped A, and alpha applies to db as it does to c.  As for kantts_bgemm_nt, B
 * holds every row of the last sequence when M is no multiple of T.  After the KANTTS_E_BADARG checks (negative M, N < 1,
 * K < 1, ntaps < 1, nprob) M == 0 returns KANTTS_OK before any other check and writes nothing. */
typedef struct kantts_bgemm_tn_args {
  const void* a;
  const void* b;
  int64_t lda, ldb;
  int32_t M, N, K, T;
  int32_t a_f32, b_f32;
  int32_t ntaps, shift0, shift_step, slices;
  float* c;
  int64_t c_ns, c_ks, c_ts;
  float* db;
  float alpha;
  float a_drop_p;
  uint64_t a_drop_seed;
  const uint64_t* seed_dev;
} kantts_bgemm_tn_args;
int kantts_bgemm_tn(const kantts_bgemm_tn_args* args, void* stream);

/* Up to KANTTS_TN_MAX_GROUP weight gradients of ONE shape (shape / dtypes / strides / alpha / dropout probability from
 * *shape; operand, output, bias-gradient pointers and dropout seeds per problem, arrays in HOST memory) in a single
 * launch.  The host layer defers the weight gradients of a backward pass and issues them grouped by shape. */
#define KANTTS_TN_MAX_GROUP 16
int kantts_bgemm_tn_grouped(const kantts_bgemm_tn_args* shape, int nprob, const void* const* a_host, const void* const* b_host,
                            float* const* c_host, float* const* db_host, const uint64_t* a_drop_seed_host, void* stream);

/* fp32 -> bf16 (round to nearest even) over n elements (n % 8 == 0, 16-byte aligned): the parameter arena's shadow. */
int kantts_cast_f32_bf16(const float* src, void* dst_bf16, long long n, void* stream);

/* Conv1d weights (N, Cin, KT) fp32 at src + src_off -> tap-major (KT, N, Cin) bf16 at dst + dst_off, one table entry
 * per weight (table in device memory), one launch for all of them (kantts/models/sambert/__init__.py:115-127).
 * Element-wise accesses: N, Cin, KT and both offsets need no granularity or alignment beyond that of their element type. */
typedef struct kantts_tapmajor_desc {
  int64_t src_off, dst_off;
  int32_t N, Cin, KT, pad_;
} kantts_tapmajor_desc;
int kantts_tapmajor_bf16(const float* src, void* dst_bf16, const kantts_tapmajor_desc* table_dev, int ndesc,
                         int blocks_per_desc, void* stream);

/* dz = (y > 0) ? dy * scale : 0 over n elements (n % 8 == 0), bf16 output: ReLU (+ dropout: scale = 1/(1-p), y is the
 * post-dropout activation) backward of a fused linear whose output was stored for the gate
 * (kantts/models/sambert/__init__.py:40-49,141-142). */
int kantts_relu_gate_bf16(const void* dy, int dy_bf16, const void* y, int y_bf16, void* dz_bf16, float scale, long long n,
                          void* stream);

/* kantts_ffn_pair: the two contractions of a position-wise feed-forward block in one launch
 * (kantts/models/sambert/__init__.py:134-149; forward and, with `gate`, the input-gradient pass).
 *   phase 1   t[m][f] = epi1( sum_tap x[m + tap - pad][:] . w1[tap][f][:] )          m < M, f < F, reduction K1 = 128
 *             forward  (gate == NULL): epi1 = rowmask1( dropout_{drop1}( relu?( . + bias1 ) ) )
 *             backward (gate != NULL): epi1 = gate[m][f] > 0 ? alpha1 * . : 0                      (KT == 1 only)
 *   phase 2   y[m][n] = rowmask2( dropout_{drop2}( t[m][:] . w2[n][:] + bias2 ) + res[m][n] )      n < N = 128
 * x: (M, 128) bf16 or fp32 (x_f32; fp32 rows may carry a regenerated dropout xdrop_* with index m*128 + k and are zeroed
 * where xrowmask[m] != 0).  w1: the (KT*F, 128) matrix [tap*F + f][k], w2: the (128, F) matrix [n][f], both bf16 in the
 * FRAGMENT-MAJOR layout of kantts_fragmajor_bf16 -- the backward pass hands in the transposed weights (w1 := W2^T as
 * (F, 128), w2 := W1^T as (128, F)).  t_out (optional): bf16 (M, F) row-major, the intermediate the weight gradients need.
 * Taps do not cross sequence boundaries: rows are B sequences of T tokens.  Dropout indices: m*F + f (drop1), m*128 + n
 * (drop2); seeds are offset by *seed_dev (graph replay).  KT2 = 3 (backward form only, M % T == 0): phase 2
 * sums three taps of the intermediate, w2 = three (128, F) images -- the input gradient of a k = 3 first convolution.
 * Geometries (K1, N, F): (128, 128, 1024) -- everything above (the widths written as 128 are K1 / N in general); and the FSMN
 * feed-forward nets (256, 256, 512) and (128, 128, 256) with KT = 1, KT2 <= 1 only, without ln_*, xdrop, xrowmask, rowmask1 /
 * rowmask2: forward form (bias1, relu, drop1; t_out may be NULL: the intermediate is then not written) and backward form
 * (gate, alpha1, t_out = dz, res = fp32 addend at row pitch ldr).  Returns KANTTS_E_UNSUPPORTED for anything else: the
 * caller falls back to two kantts_bgemm_nt launches. */
typedef struct kantts_ffn_args {
  const void* x;
  int64_t ldx;
  int32_t x_f32;
  int32_t M, T, K1, F, N, KT, pad;
  const void* w1;
  const void* w2;
  const float* bias1;
  const float* bias2;
  int32_t relu;
  float alpha1;
  float drop1_p;
  float drop2_p;
  float xdrop_p;
  uint64_t drop1_seed;
  uint64_t drop2_seed;
  uint64_t xdrop_seed;
  const uint64_t* seed_dev;
  const void* gate;
  const uint8_t* rowmask1;
  const uint8_t* rowmask2;
  const uint8_t* xrowmask;
  void* t_out;
  const float* res;
  int64_t ldr;
  void* y;
  int64_t ldy;
  int32_t y_bf16;
  int32_t KT2, s2_first, s2_step; /* taps of phase 2 (0 / 1: none): y[m] = sum_t t[m + s2_first + t*s2_step] . w2[t]^T */
  /* optional (forward form, KT2 <= 1): LayerNorm(128) of the output rows in the epilogue, as kantts_bgemm_args ln_* --
   * the block's output feeds the next block's pre-LN attention sub-layer (kantts/models/sambert/__init__.py:63, 198) */
  const float* ln_gamma;
  const float* ln_beta;
  void* ln_out;
  int32_t ln_out_bf16;
  float ln_eps;
  float* ln_mean;
  float* ln_rstd;
} kantts_ffn_args;
int kantts_ffn_pair(const kantts_ffn_args* args, void* stream);
/* Two kantts_ffn_pair problems of the (K1, N, F) = (128, 128, 256) geometry in ONE launch (second grid dimension = problem):
 * each is checked and computed exactly as its own kantts_ffn_pair call (same bits).  Both must have the same M and the same
 * form (forward: no gate; backward: gate); another geometry or a mismatch is KANTTS_E_UNSUPPORTED and launches nothing. */
int kantts_ffn_pair2(const kantts_ffn_args* a, const kantts_ffn_args* b, void* stream);

/* [round 5] One PNCA decoder block forward as ONE launch (csrc/pnca_block.hip; reference
 * kantts/models/sambert/__init__.py:212-348 with the feed-forward of :134-149; band masks kantts_sambert.py:135-166):
 *   [q|k|v] = xn Wqkv^T + bqkv;  ox / oh = x-band / memory-band attention (csrc/attn.hip conventions, 8 heads x 16);
 *   y1 = rowmask(dropout_fc(ox Wfcx^T + oh Wfch^T + bfcx + bfch) + x);  xn1 = LN1(y1);
 *   hid = rowmask(dropout_1(relu(xn1 W1^T + b1)));  out = rowmask(dropout_2(hid W2^T + b2) + y1);  ln2_out = LN2(out).
 * x (M, 128) fp32 block input and xn (M, 128) bf16 its LayerNorm (M = B * L rows); hkv: this block's memory K | V rows,
 * fp32, row pitch ldh >= 256 floats; wqkv (384 x 128), wfcx / wfch (128 x 128), w1 (1024 x 128), w2 (128 x 1024):
 * fragment-major bf16 images (kantts_fragmajor_bf16).  Written for the backward pass (each optional unless noted): qkv
 * (M, 384) fp32, ox / oh (M, 128) fp32 (required), lse_x / lse_h (B, 8, L) (required), y1 fp32, xn1 bf16 + mean1 / rstd1,
 * hid (M, 1024) bf16; out (M, 128) fp32 (required); ln2_* as the ln_* fields of kantts_ffn_args.  Dropout seeds are offset
 * by *seed_dev; indices are those of the separate launches (kantts_pnca_attn_fwd, kantts_bgemm_nt, kantts_ffn_pair), so the
 * fused launch and the chain draw the same masks.  bw_dev (device scalar) overrides bw_x / bw_h.  Band widths above 16 are
 * not supported: KANTTS_E_UNSUPPORTED when known on the host, NaN outputs when only the device knows. */
typedef struct kantts_pnca_block_args {
  const float* x;
  const void* xn;
  const float* hkv;
  int64_t ldh;
  int32_t B, L, H, C, F;
  const int32_t* lens;
  const int32_t* bw_dev;
  int32_t bw_x, bw_h;
  const uint8_t* rowmask;
  const void* wqkv;
  const float* bqkv;
  const void* wfcx;
  const void* wfch;
  const float* bfcx;
  const float* bfch;
  const float* ln1_gamma;
  const float* ln1_beta;
  float ln1_eps;
  const void* w1;
  const void* w2;
  const float* bias1;
  const float* bias2;
  float att_p, fc_p, drop1_p, drop2_p;
  uint64_t seed_x, seed_h, fc_seed, drop1_seed, drop2_seed;
  const uint64_t* seed_dev;
  float* qkv;
  float* ox;
  float* oh;
  float* lse_x;
  float* lse_h;
  float* y1;
  void* xn1;
  float* mean1;
  float* rstd1;
  void* hid;
  float* out;
  const float* ln2_gamma;
  const float* ln2_beta;
  void* ln2_out;
  int32_t ln2_out_bf16;
  float ln2_eps;
  float* ln2_mean;
  float* ln2_rstd;
} kantts_pnca_block_args;
int kantts_pnca_block_fwd(const kantts_pnca_block_args* args, void* stream);

/* [round 5] The row-local half of a PNCA block's backward as one launch (csrc/pnca_block.hip): kantts_ffn_pair (backward
 * form) + kantts_ln128_bwd_rows + the two input-gradient launches of the output projection, same arithmetic
 * (kantts/models/sambert/__init__.py:134-149, 286-306 differentiated):
 *   dz = gate_{hid > 0}(dropout_2(dy) W2) * alpha1 (bf16, (M, 1024); the weight gradient of W1 reads it);
 *   dh = dz W1 (rounded to bf16);  g1 = rowmask(LN1'(dh; y1, mean1, rstd1, gamma1) + dy) (fp32 (M, 128));
 *   d_ox = dropout_fc(g1) Wfcx, d_oh = dropout_fc(g1) Wfch (fp32 (M, 128)).  The gradients of LN1's gamma / beta leave as
 *   PARTIAL ROWS: workgroup w writes 128 dgamma sums and 128 dbeta sums of its 32 rows to ws[w*256 ..]; the caller adds the
 *   rows (kantts_rows_sum_accum) -- same-address atomics from 204 workgroups cost half of the launch.
 * dy: gradient of the block output (rows of rowmask are read as zero).  wt2 = W2^T (1024 x 128), wt1 = W1^T (128 x 1024),
 * wfcxT / wfchT = Wfcx^T / Wfch^T (128 x 128): fragment-major bf16 images.  Dropout indices as in the forward launches. */
typedef struct kantts_pnca_block_bwd_args {
  const float* dy;
  const void* hid;
  const float* y1;
  const float* mean1;
  const float* rstd1;
  const float* ln1_gamma;
  const uint8_t* rowmask;
  int32_t M, C, F;
  const void* wt2;
  const void* wt1;
  const void* wfcxT;
  const void* wfchT;
  float alpha1, drop2_p, fc_p;
  uint64_t drop2_seed, fc_seed;
  const uint64_t* seed_dev;
  void* dz;
  float* g1;
  float* d_ox;
  float* d_oh;
  float* ws;            /* caller-owned, >= kantts_pnca_block_bwd_ws_floats(M) floats, 16-byte aligned: ceil(M / 32) rows */
  long long ws_floats;  /* of [128 dgamma | 128 dbeta] partial sums, every element written */
} kantts_pnca_block_bwd_args;
int kantts_pnca_block_bwd(const kantts_pnca_block_bwd_args* args, void* stream);
long long kantts_pnca_block_bwd_ws_floats(int M);
/* [round 5] The cross-row half of a PNCA block's backward as one launch (csrc/pnca_block.hip): kantts_pnca_attn_bwd +
 * kantts_bgemm_nt_lnbwd of the chain, same arithmetic and conventions (kantts/models/sambert/__init__.py:212-306
 * differentiated; band masks kantts_sambert.py:135-166):
 *   dqkv (M, 384) fp32 = [query | key | value] gradients of both attention bands (the memory band's query gradient added);
 *   dhkv: gradient of this block's memory K | V rows, row pitch lddh;
 *   dx (M, 128) = rowmask_{zero_rows}(LN0'(bf16(dqkv Wqkv); x, mean0, rstd0, gamma0) + dres);
 *   ws: ceil(M / 32) partial rows of [128 dgamma0 | 128 dbeta0] (kantts_rows_sum_many).
 * wqkvT: fragment-major bf16 image of Wqkv^T (128 x 384).  Band widths above 16: KANTTS_E_UNSUPPORTED / NaN as the forward. */
typedef struct kantts_pnca_attn_bwd_args {
  const float* qkv;
  const float* hkv;
  int64_t ldh;
  const float* ox;
  const float* oh;
  const float* d_ox;
  const float* d_oh;
  const float* lse_x;
  const float* lse_h;
  int32_t B, L, H, C;
  const int32_t* lens;
  const int32_t* bw_dev;
  int32_t bw_x, bw_h;
  float att_p;
  uint64_t seed_x, seed_h;
  const uint64_t* seed_dev;
  const void* wqkvT;
  const float* x;
  const float* mean0;
  const float* rstd0;
  const float* ln0_gamma;
  const float* dres;
  const uint8_t* zero_rows;
  float* dqkv;
  float* dhkv;
  int64_t lddh;
  float* dx;
  float* ws;
  long long ws_floats;
} kantts_pnca_attn_bwd_args;
int kantts_pnca_attn_qkv_bwd(const kantts_pnca_attn_bwd_args* args, void* stream);
/* The seam between two blocks of a stack's backward as one launch (csrc/pnca_block.hip: pnca_bwd_seam_kernel):
 * kantts_pnca_attn_qkv_bwd(upper) followed by kantts_pnca_block_bwd(lower), where the lower block's dy IS the upper block's
 * dx.  The row-local half reads of the block above nothing but the 32 dx rows its own workgroup has just produced, so the
 * two halves run back to back on every tile without a launch boundary; both are the code of the separate launches and every
 * value those write -- dqkv, dhkv, dx and the upper partial rows; dz, g1, d_ox, d_oh and the lower partial rows -- is written
 * here bit for bit (dx too: the lower block's weight gradient and the caller read it).  lower->dy is not read.
 * Requires lower->dy == upper->dx and lower->M == upper->B * upper->L (else KANTTS_E_BADARG) and everything the two entry
 * points require of their own arguments, checked in that order -- upper first -- with the codes they return (C == 128,
 * F == 1024, H == 8, band widths <= 16 unless device-resident, row pitches, 16-byte alignment: KANTTS_E_UNSUPPORTED; NULL
 * operands: KANTTS_E_BADARG; either workspace short of kantts_pnca_block_bwd_ws_floats(M): KANTTS_E_WORKSPACE).  A refused
 * call launches nothing.  M == 0: KANTTS_OK, nothing is launched. */
int kantts_pnca_bwd_seam(const kantts_pnca_attn_bwd_args* upper, const kantts_pnca_block_bwd_args* lower, void* stream);

/* For each of n problems: dst0[c] += sum_r src[r*cols + c] for c < split, dst1[c - split] += ... for c >= split (fixed
 * summation order) -- the partial rows of kantts_pnca_block_bwd / kantts_bgemm_nt_lnbwd, many of them in one launch. */
#define KANTTS_ROWSUM_MAX 32
typedef struct kantts_rowsum_args {
  int32_t n, cols, split;
  int32_t rows[KANTTS_ROWSUM_MAX];
  const float* src[KANTTS_ROWSUM_MAX];
  float* dst0[KANTTS_ROWSUM_MAX];
  float* dst1[KANTTS_ROWSUM_MAX];
} kantts_rowsum_args;
int kantts_rows_sum_many(const kantts_rowsum_args* args, void* stream);

/* Fragment-major bf16 images of weight matrices, a table of them in one launch (the parameter arena's per-step refresh).
 * Entry: the (R, K) matrix with element (r, k) = src[src_off + r*sr + k*sk] (fp32; any orientation of the master weight)
 * is written to dst + dst_off so that every 16 x 32 block (r/16, k/32) is 1 KB in the order one A-operand load of
 * v_mfma_f32_16x16x32_bf16 reads it: dst[((r/16)*(K/32) + k/32)*512 + (((k%32)/8)*16 + r%16)*8 + k%8].
 * R % 16 == 0, K % 32 == 0. */
typedef struct kantts_fragmajor_desc {
  int64_t src_off, dst_off;
  int64_t sr, sk;
  int32_t R, K;
} kantts_fragmajor_desc;
int kantts_fragmajor_bf16(const float* src, void* dst_bf16, const kantts_fragmajor_desc* table_dev, int ndesc,
                          int blocks_per_desc, void* stream);

/* nn.LayerNorm(128, eps) forward / backward, 16 lanes per row; the output (and the incoming gradient) may be bf16 because
 * LayerNorm outputs only feed contractions (kantts/models/sambert/__init__.py:63,130,198; kantts_sambert.py:58,128). */
int kantts_ln128_fwd(const float* x, const float* gamma, const float* beta, void* y, int y_bf16, float* mean, float* rstd,
                     int M, float eps, void* stream);
/* dres (optional, fp32 (M,128)): gradient of a residual branch taken from the same x; dx = LN-gradient + dres in one pass. */
int kantts_ln128_bwd(const void* dy, int dy_bf16, const float* x, const float* gamma, const float* mean, const float* rstd,
                     const float* dres, float* dx, float* dgamma_accum, float* dbeta_accum, int M, void* stream);
/* ... and zero_rows (optional, uint8 (M)): rows of dx written as 0.  A pre-LN sub-layer's input x is the output of the
 * previous sub-layer, which zeroes the padded rows of its output (kantts/models/sambert/__init__.py:177-178, 340-341) and
 * therefore of its incoming gradient: when this LayerNorm is the only consumer of x, that masking is this kernel's store
 * instead of a separate pass over the gradient. */
int kantts_ln128_bwd_rows(const void* dy, int dy_bf16, const float* x, const float* gamma, const float* mean,
                          const float* rstd, const float* dres, float* dx, float* dgamma_accum, float* dbeta_accum,
                          const unsigned char* zero_rows, int M, void* stream);

/* Backward of kantts_melspec_fwd's magnitude output (the reference's stft(), kantts/utils/audio_torch.py:8-31:
 * sqrt(clamp(re^2 + im^2, eps_power))): dwav_accum (B,T) += d loss / d wav given dmag (B, frames, n_fft/2+1).  Gradient
 * path of STFTLoss / MultiResolutionSTFTLoss (kantts/train/loss.py:312-441); zero where the clamp is active. */
int kantts_stft_mag_bwd(const float* wav, const float* dmag, int B, int T, int n_fft, int hop, int frames, int pad_mode,
                        const float* window, const float* twiddle, float eps_power, float* dwav_accum, void* stream);

/* out[0] = sum x^2 with a fixed summation order (bit-reproducible: data-parallel replicas must derive the same
 * clipping factor from the same all-reduced gradient).  workspace: >= 1025 floats, zero before the first call (word 0 is
 * a ticket counter the kernel resets itself).  kantts/train/trainer.py:997-1004 (clip_grad_norm_). */
int kantts_sumsq_det(const float* x, float* out, float* workspace, long long ws_floats, long long n, void* stream);

/* ------------------------------------------------------------------------------------------
 * Free-running decode with the step index in device memory (csrc/decode.hip; BASELINE config 5): one decoder step is a
 * static launch sequence that a hipGraph replays per step.  `step_dev` (int32 device scalar) overrides `step` when set.
 *
 * kantts_pnca_decode_step -- MultiHeadPNCAAttention under update_x_state / update_h_state
 *   (kantts/models/sambert/__init__.py:217-306): qkv (B, 3*H*16) rows = this step's [q | k | v]; k / v are appended to
 *   xkv_cache (B, L, 2*H*16) at row `step`; ox / oh (B, H*16) = causal-band attention over the cache and look-ahead-band
 *   attention over the memory projections hkv (B, L, 2*H*16).  Padded queries (step >= lens[b]) give 0.
 * kantts_step_rows -- dst[b*dst_bs + step*dst_ss + e] = src[b*src_bs + step*src_ss + e], e < n  (memory[:, step, :] gather,
 *   output-frame scatter; kantts_sambert.py:589-603).
 * kantts_step_rowmask -- mask[b] = step >= lens[b]. */
int kantts_pnca_decode_step(const float* qkv, int ldq, float* xkv_cache, const float* hkv, float* ox, float* oh,
                            const int32_t* lens, const int32_t* bw_seq, int B, int H, int L, int d_head, int step,
                            const int32_t* step_dev, int bw, void* stream);
int kantts_step_rows(const float* src, float* dst, int B, int n, long long src_batch_stride, long long dst_batch_stride,
                     long long src_step_stride, long long dst_step_stride, int step, const int32_t* step_dev, void* stream);
int kantts_step_rowmask(const int32_t* lens, uint8_t* mask, int B, int step, const int32_t* step_dev, void* stream);

/* [round 4] HiFi-GAN multi-receptive-field fusion (kantts/models/hifigan/hifigan.py:160-176: xs += resblock(x) over the
 * num_kernels residual stacks of a stage, then xs / num_kernels): out = scale * sum_k xs[k] in one pass, optionally with the
 * bf16 image of LeakyReLU(out, slope) that the next convolution reads (act_bf16 may be NULL).  xs_host / outs_host: HOST
 * arrays of n <= 8 DEVICE pointers; numel % 4 == 0, 16-byte aligned buffers.
 * kantts_scale_to_many: its backward -- outs[k] = scale * g for every k (each branch its own gradient buffer). */
int kantts_mean_many(const float* const* xs_host, int n, float scale, float* out, void* act_bf16, float slope,
                     long long numel, void* stream);
int kantts_scale_to_many(const float* g, float scale, float* const* outs_host, int n, long long numel, void* stream);

/* ------------------------------------------------------------------------------------------
 * HiFi-GAN upsampling as an HBM stream (csrc/upsample.hip): CausalConvTranspose1d with kernel 2*S, stride S
 * (kantts/models/hifigan/layers.py:125-165, hifigan.py:67-80,160) in polyphase form on bf16 activations:
 *   out[(b*T + t)*S + r][co] = bias[co] + sum_{j=0,1} sum_ci lrelu(x[b*T + t - j][ci]) * w[ci][co][r + j*S]  (+ res)
 * x (B*T, Cin) bf16; wp (S*Cout, 2*Cin) bf16 = the weight with rows permuted for 16-byte stores: row mt*16 + rho,
 * mt = (r*(Cout/32) + cb)*2 + h, holds output channel cb*32 + (rho >> 2)*8 + h*4 + (rho & 3) of phase r; column j*Cin + ci
 * holds w[ci][co][r + j*S].  out / res (B*T*S, Cout) bf16 (out_bf16) or fp32.  in_slope = 1 for pre-activated input.
 * Shapes: (Cin, Cout, S) in {(128, 64, 2), (64, 32, 2)}; wider layers are contractions (kantts_bgemm_nt, two segments). */
int kantts_upsample_stream(const void* x_bf16, const void* wp_bf16, const float* bias, const void* res, void* out, int B,
                           int T, int Cin, int Cout, int S, float in_slope, int out_bf16, void* stream);
/* y = sin(x) + x (hifigan.py:157) and act = bf16(LeakyReLU(y, slope)) in one pass. */
int kantts_sinadd_lrelu_fwd(const float* x, float* y, void* act_bf16, float slope, long long n, void* stream);

/* y[i] = x[i] * keep_{p1,seed1}(i) * keep_{p2,seed2}(i) (+ res[i]): two stacked dropouts and a residual add in one pass
 * with regenerated masks -- FsmnEncoderV2 / MemoryBlockV2 (kantts/models/sambert/fsmn.py:66-70,114-121).  The backward
 * is the same call with x := dy, res := NULL.  n % 4 == 0, 16-byte aligned; seeds are offset by *seed_dev. */
int kantts_dropout2_add(const float* x, const float* res, float* y, long long n, float p1, uint64_t seed1, float p2,
                        uint64_t seed2, const uint64_t* seed_dev, void* stream);

/* ------------------------------------------------------------------------------------------
 * bf16 convolution contractions for the HiFi-GAN layers (csrc/cconv.hip, round 3): the same token rule as
 * kantts_conv_win_launch, but both operands are bf16 IN MEMORY (activations pre-activated by their producer, weights a
 * bf16 tap-major image) and are copied global -> LDS by `global_load_lds` (16 bytes per lane, no VGPR staging, no
 * conversion); a tile's rows run across batch items, padding / phase / group edges are lanes whose source address is a
 * 16-byte block of zeros.  Replaces Conv1d / CausalConv1d / the (k,1) Conv2d of the period discriminators / the
 * polyphase form of ConvTranspose1d and their input gradients (kantts/models/hifigan/layers.py:15-165,
 * hifigan.py:200-267,305-407) for channel counts that are multiples of 8.
 *   for phase in [0, phases), m in [0, ceil((Tdst - phase) / phases)):      d = m*phases + phase
 *     v[b,d,p,n] = bias[n] + sum_{k : u_k % in_div == 0} sum_c in[b, (m*in_mul + u_k/in_div) / up, p, g*CR + c] * w[k][n][c]
 *     u_k = in_add + phase + k*in_kstep;  virtual source tokens outside [0, Tsrc*up) contribute 0;  g = n / NG
 *     v = LeakyReLU(v, out_slope) when out_act;  v += res;  v *= (out_gate > 0 ? 1 : out_gate_slope)
 *     (res_after_gate: the residual is added after the gate instead -- identity path of a gated input gradient)
 *     out[b,d,p,n] = v (fp32, optional);  out_bf[b,d,p,n] = bf16(bf_act ? LeakyReLU(v, bf_slope) : v) (optional)
 * in (B, Tsrc, inner, Cin_tot) bf16;  w (K, Ntot, CR) bf16;  bias / res fp32;  out_gate bf16 (out_gate_bf16) or fp32.
 * KANTTS_E_UNSUPPORTED unless CR % 8 == 0, NG % 8 == 0, K <= 64, phases <= 8 and all pointers are 16-byte aligned. */
typedef struct {
  const void* in;
  const void* w;
  const float* bias;
  const float* res;
  const void* out_gate;
  float* out;
  void* out_bf;
  int B, Tsrc, Tdst, Cin_tot, Ntot, CR, NG, groups, K;
  int in_mul, in_add, in_kstep, in_div, phases;
  int inner;
  int up;
  float out_slope;
  int out_act;
  float out_gate_slope;
  int out_gate_bf16;
  float bf_slope;
  int bf_act;
  int tile; /* 0 = automatic; else BM*1000 + BN of a compiled tile (bench / tests) */
  int res_after_gate;
} kantts_cconv_args;
int kantts_cconv_launch(const kantts_cconv_args* args, void* stream);

/* Weight / bias gradients of the same convolutions from bf16 operands (csrc/cconv.hip):
 *   dw[k][n][c] += sum_{b,p,q} dy[b,q,p,n] * x[b, (q*stride + k*dil - pad) / up, p, g*CR + c];   db[n] += sum dy[b,q,p,n]
 * x (B, Tsrc, inner, Cin_tot) bf16 (already activated), dy (B, Tdst, inner, Ntot) bf16 (already gated); dw tap-major
 * (K, Ntot, CR) fp32, db fp32 or NULL.  Every workgroup owns one (tap, 128 x 128) output tile and walks a contiguous
 * slice of the tokens; `slices` > 1 splits the token axis (0 = automatic: 1 whenever the output tiles alone fill the
 * chip).  The slices' partial tiles go to `workspace` (caller-owned, >= kantts_cconv_wgrad_ws_floats(args) floats, 16-byte
 * aligned, contents irrelevant) and are summed into dw by a second kernel in a fixed order; without a workspace they
 * meet in fp32 atomics.  dw / db must be zero (or hold a value to accumulate onto) before the call. */
typedef struct {
  const void* x;
  const void* dy;
  float* dw;
  float* db;
  int B, Tsrc, Tdst, Cin_tot, Ntot, CR, NG, groups, K;
  int stride, dil, pad, inner, up;
  int slices;
  float* workspace;
  long long ws_floats;
} kantts_cconvw_args;
int kantts_cconv_wgrad_launch(const kantts_cconvw_args* args, void* stream);
long long kantts_cconv_wgrad_ws_floats(const kantts_cconvw_args* args);

/* dst = bf16(f(src)) over a flat fp32 buffer, n % 8 == 0: the bf16 operand images the kernels above read.
 *   gate == NULL:  f(v) = act ? LeakyReLU(v, slope) : v                  (activated input image)
 *   gate != NULL:  f(v) = v * (gate > 0 ? 1 : slope)                     (gated output gradient; gate fp32 or bf16) */
int kantts_act_cast_bf16(const float* src, const void* gate, int gate_bf16, void* dst, int act, float slope, long long n,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * Batch assembly on the device (csrc/batching.hip): padding / cropping of ragged utterances resident in
 * HBM -- Padder and the collate functions of kantts/datasets/dataset.py:34-85, 278-311, 690-827.
 *   out[b][t][c] = t < len[b] ? src[(row_off[b] + start[b] + t) * C + c] : pad[c]     b < B, t < Tmax, c < C
 * transpose != 0 writes out[b][c][t] instead (the vocoder's mel crop, (frames, C) -> (C, frames)).  row_off (B) int64 =
 * first row of utterance b in the flat (rows, C) source; start (B) int32 or NULL = crop offset in rows; len (B) int32 =
 * rows to copy (<= Tmax); pad (C) or NULL (zeros). */
int kantts_ragged_rows_f32(const float* src, const int64_t* row_off, const int32_t* start, const int32_t* len,
                           const float* pad, float* out, int B, int Tmax, int C, int transpose, void* stream);
int kantts_ragged_rows_i64(const int64_t* src, const int64_t* row_off, const int32_t* start, const int32_t* len,
                           const int64_t* pad, int64_t* out, int B, int Tmax, int C, int transpose, void* stream);
/* The inverse of kantts_ragged_rows_f32 (no transpose): in (B, Tmax, C) packed rows go back to the flat (rows, C) buffer,
 *   dst[(row_off[b] + start[b] + t) * C + c] = in[b][t][c]      for t < min(len[b], Tmax)
 * and nothing else of dst is written (start may be NULL).  16-byte accesses when C % 4 == 0 and both bases are 16-byte
 * aligned.  The caller guarantees that the addressed rows exist. */
int kantts_scatter_rows_f32(const float* in, const int64_t* row_off, const int32_t* start, const int32_t* len, float* dst,
                            int B, int Tmax, int C, void* stream);

/* The hand-over from the acoustic slot pool to the chunked vocoder (csrc/handover.hip): final post-net rows of every slot,
 * channels-last, become the vocoder's step input, channels-first, in one launch.
 *   src (S, T, C) fp32 (row stride C, slot stride T * C); start, rows (S) int32 on the device; out (S, C, Tc) fp32
 *   start_s = clamp(start[s], 0, T);  n_s = clamp(rows[s], 0, min(Tc, T - start_s))
 *   out[s][c][t] = t < n_s ? f_c(src[s][start_s + t][c]) : 0.0f
 * Nothing outside a slot's clamped window is read, every element of out is written, start / rows are not read back.
 * f_c is the identity; with nsf != 0 the last two channels (normalised f0 and a voicing score behind the mel bins) become
 * what the vocoder's source module takes, as denorm_f0 of kantts/bin/infer_sambert.py computes them:
 *   c == C - 2:  fmaxf(v * scale + offset, f0_floor)      product and sum rounded separately (no fused multiply-add)
 *   c == C - 1:  v < uv_threshold ? 0.0f : 1.0f
 * 16-byte loads when C % 4 == 0 and src is 16-byte aligned.
 * KANTTS_E_BADARG: src, start, rows or out NULL, S < 0, Tc < 0, T < 1, C < 1, nsf with C < 3.  S == 0 or Tc == 0: no-op.
 * KANTTS_E_UNSUPPORTED: S > 65535. */
int kantts_mel_handover_rows(const float* src, const int32_t* start, const int32_t* rows, float* out, int S, int T, int C,
                             int Tc, int nsf, float scale, float offset, float f0_floor, float uv_threshold, void* stream);

/* Launch-shape knobs for sweeps and tests -- they never change a result.  tn_tile: output tile of kantts_bgemm_tn* as
 * BN * 1000 + BK (64128 / 128128 / 64256 / 128256; anything else = the library's rule; the code + 1, e.g. 64129, selects
 * that tile WITHOUT the XCD-aware workgroup mapping of round 6 -- the 3-D grid of rounds 2-5, for A/B runs); tn_slices: token slices of the
 * same launches (0 = the rule); c1_wgrad_wgs: workgroup cap of the persistent weight-gradient launch of kantts_conv_c1_launch
 * (0 = 256).  The host layer maps KANTTS_TN_TILE / KANTTS_TN_SLICES / KANTTS_C1_WGRAD_WGS onto this call; the library reads
 * no environment variable for them (until round 5 it did, per launch). */
int kantts_launch_tuning(int tn_tile, int tn_slices, int c1_wgrad_wgs);

/* ------------------------------------------------------------------------------------------
 * [round 5] Free-running inference loops as ONE launch each (csrc/ar_infer.hip; SURVEY 8 row e1, bf16 mode).
 *
 * kantts_pnca_decode_run: every step of the free-running mel decoder for every sequence of a batch -- the loop of
 * kantts/models/sambert/kantts_sambert.py:569-610 around HybridAttentionDecoder.infer (:208-253; PNCA state updates
 * kantts/models/sambert/__init__.py:217-306).  One workgroup owns one sequence and walks its steps; per step the
 * matrix-vector products stream the bf16 weights from L2 as MFMA A operands (every column of the B operand is the
 * sequence's vector), activations stay in LDS, the decoder's K / V cache and the output frames are the only HBM writes.
 * Shapes fixed by the kernel: d_model 128, 8 heads x 16, feed-forward width 1024, prenet (d_mel -> 256 -> 256 -> 128).
 *   w : bf16 blob; every matrix (out, in) has its input width padded to a multiple of 128 (zeros) and is stored
 *       fragment-major like the images of kantts_fragmajor_bf16: element (16 t + i, 32 kb + 8 q + e) at
 *       (((t * in/32 + kb) * 4 + q) * 16 + i) * 8 + e -- the 1 KB one MFMA A operand needs is contiguous:
 *       P1 256 x pad(d_mel) | P2 256 x 256 | P3 128 x 256 | IN 128 x pad(d_mem + 128)  [columns: memory, prenet]
 *       per layer: QKV 384 x 128 | FC 128 x 256 [fc_x | fc_h] | W1 1024 x 128 | W2 128 x 1024
 *       OUT pad16(d_out) x 128
 *   f : fp32 blob: b_P1 256 | b_P2 256 | b_P3 128 | b_IN 128 |
 *       per layer: ln0 gamma 128, beta 128 | b_QKV 384 | b_FC 128 (= fc_x.bias + fc_h.bias) | ln1 gamma 128, beta 128 |
 *                  b_W1 1024 | b_W2 128
 *       final ln gamma 128, beta 128 | b_OUT pad16(d_out)
 *   (kantts_pnca_decode_blob_sizes reports both element counts.)
 *   memory (B, L, d_mem) fp32; hkv (B, L, n_layer * 256) fp32: the memory K | V projection of layer i at columns
 *   [256 i, 256 i + 256); xkv (n_layer, B, L, 256) fp32 workspace (the decoder's own K | V cache, contents irrelevant);
 *   out (B, L, d_out); lens (B) steps per sequence (rows at and after lens[b] are the reference's masked rows: x = 0);
 *   bw_seq (B) band width per sequence or NULL (then `bw`).  Band widths above 127: KANTTS_E_UNSUPPORTED (bw) / NaN in
 *   `out` (device-side bw_seq).  Frame fed back: the last d_mel values of a step's output. */
typedef struct kantts_decode_args {
  const void* w;
  const float* f;
  const float* memory;
  const float* hkv;
  float* xkv;
  float* out;
  const int32_t* lens;
  const int32_t* bw_seq;
  int B, L, d_mem, d_mel, d_out, n_layer, bw;
  float in_scale; /* sqrt(d_model): the input projection's alpha */
  float eps;      /* of every LayerNorm */
} kantts_decode_args;
int kantts_pnca_decode_run(const kantts_decode_args* args, void* stream);
/* Streaming form: decoder steps [t0, t1) of every sequence; kantts_pnca_decode_run is the range (0, L) of the same kernel.
 * All buffers are the full-length ones above and persist between calls: the frame fed into step t0 > 0 is the last d_mel
 * values of out[b, t0 - 1] (zero at t0 == 0), the K | V rows of earlier steps come from xkv.  Nothing outside rows [t0, t1)
 * of out and xkv is written, nothing at or after row t1 of out is read.  A device-side band width above 127 poisons rows
 * [t0, t1) of that sequence only.  t0 < 0, t1 > L or t0 > t1: KANTTS_E_BADARG; t0 == t1: no-op. */
int kantts_pnca_decode_range(const kantts_decode_args* args, int t0, int t1, void* stream);
/* Pool form (kantts/models/sambert/slots.py): every sequence advances over its own range.  t0 / t1: DEVICE int32[B]; the
 * kernel clamps them -- c0 = clamp(t0[b], 0, L), c1 = clamp(t1[b], c0, L) -- and the host never reads them back (the
 * convention of `rows` in kantts_sconv_rows_launch).  Rows [c0, c1) of out and xkv of sequence b are bit for bit what
 * kantts_pnca_decode_range(args, c0, c1) writes there; nothing else of that sequence is written, no row of out at or after
 * c1 is read, and a sequence with c0 == c1 reads and writes nothing.  A device-side band width above 127 poisons rows
 * [c0, c1) of that sequence only.  t0 == NULL or t1 == NULL: KANTTS_E_BADARG. */
int kantts_pnca_decode_slots(const kantts_decode_args* args, const int32_t* t0, const int32_t* t1, void* stream);
int kantts_pnca_decode_blob_sizes(int d_mel, int d_mem, int d_out, int n_layer, long long* w_elems, long long* f_elems);

/* kantts_dur_ar_run: the free-running duration predictor (VarRnnARPredictor.infer, kantts/models/sambert/adaptors.py:67-83):
 * token i consumes the prediction of token i - 1 through prenet (1 -> 128 -> 128) -> 2 LSTM cells (H = 128) -> Linear -> ReLU.
 * One workgroup per sequence walks its tokens.  The part of the first cell's gate pre-activations that depends on the
 * conditioning only is one GEMM the caller runs before:  gc (B, T, 512) = cond . W_ih0[:, 128:]^T + b_ih0 + b_hh0.
 *   w : bf16 blob (fragment-major matrices, as above): P2 128 x 128 | G0 512 x 256 [W_ih0[:, :128] | W_hh0] |
 *       G1 512 x 256 [W_ih1 | W_hh1]
 *   f : fp32 blob: w_P1 128 | b_P1 128 | b_P2 128 | b_G1 512 (= b_ih1 + b_hh1) | w_fc 128 | b_fc 1 | 0 0 0
 *       (the one-input prenet layer and the one-row output layer are evaluated in fp32)
 *   out (B, T): ReLU(fc(h1)) per token, 0 at and after lens[b] (lens NULL: every sequence has T tokens). */
typedef struct kantts_durar_args {
  const void* w;
  const float* f;
  const float* gc;
  float* out;
  const int32_t* lens;
  int B, T;
} kantts_durar_args;
int kantts_dur_ar_run(const kantts_durar_args* args, void* stream);
/* kantts_dur_ar_run_f32: the same loop in fp32 arithmetic (products are fp32 FMAs in k order) -- what inference uses for
 * the duration predictor in EVERY precision mode, so that the index tensors derived from its output (durations, regulated
 * lengths, band widths: kantts/models/sambert/kantts_sambert.py:455-460,989-993) equal the reference's bit for bit.
 *   w : fp32 blob, the same three matrices, each (N, K) stored k-chunk-major: element (n, k) at ((k / 4) * N + n) * 4 + k % 4
 *   f, gc, out, lens: as kantts_dur_ar_run. */
int kantts_dur_ar_run_f32(const kantts_durar_args* args, void* stream);

/* kantts_ctc_attn: AttentionCTCLoss (kantts/train/loss.py:481-508) and its gradient in one launch, a workgroup per utterance
 * (replaces torch.nn.CTCLoss, whose ATen implementation copies the lengths to the host: the MAS training step could not be
 * captured).  Per utterance b: classes 0..S (S = in_lens[b]) with logit[t, 0] = `blank` (a constant) and logit[t, c] =
 * logits[b, t, c - 1]; log_softmax over those classes; CTC with the target 1..S over the first out_lens[b] frames;
 * zero_infinity semantics.
 *   logits (B, T1, T2) fp32 (attn_logprob[:, 0]); in_lens / out_lens (B) int32 on the device;
 *   ws: workspace of kantts_ctc_attn_workspace(B, T1, T2) floats (alpha and beta rows; contents irrelevant);
 *   loss (B): nll_b / S_b (0 for an impossible alignment or an empty utterance);
 *   grad (B, T1, T2): grad_scale * d loss[b] / d logits (zero at frames >= out_lens[b] and columns >= in_lens[b]) -- the
 *   caller passes grad_scale = 1 / B for the reference's mean over the batch and multiplies by the incoming gradient.
 * Limits: T2 <= 511 phonemes, T1 <= 24576 frames (KANTTS_E_UNSUPPORTED beyond). */
typedef struct kantts_ctc_args {
  const float* logits;
  const int32_t* in_lens;
  const int32_t* out_lens;
  float* ws;
  float* loss;
  float* grad;
  int B, T1, T2;
  float blank;
  float grad_scale;
} kantts_ctc_args;
long long kantts_ctc_attn_workspace(int B, int T1, int T2);
int kantts_ctc_attn(const kantts_ctc_args* args, void* stream);
/* kantts_ctc_attn_wide: the same arguments, workspace and arithmetic with eight states per thread instead of four, for the
 * token counts of byte-input voices; the gradient pass is a second launch on `stream` (a wave per frame, the whole chip)
 * instead of the tail of the first.  Writes every cell of loss and grad.  Limits: T2 <= 1023 tokens (2 T2 + 1 <= 2048 states, the width of kantts_align_attn_fwd),
 * T1 <= 24576 frames (KANTTS_E_UNSUPPORTED beyond).  It takes narrow shapes too; kantts_ctc_attn prefetches deeper there. */
int kantts_ctc_attn_wide(const kantts_ctc_args* args, void* stream);

/* kantts_enc_attn_fwd: the attention sub-layer of an encoder FFT block (MultiHeadSelfAttention.forward,
 * kantts/models/sambert/__init__.py:52-106 inside FFTBlock.forward :152-184) as ONE launch, a workgroup per sequence:
 *   qkv = xn . W_qkv^T + b;  8-head attention over the keys [0, lens[b]) of every query (+ attention dropout);
 *   y1 = rowmask(dropout(context . W_fc^T + b_fc) + x);  xn1 = LayerNorm(y1)  (the feed-forward sub-layer's, optional)
 * -- what kantts_bgemm_nt + kantts_attn_fwd (mode 0) + kantts_bgemm_nt with its LayerNorm epilogue compute, with the same
 * dropout streams (element index (row, channel) for the projection; ((head * B + b) * L + query) * L + key for the attention).
 *   x (M, 128) fp32, M = B * L; xn (M, 128) bf16: LayerNorm of x (the caller's); lens (B) or NULL; rowmask (M) or NULL;
 *   wqkv / wfc: fragment-major bf16 images (kantts_fragmajor_bf16) of the (384, 128) / (128, 128) weights;
 *   written for the backward pass: qkv (M, 384) fp32, o (M, 128) contexts, lse (B, 8, L), y1 (M, 128), xn1 (M, 128) bf16 or
 *   fp32 (xn1_bf16) with mean1 / rstd1 (M).  d_model 128, 8 heads of 16, L <= 128 (KANTTS_E_UNSUPPORTED beyond). */
typedef struct kantts_enc_attn_args {
  const float* x;
  const void* xn;
  const int32_t* lens;
  const uint8_t* rowmask;
  const void* wqkv;
  const float* bqkv;
  const void* wfc;
  const float* bfc;
  const float* ln1_gamma;
  const float* ln1_beta;
  float ln1_eps;
  float att_p, fc_p;
  uint64_t att_seed, fc_seed;
  const uint64_t* seed_dev;
  float* qkv;
  float* o;
  float* lse;
  float* y1;
  void* xn1;
  int xn1_bf16;
  float* mean1;
  float* rstd1;
  int B, L;
} kantts_enc_attn_args;
int kantts_enc_attn_fwd(const kantts_enc_attn_args* args, void* stream);

/* ---- Causal stride-1 dilated channels-last convolution WITH HISTORY (csrc/sconv.hip): the layer of chunked inference.
 * S independent slots advance together by Tc rows; every slot carries the last H = (K - 1) * step input rows of the
 * previous call.  Token rule:
 *   out[s, q, n]      = post( bias[n] + sum_j sum_c pre( X[s, q - j*step, c] ) * w[j][n][c] ),   q in [0, Tc)
 *   X[s, t, c]        = in[s, t, c]             for t >= 0
 *                     = hist_in[s, H + t, c]    for -H <= t < 0
 *   hist_out[s, h, c] = X[s, Tc - H + h, c]     for h in [0, H)   (the last H rows of [hist_in ; in], also when Tc < H)
 *   pre(v)  = in_act  ? LeakyReLU(v, in_slope)  : v
 *   post(v) = (out_act ? LeakyReLU(v, out_slope) : v) + res[s, q, n]
 * Tap j reads j*step rows BACK (a torch Conv1d weight (N, Cin, K) left-padded by (K-1)*dilation is w[j] = W[:, :, K-1-j]).
 * The polyphase form of a causal transposed convolution of stride u and the fused dual-path stage of the generator are this
 * rule with step = 1, K = J taps and N = u * Cout (row q of out is the u output samples of input token q).
 *   in (S, Tc, Cin), out / res (S, Tc, N), bias (N): fp32, dense.  hist_in / hist_out: fp32 raw (not activated) rows,
 *   slot s at base + s * hist_ss floats, (H, Cin) dense inside a slot; two DIFFERENT buffers (ping-pong); hist_out is
 *   written by extra workgroups of the same launch.  Both may be NULL when K == 1.
 *   w (K, N, Cin): fp32 when precision == 0 or N == 1, bf16 when precision == 1 and N > 1.
 * precision 0: fp32 operands on v_mfma_f32_16x16x4_f32; 1: bf16 operands (the activated input is rounded as it enters LDS)
 * on v_mfma_f32_16x16x32_bf16, fp32 accumulation.  N == 1 is a direct fp32 dot product in both modes.
 * KANTTS_E_UNSUPPORTED unless Cin % 8 == 0, 16 <= Cin <= 512, (N == 1 or 16 <= N <= 4096), 1 <= K <= 11, 1 <= step <= 7,
 * all pointers 16-byte aligned and hist_ss % 4 == 0.  S <= 0 or Tc <= 0: nothing is launched, KANTTS_OK. */
typedef struct {
  const float* in;
  const float* hist_in;
  float* hist_out;
  const void* w;
  const float* bias;
  const float* res;
  float* out;
  long long hist_ss;
  int S, Tc, Cin, N, K, step;
  float in_slope;
  int in_act;
  float out_slope;
  int out_act;
  int precision;
} kantts_sconv_args;
int kantts_sconv_launch(const kantts_sconv_args* args, void* stream);

/* ---- The same layer with a PER-SLOT ROW COUNT: the slots of a call advance independently (continuous batching of a
 * chunked vocoder: utterances of different lengths, a paused slot, a slot that takes the next request).
 *   rows (S) int32, DEVICE memory (read by the kernel: a captured launch stays valid while the counts change), in units of
 *   the frame rate of the step; row_mul: rows of THIS layer per frame (1 for the first layer, the running product of the
 *   upsampling scales behind each stage).  Slot s has
 *     n_s = clamp(rows[s], 0, Tc / row_mul) * row_mul          (clamped from both sides)
 *   live rows.  Token rule:
 *   out[s, q, n]      for q <  n_s: the rule of kantts_sconv_launch, same arithmetic and summation order (the tiles are
 *                     chosen from Tc, as there), with X[s, t] read for t < n_s only
 *   out[s, q, n]      for q >= n_s: not written; written as 0.0f when zero_tail != 0
 *   hist_out[s, h, c] = X[s, n_s - H + h, c]   for h in [0, H)   (the last H rows of [hist_in[s] ; in[s, 0:n_s]], also when
 *                     n_s < H; n_s == 0: a copy of hist_in[s] -- the caller flips its ping-pong halves for every slot)
 * No row >= n_s of in or res is loaded: such rows may hold NaN or uninitialised memory.
 * The fields before `rows` are those of kantts_sconv_args, in the same order; shape contract and alignment rules as there.
 * zero_tail is supported for N == 1 only (KANTTS_E_UNSUPPORTED otherwise).
 * KANTTS_E_BADARG: rows == NULL, row_mul < 1, Tc % row_mul != 0. */
typedef struct {
  const float* in;
  const float* hist_in;
  float* hist_out;
  const void* w;
  const float* bias;
  const float* res;
  float* out;
  long long hist_ss;
  int S, Tc, Cin, N, K, step;
  float in_slope;
  int in_act;
  float out_slope;
  int out_act;
  int precision;
  const int32_t* rows;
  int row_mul;
  int zero_tail;
} kantts_sconv_rows_args;
int kantts_sconv_rows_launch(const kantts_sconv_rows_args* args, void* stream);

/* ---- The per-slot layer for SYMMETRIC (non-causal) networks (csrc/sconv_sym.hip): a symmetric convolution of padding p
 * is the causal one with the same taps whose output stream is p rows late, zero outside the utterance.  Every tensor of
 * such a network has an integer delay: row n of its stream, counted from the slot's reset, is true row n - delay.
 * The rule of kantts_sconv_rows_launch (same tiles, arithmetic and summation order) with
 *   n_s      = clamp(rows[s], 0, Tc / row_mul) * row_mul           live rows of slot s, as there
 *   pos_s    = pos_in[s * pos_ss]                                  frames slot s consumed before this call
 *   end_s    = end[s]                                              frames of the slot's utterance; < 0: open
 *   Hs       = (K - 1) * step + lag                                state rows of the layer
 *   X[s, t]  = in[s, t] (0 <= t < n_s),  hist_in[s, Hs + t] (-Hs <= t < 0); with in_end != 0 and end_s >= 0 a row whose
 *              stream position pos_s * row_mul + t is >= end_s * row_mul is 0.0f and is NOT loaded (flush rows)
 *   R[s, t]  = res[s, t] (t >= 0),  res_hist[s, res_hist_rows + t] (-res_hist_rows <= t < 0)
 *   y[s,q,n] = post( bias[n] + sum_j sum_c pre( X[s, q - lag - j*step, c] ) * w[j][n][c] ) + R[s, q - res_lag, n]
 *   g(q, n)  = (pos_s * row_mul + q) * sub + (sub > 1 ? n / (N / sub) : 0) - delay        true sample index, 64-bit
 *   out[s, q, n] = y[s, q, n]  when 0 <= g(q, n) and (end_s < 0 or g(q, n) < end_s * row_mul * sub),  else 0.0f,  q < n_s
 *   out[s, q, n] for q >= n_s: not written; written as 0.0f when zero_tail != 0 (N == 1 only)
 *   hist_out[s, h, c] = X[s, n_s - Hs + h, c]   for h in [0, Hs)
 *   pos_out[s * pos_ss] = pos_s + n_s / row_mul   when pos_out != NULL (written by the state workgroup of slot s; the
 *              first layer of a step passes it, every launch of the step reads the same pos_in: ping-pong with the state)
 * res_hist is another layer's carried state (read only), (res_hist_rows, N) dense inside a slot, res_hist_ss floats between
 * slots.  A polyphase layer of stride u passes sub = u: row q, column n of out is sample q * u + n / (N / u).
 * No row >= n_s of in / res, and no flush row of in, is loaded: such rows may hold NaN.  w, precision, alignment and the
 * shape contract are those of kantts_sconv_launch (hist_ss >= Hs * Cin when S > 1).
 * KANTTS_E_BADARG: rows / end / pos_in == NULL, row_mul < 1, Tc % row_mul != 0, lag < 0, res_lag < 0, delay < 0, sub < 1,
 * N % sub != 0, res_lag > 0 without res and res_hist or beyond res_hist_rows, res_hist without res, missing hist_in /
 * hist_out when Hs > 0.  KANTTS_E_UNSUPPORTED: zero_tail with N != 1, and what kantts_sconv_launch declines. */
typedef struct {
  const float* in;
  const float* hist_in;
  float* hist_out;
  const void* w;
  const float* bias;
  const float* res;
  const float* res_hist;
  float* out;
  const int32_t* rows;
  const int32_t* end;
  const int32_t* pos_in;
  int32_t* pos_out;
  long long hist_ss;
  long long res_hist_ss;
  long long pos_ss;
  long long delay;
  int S, Tc, Cin, N, K, step;
  float in_slope;
  int in_act;
  float out_slope;
  int out_act;
  int precision;
  int row_mul;
  int zero_tail;
  int lag;
  int res_lag;
  int res_hist_rows;
  int sub;
  int in_end;
} kantts_sconv_sym_args;
int kantts_sconv_sym_rows_launch(const kantts_sconv_sym_args* args, void* stream);

/* ---- The NSF excitation of chunked inference (csrc/nsf_source.hip): a sine source that can be cut at any frame boundary
 * and the strided one-channel convolutions that bring it to every upsampling stage's rate.  Both entry points are per slot
 * and read the same device `rows` buffer as kantts_sconv_rows_launch:
 *   n_s = clamp(rows[s], 0, Tc) live FRAMES of slot s (rows == NULL: n_s = Tc for every slot);
 *   nothing at or after frame n_s of a slot's inputs is loaded (such frames may hold NaN), nothing at or after it is written;
 *   a slot with n_s == 0 has its state copied bit for bit.
 * fp32 arithmetic in both precision modes; no alignment rules beyond the 8 bytes of the state.
 *
 * kantts_nsf_source_rows: frame-level f0 (Hz) and voicing -> the projected excitation, SourceModule.forward_cl in one launch.
 * Sample j of frame k of slot s (sample k * hop + j of the call, absolute sample n = cursor + k * hop + j of the utterance):
 *   inc_k[h]   = round(frac((h + 1) * f0[s, k] / sr) * 2^32)            (fp64, then a wrapping uint32)
 *   P_0        = state_in.phase,   P_{k+1} = P_k + hop * inc_k          (uint32, wrap-around == the reference's `% 1`)
 *   theta      = 2 pi * (int32)(P_k[h] + (j + 1) * inc_k[h]) / 2^32     (a signed fraction of a cycle: [-pi, pi))
 *   x_h        = uv[s, k] * (alpha * sin(theta + phase0[h]) + z_h) + (1 - uv[s, k]) * (alpha / 3 / sigma) * z_h
 *   e[s, k * hop + j] = tanh(bias[0] + sum_h w[h] * x_h),               h in [0, H1), H1 = nb_harmonics + 1
 *   z_h        = noise[s, k * hop + j, h] when noise != NULL (used as it is: the caller's N(0, sigma) draws), else
 *                sigma * N(0, 1) by Box-Muller on the 64-bit hash of common.h keyed by (state.key, 8 * n + h / 2): one hash
 *                gives the pair (cos, sin) for harmonics 2i and 2i + 1.  Same key and same n: same bits, whatever the chunking.
 *   harm[s, k * hop + j, h] = x_h when harm != NULL (the excitation before its projection).
 * Frame indexing is exact (sample n belongs to frame n / hop): the float-scale rounding of
 * torch.nn.functional.interpolate(mode="nearest"), which can pick the neighbouring frame at a frame boundary when hop is no
 * power of two, is NOT reproduced.
 * State: KANTTS_NSF_STATE_WORDS 32-bit words per slot, slot s at base + s * state_ss words, two DIFFERENT buffers
 * (ping-pong; state_out is written by extra workgroups of the same launch):
 *   words  0..15  uint32 phase[16]    running phase per harmonic, 2^32 = one cycle
 *   words 16..31  float  phase0[16]   initial phase per harmonic (the reference has phase0[0] == 0)
 *   words 32..33  uint64 cursor       absolute sample index of the slot's utterance
 *   words 34..35  uint64 key          noise key
 *   state_out = {P_{n_s}, phase0, cursor + n_s * hop, key}.
 *   f0, uv (S, Tc); noise, harm (S, Tc * hop, H1); w (H1); bias (1) or NULL; e (S, Tc * hop): fp32, dense.
 * KANTTS_E_BADARG: a NULL required pointer (f0, uv, w, state_in, state_out, e), state_in == state_out, Tc < 1, hop < 1,
 * H1 < 1, sr <= 0, sigma <= 0, state_ss < KANTTS_NSF_STATE_WORDS with S > 1.  KANTTS_E_UNSUPPORTED: H1 > 16, a state that is
 * not 8-byte aligned or an odd state_ss, S * Tc * hop >= 2^31.  S <= 0: nothing is launched, KANTTS_OK. */
#define KANTTS_NSF_STATE_WORDS 36
typedef struct {
  const float* f0;
  const float* uv;
  const float* noise;
  const float* w;
  const float* bias;
  const int32_t* state_in;
  int32_t* state_out;
  float* e;
  float* harm;
  const int32_t* rows;
  long long state_ss;
  int S, Tc, hop, H1;
  float sr, alpha, sigma;
} kantts_nsf_source_args;
int kantts_nsf_source_rows(const kantts_nsf_source_args* args, void* stream);

/* kantts_nsf_downs_rows: all source_downs convolutions of a generator in one launch.  Stage i (i < nstages <= 8) has stride
 * u[i] (a divisor of hop), k[i] taps and C[i] output channels:
 *   d_i[s, q, c]   = bias_i[c] + sum_j w_i[j][c] * E[s, q * u[i] - (k[i] - 1) + j],     q in [0, n_s * hop / u[i])
 *   E[s, t]        = e[s, t]                 for t >= 0
 *                  = hist_in[s, Hh + t]      for -Hh <= t < 0,    Hh = max_i (k[i] - 1)
 *   hist_out[s, h] = E[s, n_s * hop - Hh + h]   for h in [0, Hh)  (the last Hh samples of [hist_in[s] ; e[s, 0 : n_s * hop]];
 *                    n_s == 0: a copy of hist_in[s])
 * A torch Conv1d weight (C, 1, k) left-padded by k - 1 is w_i[j][c] = W[c, 0, j].  The generator's stages have
 * u[i] = hop / prod(scales[:i+1]), k[i] = 2 * u[i] (the last, u = 1: k = 1, the 1x1 convolution), so Hh = 2 * u[0] - 1 < hop;
 * zero history == the reference's zero left pad.
 *   e (S, Tc * hop); w_i (k[i], C[i]) tap-major; bias_i (C[i]) or NULL; out_i (S, Tc * hop / u[i], C[i]) -- byte for byte the
 *   (S, rows, scale * Cout) `res` of the polyphase up-layer that adds it; hist_in / hist_out: slot s at base + s * hist_ss
 *   floats, two DIFFERENT buffers (NULL allowed when Hh == 0).  All fp32, dense.
 * KANTTS_E_BADARG: e == NULL, Tc < 1, hop < 1, nstages < 1, a stage with a NULL w / out or u, k, C < 1, missing or equal
 * history buffers with Hh > 0, hist_ss < Hh with S > 1.  KANTTS_E_UNSUPPORTED: nstages > 8, a stage whose u does not divide
 * hop, k[i] > 8192 (the window of a one-row tile must fit its LDS buffer).  S <= 0: nothing is launched. */
typedef struct {
  const float* e;
  const float* hist_in;
  float* hist_out;
  const int32_t* rows;
  const float* w[8];
  const float* bias[8];
  float* out[8];
  long long hist_ss;
  int S, Tc, hop, nstages;
  int u[8];
  int k[8];
  int C[8];
} kantts_nsf_downs_args;
int kantts_nsf_downs_rows(const kantts_nsf_downs_args* args, void* stream);

/* ---- The NSF excitation of chunked inference for NON-CAUSAL generators (csrc/nsf_source_sym.hip): the two entry points
 * above for a network whose tensors are delayed and whose utterance ends (the rule of kantts_sconv_sym_rows_launch).  Both
 * are per slot, fp32 in both precision modes, and read the device buffers a step of that layer reads:
 *   n_s   = clamp(rows[s], 0, Tc)      frames of slot s in this call, flush frames included (rows == NULL: Tc)
 *   end_s = end[s]                     frames of the slot's utterance; < 0: open.  end == NULL: every slot is open
 *   pos_s = pos_in[s * pos_ss]         frames slot s consumed before this call (read only when end != NULL)
 *   l_s   = n_s when end_s < 0, else clamp(end_s - pos_s, 0, n_s)      the frames of this call inside the utterance
 *
 * kantts_nsf_source_end_rows: `src` is the argument of kantts_nsf_source_rows, rule, shapes and state included, and the
 * launch does for l_s frames of slot s exactly what that entry point does for n_s: the same bits of e, harm and state_out
 * (state_out.cursor = cursor + l_s * hop: the source's cursor stops at the end, which is why pos comes from elsewhere).
 * Frames at or beyond l_s of f0 / uv / noise are not loaded (they may hold NaN), samples at or beyond l_s * hop of e / harm
 * are not written, l_s == 0 copies the state bit for bit.
 * KANTTS_E_BADARG: args == NULL, end != NULL with pos_in == NULL, pos_ss < 0, and what kantts_nsf_source_rows answers with
 * it for `src`; KANTTS_E_UNSUPPORTED: as there.  S <= 0: nothing is launched, KANTTS_OK. */
typedef struct {
  kantts_nsf_source_args src;
  const int32_t* end;
  const int32_t* pos_in;
  long long pos_ss;
} kantts_nsf_source_end_args;
int kantts_nsf_source_end_rows(const kantts_nsf_source_end_args* args, void* stream);

/* kantts_nsf_downs_sym_rows: all source_downs convolutions of a non-causal generator in one launch, stage i read lag[i]
 * samples back.  `d` is the argument of kantts_nsf_downs_rows (stages, weights tap-major (k, C), outputs, history buffers
 * and their stride), except that the history holds Hh samples, an argument.  With A_s = pos_s * hop:
 *   E[s, t]        = d.e[s, t]               for 0 <= t < n_s * hop and (end_s < 0 or A_s + t < end_s * hop)
 *                  = 0.0f, NOT loaded        for t >= 0 otherwise (flush frames: they may hold NaN)
 *                  = d.hist_in[s, Hh + t]    for -Hh <= t < 0
 *   d_i[s, q, c]   = bias_i[c] + sum_{j < k[i]} w_i[j][c] * E[s, q * u[i] - lag[i] + j],     q in [0, n_s * hop / u[i])
 *   hist_out[s, h] = E[s, n_s * hop - Hh + h]   for h in [0, Hh)      (n_s == 0: a copy of hist_in[s])
 * Rows q >= n_s * hop / u[i] of out_i are not written.  out_i is byte for byte the `res` of stage i's polyphase up-layer
 * (kantts_sconv_sym_rows_launch with res_lag = 0), whose own window stores 0.0f where the true index is outside the
 * utterance, whatever this formula gave there.  A torch Conv1d(1, C, k, stride u, padding p) whose output the up-layer
 * holds D rows late is lag = D * u + p with w_i[j][c] = W[c, 0, j]; a zeroed history is its zero left pad, the zeros behind
 * end_s * hop its right pad.  lag[i] = k[i] - 1, end == NULL and Hh = max_i (k[i] - 1) is kantts_nsf_downs_rows bit for bit
 * (same tiles, same summation order).  The tile's window does not grow with the lag: neither lag nor Hh has a cap.
 * KANTTS_E_BADARG: args == NULL, end != NULL with pos_in == NULL, pos_ss < 0, Hh < 0, lag[i] < k[i] - u[i] (a tap in the
 * slot's future), lag[i] > Hh, d.e == NULL, Tc < 1, hop < 1, nstages < 1, a stage with a NULL w / out or u, k, C < 1,
 * missing or equal history buffers with Hh > 0, hist_ss < Hh with S > 1.  KANTTS_E_UNSUPPORTED: nstages > 8, a stage
 * whose u does not divide hop, k[i] > 8192.  S <= 0: nothing is launched. */
typedef struct {
  kantts_nsf_downs_args d;
  const int32_t* end;
  const int32_t* pos_in;
  long long pos_ss;
  int Hh;
  int lag[8];
} kantts_nsf_downs_sym_args;
int kantts_nsf_downs_sym_rows(const kantts_nsf_downs_sym_args* args, void* stream);

/* ---- The NSF excitation in TRAINING (csrc/nsf_train.hip).  The forward of a training step is kantts_nsf_source_rows as it
 * stands (S = batch items, Tc = frames, rows = NULL); these two entry points give it starting words drawn on the device
 * and the gradient of its projection, so that a whole GAN step of an NSF generator can be captured and replayed.
 *
 * kantts_nsf_draw_states: the device twin of kantts.models.hifigan.chunked_nsf.initial_state.  seed_counter: two 64-bit
 * words {seed, counter} in DEVICE memory.  One workgroup reads both and writes, for item s in [0, S), the
 * KANTTS_NSF_STATE_WORDS words at state_out + s * state_ss of utterance key (counter << 20) | s under `seed`:
 *   key64     = mix(mix(seed, 0x4E5346), (counter << 20) | s)          mix: kantts_rng_mix of csrc/common.h
 *   phase     = 0 (16 words),  cursor = 0,  key = key64
 *   phase0[0] = 0,  phase0[h] = (float)(((mix(key64, 2^63 + h) >> 40) / 2^24 * 2 - 1) * pi)   for h in [1, H1): computed in
 *               fp64 and rounded ONCE, the bits of the Python function;  phase0[h] = 0 for h in [H1, 16)
 * then, behind a barrier, stores counter + 1: consecutive launches (and replays of one captured launch) draw different
 * numbers, and a counter set back replays them.  Exactly words [0, KANTTS_NSF_STATE_WORDS) of every item are written, with
 * plain 32-bit vector stores; the words between items (state_ss > KANTTS_NSF_STATE_WORDS) and `seed` are not.
 * KANTTS_E_BADARG: a NULL pointer, a pointer that is not 8-byte aligned, an odd state_ss, state_ss < KANTTS_NSF_STATE_WORDS
 * with S > 1, H1 < 1.  KANTTS_E_UNSUPPORTED: S outside [1, 2^20) (the key holds the item in 20 bits), H1 > 16.  Nothing is
 * written when a call is refused. */
int kantts_nsf_draw_states(uint64_t* seed_counter, int S, int H1, int32_t* state_out, long long state_ss, void* stream);

/* kantts_nsf_source_wgrad: the backward of the projection of kantts_nsf_source_rows, for the call that produced `e`:
 *   dpre[s, n] = de[s, n] * (1 - e[s, n]^2)
 *   dw[h]      = sum_{s, n} dpre[s, n] * x_h[s, n]      h in [0, H1)
 *   dbias[0]   = sum_{s, n} dpre[s, n]                  (dbias == NULL: not written)
 * x_h is the excitation before the projection (`harm` of the forward).  It is recomputed, not read: f0, uv, state_in, noise,
 * hop, H1, sr, alpha, sigma and state_ss are the forward's (rows == NULL there: every item has Tc live frames), and forward
 * and backward evaluate x_h through the same function, so the bits are the forward's.  dw and dbias are WRITTEN, not
 * accumulated into, and the same inputs give the same bits from run to run: one workgroup per (item, frame) leaves H1 + 1
 * partial sums in ws (a fixed in-workgroup tree, no atomics), a second launch behind it on the stream adds the S * Tc
 * partials of every sum in a fixed order.  ws: S * Tc * (H1 + 1) floats of device memory that the call may overwrite;
 * ws_floats says how many there are.
 *   f0, uv (S, Tc); noise (S, Tc * hop, H1) or NULL; e, de (S, Tc * hop); dw (H1); dbias (1) or NULL: fp32, dense.
 * KANTTS_E_BADARG: args == NULL, a NULL required pointer (f0, uv, state_in, e, de, dw, ws), S < 1, Tc < 1, hop < 1, H1 < 1,
 * sr <= 0, sigma <= 0, state_ss < KANTTS_NSF_STATE_WORDS with S > 1, ws_floats < S * Tc * (H1 + 1).  KANTTS_E_UNSUPPORTED:
 * H1 > 16, a state that is not 8-byte aligned or an odd state_ss, S * Tc * hop >= 2^31.  Nothing is written when a call is
 * refused. */
typedef struct {
  const float* f0;
  const float* uv;
  const float* noise;
  const int32_t* state_in;
  const float* e;
  const float* de;
  float* dw;
  float* dbias;
  float* ws;
  long long state_ss;
  long long ws_floats;
  int S, Tc, hop, H1;
  float sr, alpha, sigma;
} kantts_nsf_wgrad_args;
int kantts_nsf_source_wgrad(const kantts_nsf_wgrad_args* args, void* stream);

/* ---- The tail of a MULTI-BAND generator in chunked inference (csrc/mb_tail.hip), one launch: conv_post (causal, K taps,
 * step 1, Cin -> B sub-bands), tanh, and a PQMF synthesis that can be cut at any chunk boundary.  Per slot, driven by the
 * same device `rows` buffer and row_mul as kantts_sconv_rows_launch:
 *   n_s = clamp(rows[s], 0, Tq / row_mul) * row_mul live rows of slot s (rows == NULL: n_s = Tq for every slot);
 *   last (S) int32, DEVICE memory, read the same way: last[s] != 0 ends the slot's utterance with this call (NULL: all 0).
 * Sub-band rows (conv_post follows the rule of kantts_sconv_launch with step 1 and N = B; tap j reads j rows back):
 *   z[s, t, k] = tanh( bias[k] + sum_j sum_c pre( X[s, t - j, c] ) * w[j][k][c] ),   t in [0, n_s)
 *   X[s, t, c] = in[s, t, c] for t >= 0, hist_in[s, K - 1 + t, c] for -(K - 1) <= t < 0;   pre(v) = in_act ? LeakyReLU(v, in_slope) : v
 *   w == NULL is the PASS-THROUGH form: in is (S, Tq, B) and z[s, t, k] = in[s, t, k] -- streaming PQMF.synthesis alone.
 * Synthesis: with z the sub-band rows of the whole utterance, zero before its first row and after its last,
 *   full[q * B + r] = sum_{d = -D .. D} sum_k poly[r, k, d + D] * z[q + d, k]
 * (poly: the polyphase weights (B, B, 2 D + 1), D = ceil((taps / 2) / B)).  Row q looks AHEAD by D rows, so a slot holds back
 * the rows whose future it has not seen.  State: KANTTS_MB_STATE_WORDS(D, B) 32-bit words per slot, slot s at
 * base + s * state_ss words, two DIFFERENT buffers (ping-pong; state_out, hist_out and emitted are written by S extra
 * workgroups of the same launch):
 *   words 0 .. 2 D B - 1   float  the last 2 D rows of z seen so far, (2 D, B) dense, zero at the start
 *   word  2 D B            int32  pending = min(rows of z seen so far, D): the rows held back
 * A call with n = n_s new rows:              last == 0                       last != 0
 *   low-rate rows emitted E                  max(0, n + pending - D)         n + pending (the future is zeros)
 *   pending afterwards                       min(n + pending, D)             0
 *   z state afterwards                       last 2 D rows of [state ; z]    zeros (the slot is as after a reset)
 *   hist_out[s]                              last K - 1 rows of              zeros
 *                                            [hist_in[s] ; in[s, 0:n]]
 * The emitted rows are the next rows of the utterance in order: row i of the call is out[s, i * B .. i * B + B), centred on
 * row 2 D - pending + i of [state ; z ; zeros]; out[s, E * B .. (Tq + D) * B) is written as 0.0f; emitted[s] = E * B.
 * n == 0 with last == 0 emits nothing and copies state and history bit for bit; n == 0 with last != 0 is a flush of
 * pending * B samples; a second flush emits nothing.  pending saturates at D: no cursor grows with the utterance.
 * The bits of an utterance's samples do not depend on the chunking, the slot, its batch-mates or the tile: a z row is one
 * fmaf chain, tap-major and channel-inner, wherever it is computed; a sample is one fmaf chain, d ascending and k inner;
 * rows taken from the state are used as stored.  fp32 arithmetic in both precision modes.
 * No row >= n_s of in is loaded: such rows may hold NaN.
 *   in (S, Tq, Cin), w (K, B, Cin), bias (B) or NULL, poly (B, B, 2 D + 1), out (S, (Tq + D) * B), emitted (S) int32 or NULL:
 *   dense; hist_in / hist_out: K - 1 raw rows, slot s at base + s * hist_ss floats (NULL allowed when K == 1 or w == NULL).
 * KANTTS_E_BADARG: NULL in, poly, out, state_in or state_out, state_in == state_out, row_mul < 1, Tq % row_mul != 0, missing or
 * equal history buffers with w != NULL and K > 1, state_ss / hist_ss smaller than a slot's state with S > 1.
 * KANTTS_E_UNSUPPORTED unless 2 <= B <= 8, 1 <= D <= 16, 1 <= K <= 11, Cin % 4 == 0, 4 <= Cin <= 512 (Cin == B when w == NULL),
 * in, w, hist_in, hist_out, poly, state_in, state_out and out 16-byte aligned, hist_ss % 4 == 0.
 * S <= 0 or Tq <= 0: nothing is launched, KANTTS_OK (a flush needs Tq >= 1 and rows[s] = 0). */
#define KANTTS_MB_STATE_WORDS(D, B) (2 * (D) * (B) + 1)
typedef struct {
  const float* in;
  const float* hist_in;
  float* hist_out;
  const float* w;
  const float* bias;
  const float* poly;
  const float* state_in;
  float* state_out;
  float* out;
  int32_t* emitted;
  const int32_t* rows;
  const int32_t* last;
  long long hist_ss;
  long long state_ss;
  int S, Tq, Cin, B, K, D;
  int row_mul;
  float in_slope;
  int in_act;
} kantts_mb_tail_args;
int kantts_mb_tail_rows(const kantts_mb_tail_args* args, void* stream);

/* ---- Filled-pause voices (FP: True; csrc/fp.hip) --------------------------------------------------------------------------
 * B sequences of T token slots, C = encoder_projection_units channels, fp32, C % 4 == 0 (else KANTTS_E_UNSUPPORTED; so are
 * C > 1024 where noted, B > 65535 and float tensors that are not 16-byte aligned).  NULL required pointers and negative
 * sizes: KANTTS_E_BADARG.  No entry uses atomics: two calls on equal inputs give equal bits.
 *
 * kantts_fp_head: probs (B, T, 4) = softmax(rows (B T, C) . weight (4, C)^T + bias (4)), and the insertion decision:
 *   fp_label == NULL (inference): for j < lens[b], m_c = (p_c == max_k p_k), c = 1..3; label[b, j] = the smallest c with
 *     m_c, 0 if none (and 0 for j >= lens[b]); fp_number[b] = sum_j sum_c m_c -- ties count severally, a tie with class 0
 *     still inserts (reference kantts_sambert.py:787-791, :830-844).
 *   fp_label != NULL (int32 (B, T)): label = fp_label, fp_number[b] = #(fp_label[b] > 0) over all T slots, padding included.
 *   C <= 1024.  One launch, a workgroup per sequence.
 * kantts_fp_head_bwd: d_rows (N, C), d_weight (4, C), d_bias (4) from d_probs (N, 4), N = B T; probs as the forward wrote
 *   them.  C <= 1024.  One launch; the two parameter gradients are sums over the rows in a fixed order.
 *
 * kantts_fp_plan: one workgroup per sequence scans label (B, T) (values outside [0, 3] count as 0) and writes
 *   inter_len[b] = lens[b] + 3 fp_number[b];   meta[0] = T' = T + max_b inter_len[b] - max_b lens[b];
 *   src (B, cap) int32, entries q < min(T', cap): >= 0 = that row of text_hid[b]; -(1 + 3 (c - 1) + k) = row k of filler c;
 *   pos (B, T): the place of token j in the output (>= T' when the output ends before it); nins (B): labels > 0 in the row;
 *   emo_out / spk_out (B, cap) int64: emo[b, q mod T] / spk[b, q mod T] for q < min(T', cap) (either pair may be NULL) --
 *   the ids are NOT shifted by the insertions, as in the reference;
 *   meta[1 + b]: 0, or the sum of 1 (cap < T': the caller must re-plan with a larger cap -- a second launch and a second
 *   host read of meta; the Python side starts at cap = 4 T, which only tie-inflated counts exceed), 2 (lens[b] outside [0, T] or
 *   fp_number[b] outside [0, 3 T]; clamped), 4 (a label outside [0, 3]).  meta has 1 + B words.
 *   Nothing is written at or past column min(T', cap) of src, emo_out, spk_out.  B, T, cap >= 1; T <= 2^24.
 *   The output of sequence b is the first T' rows of: for p = 0, 1, ...: [3 rows of filler label[b, p] if p < T and it is
 *   > 0], text_hid[b, p mod T] -- rows past the end wrap to the start of the sequence, as the reference's padding does.
 *
 * kantts_fp_plan_given: the same map from GIVEN labels at a GIVEN width W, for teacher-forced steps that must not read the
 *   device (a captured step): there the labels come from the batch and T' is the width of the duration targets.  It takes
 *   no counts: fp_number[b] = nins[b] = #(1 <= label[b, p] <= 3) over all T slots, padding included (what kantts_fp_head
 *   with given labels counts); inter_len[b] = lens[b] + 3 fp_number[b]; meta[0] = the T' of these labels and lengths.
 *   src, emo_out, spk_out are (B, W): ALL of columns [0, W) is written, the first W entries of the stream below and
 *   emo[b, q mod T] / spk[b, q mod T] (a W > T' continues the wrap), and nothing at or past column W.  pos (B, T) as above:
 *   places >= W mean "not in the output", which kantts_fp_insert_bwd with Tp = cap = W skips, so that call stays in
 *   bounds for any labels.  meta[1 + b]: 0, or the sum of 2 (lens[b] outside [0, T]; clamped), 4 (a label outside [0, 3];
 *   taken as 0) and 8 (FP_ERR_WIDTH, in EVERY word: T' != W -- the batch is inconsistent and the step's result is to be
 *   discarded).  One launch, a workgroup per sequence; every workgroup counts the labels of all B rows for T'.
 *   B, T, W >= 1; T <= 2^24, W <= 2^26.
 *
 * kantts_fp_insert_fwd: out (B, Tp, C)[b, q] = src[b, q] >= 0 ? text_hid (B, T, C)[b, src] : fill (9, C)[-src - 1]; an entry
 *   outside [-9, T) gives a zero row.  Tp <= cap, else KANTTS_E_BADARG.
 * kantts_fp_insert_bwd: d_text_hid (B, T, C)[b, j] = sum of the rows of d_out (B, Tp, C) that hold token j (its place, then
 *   the wrapped copies in ascending place); d_fill (9, C)[r] = sum over the batch of the rows that hold filler row r, in a
 *   fixed order.  src, pos, nins as kantts_fp_plan wrote them.  C <= 1024.
 *
 * kantts_fp_ce: FpCELoss.  loss[0] = sum_{b, j < lens[b]} weight[y] * (-log softmax(probs[b, j])[y]) / sum_b min(lens[b], T),
 *   y = label[b, j] -- the probabilities are taken as logits, a second softmax, as the reference does (loss.py:88-105);
 *   d_probs (B, T, 4) (may be NULL) = d loss / d probs, zero on padding.  One launch, one workgroup.  A label outside [0, 3]
 *   on a valid token, or no valid token, gives NaN. */
int kantts_fp_head(const float* rows, const float* weight, const float* bias, const int32_t* lens, const int32_t* fp_label,
                   float* probs, int32_t* label, int32_t* fp_number, int B, int T, int C, void* stream);
int kantts_fp_head_bwd(const float* rows, const float* weight, const float* probs, const float* d_probs, float* d_rows,
                       float* d_weight, float* d_bias, long long N, int C, void* stream);
int kantts_fp_plan(const int32_t* label, const int32_t* lens, const int32_t* fp_number, const int64_t* emo, const int64_t* spk,
                   int32_t* inter_len, int32_t* meta, int32_t* src, int32_t* pos, int32_t* nins, int64_t* emo_out,
                   int64_t* spk_out, int B, int T, int cap, void* stream);
int kantts_fp_plan_given(const int32_t* label, const int32_t* lens, const int64_t* emo, const int64_t* spk, int32_t* inter_len,
                         int32_t* meta, int32_t* src, int32_t* pos, int32_t* nins, int64_t* emo_out, int64_t* spk_out,
                         int32_t* fp_number, int B, int T, int W, void* stream);
int kantts_fp_insert_fwd(const float* text_hid, const float* fill, const int32_t* src, float* out, int B, int T, int Tp, int cap,
                         int C, void* stream);
int kantts_fp_insert_bwd(const float* d_out, const int32_t* src, const int32_t* pos, const int32_t* nins, float* d_text_hid,
                         float* d_fill, int B, int T, int Tp, int cap, int C, void* stream);
int kantts_fp_ce(const float* probs, const int32_t* label, const int32_t* lens, const float* weight, float* loss, float* d_probs,
                 int B, int T, void* stream);

/* ---- Speaker-embedding extractor for SE voices (csrc/spk_embed.hip) --------------------------------------------------------
 * Kaldi fbank and the inference graph of the D-TDNN (CAM++ style) extractor, for a RAGGED batch: every entry takes the
 * per-item lengths and no item reads a neighbour's or its own padding.  Everything is fp32 on the VALU; BatchNorm arrives
 * folded into (scale, shift) tables, y = x * scale + shift.  No entry uses atomics: two calls on equal inputs give equal
 * bits, and an item's result does not depend on what else is in the batch.  NULL required pointers and sizes < 1:
 * KANTTS_E_BADARG; shapes outside the stated limits: KANTTS_E_UNSUPPORTED.  B <= 65535 everywhere.
 *
 * kantts_kaldi_fbank: wav (B, ld) fp32, nsamp (B) samples per item (clamped to ld) -> out (B, Tmax, nmel) log-mel, item b
 *   has T_b = nsamp < 400 ? 0 : 1 + (nsamp - 400) / 160 frames (clamped to Tmax); rows T_b .. Tmax - 1 are written as zeros.
 *   Per frame (400 samples, hop 160, snip_edges): subtract the frame mean, pre-emphasis 0.97 (the first sample against
 *   itself), times window (400), zero-padded 512-point FFT with tw (512: cos(2 pi k / 512), k < 256, then sin), power
 *   spectrum, mel bin m = sum_j mel_w[m, j] * power[mel_lo[m] + j], j < mel_n[m] (mel_w (nmel, wmax); mel_lo + mel_n <= 257),
 *   log(max(., FLT_EPSILON)).  cmn != 0: a second launch subtracts from every bin its mean over the item's own T_b frames.
 *   nmel <= 128.  The tables are the host's (kantts.preprocess.se_processor.kaldi_tables()).
 *
 * kantts_spk_conv2d: 3 x 3 convolution over (F, T) with stride (sf, 1) and padding 1, folded BN, optional residual, ReLU:
 *   out (B, Cout, Fout, T)[b, co, fo, t] = relu((sum_{ci, r, k} w (Cout, Cin, 3, 3) * in[b, ci, fo sf - 1 + r, t - 1 + k])
 *   * scale[co] + shift[co] + R), Fout = (Fin - 1) / sf + 1; `in` is read through the element strides (in_sb, in_sc, in_sf,
 *   in_st); a tap outside [0, Fin) x [0, lens[b]) is zero and out is written as zero for t >= lens[b].  R: res == NULL: 0;
 *   res (B, Cres, Fres, T) with sc_w == NULL: res[b, co, fo, t] (Cres == Cout, Fres == Fout); with sc_w (Cout, Cres): the
 *   1 x 1 shortcut (sum_ci sc_w[co, ci] * res[b, ci, fo rsf, t]) * sc_scale[co] + sc_shift[co].
 *   Cin <= 32, Cout % 8 == 0, Cout <= 32.
 *
 * kantts_spk_conv1d: y (B, CY, TY)[b, co_off + co, t] = post(sum_{ci < Cin, k < K} w (Cout, Cin, K)[co, ci, k] *
 *   pre(x (B, CX, TX)[b, ci, t stride + (k - K / 2) dil])) for t < len_out(b) = (lens[b] - 1) / stride + 1; columns at or
 *   past len_out(b) are not written.  pre (pre_scale != NULL) = relu(x * pre_scale[ci] + pre_shift[ci]); a tap outside
 *   [0, lens[b]) is zero AFTER pre.  post (post_scale != NULL) = relu(. * post_scale[co] + post_shift[co]).  K odd.
 *   psum != NULL (needs stride 1): per workgroup tile i of 64 columns, psum (B, NT, Cout)[b, i, co] = the sum of y over the
 *   tile's valid columns and pmax (B, NT, 2, Cout)[b, i, s, co] = the maximum over those of them in 100-column segment
 *   (64 i) / 100 + s (-FLT_MAX when there is none); NT = (max_out + 63) / 64, tiles at or past len_out(b) are not written.
 *   max_out: the widest len_out of the batch (sizes the launch).  Any Cin, Cout (tails are handled).
 *
 * kantts_spk_cam_gate_conv: the context-aware mask of one dense layer and its dilated convolution, from the h, psum, pmax
 *   of kantts_spk_conv1d: for item b and segment s, gate (G) = sigmoid(wb (G, Ch) . relu(wa (Ch, Cb) . (mean_b + segmax_b,s)
 *   + ba) + bb), mean_b = sum of the item's psum tiles (ascending) / lens[b]; y (B, CY, TY)[b, co_off + o, t] =
 *   gate[t / 100][o] * sum_{c, k < 3} w (G, Cb, 3)[o, c, k] * h (B, Cb, TH)[b, c, t + (k - 1) dil] for t < lens[b], taps
 *   outside [0, lens[b]) zero; nothing else of y is written.  Cb <= 128, Ch <= 64, G in {8, 16, 32, 64}, 1 <= dil <= 4.
 *
 * kantts_spk_tail: out (B, E)[b] = (w (E, 2 C) . [mean_t v, std_t v]) * oscale + oshift with v = relu(x (B, CX, TX)[b, c, t] *
 *   scale[c] + shift[c]) over t < lens[b]; std is the UNBIASED one (two passes; lens[b] == 1 gives NaN).  C <= 1024. */
int kantts_kaldi_fbank(const float* wav, const int32_t* nsamp, const float* window, const float* tw, const int32_t* mel_lo,
                       const int32_t* mel_n, const float* mel_w, float* out, int B, int ld, int Tmax, int nmel, int wmax,
                       int cmn, void* stream);
int kantts_spk_conv2d(const float* in, long long in_sb, long long in_sc, long long in_sf, long long in_st, const float* w,
                      const float* scale, const float* shift, const float* res, const float* sc_w, const float* sc_scale,
                      const float* sc_shift, const int32_t* lens, float* out, int B, int Cin, int Cout, int Fin, int T, int sf,
                      int Cres, int Fres, int rsf, void* stream);
int kantts_spk_conv1d(const float* x, const int32_t* lens, const float* w, const float* pre_scale, const float* pre_shift,
                      const float* post_scale, const float* post_shift, float* y, float* psum, float* pmax, int B, int Cin,
                      int CX, int TX, int Cout, int CY, int TY, int co_off, int K, int stride, int dil, int max_out,
                      void* stream);
int kantts_spk_cam_gate_conv(const float* h, const int32_t* lens, const float* psum, const float* pmax, const float* wa,
                             const float* ba, const float* wb, const float* bb, const float* w, float* y, int B, int Cb,
                             int TH, int Ch, int G, int CY, int TY, int co_off, int dil, int NT, int max_len, void* stream);
int kantts_spk_tail(const float* x, const int32_t* lens, const float* scale, const float* shift, const float* w,
                    const float* oscale, const float* oshift, float* out, int B, int C, int CX, int TX, int E, void* stream);

/* ------------------------------------------------------------------------------------------
 * Device-resident corpus of duration-free (MAS) and speaker-embedding (SE) voices (csrc/attn_prior.hip): the two batch
 * fields the collate of kantts/datasets/dataset.py builds per utterance on the host (:20-31 the beta-binomial alignment
 * prior, :757-762 the utterance's speaker embedding repeated over its symbols, :798-827 their padding).
 *
 * kantts_attn_prior_rows: the padded prior of a whole batch in one launch; every cell of out (B, Tout, Tin) fp32 is
 *   written (no memset in front).  With P = min(n_sym[b], Tin) -- the symbol count INCLUDING the trailing "~" -- and
 *   M = min(n_mel[b], Tout):
 *     out[b][i][k] = pmf of Beta-Binomial(P, i + 1, M - i) at k         for i < M and k < P
 *                  = 0                                                  elsewhere
 *   (the support point k = P is left out as in the reference, so a row does not sum to 1).  All gamma arguments are
 *   positive integers; with lfact[n] = log n! (fp64, n < n_lfact) the cell is
 *     exp(  lfact[P] - lfact[k] - lfact[P - k]
 *         + lfact[k + i] + lfact[P - k + M - i - 1] - lfact[P + M]
 *         - lfact[i] - lfact[M - i - 1] + lfact[M] )
 *   summed and exponentiated in fp64 and rounded once to fp32.  An item with P < 1 or M < 1 is all zeros.  An item with
 *   P + M >= n_lfact (the table does not reach it) gets NaN in its live cells and zeros elsewhere, and the table is not
 *   read for it.  Nothing outside out (B, Tout, Tin) is written and nothing of lfact at or past n_lfact is read, whatever
 *   n_sym / n_mel hold.  16-byte stores when out is 16-byte aligned.
 *   BADARG: a NULL pointer, B / Tout / Tin < 1, n_lfact < 2.  UNSUPPORTED: B > 65535 or Tout * Tin >= 2^31.
 *
 * kantts_broadcast_rows_f32: out (B, Tmax, D)[b][t][:] = table (n, D)[item[b]][:] for t < min(len[b], Tmax), zeros
 *   beyond; every cell of out is written, bit-exact copies.  item (B) int64, len (B) int32.  An item index outside [0, n)
 *   gives a row of zeros (nothing is read for it).  16-byte stores when out is 16-byte aligned.
 *   BADARG: a NULL pointer, B / Tmax / D / n < 1.  UNSUPPORTED: B > 65535 or Tmax * D >= 2^31. */
int kantts_attn_prior_rows(const double* lfact, int n_lfact, const int32_t* n_sym, const int32_t* n_mel, float* out, int B,
                           int Tout, int Tin, void* stream);
int kantts_broadcast_rows_f32(const float* table, int n, const int64_t* item, const int32_t* len, float* out, int B, int Tmax,
                              int D, void* stream);

/* ---- sy-BERT pre-training (csrc/sybert.hip): the BERT masking of a padded batch on the device, and the masked-LM head
 * (Linear(d_model -> |sy|) + SeqCELoss) fused.  Reference: kantts/datasets/dataset.py:873-925,1023-1042 (BERT_Text_Dataset
 * .bert_masking, MaskingActor), kantts/models/sambert/kantts_sambert.py (KanTtsTextsyBERT.fc), kantts/train/loss.py:444-460.
 *
 * kantts_bert_mask_rows: the device twin of kantts.datasets.bert_masking.draw.  seed_counter: two 64-bit words
 * {seed, counter} in DEVICE memory, the convention of kantts_nsf_draw_states.  With mix = kantts_rng_mix of csrc/common.h,
 * L = clamp(lens[b], 0, T) (the length INCLUDING the closing "~") and, for sequence b of draw number `counter`,
 *   key_b     = mix(mix(seed, 0x53594245), (counter << 20) | b)
 *   masked(j) = j < L - 1  and  (mix(key_b, j) >> 40) < thr              thr = floor(mask_ratio * 2^24), in [0, 2^24]
 *   n         = the number of masked positions,  n2 = 4 n / 5,  n3 = n / 10     (integer divisions)
 *   rank(j)   = the place of (mix(key_b, 2^32 + j), j) among the masked positions in ascending order
 *   rnd_b     = (hi32(mix(key_b, 2^33)) * nsym) >> 32                    ONE random symbol per sequence, as in the reference
 *   id(j)     = mask_id   for masked j with rank < n2
 *             = rnd_b     for masked j with n2 <= rank < n2 + n3
 *             = t(b, j)   otherwise (masked or not),   t(b, j) = targets[(b * T + j) * tgt_ts], the unmasked id
 * the launch writes, for every b < B and j < T,
 *   input_lings[(b * T + j) * ling_ts] = id(j)        (int64; ling_ts = 4 and the base of column 0 for a (B, T, 4) tensor)
 *   bert_masks[b * T + j]              = masked(j) ? 1.0f : 0.0f
 *   targets_out[b * T + j]             = t(b, j)      (targets_out == NULL: not written)
 * and nothing else: `targets` may be column 0 of input_lings ITSELF (tgt_ts == ling_ts, the same base: a thread reads its
 * cell before it writes it, and no other thread reads that cell) -- a batch gathered as (B, T, 4) rows is then masked in
 * place and its dense targets come out of the same launch; the cells between two positions (ling_ts > 1) and `seed` are not written.  Position L - 1 and the
 * padding at or past L are never masked.  Behind a barrier the launch stores counter + 1: consecutive launches (and replays
 * of one captured launch) draw different numbers, and a counter set back replays them.  ONE workgroup, a wave per sequence
 * (wave w takes sequences w, w + 16, ...): the counter is read and advanced by the same launch, and only inside one
 * workgroup does a barrier stand between every read and the store -- with a workgroup per sequence a workgroup that starts
 * late would read the advanced counter.  T may exceed the thread count: a wave walks its sequence 64 positions at a time.
 * Plain vector stores only, no atomics.
 * KANTTS_E_BADARG: a NULL pointer, seed_counter / targets / input_lings not 8-byte aligned, lens / bert_masks not 4-byte
 * aligned, targets_out not 8-byte aligned, B < 1, T < 1, ling_ts < 1, tgt_ts < 1, thr outside [0, 2^24].
 * KANTTS_E_UNSUPPORTED: T > 4096, B >= 2^20 (the key holds the item in 20 bits), nsym < 1.  Nothing is written when a call is
 * refused. */
int kantts_bert_mask_rows(uint64_t* seed_counter, const int64_t* targets, long long tgt_ts, const int32_t* lens,
                          int64_t* input_lings, long long ling_ts, float* bert_masks, int64_t* targets_out, int B, int T,
                          int thr, int mask_id, int nsym, void* stream);

/* kantts_mlm_head_fwd: logits[r][v] = bias[v] + sum_c hid[r][c] * W[v][c] are formed 16 rows at a time on
 * v_mfma_f32_16x16x4_f32 and never stored; per row an online softmax keeps the maximum, the sum of exponentials, the
 * arg-max (the LOWEST index among equal maxima, torch.argmax on the CPU) and the target's logit:
 *   lse[r]  = log sum_v exp(logits[r][v])                                  written for every r < M
 *   ce[r]   = lse[r] - logits[r][targets[r]]
 *   out[0]  = sum_r mask[r] * ce[r] / sum_r mask[r]                         the loss of SeqCELoss
 *   out[1]  = sum_r mask[r] * [argmax_v logits[r][v] != targets[r]] / sum_r mask[r]      its error rate
 *   out[2]  = sum_r mask[r]                                                 (the backward reads it)
 * A row with mask[r] == 0 adds exactly 0 to the three sums whatever its logits and its target are: a non-finite logit on
 * an unmasked row does NOT poison the loss as it would in the reference (0 * NaN there).  sum(mask) == 0 gives NaN in out[0]
 * and out[1], as the reference does.  A target outside [0, V) on a row with mask != 0 gives NaN in out[0].
 * fp32 operands and fp32 accumulation in every precision mode.  No atomics; equal inputs give equal bits: workgroup g (rows
 * 16 g ...) leaves its three sums in ws[3 g ..], a second launch behind it on the stream adds them in a fixed order.
 *   hid (M, C), W (V, C), bias (V) or NULL, targets (M) int64, mask (M), out (3), lse (M): dense; ws: 3 * ceil(M / 16) floats
 *   the call may overwrite, ws_floats says how many there are.
 *
 * kantts_mlm_head_bwd: for the forward that wrote `lse` and `out`, with g[r] = gscale * dloss[0] * mask[r] / out[2]
 * (dloss: the upstream gradient of out[0], ONE float in device memory; gscale: a host scalar, the trainer's 1 / V):
 *   dlogits[r][v] = g[r] * (exp(logits[r][v] - lse[r]) - [v == targets[r]])      mask[r] != 0;   exactly 0 otherwise
 *   d_hid[r][c]   = sum_v dlogits[r][v] * W[v][c]            exactly 0 on rows with mask[r] == 0
 *   d_W[v][c]     = sum_r dlogits[r][v] * hid[r][c]
 *   d_bias[v]     = sum_r dlogits[r][v]                      (d_bias == NULL: not written)
 * All three are WRITTEN, not accumulated into.  out[2] == 0, or a target outside [0, V) on a row with mask != 0, gives NaN
 * gradients.  Two launches: the first recomputes the logits as the forward did and leaves dlogits, zero-padded to
 * (16 ceil(M / 16), 16 ceil(V / 16)), in ws; the second holds one workgroup per 16 x 16 tile of d_W (its 8 waves take
 * interleaved 16-row blocks, the partial tiles are added in wave order through LDS; the tiles of the first 16 channels also
 * sum d_bias) and one workgroup per 16 rows of d_hid.  No atomics; equal inputs give equal bits.
 *   d_hid (M, C), d_W (V, C), d_bias (V); ws: 16 ceil(M / 16) * 16 ceil(V / 16) floats, 16-byte aligned.
 *
 * Both: KANTTS_E_BADARG: a NULL required pointer, M < 1, hid / W / d_hid / d_W / ws (backward) not 16-byte aligned.
 * KANTTS_E_UNSUPPORTED: C not a multiple of 16 or outside [16, 512], V outside [1, 4096], M > 2^24.  KANTTS_E_WORKSPACE:
 * ws_floats too small.  Nothing is written when a call is refused. */
int kantts_mlm_head_fwd(const float* hid, const float* W, const float* bias, const int64_t* targets, const float* mask,
                        float* out, float* lse, float* ws, long long ws_floats, int M, int C, int V, void* stream);
int kantts_mlm_head_bwd(const float* hid, const float* W, const float* bias, const int64_t* targets, const float* mask,
                        const float* lse, const float* out, const float* dloss, float gscale, float* d_hid, float* d_W,
                        float* d_bias, float* ws, long long ws_floats, int M, int C, int V, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KANTTS_HIP_H */
