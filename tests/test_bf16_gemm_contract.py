"""The bf16 contraction kernels of the SAM-BERT step -- kantts_bgemm_nt, _nt_pair, _nt_lnbwd, kantts_bgemm_tn, _tn_grouped
(csrc/gemm_bf16.hip, gemm_bf16_nt_body.inc) -- and the small kernels that write their operand images or consume their
partial sums (kantts_cast_f32_bf16, _tapmajor_bf16, _fragmajor_bf16, _relu_gate_bf16, _act_cast_bf16, _rows_sum_many)
against an fp64 interpreter of their contract (include/kantts_hip.h).

The form is that of tests/test_seq_contract.py: arena, builder, legs and device memory are imported from there and from
tests/test_step_tail_contract.py.  ``_evaluate`` (the ``_op_*`` functions) is written from the header comments alone -- not
from oracle/cabi_numpy.py, not from the kernels -- over ONE flat guarded arena that holds fp32, bf16, uint8 and the seed_dev
word, every block 16-byte aligned.  Operand rule: an fp32 operand is multiplied in float32 by its regenerated keep-scale
(index rule of csrc/common.h through cabi_numpy.dropout_scale), then rounded to bf16, ties to even; bf16 x bf16 products are
exact, so what is left to bound is the fp32 accumulation and the epilogue.  The LayerNorm(128) epilogues are the interpreter
functions and S expressions of test_seq_contract.py (kantts_ln128_fwd / kantts_ln128_bwd_rows); every case that uses them
takes its contraction from the exact class below, so that the LayerNorm finds the same input on every leg.  One table
(``_TABLE``) runs on three legs: the emulated ABI (which has no kantts_bgemm_nt_pair and takes no NULL host arrays), the
kernel sources on the CPU, and the device.  Every case names the branches it is there for (``_BRANCHES``).

Exactly, on every leg:
  * every element no call of the case writes keeps its bits: guards, inputs, columns beyond N (ldc / ldr / ldg > N), c when
    NULL is allowed, the accumulators when part_rows is set; return codes;
  * rows under rowmask are 0, dropped elements are 0, gated elements are 0 for gate values 0, -0 and < 0 (their S is 0);
  * the exact class: operands, res and bias from {+-0.5, +-1}, alpha / scale powers of two, dropout with p = 0.5 (keep-scale
    2); the interpreter asserts that the sum of absolute values stays below 2^24 units, so every output equals the fp64
    value bit for bit in any summation order, split-token atomics included.  All seam sizes live in this class: a dropped,
    doubled or misplaced tap, row, tile or slice moves a result by >= 1 unit.  Padding columns (lda / ldb > klen) and the
    rows behind a (klen, N) operand hold NaN: a staging predicate that lets them in shows as NaN;
  * kantts_bgemm_nt_pair: each problem has the bits of its own kantts_bgemm_nt call; kantts_bgemm_tn_grouped: of its own
    kantts_bgemm_tn call; kantts_rows_sum_many: two calls give the same bits; the partial rows of _nt_lnbwd summed by
    kantts_rows_sum_many give dbeta the bits of the accumulator form;
  * the casts (cast, tapmajor, fragmajor, relu_gate, act_cast): every output is the round-to-nearest-even bf16 of the
    float32 value -- ties in both directions, a carry into the exponent, +-0, +-inf, the largest finite fp32 (-> inf), NaN
    (stays NaN, quiet or signalling), and fp32 subnormals, which every leg rounds to nearest like any other value.
Measured, per element, for real-valued cases: |got - ref| <= R * (Ktot + 16) * 2^-24 * S, S = the same expression over
absolute values (tests/test_gemm_contract.py), Ktot = the summed klen (NT) or the M tokens (TN); R = 1 on the emulated ABI
and the kernel sources, 2 on the device.  LayerNorm epilogues: |got - ref| <= R * c * 2^-24 * S over test_seq_contract's S
expressions, c = 4 * ratio, ratio measured in every session from a float32 left-to-right and right-to-left evaluation of
the reference and refused when more than 10 % above the recorded one.  A bf16 output must be the round-to-nearest-even bf16
of some float within the bound.  The project's cap (tests/test_gpu_bf16_ops.py) holds as well: rel-L2 <= 2e-5 per fp32
tensor; tensors whose reference is exact cancellation (||ref|| <= 1e-9 ||S||) are exempt from it (EXEMPT_RECORDED) and
none lies between 1e-9 and 1e-3.
KANTTS_BGEMM_BM (read once per process) is forced to 64 and 128 in a child process each, on the kernel sources on the CPU
only: the 64-row fp32-A instantiations and the 128-row tiles are experiment switches no model code sets.
The measured ratio, c and the worst ratio to the bound per leg and entry point go to bf16_gemm_contract.json beside
gemm_contract.json.

Measured when this file was written: ratio = 8.290 (the rstd of nt_ln4, a LayerNorm row behind an exact contraction),
c = 33.16; none of the table's real-valued fp32 tensors is exempt from the relative cap.  Worst error on the device in units
of its bound (R = 2 there), per entry point: bgemm_nt 0.064 (nt_M65_real), bgemm_nt_pair 0.014, bgemm_nt_lnbwd 0.023 and the
kantts_ln128_fwd in front of it 0.026 (both of c * 2^-24 * S), bgemm_tn / _tn_grouped 0.059 (tn_real5), rows_sum_many 0.099; the
casts are exact.  Mutations of the kernel sources that the table was checked to catch (kernel-source leg, first failing case):
tap predicate t <= T (nt_taps0_f00), B staged without kc < klen (nt_inf_head_f00), bg_xcd_remap without its remainder
(nt_wg65), res added before the dropout (nt_M100), A-dropout index with lda (nt_taps0_f10), tap / slice decode swapped
(tn_v00_64128_f00), do_bias without bx == 0 (tn_v06_64129_f10), loop stride st (tn_v04_64129_f00), pg / pb added for dead rows
(lnb0_M1), bg_pack2 truncating (nt_M31_real).
"""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cabi_numpy
import test_seq_contract as Q
import test_step_tail_contract as T
from test_seq_contract import E_UNSUPPORTED, LN_EPS, _Mem, a64, ar
from test_step_tail_contract import E_BADARG, F32, F64, OK, U, _bf16_rne, _Leg

_REPORT = os.path.join(os.path.dirname(T._REPORT), "bf16_gemm_contract.json")
CAP_L2 = 2e-5             # tests/test_gpu_bf16_ops.py
RATIO_RECORDED = 8.290     # the float32 evaluation of the LayerNorm epilogues' reference, see above
EXEMPT_RECORDED = 0
MAX_SEG, TN_MAX_GROUP, ROWSUM_MAX = 12, 16, 32
_NAN16 = float("nan")
_TILES = (64128, 128128, 64256, 128256)
_FORMS = ((0, 0), (0, 1), (1, 0), (1, 1))
_NT_MS, _NT_NS, _NT_KS = (1, 31, 32, 33, 63, 64, 65, 100), (8, 120, 128, 136, 264), (8, 56, 64, 72, 128, 136)
_TN_MS, _TN_NS, _TN_KS, _TN_SL = (1, 63, 64, 65, 127, 128, 129, 200), (8, 56, 64, 72, 136), (8, 120, 128, 136, 264), (1, 2, 3, 5)
_TN_VARIANTS = ["tn:%d/%s/a_f32=%d,b_f32=%d" % (t, g, a, b) for t in _TILES for g in ("1d", "3d") for a, b in _FORMS]

_BRANCHES = [
    *["nt:M=%d" % m for m in _NT_MS], *["nt:N=%d" % n for n in _NT_NS], *["nt:klen=%d" % k for k in _NT_KS],
    *["nt:nseg=%d" % n for n in (1, 2, 3, 12)], *["nt:tiles=%d" % n for n in (1, 2, 3, 4)], "nt:segment-ends-inside-a-tile",
    *["nt:a_f32=%d,b_kn=%d" % f for f in _FORMS], "nt:taps-1/0/+1", "nt:taps-2/0/+2", *["nt:T=%d" % t for t in (5, 7, 33)],
    "nt:M%T!=0", "nt:|a_shift|>=T", "nt:bias", "nt:bias2", "nt:bias+bias2", "nt:alpha", "nt:relu", "nt:drop_p+seed_dev",
    "nt:res+ldr>N", "nt:gate-f32+ldg>N", "nt:gate-bf16+ldg>N", "nt:rowmask", "nt:c_bf16=0", "nt:c_bf16=1", "nt:ldc>N",
    "nt:a_drop_p+a_drop_ld!=lda", "nt:a_drop_p+tap", "nt:ln_out-f32", "nt:ln_out-bf16", "nt:ln-masked-row", "nt:ln-constant-row",
    "nt:bm64-by-rule,b_kn=0", "nt:bm64-by-rule,b_kn=1", *["nt:workgroups=%d" % w for w in (63, 64, 65, 71)], "nt:two-column-tiles",
    "nt:M=0", "nt:N=0",
    *["pair:a_f32=%d,b_kn=%d" % f for f in _FORMS], "pair:M=0", "pair:refusals",
    *["lnb:M=%d" % m for m in (1, 31, 32, 33, 65)], "lnb:a_f32=0", "lnb:a_f32=1", "lnb:c=NULL", "lnb:c-f32", "lnb:c-bf16",
    "lnb:c=NULL+c_bf16", "lnb:dres=NULL", "lnb:dres", "lnb:zero_rows=NULL", "lnb:zero_rows-some", "lnb:zero_rows-all",
    "lnb:accumulate", "lnb:part_rows", "lnb:part_rows==accumulators",
    *_TN_VARIANTS, *["tn:M=%d" % m for m in _TN_MS], *["tn:slices=%d" % s for s in _TN_SL], "tn:slices>ntile",
    *["tn:N=%d" % n for n in _TN_NS], *["tn:K=%d" % k for k in _TN_KS], "tn:taps(-1,1)", "tn:taps(-2,2)", "tn:shift>=T",
    *["tn:T=%d" % t for t in (5, 7, 65)], *["tn:groups=%d" % g for g in (5, 6, 8, 9, 12, 16)], "tn:slices=0,nprob=1",
    "tn:slices=0,nprob=7", "tn:c(K,1,NK)", "tn:c-parameter-layout", "tn:accumulate", "tn:alpha", "tn:db=NULL", "tn:db",
    "tn:db+N>BN", "tn:db+K>BK", "tn:db+slices", "tn:a_drop_p+seed_dev", *["tng:nprob=%d" % n for n in (1, 2, 7, 16)],
    "tng:db_host=NULL", "tng:db_host[p]=NULL", "tng:seeds=NULL", "tng:==single",
    *["flat:n=%d" % n for n in (0, 8, 2040, 2048, 2056)], "cast:edges", "cast:subnormals",
    *["relu_gate:dy_bf16=%d,y_bf16=%d" % f for f in _FORMS], "relu_gate:y+/0/-0/-", "act_cast:act=0", "act_cast:act=1",
    "act_cast:gate-f32", "act_cast:gate-bf16", *["tapmajor:ndesc=%d" % n for n in (0, 1, 3)],
    *["tapmajor:blocks=%d" % n for n in (1, 2, 5)], "tapmajor:KT=1", "tapmajor:KT=3", "tapmajor:N!=Cin",
    "fragmajor:sk=1", "fragmajor:sr=1", "fragmajor:(16,32)", "fragmajor:(48,96)", "fragmajor:blocks=1", "fragmajor:blocks=3",
    *["rowsum:n=%d" % n for n in (0, 1, 32)], *["rowsum:cols=%d" % n for n in (1, 31, 32, 33, 256)], "rowsum:split=0",
    "rowsum:split-middle", "rowsum:split=cols", *["rowsum:rows=%d" % n for n in (0, 1, 7, 8, 9, 205)], "rowsum:prior",
    "rowsum:same-bits",
]


def _r16(x):
    """float32 values -> the float32 values of their round-to-nearest-even bf16"""
    x = np.ascontiguousarray(x, dtype=F32)
    return (_bf16_rne(x.reshape(-1)).astype(np.uint32) << 16).view(F32).reshape(x.shape)


def _record(key, val):
    saved, Q._REPORT = Q._REPORT, _REPORT  # test_seq_contract's writer, pointed at this file's report
    try:
        Q._record(key, val)
    finally:
        Q._REPORT = saved


# ---------------------------------------------------------------------------------------------------------------------
# 1. the arena and the case builder
class _Builder(Q._Builder):
    def hout(self, n):
        """n bf16 elements of the arena's own noise (an output); returns the offset in bf16 elements"""
        return 2 * self.f32(n=(int(n) + 1) // 2)

    def u64(self, v):
        return self.raw(np.asarray([v], dtype=np.uint64).tobytes())

    def bits(self, u32):
        return self.f32(np.asarray(u32, dtype=np.uint32).view(F32))


class _Case:
    def __init__(self, name, build, emu=True):
        self.name, self._build, self.emu = name, build, emu
        self._built = self._ref = None

    def built(self):
        if self._built is None:
            b = _Builder(self.name)
            tags = set(self._build(b) or ())
            for c in b.calls:
                tags |= set(c.get("tags", ()))
            self._built = (b.finish(), b.calls, tuple(sorted(tags & set(_BRANCHES))))
        return self._built

    @property
    def branches(self):
        return self.built()[2]

    def reference(self):
        """the float64 evaluation, computed once and shared by every leg"""
        if self._ref is None:
            self._ref = _evaluate(self, F64)
        return self._ref


# ---------------------------------------------------------------------------------------------------------------------
# 2. the interpreter
class _Shadow(Q._Shadow):
    """test_seq_contract's shadow; ``f`` returns what the calls so far have left (for an input: the bytes the calls find), so
    that a LayerNorm epilogue reads the contraction's result.  Behind the arena lie ``scratch`` floats that are no memory of
    the case: the dy of kantts_bgemm_nt_lnbwd, which need not be stored."""

    def __init__(self, raw, dt, rev, scratch):
        self.n = raw.size
        super().__init__(np.concatenate([raw, np.zeros(scratch, dtype=F32)]), dt, rev)

    def f(self, idx):
        idx = np.asarray(idx, dtype=np.int64)
        assert idx.size == 0 or (idx.min() >= 0 and idx.max() < self.raw.size), "the case reads outside its arena"
        return self.val[idx]

    def h(self, idx):
        """bf16 elements ``idx`` of the arena as the calls find it, as float32"""
        idx = np.asarray(idx, dtype=np.int64)
        assert idx.size == 0 or (idx.min() >= 0 and idx.max() < 2 * self.n), "the case reads outside its arena"
        return (self.raw.view(np.uint16)[idx].astype(np.uint32) << 16).view(F32)

    def seed(self, off):
        return 0 if off is None else int(self.raw.view(np.uint64)[off // 2])

    def u8(self, off, n):
        return self.raw.view(np.uint8)[4 * off + ar(n)]


def _tok(rows, Tt, shift):
    """header: row i reads token i + shift of its own sequence of T tokens, zero outside [0, T)"""
    if shift == 0:
        return np.ones(rows.size, dtype=bool), rows
    t = rows % Tt + shift
    ok = (t >= 0) & (t < Tt)
    return ok, np.where(ok, rows + shift, 0)


def _operand(sh, off, idx, is_f32, ok, keep=None):
    """the bf16 value of every element as float64: fp32 operands times their keep-scale in float32, then rounded"""
    if is_f32:
        v = sh.raw[off + idx]
        if keep is not None:
            v = (v * keep).astype(F32)
        v = _r16(v)
    else:
        v = sh.h(off + idx)
    return np.where(ok, v, F32(0)).astype(F64)


def _nt_values(sh, c):
    """header: C[i][j] = epilogue(sum_s sum_k A_s[tok(i) + a_shift_s][k] * B_s(j, k)); v = (acc + bias[j] + bias2[j]) * alpha;
    relu; dropout(drop_p; element i*N + j of drop_seed + *seed_dev); v += res[i][j]; v = gate[i][j] > 0 ? v : 0; rowmask[i] -> 0.
    a_drop_p: element (i, k) of A is multiplied by the keep-scale of (a_drop_seed + *seed_dev, (i + a_shift) * a_drop_ld + k)."""
    dt, M, N = sh.dt, c["M"], c["N"]
    soff, rows, cols = sh.seed(c["seed_dev"]), ar(M), ar(N)
    acc, S = np.zeros((M, N), dtype=dt), np.zeros((M, N))
    for s in c["segs"]:
        K = s["klen"]
        ok, src = _tok(rows, c["T"], s["a_shift"])
        keep = None
        if c["a_f32"] and c["a_drop_p"] > 0:
            keep = cabi_numpy.dropout_scale(c["a_drop_p"], c["a_drop_seed"] + soff, src[:, None] * c["a_drop_ld"] + ar(K)[None, :])
        A = _operand(sh, s["a"], src[:, None] * s["lda"] + ar(K)[None, :], c["a_f32"], ok[:, None], keep)
        if c["b_kn"]:
            B = sh.h(s["b"] + ar(K)[:, None] * s["ldb"] + cols[None, :]).astype(F64)
        else:
            B = sh.h(s["b"] + cols[:, None] * s["ldb"] + ar(K)[None, :]).astype(F64).T
        acc = acc + A.astype(dt) @ B.astype(dt)
        S += np.abs(A) @ np.abs(B)
    for k in ("bias", "bias2"):
        if c[k] is not None:
            acc, S = acc + sh.f(c[k] + cols)[None, :], S + a64(sh.f(c[k] + cols))[None, :]
    alpha = dt(F32(c["alpha"]))
    v, S = acc * alpha, S * abs(float(alpha))
    if c["relu"]:
        v = np.maximum(v, dt(0))
    if c["drop_p"] > 0:
        keep = cabi_numpy.dropout_scale(c["drop_p"], c["drop_seed"] + soff, rows[:, None] * N + cols[None, :])
        v, S = v * keep.astype(dt), S * keep.astype(F64)
    if c["res"] is not None:
        r = sh.f(c["res"] + rows[:, None] * c["ldr"] + cols[None, :])
        v, S = v + r, S + a64(r)
    if c["gate"] is not None:
        gi = c["gate"] + rows[:, None] * c["ldg"] + cols[None, :]
        live = (sh.h(gi) if c["gate_bf16"] else sh.raw[gi]) > 0
        v, S = np.where(live, v, dt(0)), np.where(live, S, 0.0)
    if c["rowmask"] is not None:
        dead = (sh.u8(c["rowmask"], M) != 0)[:, None]
        v, S = np.where(dead, dt(0), v), np.where(dead, 0.0, S)
    return v, S, sum(s["klen"] for s in c["segs"])


def _unit(c):
    return min(0.25 * abs(float(F32(c["alpha"]))), 0.5)


def _nt_store(sh, c, v, S, Kt):
    M, N = v.shape
    idx = c["c"] + ar(M)[:, None] * c["ldc"] + ar(N)[None, :]
    what = "%s c%s@%d" % (c["ep"], "(bf16)" if c["c_bf16"] else "", c["c"])
    if c["c_bf16"]:
        sh.region(what, c["ep"], "bf16", None, u16=idx.reshape(-1), want=v.reshape(-1).astype(F64), S=S.reshape(-1), K=Kt,
                  exact=c.get("exact", False), unit=_unit(c))
    else:
        sh.put(idx, v, S)
        if c.get("skip_cols"):
            sh.region(what + " head columns", c["ep"], "scratch", idx[:, :c["skip_cols"]])
            idx = idx[:, c["skip_cols"]:]
        if c.get("exact"):
            sh.region(what, c["ep"], "exact", idx, unit=_unit(c))
        else:
            sh.region(what, c["ep"], "gemm", idx, K=Kt, cap_l2=True)


def _op_nt(sh, c):
    """header: M == 0 or N == 0 returns OK before any other check of the operands; the result is stored as bf16 (c_bf16) or
    fp32; ln_out: LayerNorm(128) of the output rows as kantts_ln128_fwd writes it"""
    if c["rc"] != OK or c["M"] == 0 or c["N"] == 0:
        return
    v, S, Kt = _nt_values(sh, c)
    _nt_store(sh, c, v, S, Kt)
    if c["ln_out"] is not None:
        assert c.get("exact") and c["ldc"] == 128 and not c["c_bf16"]
        Q._ln_fwd(sh, dict(ep=c["ep"], rc=OK, M=c["M"], x=c["c"], gamma=c["ln_gamma"], beta=c["ln_beta"], y=c["ln_out"], y_bf16=c["ln_out_bf16"],
                           mean=c["ln_mean"], rstd=c["ln_rstd"], eps=c["ln_eps"]), 128)


def _op_nt_pair(sh, c):
    """header: each problem is checked and computed exactly as its own kantts_bgemm_nt call"""
    if c["rc"] != OK:
        return
    for p in c["probs"]:
        _op_nt(sh, dict(p, ep=c["ep"], rc=OK))


def _op_nt_lnbwd(sh, c):
    """header: the contraction's result is the gradient dy of a LayerNorm's output; what the launch writes is what
    kantts_ln128_bwd_rows makes of it: dx (+ dres; rows of zero_rows written as 0) and the dgamma / dbeta accumulations.  dy is
    rounded to bf16 first when c_bf16 is set and is itself stored only if c is not NULL.  part_rows: workgroup w (rows
    32 w .. 32 w + 31) writes its 128 dgamma + 128 dbeta sums to row w INSTEAD of adding them to the accumulators."""
    if c["rc"] != OK or c["M"] == 0:
        return
    M, l, ep = c["M"], c["ln"], c["ep"]
    v, S, Kt = _nt_values(sh, c)
    assert c.get("exact")
    if c["c"] is not None:
        _nt_store(sh, c, v, S, Kt)
    if c["c_bf16"]:
        v = _r16(v.astype(F32)).astype(sh.dt)
    scr = sh.n
    sh.put(scr + ar(M * 128), v, a64(v))
    base = dict(ep=ep, rc=OK, gamma=l["gamma"], dy_bf16=0, exact=True)

    def rows(r0, mb, dgamma, dbeta):
        sub = lambda k, per: None if l[k] is None else l[k] + r0 * per // 4
        Q._ln_bwd(sh, dict(base, M=mb, x=l["x"] + 128 * r0, dy=scr + 128 * r0, mean=l["mean"] + r0, rstd=l["rstd"] + r0, dres=sub("dres", 512),
                           zero_rows=sub("zero_rows", 1), dx=l["dx"] + 128 * r0, dgamma=dgamma, dbeta=dbeta), 128)

    if l["part_rows"] is None:
        rows(0, M, l["dgamma"], l["dbeta"])
    else:
        for w in range((M + 31) // 32):
            pr = l["part_rows"] + 256 * w
            sh.put(pr + ar(256), np.zeros(256), np.zeros(256))
            rows(32 * w, min(32, M - 32 * w), pr, pr + 128)


def _tn_problem(sh, c, p, tag):
    """header: c[n*c_ns + k*c_ks + tap*c_ts] += alpha * sum_m A[m][n] * B[tok(m) + shift0 + tap*shift_step][k];
    db[n] += alpha * sum_m A[m][n] (of the rounded, dropped A); a_drop_* with the logical index m*N + n; operands given as fp32
    are rounded to bf16 when staged"""
    dt, M, N, K = sh.dt, c["M"], c["N"], c["K"]
    soff, rows = sh.seed(c["seed_dev"]), ar(M)
    keep = None
    if c["a_f32"] and c["a_drop_p"] > 0:
        keep = cabi_numpy.dropout_scale(c["a_drop_p"], p["seed"] + soff, rows[:, None] * N + ar(N)[None, :])
    A = _operand(sh, p["a"], rows[:, None] * c["lda"] + ar(N)[None, :], c["a_f32"], True, keep)
    alpha = dt(F32(c["alpha"]))
    kind = dict(kind="exact", unit=_unit(c)) if c.get("exact") else dict(kind="gemm", K=M, cap_l2=True)
    if p["db"] is not None:
        sh.acc(p["db"] + ar(N), alpha * A.astype(dt).sum(0), abs(float(alpha)) * np.abs(A).sum(0))
        sh.region("%s db@%d" % (tag, p["db"]), c["ep"], idx=p["db"] + ar(N), **kind)
    allidx = []
    for tap in range(c["ntaps"]):
        ok, src = _tok(rows, c["T"], c["shift0"] + tap * c["shift_step"])
        B = _operand(sh, p["b"], src[:, None] * c["ldb"] + ar(K)[None, :], c["b_f32"], ok[:, None])
        idx = p["c"] + ar(N)[:, None] * c["c_ns"] + ar(K)[None, :] * c["c_ks"] + tap * c["c_ts"]
        sh.acc(idx, alpha * (A.astype(dt).T @ B.astype(dt)), abs(float(alpha)) * (np.abs(A).T @ np.abs(B)))
        allidx.append(idx.reshape(-1))
    allidx = np.concatenate(allidx)
    assert np.unique(allidx).size == allidx.size
    sh.region("%s c@%d" % (tag, p["c"]), c["ep"], idx=allidx, **kind)


def _op_tn(sh, c):
    """header: M == 0 returns OK and writes nothing"""
    if c["rc"] != OK or c["M"] == 0:
        return
    for i, p in enumerate(c["probs"]):
        _tn_problem(sh, c, p, "%s[%d]" % (c["ep"], i))


def _rne_region(sh, c, dst_idx, value32):
    sh.region("%s dst@%d" % (c["ep"], c["dst"]), c["ep"], "rne", None, u16=np.asarray(dst_idx, dtype=np.int64).reshape(-1),
              src=np.ascontiguousarray(value32, dtype=F32).reshape(-1))


def _op_cast(sh, c):
    """header: fp32 -> bf16 (round to nearest even) over n elements"""
    if c["rc"] == OK and c["n"]:
        _rne_region(sh, c, c["dst"] + ar(c["n"]), sh.raw[c["src"] + ar(c["n"])])


def _op_relu_gate(sh, c):
    """header: dz = (y > 0) ? dy * scale : 0 over n elements, bf16 output"""
    if c["rc"] != OK or not c["n"]:
        return
    n = ar(c["n"])
    dy = sh.h(c["dy"] + n) if c["dy_bf16"] else sh.raw[c["dy"] + n]
    y = sh.h(c["y"] + n) if c["y_bf16"] else sh.raw[c["y"] + n]
    _rne_region(sh, c, c["dst"] + n, np.where(y > 0, dy * F32(c["scale"]), F32(0)))


def _op_act_cast(sh, c):
    """header: dst = bf16(f(src)); gate == NULL: f(v) = act ? LeakyReLU(v, slope) : v; gate != NULL: f(v) = v * (gate > 0 ? 1 : slope)"""
    if c["rc"] != OK or not c["n"]:
        return
    n, slope = ar(c["n"]), F32(c["slope"])
    v = sh.raw[c["src"] + n]
    if c["gate"] is not None:
        g = sh.h(c["gate"] + n) if c["gate_bf16"] else sh.raw[c["gate"] + n]
        v = v * np.where(g > 0, F32(1), slope)
    elif c["act"]:
        v = np.where(v > 0, v, v * slope)
    _rne_region(sh, c, c["dst"] + n, v)


def _op_tapmajor(sh, c):
    """header: Conv1d weights (N, Cin, KT) fp32 at src + src_off -> tap-major (KT, N, Cin) bf16 at dst + dst_off"""
    if c["rc"] != OK or not c["ndesc"]:
        return
    src, dst = [], []
    for so, do, N, Cin, KT in c["descs"][:c["ndesc"]]:
        tap, n, ci = np.meshgrid(ar(KT), ar(N), ar(Cin), indexing="ij")
        src.append((c["src"] + so + (n * Cin + ci) * KT + tap).reshape(-1))
        dst.append((c["dst"] + do + (tap * N + n) * Cin + ci).reshape(-1))
    _rne_region(sh, c, np.concatenate(dst), sh.raw[np.concatenate(src)])


def _op_fragmajor(sh, c):
    """header: element (r, k) = src[src_off + r*sr + k*sk] goes to
    dst[dst_off + ((r/16)*(K/32) + k/32)*512 + (((k%32)/8)*16 + r%16)*8 + k%8]"""
    if c["rc"] != OK or not c["ndesc"]:
        return
    src, dst = [], []
    for so, do, sr, sk, R, K in c["descs"][:c["ndesc"]]:
        r, k = np.meshgrid(ar(R), ar(K), indexing="ij")
        src.append((c["src"] + so + r * sr + k * sk).reshape(-1))
        dst.append((c["dst"] + do + ((r // 16) * (K // 32) + k // 32) * 512 + (((k % 32) // 8) * 16 + r % 16) * 8 + k % 8).reshape(-1))
    _rne_region(sh, c, np.concatenate(dst), sh.raw[np.concatenate(src)])


def _op_rows_sum(sh, c):
    """header: for each of n problems dst0[c] += sum_r src[r*cols + c] for c < split, dst1[c - split] += ... for c >= split"""
    if c["rc"] != OK:
        return
    cols, split = c["cols"], c["split"]
    for i in range(c["n"]):
        rows = c["rows"][i]
        x, S = sh.f(c["src"][i] + ar(rows * cols)).reshape(rows, cols), sh.S[c["src"][i] + ar(rows * cols)].reshape(rows, cols)
        for dst, lo, hi in ((c["dst0"][i], 0, split), (c["dst1"][i], split, cols)):
            if hi > lo:
                idx = dst + ar(hi - lo)
                sh.acc(idx, sh.sum0(x[:, lo:hi]) if rows else np.zeros(hi - lo), S[:, lo:hi].sum(0))
                kind = dict(kind="exact", unit=0.25) if c.get("exact") else (dict(kind="measured") if c.get("ln_rows") else dict(kind="gemm", K=rows))
                sh.region("%s[%d] dst@%d" % (c["ep"], i, dst), c["ep"], idx=idx, **kind)


def _op_check(sh, c):
    """not a call: two element lists (fp32, or bf16 with ``half``) that must hold the same bits afterwards"""
    sh.region("same %s" % c["what"], "-", "same", None, a=np.asarray(c["a"]).reshape(-1), b=np.asarray(c["b"]).reshape(-1),
              half=c.get("half", False))


_OPS = {"kantts_bgemm_nt": _op_nt, "kantts_bgemm_nt_pair": _op_nt_pair, "kantts_bgemm_nt_lnbwd": _op_nt_lnbwd, "kantts_bgemm_tn": _op_tn,
        "kantts_bgemm_tn_grouped": _op_tn, "kantts_cast_f32_bf16": _op_cast, "kantts_relu_gate_bf16": _op_relu_gate,
        "kantts_act_cast_bf16": _op_act_cast, "kantts_tapmajor_bf16": _op_tapmajor, "kantts_fragmajor_bf16": _op_fragmajor,
        "kantts_rows_sum_many": _op_rows_sum, "kantts_ln128_fwd": Q._OPS["kantts_ln128_fwd"], "same": _op_check}
_ENTRY_POINTS = sorted(set(_OPS) - {"same", "kantts_ln128_fwd"})


def _evaluate(case, dt, rev=False):
    raw, calls, _ = case.built()
    scratch = max([c["M"] * 128 for c in calls if c["ep"] == "kantts_bgemm_nt_lnbwd"] + [4])
    with np.errstate(all="ignore"):
        sh = _Shadow(raw, dt, rev, (scratch + 3) // 4 * 4)
        for c in calls:
            _OPS[c["ep"]](sh, c)
    if dt is F64:  # the exact class: every partial sum in any order is a whole number of units below 2^24
        for r in sh.regions.values():
            if r["kind"] == "exact" or (r["kind"] == "bf16" and r.get("exact")):
                val, S = (r["want"], r["S"]) if r["kind"] == "bf16" else (sh.val[r["idx"]], sh.S[r["idx"]])
                assert np.isfinite(val).all(), (case.name, r["what"])
                assert np.array_equal(val.astype(F32).astype(F64), val), (case.name, r["what"])
                if r.get("unit"):
                    units = S / r["unit"]
                    assert np.array_equal(units, np.floor(units)) and (units < 2 ** 24).all(), (case.name, r["what"])
    return sh


# ---------------------------------------------------------------------------------------------------------------------
# 3. the case table
_NT0 = dict(T=0, a_f32=0, b_kn=0, c_bf16=0, relu=0, bias=None, bias2=None, alpha=1.0, drop_p=0.0, drop_seed=0, seed_dev=None, res=None, ldr=0,
            gate=None, ldg=0, gate_bf16=0, a_drop_p=0.0, a_drop_seed=0, a_drop_ld=0, rowmask=None, ln_gamma=None, ln_beta=None, ln_out=None,
            ln_out_bf16=0, ln_eps=0.0, ln_mean=None, ln_rstd=None)
_TN0 = dict(T=0, a_f32=0, b_f32=0, ntaps=1, shift0=0, shift_step=0, slices=0, alpha=1.0, a_drop_p=0.0, seed_dev=None, tune=(0, 0))
_SEED = 0x9E3779B97F4A7C15


def _gate_values(b, n):
    """y in {+, 0, -0, -}"""
    g = b.randn(n)
    g[b.rng.integers(0, 7, size=n) == 0] = 0.0
    g[b.rng.integers(0, 7, size=n) == 0] = -0.0
    return g


def _nt(b, M, N, ks, form=(0, 0), exact=True, T=0, shifts=None, opts=(), alpha=1.0, c="f32", tags=(), **over):
    """the arguments of one kantts_bgemm_nt call with fresh operands.  Padding columns (lda, ldb > klen on every other segment)
    and the 8 rows behind a (klen, N) operand hold NaN; with T the A operand holds the whole last sequence."""
    a_f32, b_kn = form
    gen = b.dyadic if exact else b.randn
    rows_a = M if not T else -(-M // T) * T
    opts, segs, tags = set(opts), [], set(tags)
    zero_row = M // 2 if "constrow" in opts else None
    for i, K in enumerate(ks):
        lda, ldb = K + 8 * (i % 2), (N if b_kn else K) + 8 * ((i + 1) % 2)
        A = gen(max(rows_a, 1) * lda).reshape(max(rows_a, 1), lda)
        A[:, K:] = np.nan
        if zero_row is not None:
            A[zero_row, :K] = 0
        Bm = gen(((K + 8) if b_kn else max(N, 1)) * ldb).reshape(-1, ldb)
        if b_kn:
            Bm[K:], Bm[:, N:] = np.nan, np.nan
        else:
            Bm[:, K:] = np.nan
        if "inf0" in opts and i == 0:  # the operand's first 16 bytes: what a predicated-off chunk loads in place of its own address
            Bm[0, :8] = np.inf
        segs.append(dict(a=b.f32(A) if a_f32 else b.bf16(A), b=b.bf16(Bm), lda=lda, ldb=ldb, klen=K, a_shift=shifts[i] if shifts else 0))
    tiles = sum((K + 63) // 64 for K in ks)
    tags |= {"nt:M=%d" % M, "nt:N=%d" % N, "nt:nseg=%d" % len(ks), "nt:tiles=%d" % tiles, "nt:a_f32=%d,b_kn=%d" % form,
             "nt:c_bf16=%d" % (c == "bf16")} | {"nt:klen=%d" % K for K in ks}
    if len(ks) > 1 and any(K % 64 for K in ks[:-1]):
        tags.add("nt:segment-ends-inside-a-tile")
    if T:
        tags |= {"nt:T=%d" % T} | ({"nt:M%T!=0"} if M % T else set()) | ({"nt:|a_shift|>=T"} if any(abs(s) >= T for s in shifts) else set())
    ldc = N + 8 if "ldc" in opts else N
    g = dict(_NT0, ep="kantts_bgemm_nt", rc=OK, segs=segs, M=M, N=N, T=T, a_f32=a_f32, b_kn=b_kn, alpha=alpha, exact=exact, ldc=ldc,
             c_bf16=int(c == "bf16"), c=None if c is None else (b.hout(M * ldc) if c == "bf16" else b.f32(n=M * ldc)))
    if "ldc" in opts:
        tags.add("nt:ldc>N")
    if alpha != 1.0:
        tags.add("nt:alpha")
    for k in ("bias", "bias2"):
        if k in opts:
            g[k] = b.f32(gen(N))
            tags.add("nt:" + k)
    if {"bias", "bias2"} <= opts:
        tags.add("nt:bias+bias2")
    if "relu" in opts:
        g["relu"] = 1
        tags.add("nt:relu")
    if opts & {"drop", "adrop"}:
        g["seed_dev"] = b.u64(0x0123456789ABCDEF ^ (M * 977 + N))
    if "drop" in opts:
        g.update(drop_p=0.5 if exact else 0.3, drop_seed=_SEED + 31 * M + N)
        tags.add("nt:drop_p+seed_dev")
    if "adrop" in opts:
        assert a_f32
        g.update(a_drop_p=0.5 if exact else 0.3, a_drop_seed=_SEED ^ (M + 7 * N), a_drop_ld=max(s["lda"] for s in segs) + 16)
        tags |= {"nt:a_drop_p+a_drop_ld!=lda"} | ({"nt:a_drop_p+tap"} if shifts and any(shifts) else set())
    if "res" in opts:
        g["ldr"] = N + 4
        r = gen(M * g["ldr"]).reshape(M, -1)
        if zero_row is not None:
            r[zero_row] = 0.5
        g["res"] = b.f32(r)
        tags.add("nt:res+ldr>N")
    if opts & {"gate32", "gate16"}:
        g["ldg"], g["gate_bf16"] = N + 8, int("gate16" in opts)
        v = _gate_values(b, M * g["ldg"])
        g["gate"] = b.bf16(v) if g["gate_bf16"] else b.f32(v)
        tags.add("nt:gate-bf16+ldg>N" if g["gate_bf16"] else "nt:gate-f32+ldg>N")
    if "rowmask" in opts:
        z = (b.rng.integers(0, 3, size=M) == 0).astype(np.uint8) * 7
        z[0], z[-1] = 1, 0 if M > 1 else 1
        g["rowmask"] = b.u8(z)
        tags.add("nt:rowmask")
    if opts & {"ln32", "ln16"}:
        assert N == 128 and exact
        bf = int("ln16" in opts)
        g.update(ln_gamma=b.f32(1 + b.randn(128, 0.3)), ln_beta=b.f32(b.randn(128, 0.3)), ln_out_bf16=bf, ln_eps=LN_EPS, ln_mean=b.f32(n=M), ln_rstd=b.f32(n=M),
                 ln_out=b.hout(M * 128) if bf else b.f32(n=M * 128))
        tags |= {"nt:ln_out-bf16" if bf else "nt:ln_out-f32"} | ({"nt:ln-masked-row"} if "rowmask" in opts else set()) | (
            {"nt:ln-constant-row"} if zero_row is not None else set())
    if "inf0" in opts:  # columns 0 .. 7 (b_kn; column 0 otherwise) are not finite by the contract itself and are not compared
        assert N >= 16 and c == "f32"
        g["skip_cols"] = 8
    g.update(over)
    g["tags"] = tags
    return g


def _nt_cases():
    cs = []

    def add(name, emu=True, **kw):
        def build(b):
            b.calls.append(_nt(b, **kw))
        cs.append(_Case(name, build, emu=emu))

    epi = (("bias",), ("bias2", "relu"), ("bias", "bias2", "res"), ("drop", "ldc"), ("gate32", "res"), ("gate16", "drop"), ("rowmask", "bias"),
           ("rowmask", "res", "drop", "relu", "ldc"))
    for i, M in enumerate(_NT_MS):  # every M, N, klen and form on the 32-row tile, exact and real-valued
        for exact in (True, False):
            add("nt_M%d%s" % (M, "" if exact else "_real"), M=M, N=_NT_NS[i % 5], ks=[_NT_KS[i % 6]], form=_FORMS[i % 4], exact=exact, opts=epi[i],
                alpha=(1.0, 0.5, 2.0)[i % 3] if exact else (1.0, 0.37)[i % 2], c=("f32", "bf16")[i % 2])
    for i, N in enumerate(_NT_NS):
        add("nt_N%d" % N, M=_NT_MS[(2 * i + 3) % 8], N=N, ks=[_NT_KS[(i + 3) % 6]], form=_FORMS[(i + 1) % 4], opts=epi[(i + 4) % 8], c=("bf16", "f32")[i % 2])
    for i, K in enumerate(_NT_KS):
        for form in (_FORMS[i % 4], _FORMS[(i + 2) % 4]):
            add("nt_K%d_f%d%d" % ((K,) + form), M=_NT_MS[(3 * i + 1) % 8], N=_NT_NS[(i + 2) % 5], ks=[K], form=form, opts=epi[(i + 2) % 8])
    # segments: different klen, one ends inside a 64-deep tile, 2 / 3 / 4 / 12 tiles (odd and even pipelines)
    for j, ks in enumerate(([64, 56], [72, 8], [64, 8, 128], [8, 16] * 6, [136, 72, 56])):
        for form in _FORMS:
            for exact in ((True, False) if form in ((0, 0), (1, 1)) else (True,)):
                add("nt_segs%d_f%d%d%s" % ((j,) + form + ("" if exact else "_real",)), M=(33, 65, 31, 64, 100)[j], N=(136, 8, 128, 120, 264)[j], ks=ks, form=form,
                    exact=exact, opts=epi[(j + 2 * form[0] + form[1]) % 8], c=("f32", "bf16")[j % 2])
    # conv taps: the sequence boundary inside a 32-row tile, M % T != 0, rows next to a sequence end hold non-zero neighbours
    for j, (T_, sh_, M) in enumerate(((5, (-1, 0, 1), 33), (7, (-2, 0, 2), 65), (33, (-1, 0, 1), 100), (5, (-5, 0, 5), 32), (7, (2, 0, -2), 63),
                                      (33, (-2, 0, 2), 64))):
        for form in _FORMS:
            tags = ["nt:taps-1/0/+1" if 1 in sh_ else "nt:taps-2/0/+2"] if abs(sh_[0]) < 3 else []
            add("nt_taps%d_f%d%d" % ((j,) + form), M=M, N=(8, 136)[j % 2], ks=[(8, 72, 64)[(j + t) % 3] for t in range(3)], form=form, T=T_, shifts=sh_,
                opts=("adrop", "bias") if form[0] else ("bias", "res"), tags=tags)
            if form == (1, 0):
                add("nt_taps%d_real" % j, M=M, N=(8, 136)[j % 2], ks=[72, 8, 64], form=form, T=T_, shifts=sh_, exact=False, opts=("adrop", "bias", "relu"), tags=tags)
    for form in ((1, 0), (1, 1)):  # the A-operand dropout without taps: a_drop_ld != lda
        for exact in (True, False):
            add("nt_adrop_f%d%d%s" % (form + ("" if exact else "_real",)), M=65, N=120, ks=[72, 56], form=form, exact=exact, opts=("adrop", "drop", "res"))
    for j, (M, o) in enumerate(((33, ("ln32", "rowmask", "constrow", "res")), (33, ("ln16", "rowmask", "constrow", "res")), (1, ("ln32",)), (64, ("ln16", "bias")),
                                (100, ("ln32", "drop", "res", "constrow")))):
        add("nt_ln%d" % j, M=M, N=128, ks=[72, 64][:1 + j % 2], form=_FORMS[j % 4], opts=o)
    for form in _FORMS:  # the first 16 bytes of B hold +inf: a chunk past klen that is staged although its predicate is off turns the tile into NaN
        add("nt_inf_head_f%d%d" % form, M=33, N=136, ks=[72, 8], form=form, opts=("inf0", "bias"))
    for k in ("M", "N"):  # M == 0 / N == 0: OK, nothing written, whatever else the arguments hold
        add("nt_%s0" % k, **dict(dict(M=33, N=8, ks=[8], tags=["nt:%s=0" % k]), **{k: 0}))
    return cs


def _nt_tile_cases():
    cs = []

    def add(name, tags, **kw):
        def build(b):
            b.calls.append(_nt(b, tags=tags, **kw))
        cs.append(_Case(name, build))

    for kn in (0, 1):  # the 64-row tile by the rule itself: bf16 A and the smallest grid that qualifies (256 workgroups)
        add("nt_bm64_kn%d" % kn, ["nt:bm64-by-rule,b_kn=%d" % kn], M=16321, N=8, ks=[8], form=(0, kn), opts=("bias",))
    for i, total in enumerate((63, 64, 65, 71)):  # bg_xcd_remap from 64 workgroups on, with and without a remainder
        add("nt_wg%d" % total, ["nt:workgroups=%d" % total], M=32 * total - 1, N=8, ks=[8], form=_FORMS[i], opts=("res",))
    add("nt_two_column_tiles", ["nt:two-column-tiles"], M=33 * 32 - 5, N=136, ks=[8], form=(1, 1), opts=("bias2",))
    return cs


def _pair_cases():
    cs = []
    for i, form in enumerate(_FORMS):
        for exact in (True, False):
            def build(b, i=i, form=form, exact=exact):
                M, N = (33, 64, 100, 31)[i], (136, 8, 120, 128)[i]
                kw0 = dict(M=M, N=N, ks=[72, 8], form=form, exact=exact, opts=("bias", "drop", "ldc") + (("adrop",) if form[0] else ()), c="f32")
                kw1 = dict(M=M, N=N, ks=[64], form=form, exact=exact, opts=("res", "relu", "rowmask"), alpha=2.0 if exact else 0.7, c="bf16")
                own = [_nt(b, **kw) for kw in (kw0, kw1)]
                b.calls.extend(own)
                probs = [dict(o, c=b.hout(M * o["ldc"]) if o["c_bf16"] else b.f32(n=M * o["ldc"])) for o in own]
                probs[1] = dict(probs[1], drop_p=0.5 if exact else 0.2, drop_seed=_SEED + 5, seed_dev=own[0]["seed_dev"])  # a seed of its own
                own[1].update(drop_p=probs[1]["drop_p"], drop_seed=probs[1]["drop_seed"], seed_dev=probs[1]["seed_dev"])
                b.call("kantts_bgemm_nt_pair", probs=probs, tags=["pair:a_f32=%d,b_kn=%d" % form])
                for o, p in zip(own, probs):
                    idx = ar(M)[:, None] * o["ldc"] + ar(N)[None, :]
                    b.call("same", what="pair problem c@%d" % p["c"], a=o["c"] + idx, b=p["c"] + idx, half=bool(o["c_bf16"]))
            cs.append(_Case("pair_f%d%d%s" % (form + ("" if exact else "_real",)), build, emu=False))

    def empty(b):
        probs = [_nt(b, M=33, N=8, ks=[8]), _nt(b, M=33, N=8, ks=[16])]
        b.call("kantts_bgemm_nt_pair", probs=[dict(p, M=0) for p in probs], tags=["pair:M=0"])
    cs.append(_Case("pair_M0", empty, emu=False))
    return cs


def _lnb(b, M, a_f32, c, c_bf16, dres, zr, part, ks=(72, 8), opts=("bias",), prior=None):
    """one kantts_bgemm_nt_lnbwd call behind the kantts_ln128_fwd that leaves mean / rstd; alpha = 2: dy in units of 0.5"""
    x = b.randn(M * 128).reshape(M, 128) + F32(0.3)
    d = dict(x=b.f32(x), gamma=b.f32(1 + b.randn(128, 0.3)), beta=b.f32(b.randn(128, 0.3)), mean=b.f32(n=M), rstd=b.f32(n=M), M=M)
    b.call("kantts_ln128_fwd", y=b.f32(n=M * 128), y_bf16=0, eps=LN_EPS, **d)
    g = _nt(b, M=M, N=128, ks=list(ks), form=(a_f32, 1), opts=opts, alpha=2.0, c=c)
    z = None
    if zr is not None:
        z = np.ones(M, np.uint8) if zr == "all" else (b.rng.integers(0, 3, size=M) == 0).astype(np.uint8) * 7
        if zr == "some":
            z[0], z[-1] = 1, 0 if M > 1 else 1
    dres = b.f32(b.randn(M * 128)) if dres else None
    prior = prior or (b.randn(128), b.dyadic(128))
    ln = dict(x=d["x"], gamma=d["gamma"], mean=d["mean"], rstd=d["rstd"], dres=dres,
              zero_rows=None if z is None else b.u8(z), dx=b.f32(n=M * 128), dgamma=b.f32(prior[0]), dbeta=b.f32(prior[1]),
              part_rows=b.f32(n=(M + 31) // 32 * 256) if part else None)
    tags = {"lnb:M=%d" % M, "lnb:a_f32=%d" % a_f32, {None: "lnb:c=NULL", "f32": "lnb:c-f32", "bf16": "lnb:c-bf16"}[c], "lnb:dres" if dres is not None else "lnb:dres=NULL",
            {None: "lnb:zero_rows=NULL", "some": "lnb:zero_rows-some", "all": "lnb:zero_rows-all"}[zr], "lnb:part_rows" if part else "lnb:accumulate"}
    if c is None and c_bf16:
        tags.add("lnb:c=NULL+c_bf16")
    g.update(ep="kantts_bgemm_nt_lnbwd", ln=ln, c_bf16=int(c_bf16), tags=tags)
    b.calls.append(g)
    return g, prior


def _lnbwd_cases():
    cs = []
    spec = ((1, 0, None, 0, False, None, False), (31, 1, "f32", 0, True, "some", False), (32, 0, "bf16", 1, False, "all", True),
            (33, 1, None, 1, True, "some", True), (65, 0, "f32", 0, True, None, True), (65, 1, "bf16", 1, False, "some", False),
            (33, 0, None, 1, False, None, False), (1, 1, "bf16", 1, True, "all", True))
    for j, (M, af, c, cb, dres, zr, part) in enumerate(spec):
        def build(b, a=(M, af, c, cb, dres, zr, part), j=j):
            _lnb(b, *a, ks=((72, 8), (64,), (8, 136))[j % 3], opts=(("bias",), ("bias", "res"), ("rowmask",))[j % 3] + (("adrop",) if a[1] else ()))
        cs.append(_Case("lnb%d_M%d" % (j, M), build))
    for M, af in ((33, 0), (65, 1)):  # the partial rows summed by kantts_rows_sum_many: dbeta has the bits of the accumulator form
        def build(b, M=M, af=af):
            state = b.rng.bit_generator.state
            g1, prior = _lnb(b, M, af, None, 1, True, "some", False)
            b.rng.bit_generator.state = state  # the same operands again
            g2, _ = _lnb(b, M, af, None, 1, True, "some", True, prior=prior)
            l1, l2 = g1["ln"], g2["ln"]
            b.call("kantts_rows_sum_many", n=1, cols=256, split=128, rows=[(M + 31) // 32], src=[l2["part_rows"]], dst0=[l2["dgamma"]], dst1=[l2["dbeta"]],
                   ln_rows=True, tags=["lnb:part_rows==accumulators"])
            b.call("same", what="dbeta of both forms", a=l1["dbeta"] + ar(128), b=l2["dbeta"] + ar(128))
            b.call("same", what="dx of both forms", a=l1["dx"] + ar(M * 128), b=l2["dx"] + ar(M * 128))
        cs.append(_Case("lnb_part_rows_sum_M%d" % M, build))
    return cs


def _tn(b, M, N, K, form=(0, 0), exact=True, tune=(0, 0), T=0, taps=(1, 0, 0), layout="nk", prior=True, db=False, alpha=1.0, adrop=False, nprob=1,
        grouped=False, db_null=(), seeds_null=False, tags=(), **over):
    """the arguments of one kantts_bgemm_tn / _grouped call with fresh operands (padding columns hold NaN)"""
    a_f32, b_f32 = form
    gen = b.dyadic if exact else b.randn
    ntaps, shift0, step = taps
    rows_b = M if not T else -(-M // T) * T
    lda, ldb = N + 8, K + 8
    g = dict(_TN0, ep="kantts_bgemm_tn_grouped" if grouped else "kantts_bgemm_tn", rc=OK, M=M, N=N, K=K, T=T, a_f32=a_f32, b_f32=b_f32, ntaps=ntaps,
             shift0=shift0, shift_step=step, lda=lda, ldb=ldb, alpha=alpha, exact=exact, tune=tune, db_null=db_null == "all", seeds_null=seeds_null)
    g.update(dict(c_ns=K, c_ks=1, c_ts=N * K) if layout == "nk" else dict(c_ns=K * ntaps, c_ks=ntaps, c_ts=1))
    if adrop:
        assert a_f32
        g.update(a_drop_p=0.5 if exact else 0.3, seed_dev=b.u64(0xFEDCBA9876543210 ^ (M * 131 + K)))
    probs = []
    for p in range(nprob):
        A = gen(max(M, 1) * lda).reshape(-1, lda)
        A[:, N:] = np.nan
        Bm = gen(max(rows_b, 1) * ldb).reshape(-1, ldb)
        Bm[:, K:] = np.nan
        c0 = (gen(ntaps * N * K) if prior else np.zeros(ntaps * N * K, F32))
        no_db = not db or db_null == "all" or p in (db_null or ())
        probs.append(dict(a=b.f32(A) if a_f32 else b.bf16(A), b=b.f32(Bm) if b_f32 else b.bf16(Bm), c=b.f32(c0), c0=c0,
                          db=None if no_db else b.f32(gen(N) if prior else np.zeros(N, F32)), seed=(_SEED + 17 * p) if adrop else 0))
    if seeds_null:  # header: a_drop_seed_host NULL means the shape's seed for every problem
        for p in probs:
            p["seed"] = _SEED + 99
    g["probs"] = probs
    tile, sl = tune
    ntile = (M + 63) // 64
    tags = set(tags) | {"tn:M=%d" % M, "tn:N=%d" % N, "tn:K=%d" % K, "tn:c(K,1,NK)" if layout == "nk" else "tn:c-parameter-layout",
                        "tn:db" if db and db_null != "all" else "tn:db=NULL"}
    if sl:
        tags |= {"tn:slices=%d" % sl} | ({"tn:slices>ntile"} if sl > ntile else set())
        groups = nprob * ntaps * min(sl, ntile)
        one_d = tile % 2 == 0 and groups * 4 >= 3 * 8 * ((groups + 7) // 8)  # the launcher's rule for the XCD-aware 1-D grid
        tags.add("tn:groups=%d" % groups)
        if tile:
            tags.add("tn:%d/%s/a_f32=%d,b_f32=%d" % (tile - tile % 2, "1d" if one_d else "3d", a_f32, b_f32))
        BN, BK = (tile - tile % 2) // 1000, (tile - tile % 2) % 1000
        if db and tile:
            tags |= ({"tn:db+N>BN"} if N > BN else set()) | ({"tn:db+K>BK"} if K > BK else set()) | ({"tn:db+slices"} if min(sl, ntile) > 1 else set())
    else:
        tags.add("tn:slices=0,nprob=%d" % nprob)
    if T:
        tags |= {"tn:T=%d" % T, {1: "tn:taps(-1,1)", 2: "tn:taps(-2,2)"}.get(step, "")} | ({"tn:shift>=T"} if abs(shift0) >= T else set())
    tags |= ({"tn:accumulate"} if prior else set()) | ({"tn:alpha"} if alpha != 1.0 else set()) | ({"tn:a_drop_p+seed_dev"} if adrop else set())
    if grouped:
        tags |= {"tng:nprob=%d" % nprob} | ({"tng:db_host=NULL"} if db_null == "all" else set()) | ({"tng:db_host[p]=NULL"} if db and db_null not in ((), "all") else set()) | (
            {"tng:seeds=NULL"} if seeds_null else set())
    g.update(over)
    g["tags"] = tags
    return g


def _tn_cases():
    cs = []
    variants = [(t + g3, a, bf) for t in _TILES for g3 in (0, 1) for a, bf in _FORMS]
    for vi, (tile, af, bf) in enumerate(variants):  # all 32 variants in the exact class, shapes cycling through every seam size
        M, N, K = _TN_MS[vi % 8], _TN_NS[(vi + vi // 8) % 5], _TN_KS[(vi // 2 + vi // 16) % 5]
        ntile = (M + 63) // 64
        # the 1-D grid needs >= 6 groups by the rule: three taps (M >= 65) or a slice count above ntile cannot give them alone
        if tile % 2 == 0:
            taps, sl = ((3, -1, 1), (3, -2, 2))[vi % 2], (2, 3, 5)[vi % 3] if ntile >= 2 else 1
            nprob = 1 if 3 * min(sl, ntile) in (6, 12) else 2
        else:
            taps, sl, nprob = ((1, 0, 0), (3, -1, 1), (3, -7, 7))[vi % 3], _TN_SL[(vi + vi // 8) % 4], 1
        kw = dict(M=M, N=N, K=K, form=(af, bf), tune=(tile, sl), T=(5, 7, 65)[vi % 3] if taps[0] > 1 else 0, taps=taps, layout=("nk", "param")[vi % 2],
                  prior=vi % 4 != 3, db=vi % 3 != 1, alpha=(1.0, 0.5, 2.0)[vi % 3], adrop=bool(af) and vi % 2 == 0, nprob=nprob, grouped=nprob > 1)

        def build(b, kw=kw):
            b.calls.append(_tn(b, **kw))
        cs.append(_Case("tn_v%02d_%d_f%d%d" % (vi, tile, af, bf), build))
    real = (dict(M=200, N=136, K=264, form=(0, 0), tune=(64128, 3), T=7, taps=(3, -1, 1), db=True),
            dict(M=129, N=72, K=136, form=(1, 1), tune=(128129, 2), adrop=True, db=True, alpha=0.37, layout="param"),
            dict(M=65, N=56, K=120, form=(1, 0), tune=(64257, 5), T=65, taps=(3, -2, 2), prior=False),
            dict(M=127, N=64, K=128, form=(0, 1), tune=(128256, 2), T=5, taps=(3, -1, 1), db=True, layout="param"),
            dict(M=200, N=8, K=8, form=(1, 1), tune=(0, 0), db=True, adrop=True), dict(M=1, N=8, K=264, form=(0, 0), tune=(0, 1), db=True))
    for j, kw in enumerate(real):
        def build(b, kw=kw):
            b.calls.append(_tn(b, exact=False, **kw))
        cs.append(_Case("tn_real%d" % j, build))
    for name, kw in (("tn_groups5", dict(M=321, N=8, K=8, tune=(64128, 5))), ("tn_groups9", dict(M=129, N=72, K=136, tune=(64128, 3), T=7, taps=(3, -1, 1), db=True)),
                     ("tn_groups6", dict(M=65, N=136, K=264, tune=(64128, 2), T=5, taps=(3, -2, 2), db=True)),
                     ("tn_groups8", dict(M=128, N=8, K=120, tune=(128128, 2), T=65, taps=(2, -1, 2), nprob=2, grouped=True)),
                     ("tn_groups12", dict(M=127, N=56, K=8, tune=(64256, 2), T=7, taps=(3, -1, 1), nprob=2, grouped=True, db=True)),
                     # the odd / even tile pipeline of one slice: 4, 3, 2 + 2, 2 + 1 and 3 + 3 token tiles
                     ("tn_pipe4", dict(M=200, N=72, K=136, tune=(64128, 1), T=7, taps=(3, -1, 1), db=True, form=(1, 1))),
                     ("tn_pipe3", dict(M=129, N=8, K=264, tune=(128256, 1), db=True)), ("tn_pipe2_2", dict(M=200, N=136, K=8, tune=(64256, 2), db=True, form=(0, 1))),
                     ("tn_pipe2_1", dict(M=129, N=56, K=120, tune=(128129, 2), T=5, taps=(3, -2, 2), form=(1, 0), adrop=True)),
                     ("tn_pipe3_3", dict(M=321, N=8, K=8, tune=(64129, 2), db=True)),
                     ("tn_shift_ge_T", dict(M=63, N=8, K=8, tune=(64128, 1), T=5, taps=(3, -5, 5), db=True)),
                     ("tn_rule_nprob1", dict(M=200, N=64, K=128, tune=(0, 0), db=True, form=(1, 0)))):
        def build(b, kw=kw):
            b.calls.append(_tn(b, **kw))
        cs.append(_Case(name, build))
    return cs


def _tng_cases():
    """grouped: every problem has the bits of its own kantts_bgemm_tn call (exact class), with NULL host arrays"""
    cs = []
    spec = ((1, dict(M=65, N=8, K=8, tune=(64128, 2), db=True), True), (2, dict(M=129, N=72, K=136, tune=(64128, 3), db=True, db_null=(1,), form=(1, 0), adrop=True), True),
            (7, dict(M=200, N=56, K=120, tune=(0, 0), db=True, db_null="all", T=5, taps=(3, -1, 1), form=(0, 1)), False),
            (16, dict(M=64, N=8, K=8, tune=(64128, 1), db=True, form=(1, 1), adrop=True, seeds_null=True, layout="param"), False),
            (7, dict(M=127, N=64, K=128, tune=(128257, 2), db=True, form=(1, 1), adrop=True), True))
    for j, (nprob, kw, emu) in enumerate(spec):
        def build(b, nprob=nprob, kw=kw):
            g = _tn(b, nprob=nprob, grouped=True, tags=["tng:==single"], **kw)
            b.calls.append(g)
            n_c = g["ntaps"] * g["N"] * g["K"]
            for p in g["probs"]:  # the same operands, fresh outputs with the same prior contents
                own = dict(p, c=b.f32(p["c0"]), db=None if p["db"] is None else b.f32(b_prior(b, g, p)))
                b.calls.append(dict(g, ep="kantts_bgemm_tn", probs=[own], tags=()))
                b.call("same", what="grouped problem c@%d" % p["c"], a=p["c"] + ar(n_c), b=own["c"] + ar(n_c))
                if p["db"] is not None:
                    b.call("same", what="grouped problem db@%d" % p["db"], a=p["db"] + ar(g["N"]), b=own["db"] + ar(g["N"]))
        cs.append(_Case("tng%d_nprob%d" % (j, nprob), build, emu=emu))
    return cs


def b_prior(b, g, p):
    """the prior contents of problem p's db block (as the builder filled it)"""
    for off, data in b.fills:
        if off == p["db"]:
            return data.view(F32).copy()
    raise AssertionError("no fill for db")


_EDGE_BITS = np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000, 0x3FFFFFFF, 0x3FFF8000, 0xBFFF8000, 0x00000000, 0x80000000,
                       0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0xFF800001, 0x3F800000],
                      dtype=np.uint32)
_SUBNORMAL_BITS = np.array([0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x00017FFF, 0x007FFFFF, 0x007F8000, 0x807FFFFF, 0x80008000,
                            0x80018000, 0x00400000, 0x0000FFFF, 0x80000001, 0x007F7FFF, 0x00800000], dtype=np.uint32)


def _flat_data(b, n, edges=True):
    v = b.randn(n)
    if edges and n:
        k = min(n, _EDGE_BITS.size)
        v[:k] = _EDGE_BITS.view(F32)[:k]
        v[n - 8:n] = _EDGE_BITS.view(F32)[:8] if n >= 16 else v[n - 8:n]
    return v


def _small_cases():
    cs = []
    flat = (0, 8, 2040, 2048, 2056)

    def cast(b):
        for n in flat:
            b.call("kantts_cast_f32_bf16", src=b.f32(_flat_data(b, max(n, 8))), dst=b.hout(max(n, 8)), n=n, tags=["flat:n=%d" % n, "cast:edges"])
    cs.append(_Case("cast_flat", cast))

    def cast_sub(b):
        b.call("kantts_cast_f32_bf16", src=b.bits(_SUBNORMAL_BITS), dst=b.hout(16), n=16, tags=["cast:subnormals"])
    cs.append(_Case("cast_subnormals", cast_sub))

    def relu_gate(b):
        for i, (db_, yb) in enumerate(_FORMS):
            for n in (flat[i], flat[i + 1]):
                dy, y = _flat_data(b, max(n, 8)), _gate_values(b, max(n, 8))
                b.call("kantts_relu_gate_bf16", dy=b.bf16(dy) if db_ else b.f32(dy), dy_bf16=db_, y=b.bf16(y) if yb else b.f32(y), y_bf16=yb,
                       dst=b.hout(max(n, 8)), scale=(1.0, 1.0 / 0.8, 2.0, 1.0 / 0.9)[i], n=n,
                       tags=["flat:n=%d" % n, "relu_gate:dy_bf16=%d,y_bf16=%d" % (db_, yb), "relu_gate:y+/0/-0/-"])
    cs.append(_Case("relu_gate", relu_gate))

    def act_cast(b):
        for i, (gate, act) in enumerate(((None, 0), (None, 1), ("f32", 0), ("bf16", 1))):
            for n in (flat[i + 1], flat[(i + 3) % 5]):
                g = _gate_values(b, max(n, 8))
                b.call("kantts_act_cast_bf16", src=b.f32(_flat_data(b, max(n, 8))), gate=None if gate is None else (b.bf16(g) if gate == "bf16" else b.f32(g)),
                       gate_bf16=int(gate == "bf16"), dst=b.hout(max(n, 8)), act=act, slope=(0.0, 0.1, 0.2, 0.01)[i], n=n,
                       tags=["flat:n=%d" % n, "act_cast:act=%d" % act if gate is None else "act_cast:gate-%s" % gate])
    cs.append(_Case("act_cast", act_cast))

    def tapmajor(b):
        ws = ((16, 8, 3), (5, 24, 1), (7, 3, 3))  # (N, Cin, KT): unequal N and Cin, sizes that are no multiple of 8
        for ndesc, blocks in ((0, 1), (1, 2), (3, 5), (3, 1)):
            src = np.concatenate([_flat_data(b, n * ci * kt + 3) for n, ci, kt in ws])
            so, descs = 0, []
            for n, ci, kt in ws:
                descs.append((so + 1, 2 * so + 8, n, ci, kt))
                so += n * ci * kt + 3
            tab = b"".join(np.asarray(d[:2], np.int64).tobytes() + np.asarray(d[2:] + (0,), np.int32).tobytes() for d in descs)
            b.call("kantts_tapmajor_bf16", src=b.f32(src), dst=b.hout(2 * so + 16), table=b.raw(tab), descs=descs, ndesc=ndesc, blocks=blocks,
                   tags=["tapmajor:ndesc=%d" % ndesc, "tapmajor:blocks=%d" % blocks] + (["tapmajor:KT=1", "tapmajor:KT=3", "tapmajor:N!=Cin"] if ndesc == 3 else []))
    cs.append(_Case("tapmajor", tapmajor))

    def fragmajor(b):
        for (R, K), blocks in (((16, 32), 1), ((48, 96), 3), ((48, 96), 1), ((16, 32), 3)):
            src = _flat_data(b, 2 * R * K + 8)
            descs = [(4, 0, K, 1, R, K), (R * K + 5, R * K + 8, 1, R, R, K)]  # row-major (sk = 1) and its transpose (sr = 1)
            tab = b"".join(np.asarray(d[:4], np.int64).tobytes() + np.asarray(d[4:], np.int32).tobytes() for d in descs)
            b.call("kantts_fragmajor_bf16", src=b.f32(src), dst=b.hout(2 * R * K + 16), table=b.raw(tab), descs=descs, ndesc=2, blocks=blocks,
                   tags=["fragmajor:sk=1", "fragmajor:sr=1", "fragmajor:(%d,%d)" % (R, K), "fragmajor:blocks=%d" % blocks])
    cs.append(_Case("fragmajor", fragmajor))

    def rowsum(name, n, cols, split, rows, exact, twice=False):
        def build(b):
            gen = b.dyadic if exact else b.randn
            srcs = [b.f32(gen(max(r * cols, 1))) for r in rows[:n]]
            for _ in range(2 if twice else 1):
                state = b.rng.bit_generator.state
                d0 = [b.f32(gen(max(split, 1))) for _ in range(n)]
                d1 = [b.f32(gen(max(cols - split, 1))) for _ in range(n)]
                if twice:
                    b.rng.bit_generator.state = state  # the same prior contents for the second call
                b.call("kantts_rows_sum_many", n=n, cols=cols, split=split, rows=list(rows[:n]), src=srcs, dst0=d0, dst1=d1, exact=exact,
                       tags=["rowsum:n=%d" % n, "rowsum:cols=%d" % cols, "rowsum:prior", "rowsum:split=0" if split == 0 else
                             ("rowsum:split=cols" if split == cols else "rowsum:split-middle")] + ["rowsum:rows=%d" % r for r in rows[:n]])
            if twice:
                first, second = b.calls[-2], b.calls[-1]
                for k in ("dst0", "dst1"):
                    w = split if k == "dst0" else cols - split
                    for i in range(n):
                        b.call("same", what="%s[%d] of two calls" % (k, i), a=first[k][i] + ar(w), b=second[k][i] + ar(w), tags=["rowsum:same-bits"])
        cs.append(_Case(name, build))

    rr = (0, 1, 7, 8, 9, 205)
    rowsum("rowsum_n0", 0, 32, 16, (), True)
    rowsum("rowsum_n1_c1", 1, 1, 0, (205,), True)
    rowsum("rowsum_n1_c31", 1, 31, 31, (9,), True)
    rowsum("rowsum_n32_c33", 32, 33, 17, tuple(rr[i % 6] for i in range(32)), True)
    rowsum("rowsum_n32_c32_real", 32, 32, 32, tuple(rr[(i + 2) % 6] for i in range(32)), False)
    rowsum("rowsum_c256", 1, 256, 128, (7,), True)
    rowsum("rowsum_c256_real_twice", 1, 256, 128, (205,), False, twice=True)
    rowsum("rowsum_c33_real_twice", 32, 33, 0, tuple(rr[(i + 3) % 6] for i in range(32)), False, twice=True)
    return cs


def _build_table():
    table = {"ntk_shapes": _nt_cases(), "ntk_tiles": _nt_tile_cases(), "pair": _pair_cases(), "lnbwd": _lnbwd_cases(), "tn": _tn_cases(),
             "tn_grouped": _tng_cases(), "small": _small_cases()}
    names = [c.name for cs in table.values() for c in cs]
    assert len(set(names)) == len(names)
    return table


_TABLE = _build_table()
_GROUPS = list(_TABLE)
_MEASURED = {}


def _c():
    """c = 4 x the worst ratio of (float32, sequential sums in both directions) - (float64) to 2^-24 * S over the LayerNorm
    epilogues of the table (the contractions in front of them are exact in float32 as well)"""
    if not _MEASURED:
        worst, where = 0.0, None
        for cases in _TABLE.values():
            for case in cases:
                ref = case.reference()
                keys = [k for k, r in ref.regions.items() if r["kind"] == "measured" or (r["kind"] == "bf16" and "K" not in r)]
                if not keys:
                    continue
                for rev in (False, True):
                    low = _evaluate(case, F32, rev)
                    for key in keys:
                        (want, S), got = Q._values(ref, ref.regions[key]), np.asarray(Q._values(low, low.regions[key])[0], dtype=F64)
                        ok = np.isfinite(want) & (S > 0)
                        if ok.any():
                            ratio = float((np.abs(got - want)[ok] / (U * S[ok])).max())
                            if ratio > worst:
                                worst, where = ratio, "%s %s" % (case.name, ref.regions[key]["what"])
        _MEASURED.update(ratio=worst, c=4.0 * worst, case=where)
        _record("fp32_reference", {"max_ratio_to_2^-24_S": worst, "c": 4.0 * worst, "case": where})
    return _MEASURED["c"]


# ---------------------------------------------------------------------------------------------------------------------
# 4. back ends
def _leg_params(emu=True):
    ps = T._leg_params()
    return ps if emu else ps[1:]


def _ptr(m, c, key, half=False, sub=None):
    v = c.get(key) if sub is None else sub
    if v is None:
        return None
    return (m.h(v) if half else m.p(v)) + c.get("byte_shift", {}).get(key, 0)


def _bgemm_args(m, c):
    import kantts._hip as hip

    g = hip.BGemmArgs()
    for i, s in enumerate(c["segs"]):
        q = g.seg[i]
        q.a, q.b = _ptr(m, c, "a%d" % i, not c["a_f32"], s["a"]), _ptr(m, c, "b%d" % i, True, s["b"])
        q.lda, q.ldb, q.klen, q.a_shift = s["lda"], s["ldb"], s["klen"], s["a_shift"]
    g.nseg = c.get("nseg", len(c["segs"]))
    for k in ("M", "N", "T", "a_f32", "b_kn", "ldc", "c_bf16", "relu", "alpha", "drop_p", "drop_seed", "ldr", "ldg", "gate_bf16", "a_drop_p", "a_drop_seed",
              "a_drop_ld", "ln_out_bf16", "ln_eps"):
        setattr(g, k, c[k])
    g.c, g.gate, g.ln_out = _ptr(m, c, "c", c["c_bf16"]), _ptr(m, c, "gate", c["gate_bf16"]), _ptr(m, c, "ln_out", c["ln_out_bf16"])
    for k in ("bias", "bias2", "seed_dev", "res", "rowmask", "ln_gamma", "ln_beta", "ln_mean", "ln_rstd"):
        setattr(g, k, _ptr(m, c, k))
    if c["rc"] == OK:  # no call of the table reaches a kernel with a pointer the header forbids
        for k in ("c", "gate", "ln_out", "bias", "bias2", "res", "ln_gamma", "ln_beta"):
            assert not getattr(g, k) or getattr(g, k) % 16 == 0, (c["ep"], k)
        assert all(g.seg[i].a % 16 == 0 and g.seg[i].b % 16 == 0 for i in range(g.nseg))
    return g


def _tn_args(m, c, p):
    import kantts._hip as hip

    g = hip.BGemmTnArgs()
    for k in ("lda", "ldb", "M", "N", "K", "T", "a_f32", "b_f32", "ntaps", "shift0", "shift_step", "slices", "c_ns", "c_ks", "c_ts", "alpha", "a_drop_p"):
        setattr(g, k, c[k])
    g.a, g.b = _ptr(m, c, "a", not c["a_f32"], p["a"]), _ptr(m, c, "b", not c["b_f32"], p["b"])
    g.c, g.db, g.a_drop_seed, g.seed_dev = _ptr(m, c, "c", False, p["c"]), _ptr(m, c, "db", False, p["db"]), p["seed"], _ptr(m, c, "seed_dev")
    return g


def _invoke(L_, m, c):
    """one call of the table through the C ABI"""
    import kantts._hip as hip

    ep, s = c["ep"], hip.stream()
    if ep == "kantts_bgemm_nt":
        return L_.kantts_bgemm_nt(None if c.get("args_null") else ctypes.byref(_bgemm_args(m, c)), s)
    if ep == "kantts_bgemm_nt_pair":
        ga, gb = (None if p is None else ctypes.byref(_bgemm_args(m, dict(p, rc=c["rc"]))) for p in c["probs"])
        return L_.kantts_bgemm_nt_pair(ga, gb, s)
    if ep == "kantts_bgemm_nt_lnbwd":
        l, ln = hip.LnBwdArgs(), c["ln"]
        for k in ("x", "gamma", "mean", "rstd", "dres", "zero_rows", "dx", "part_rows"):
            setattr(l, k, _ptr(m, c, "ln." + k, False, ln[k]))
        l.dgamma_accum, l.dbeta_accum = _ptr(m, c, "ln.dgamma", False, ln["dgamma"]), _ptr(m, c, "ln.dbeta", False, ln["dbeta"])
        return L_.kantts_bgemm_nt_lnbwd(None if c.get("args_null") else ctypes.byref(_bgemm_args(m, c)), None if c.get("ln_null") else ctypes.byref(l), s)
    if ep in ("kantts_bgemm_tn", "kantts_bgemm_tn_grouped"):
        assert L_.kantts_launch_tuning(c["tune"][0], c["tune"][1], 0) == OK
        try:
            g = _tn_args(m, c, c["probs"][0])
            if ep == "kantts_bgemm_tn":
                return L_.kantts_bgemm_tn(None if c.get("args_null") else ctypes.byref(g), s)
            n = len(c["probs"])
            arr = lambda vals: (ctypes.c_void_p * max(n, 1))(*vals)
            a = arr([_ptr(m, c, "a", not c["a_f32"], p["a"]) for p in c["probs"]])
            b_ = arr([_ptr(m, c, "b", not c["b_f32"], p["b"]) for p in c["probs"]])
            cc, db = arr([m.p(p["c"]) for p in c["probs"]]), arr([m.p(p["db"]) for p in c["probs"]])
            seeds = (ctypes.c_uint64 * max(n, 1))(*[p["seed"] for p in c["probs"]])
            if c["seeds_null"]:
                g.a_drop_seed = c["probs"][0]["seed"]
            nulls = c.get("null_arrays", ())
            return L_.kantts_bgemm_tn_grouped(None if c.get("args_null") else ctypes.byref(g), c.get("nprob", n), None if "a" in nulls else a,
                                              None if "b" in nulls else b_, None if "c" in nulls else cc, None if c["db_null"] else db,
                                              None if c["seeds_null"] else seeds, s)
        finally:
            assert L_.kantts_launch_tuning(0, 0, 0) == OK
    if ep == "kantts_cast_f32_bf16":
        return L_.kantts_cast_f32_bf16(_ptr(m, c, "src"), _ptr(m, c, "dst", True), c["n"], s)
    if ep == "kantts_relu_gate_bf16":
        return L_.kantts_relu_gate_bf16(_ptr(m, c, "dy", c["dy_bf16"]), c["dy_bf16"], _ptr(m, c, "y", c["y_bf16"]), c["y_bf16"], _ptr(m, c, "dst", True),
                                        c["scale"], c["n"], s)
    if ep == "kantts_act_cast_bf16":
        return L_.kantts_act_cast_bf16(_ptr(m, c, "src"), _ptr(m, c, "gate", c["gate_bf16"]), c["gate_bf16"], _ptr(m, c, "dst", True), c["act"], c["slope"],
                                       c["n"], s)
    if ep in ("kantts_tapmajor_bf16", "kantts_fragmajor_bf16"):
        return getattr(L_, ep)(_ptr(m, c, "src"), _ptr(m, c, "dst", True), _ptr(m, c, "table"), c["ndesc"], c["blocks"], s)
    if ep == "kantts_rows_sum_many":
        if c.get("args_null"):
            return L_.kantts_rows_sum_many(None, s)
        g = hip.RowSumArgs()
        g.n, g.cols, g.split = c["n"], c["cols"], c["split"]
        for i in range(min(len(c["src"]), ROWSUM_MAX)):
            g.rows[i], g.src[i], g.dst0[i], g.dst1[i] = c["rows"][i], m.p(c["src"][i]), m.p(c["dst0"][i]), m.p(c["dst1"][i])
        return L_.kantts_rows_sum_many(ctypes.byref(g), s)
    return Q._invoke(L_, m, c)


_WORST = {}


def _flush():
    """the worst ratio to the bound per leg and entry point so far"""
    for (leg, ep), (w, where, bound) in list(_WORST.items()):
        _record("%s_%s" % (leg, ep), {"max_ratio_to_bound": w, "case": where, "R": 2.0 if leg == "gpu" else 1.0, "bound": bound})


def _from16(u):
    return (np.asarray(u).astype(np.uint32) << 16).view(F32)


def _check(case, leg, got, raw):
    """the arena after the calls against the reference, region by region; what no region covers must hold its old bits"""
    ref = case.reference()
    g16, r16, g32 = got.view(np.uint16), raw.view(np.uint16), got.view(np.uint32)
    covered = np.zeros(g16.size, dtype=bool)
    c = _c()

    def factor(r):
        return (r["K"] + 16.0, "(K+16)*2^-24*S") if "K" in r else (c, "c*2^-24*S")

    def ratio_of(err, S, what, r):
        f, name = factor(r)
        assert np.array_equal(err[S == 0], np.zeros(int((S == 0).sum()))), "%s: an element that must be exact is not" % what
        ratio = float((err[S > 0] / (f * U * S[S > 0])).max()) if (S > 0).any() else 0.0
        key = (leg.name, r["ep"])
        if ratio >= _WORST.get(key, (-1.0,))[0]:
            _WORST[key] = (ratio, case.name, name)
        print("%s %s: max |err| %.3e, ratio to %s %.4f" % (leg.name, what, float(err.max()) if err.size else 0.0, name, ratio))
        assert ratio <= leg.R, "%s: error %.3f x the bound %s (R = %g)" % (what, ratio, name, leg.R)

    for r in ref.regions.values():
        what, kind, idx = "%s %s" % (case.name, r["what"]), r["kind"], r["idx"]
        if kind == "same":
            a, b_ = (g16[r["a"]], g16[r["b"]]) if r["half"] else (g32[r["a"]], g32[r["b"]])
            assert np.array_equal(a, b_), "%s: the bits differ in %d of %d" % (what, int((a != b_).sum()), a.size)
            continue
        if kind == "rne":
            covered[r["u16"]] = True
            have, src = g16[r["u16"]], r["src"]
            nan = np.isnan(src)
            assert np.isnan(_from16(have[nan])).all(), "%s: a NaN did not stay NaN" % what
            bad = have[~nan] != _bf16_rne(src[~nan])
            assert not bad.any(), "%s: %d of %d are not the round-to-nearest-even bf16, first: %#x -> %#x, expected %#x" % (
                what, int(bad.sum()), bad.size, int(src[~nan][bad].view(np.uint32)[0]), int(have[~nan][bad][0]), int(_bf16_rne(src[~nan][bad][:1])[0]))
            continue
        if kind == "bf16":
            covered[r["u16"]] = True
            have = _from16(g16[r["u16"]])
            if r.get("exact"):
                bad = g16[r["u16"]] != _bf16_rne(r["want"].astype(F32))
                assert not bad.any(), "%s: %d of %d differ from the bf16 of the exact value, first at %d: %r, expected %r" % (
                    what, int(bad.sum()), bad.size, int(np.argmax(bad)), have[bad][:4], r["want"][bad][:4])
                continue
            bound = leg.R * factor(r)[0] * U * r["S"]
            lo, hi = _from16(_bf16_rne(Q._inward(r["want"] - bound, True))), _from16(_bf16_rne(Q._inward(r["want"] + bound, False)))
            bad = ~((have >= lo) & (have <= hi))
            print("%s %s: %d bf16 values, %d outside" % (leg.name, what, have.size, int(bad.sum())))
            assert not bad.any(), "%s: %d values are the bf16 of no float within the bound" % (what, int(bad.sum()))
            continue
        covered[2 * idx] = True
        covered[2 * idx + 1] = True
        have, want = got[idx], ref.val[idx]
        if kind == "scratch":
            continue
        if kind == "exact":
            bad = have.astype(F64) != want
            assert not bad.any(), "%s: %d of %d differ from the exact value, first at %d: %r, expected %r" % (
                what, int(bad.sum()), bad.size, int(np.argmax(bad)), have[bad][:4], want[bad][:4])
            continue
        S = ref.S[idx]  # gemm / measured
        assert np.isfinite(have).all(), "%s: not finite" % what
        err = np.abs(have.astype(F64) - want)
        ratio_of(err, S, what, r)
        if r.get("cap_abs") is not None:
            assert err.size == 0 or float(err.max()) <= r["cap_abs"], "%s: max |err| %.3e > %.1e" % (what, float(err.max()), r["cap_abs"])
        if r.get("cap_l2") and not Q._exempt(want, S):
            l2 = float(np.linalg.norm(err) / np.linalg.norm(want))
            print("%s %s: rel-L2 %.3e" % (leg.name, what, l2))
            assert l2 <= CAP_L2, "%s: rel-L2 %.3e" % (what, l2)
    covered = covered[:g16.size]
    same = g16[~covered] == r16[~covered]
    assert same.all(), "%s: %d two-byte words outside the outputs were written, first at float %d" % (
        case.name, int((~same).sum()), int(np.flatnonzero(~covered)[np.argmax(~same)]) // 2)


def _run_case(case, leg):
    import kantts._hip as hip

    raw, calls, _ = case.built()
    m = _Mem(raw, leg)
    for c in calls:
        if c["ep"] == "same":
            continue
        with np.errstate(all="ignore"):
            rc = _invoke(hip.lib(), m, c)
        assert rc == c["rc"], "%s %s: returned %d, expected %d" % (case.name, c["ep"], rc, c["rc"])
    _check(case, leg, m.result(), raw)


@pytest.mark.parametrize("group", _GROUPS)
@pytest.mark.parametrize("leg", T._leg_params())
def test_bf16_kernels_match_the_fp64_interpreter(leg, group):
    leg = _Leg(leg)
    ran = 0
    try:
        with leg.context():
            for case in _TABLE[group]:
                if leg.name == "emu" and not case.emu:
                    continue
                _run_case(case, leg)
                ran += 1
    finally:
        _flush()
    assert ran or (leg.name == "emu" and group == "pair")


@pytest.mark.skipif(not T._HAVE_CLANG, reason="ROCm clang not installed")
@pytest.mark.parametrize("bm", (64, 128))
def test_forced_row_tiles_in_a_fresh_process(bm):
    """KANTTS_BGEMM_BM is read once per process: the kantts_bgemm_nt part of the kernel-source leg again with 64-row tiles (the
    fp32-A instantiations no rule selects) and 128-row tiles, in a child process each.  On the CPU only: these are experiment
    switches that no model code sets."""
    if "KANTTS_BGEMM_BM" in os.environ:
        pytest.skip("already the child process")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k",
                        "test_bf16_kernels_match_the_fp64_interpreter and src and ntk"], env=dict(os.environ, KANTTS_BGEMM_BM=str(bm)),
                       capture_output=True, text=True, timeout=1800, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and "2 passed" in r.stdout, r.stdout[-2000:] + r.stderr[-1000:]


def test_c_comes_from_the_fp32_evaluation_of_the_reference():
    """the measured ratio and c (recorded in bf16_gemm_contract.json), pinned to the ratio recorded when the table was written"""
    c = _c()
    print("fp32 reference: worst ratio to 2^-24*S %.4f (%s), c = %.4f" % (_MEASURED["ratio"], _MEASURED["case"], c))
    assert c == 4.0 * _MEASURED["ratio"]
    assert 1.0 < _MEASURED["ratio"] <= 1.1 * RATIO_RECORDED, _MEASURED


def test_exempt_tensors_are_the_recorded_ones():
    """fp32 tensors whose reference is exact cancellation (no relative cap): their number is stated, and no tensor lies in the
    gap between 1e-9 and 1e-3 -- by the fp64 reference alone"""
    n = total = 0
    for cases in _TABLE.values():
        for case in cases:
            ref = case.reference()
            for r in ref.regions.values():
                if r["kind"] in ("gemm", "measured") and r.get("cap_l2"):
                    total += 1
                    n += Q._exempt(ref.val[r["idx"]], ref.S[r["idx"]])
    print("%d of %d tensors are exempt from the relative cap" % (n, total))
    _record("exempt_from_rel_l2", {"tensors": n, "of": total})
    assert n == EXEMPT_RECORDED


def test_every_listed_branch_has_a_case():
    seen = {br for cs in _TABLE.values() for case in cs for br in case.branches} | {"pair:refusals"}
    assert seen == set(_BRANCHES), sorted(set(_BRANCHES) ^ seen)
    assert any(br == "pair:refusals" for _, br, _ in _REFUSALS)
    called = {c["ep"] for cs in _TABLE.values() for case in cs for c in case.built()[1]} - {"same", "kantts_ln128_fwd"}
    assert called == set(_ENTRY_POINTS), sorted(set(_ENTRY_POINTS) ^ called)
    emulated = {c["ep"] for cs in _TABLE.values() for case in cs if case.emu for c in case.built()[1]} - {"same", "kantts_ln128_fwd"}
    assert emulated == set(_ENTRY_POINTS) - {"kantts_bgemm_nt_pair"}
    _record("branches", sorted(seen))


def test_the_table_names_all_32_weight_gradient_variants():
    """4 tiles x (1-D XCD-aware grid, 3-D grid) x the four a_f32 / b_f32 forms = the 16 instantiations of bgemm_tn_kernel on both
    grids; a case counts for the 1-D grid only when the launcher's rule keeps it there"""
    seen = {br for cs in (_TABLE["tn"], _TABLE["tn_grouped"]) for case in cs for br in case.branches if br in _TN_VARIANTS}
    assert len(_TN_VARIANTS) == 32 and seen == set(_TN_VARIANTS), sorted(set(_TN_VARIANTS) - seen)


# ---------------------------------------------------------------------------------------------------------------------
# 5. refusals: what the header or the entry point's own argument check documents
def _refusals():
    """(name, branch, build): each call returns its code and writes nothing"""
    out = []

    def add(name, build, branch=None):
        out.append((name, branch, build))

    def nt(b, rc=E_UNSUPPORTED, seg=None, opts=("bias", "bias2", "res", "gate32"), **kw):
        g = _nt(b, M=33, N=128, ks=[72, 8], form=(1, 1), opts=opts)
        if seg:
            g["segs"][1].update(seg)
        g.update(kw, rc=rc)
        b.calls.append(g)

    U_, B_ = E_UNSUPPORTED, E_BADARG
    for name, rc, kw in (("args NULL", B_, dict(args_null=True)), ("nseg 0", B_, dict(nseg=0)), ("nseg 13", B_, dict(nseg=MAX_SEG + 1)), ("M < 0", B_, dict(M=-1)),
                         ("N < 0", B_, dict(N=-8)), ("c NULL", B_, dict(c=None)), ("N % 8", U_, dict(N=124)), ("ldc % 8", U_, dict(ldc=132)),
                         ("c + 8 bytes", U_, dict(byte_shift={"c": 8})), ("ldr % 4", U_, dict(ldr=134)), ("res + 4 bytes", U_, dict(byte_shift={"res": 4})),
                         ("ldg % 8", U_, dict(ldg=132)), ("gate + 8 bytes", U_, dict(byte_shift={"gate": 8})), ("bias + 4 bytes", U_, dict(byte_shift={"bias": 4})),
                         ("bias2 + 8 bytes", U_, dict(byte_shift={"bias2": 8})), ("a_shift without T", B_, dict(seg=dict(a_shift=1))),
                         ("a NULL", U_, dict(seg=dict(a=None))), ("b NULL", U_, dict(seg=dict(b=None))), ("klen 0", U_, dict(seg=dict(klen=0))),
                         ("klen % 8", U_, dict(seg=dict(klen=12))), ("lda % 8", U_, dict(seg=dict(lda=20))), ("ldb % 8", U_, dict(seg=dict(ldb=132))),
                         ("a + 8 bytes", U_, dict(byte_shift={"a1": 8})), ("b + 8 bytes", U_, dict(byte_shift={"b0": 8}))):
        add("bgemm_nt " + name, lambda b, rc=rc, kw=kw: nt(b, rc=rc, **kw))
    for k in ("ln_gamma", "ln_beta", "ln_mean", "ln_rstd"):
        add("bgemm_nt ln_out without %s" % k, lambda b, k=k: nt(b, rc=B_, opts=("ln32",), **{k: None}))
    for name, kw in (("c_bf16", dict(c_bf16=1)), ("ln_out + 8 bytes", dict(byte_shift={"ln_out": 8})), ("ln_gamma + 4 bytes", dict(byte_shift={"ln_gamma": 4})),
                     ("ln_beta + 4 bytes", dict(byte_shift={"ln_beta": 4}))):
        add("bgemm_nt ln_out with %s" % name, lambda b, kw=kw: nt(b, opts=("ln32",), **kw))

    def ln_n(b):  # ln_out with N != 128
        g = _nt(b, M=33, N=136, ks=[8], form=(0, 0))
        l = _nt(b, M=33, N=128, ks=[8], form=(0, 0), opts=("ln32",))
        b.calls.append(dict(g, rc=U_, **{k: l[k] for k in ("ln_gamma", "ln_beta", "ln_out", "ln_mean", "ln_rstd", "ln_eps")}))
    add("bgemm_nt ln_out with N = 136", ln_n)

    def pair(b, rc=U_, first=None, **kw):
        p0, p1 = _nt(b, M=33, N=128, ks=[8], form=(0, 0)), _nt(b, M=33, N=128, ks=[16], form=(0, 0))
        if first:
            p0.update(first)
        p1.update(kw)
        b.call("kantts_bgemm_nt_pair", rc=rc, probs=[p0, p1])

    def pair_other(b, **kw):
        b.call("kantts_bgemm_nt_pair", rc=U_, probs=[_nt(b, M=33, N=128, ks=[8], form=(0, 0)), _nt(b, ks=[8], **kw)])
    add("bgemm_nt_pair M differs", lambda b: pair_other(b, M=34, N=128, form=(0, 0)), "pair:refusals")
    add("bgemm_nt_pair N differs", lambda b: pair_other(b, M=33, N=136, form=(0, 0)), "pair:refusals")
    add("bgemm_nt_pair a_f32 differs", lambda b: pair_other(b, M=33, N=128, form=(1, 0)), "pair:refusals")
    add("bgemm_nt_pair b_kn differs", lambda b: pair_other(b, M=33, N=128, form=(0, 1)), "pair:refusals")
    add("bgemm_nt_pair second: ldc % 8", lambda b: pair(b, ldc=132), "pair:refusals")
    add("bgemm_nt_pair first: c NULL", lambda b: pair(b, rc=B_, first=dict(c=None)), "pair:refusals")
    add("bgemm_nt_pair second: nseg 0", lambda b: pair(b, rc=B_, nseg=0), "pair:refusals")

    def lnb(b, rc=U_, ln=None, seg=None, **kw):
        g, _ = _lnb(b, 33, 1, "f32", 0, True, "some", False, opts=("bias", "bias2", "res"))
        b.calls.pop()
        b.calls.pop()  # (mean / rstd stay the arena's noise: nothing is computed)
        if seg:
            g["segs"][1].update(seg)
        g["ln"] = dict(g["ln"], **(ln or {}))
        g.update(kw, rc=rc)
        b.calls.append(g)

    for name, rc, kw in (("args NULL", B_, dict(args_null=True)), ("ln NULL", B_, dict(ln_null=True)), ("nseg 0", B_, dict(nseg=0)), ("nseg 13", B_, dict(nseg=13)),
                         ("M < 0", B_, dict(M=-1)), ("N = 136", U_, dict(N=136)), ("b_kn = 0", U_, dict(b_kn=0)), ("relu", U_, dict(relu=1)),
                         ("drop_p", U_, dict(drop_p=0.5)), ("ldc % 8", U_, dict(ldc=132)), ("c + 8 bytes", U_, dict(byte_shift={"c": 8})), ("ldr % 4", U_, dict(ldr=134)),
                         ("res + 4 bytes", U_, dict(byte_shift={"res": 4})), ("bias + 4 bytes", U_, dict(byte_shift={"bias": 4})),
                         ("bias2 + 4 bytes", U_, dict(byte_shift={"bias2": 4})), ("x + 4 bytes", U_, dict(byte_shift={"ln.x": 4})),
                         ("gamma + 4 bytes", U_, dict(byte_shift={"ln.gamma": 4})), ("dx + 4 bytes", U_, dict(byte_shift={"ln.dx": 4})),
                         ("dres + 4 bytes", U_, dict(byte_shift={"ln.dres": 4})), ("a_shift without T", B_, dict(seg=dict(a_shift=-1))),
                         ("a NULL", U_, dict(seg=dict(a=None))), ("klen % 8", U_, dict(seg=dict(klen=4))), ("ldb % 8", U_, dict(seg=dict(ldb=140))),
                         ("b + 8 bytes", U_, dict(byte_shift={"b1": 8}))):
        add("bgemm_nt_lnbwd " + name, lambda b, rc=rc, kw=kw: lnb(b, rc=rc, **kw))
    for k in ("x", "gamma", "mean", "rstd", "dx", "dgamma", "dbeta"):
        add("bgemm_nt_lnbwd %s NULL" % k, lambda b, k=k: lnb(b, rc=B_, ln={k: None}))

    def lnb_with(b, **kw):  # ln_out / gate set
        o = _nt(b, M=33, N=128, ks=[8], form=(0, 1), opts=("ln32", "gate32"))
        lnb(b, **{k: o[k] for k in kw["keys"]})
    add("bgemm_nt_lnbwd ln_out set", lambda b: lnb_with(b, keys=("ln_out", "ln_gamma", "ln_beta", "ln_mean", "ln_rstd")))
    add("bgemm_nt_lnbwd gate set", lambda b: lnb_with(b, keys=("gate", "ldg")))

    def tn(b, rc=U_, grouped=False, prob=None, **kw):
        g = _tn(b, M=65, N=8, K=16, form=(1, 1), T=5, taps=(3, -1, 1), db=True, nprob=2 if grouped else 1, grouped=grouped)
        if prob:
            g["probs"][-1].update(prob)
        g.update(kw, rc=rc)
        b.calls.append(g)

    for grouped in (False, True):
        nm = "bgemm_tn_grouped " if grouped else "bgemm_tn "
        for name, rc, kw in (("args NULL", B_, dict(args_null=True)), ("M < 0", B_, dict(M=-1)), ("N < 1", B_, dict(N=0)), ("K < 1", B_, dict(K=0)),
                             ("ntaps < 1", B_, dict(ntaps=0)), ("N % 8", U_, dict(N=12)), ("K % 8", U_, dict(K=12)), ("lda % 8", U_, dict(lda=20)),
                             ("ldb % 8", U_, dict(ldb=28)), ("a NULL", B_, dict(prob=dict(a=None))), ("b NULL", B_, dict(prob=dict(b=None))),
                             ("c NULL", B_, dict(prob=dict(c=None))), ("a + 8 bytes", U_, dict(byte_shift={"a": 8})), ("b + 4 bytes", U_, dict(byte_shift={"b": 4})),
                             ("taps without T", B_, dict(T=0))):
            add(nm + name, lambda b, rc=rc, kw=kw, grouped=grouped: tn(b, rc=rc, grouped=grouped, **kw))
    for name, kw in (("nprob 0", dict(nprob=0)), ("nprob 17", dict(nprob=TN_MAX_GROUP + 1)), ("a_host NULL", dict(null_arrays=("a",))),
                     ("b_host NULL", dict(null_arrays=("b",))), ("c_host NULL", dict(null_arrays=("c",)))):
        add("bgemm_tn_grouped " + name, lambda b, kw=kw: tn(b, rc=B_, grouped=True, **kw))

    def flat(b, ep, **kw):
        n = 16
        c = dict(src=b.f32(b.randn(n)), dst=b.hout(n), n=n, dy=b.f32(b.randn(n)), dy_bf16=0, y=b.f32(b.randn(n)), y_bf16=0, scale=1.5, gate=b.f32(b.randn(n)),
                 gate_bf16=0, act=1, slope=0.1)
        c.update(kw)
        b.call(ep, rc=B_, **c)

    for ep, ptrs in (("kantts_cast_f32_bf16", ("src", "dst")), ("kantts_relu_gate_bf16", ("dy", "y", "dst")), ("kantts_act_cast_bf16", ("src", "dst"))):
        for k in ptrs:
            add("%s %s NULL" % (ep[7:], k), lambda b, ep=ep, k=k: flat(b, ep, **{k: None}))
        for k in ptrs + (("gate",) if "act" in ep else ()):
            add("%s %s + 8 bytes" % (ep[7:], k), lambda b, ep=ep, k=k: flat(b, ep, byte_shift={k: 8}))
        add("%s n < 0" % ep[7:], lambda b, ep=ep: flat(b, ep, n=-8))
        add("%s n %% 8" % ep[7:], lambda b, ep=ep: flat(b, ep, n=12))

    def table(b, ep, **kw):
        c = dict(src=b.f32(b.randn(1024)), dst=b.hout(1024), table=b.raw(bytes(64)), descs=[], ndesc=1, blocks=1)
        c.update(kw)
        b.call(ep, rc=B_, **c)

    for ep in ("kantts_tapmajor_bf16", "kantts_fragmajor_bf16"):
        for k in ("src", "dst", "table"):
            add("%s %s NULL" % (ep[7:], k), lambda b, ep=ep, k=k: table(b, ep, **{k: None}))
        add("%s ndesc < 0" % ep[7:], lambda b, ep=ep: table(b, ep, ndesc=-1))
        add("%s blocks_per_desc < 1" % ep[7:], lambda b, ep=ep: table(b, ep, blocks=0))

    def rowsum(b, null=None, **kw):
        n = kw.pop("slots", 2)
        c = dict(n=2, cols=8, split=4, rows=[3] * n, src=[b.f32(b.randn(24)) for _ in range(n)], dst0=[b.f32(b.randn(4)) for _ in range(n)],
                 dst1=[b.f32(b.randn(4)) for _ in range(n)])
        c.update(kw)
        if null:
            c[null] = [c[null][0], None]
        b.call("kantts_rows_sum_many", rc=B_, **c)

    for name, kw in (("args NULL", dict(args_null=True)), ("n < 0", dict(n=-1)), ("n = 33", dict(n=ROWSUM_MAX + 1, slots=ROWSUM_MAX)), ("cols < 0", dict(cols=-1)),
                     ("split < 0", dict(split=-1)), ("split > cols", dict(split=9)), ("src NULL", dict(null="src")), ("rows < 0", dict(rows=[3, -1])),
                     ("dst0 NULL with split > 0", dict(null="dst0")), ("dst1 NULL with split < cols", dict(null="dst1"))):
        add("rows_sum_many " + name, lambda b, kw=kw: rowsum(b, **kw))
    return out


_REFUSALS = _refusals()


@pytest.mark.parametrize("leg", _leg_params(emu=False))
def test_refusals(leg):
    """each returns its code and leaves every byte of the arena as it was (the emulated ABI has no argument checks); a
    misaligned pointer is turned away by the host before any launch"""
    import kantts._hip as hip

    leg = _Leg(leg)
    with leg.context():
        assert hip.lib().kantts_launch_tuning(0, -1, 0) == E_BADARG and hip.lib().kantts_launch_tuning(0, 0, -1) == E_BADARG
        for name, _, build in _REFUSALS:
            b = _Builder(name)
            build(b)
            raw = b.finish()
            m = _Mem(raw, leg)
            for c in b.calls:
                rc = _invoke(hip.lib(), m, c)
                assert rc == c["rc"], "%s: returned %d, expected %d" % (name, rc, c["rc"])
            assert np.array_equal(m.result().view(np.uint32), raw.view(np.uint32)), "%s: a refused call wrote" % name
