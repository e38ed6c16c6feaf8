"""What a SAM-BERT step runs between its contractions -- LayerNorm (generic and the 128-wide form), the FSMN memory block, the
embedding gather-sum and the length regulator -- against an fp64 interpreter of their contract (include/kantts_hip.h).

The form is that of tests/test_step_tail_contract.py, whose arena, builder and leg machinery are imported.  ``_evaluate`` (the
``_op_*`` functions) is written from the header comments of the 17 entry points alone -- not from oracle/cabi_numpy.py, not
from the kernels -- and addresses ONE flat arena as the ABI does: element offsets, ``ldo`` with ``out_col_offset``, ``ldm``,
``(b*T + t)*C + c``.  The arena carries guard elements before the first block and after every block; int64, int32, uint8 and
bf16 data live in the same arena; every block starts 16-byte aligned (kantts_ln128_* and kantts_lr_memory_* use 16-byte
accesses and are never handed anything else -- the misaligned pointer of the refusal list is turned away by the host before
any launch).  One table of cases (``_TABLE``) runs through the C ABI on three legs: the emulated ABI (which has no
kantts_lr_memory_*, no _rows and no _slots), the kernel sources on the CPU, and the device.  Every case names the branches
it is there for (``_BRANCHES``); a module-level test asserts that each branch has a case.

Exactly, on every leg:
  * every element no call of the case writes keeps its bits (guards, inputs, the neighbouring columns of a gather with
    ldo > C, a workspace behind ws_floats); return codes;
  * every output of kantts_lr_index (reps = trunc(f32(dur) + f32(0.5)): 0.49999997 gives 1 repetition);
  * kantts_lr_gather_fwd (a copy); kantts_lr_memory_fwd: float32(float64(a) + float64(b));
  * rows of kantts_fsmn_dwconv_fwd_rows equal the same rows of the whole call bit for bit and are finite although every x row
    at or after t1 + (K - 1 - left_pad) holds NaN; rows [c0, c1) of kantts_fsmn_dwconv_fwd_slots equal the _rows call;
  * rows zeroed by zero_rows; masked rows of y, dx and the gathers: 0, or exactly res (rows at or after lens[b] hold 1e30);
  * a dy of zeros leaves dgamma and dbeta with their prior bits;
  * exact sums: with operands from {+-0.5, +-1} and scale a power of two every partial sum in any order is representable
    (the interpreter asserts that the sum of absolute values stays below 2^24 units), so FSMN y / dx / dw, the embedding
    output and table gradients, kantts_lr_gather_bwd, kantts_lr_memory_bwd and LayerNorm's dbeta equal the fp64 value bit
    for bit.  This class carries the seam sizes: a dropped, doubled or mis-masked tap or row moves the result by >= 1 unit.
Measured, per element, for real-valued cases: |got - ref| <= R * c * 2^-24 * S, S = the interpreter's expression over absolute
values.  LayerNorm carries the uncertainty of its statistics to first order: S_mean = mean|x|, S_d = |x| + S_mean,
S_var = mean(d^2) + mean(2 |d| S_d), S_rstd = rstd + rstd^3 S_var / 2, S_y = |d rstd g| + |b| + |rstd g| S_d + |d g| S_rstd;
backward (mean / rstd as the forward call of the same case left them): S_xh = rstd (|x| + |mean| + S_mean) + |d| S_rstd,
S_dx = rstd (|g| + mean|g| + S_xh |s2| + |xh| mean(|g| S_xh)) + |g - s1 - xh s2| S_rstd (+ |dres|), S_dgamma = |prior| +
sum |dy| S_xh.  R = 1 on the emulated ABI and the kernel sources, 2 on the device.  c is not chosen: the interpreter is
evaluated again in numpy float32 with every sum strictly left-to-right and right-to-left; ``ratio`` is its largest distance
from the float64 evaluation in units of 2^-24 * S over the table and c = 4 * ratio (tree-shaped sums, FMA contraction, the
device's sqrtf and division); the test measures it again in every session, uses what it measures and refuses a ratio more
than 10 % above the recorded one.  A bf16 output must be the round-to-nearest-even bf16 of some float within the bound of
the reference.
The project's caps (tests/test_gpu_ops.py) hold as well: LayerNorm y and FSMN y 2e-5 absolute, gradients 1e-4 in relative L2
per tensor.  Exempt from the relative cap are tensors whose reference is exact cancellation, ||ref|| <= 1e-9 ||S||
(EXEMPT_RECORDED of the table's gradient tensors, named below); no tensor lies between 1e-9 and 1e-3.
The measured ratio, c and the worst ratio to the bound per leg and entry point go to seq_contract.json beside
gemm_contract.json.

Measured when this file was written: ratio = 8.644 (the mean of a 1024-wide LayerNorm row, ln_bwd_M17_C1024), c = 34.58;
1 of the table's 233 gradient tensors is exempt from the relative cap (the dx of ln128_bwd_zero_dy_bf16: dy = 0, no dres).
Worst error on the device in units of c * 2^-24 * S (the bound there is R = 2), per entry point: layernorm_fwd 0.056,
layernorm_bwd 0.068, ln128_fwd 0.038, ln128_bwd 0.033, ln128_bwd_rows 0.031, fsmn_dwconv_fwd 0.132, fsmn_dwconv_bwd 0.133,
fsmn_dwconv_fwd_rows 0.097, fsmn_dwconv_fwd_slots 0.089, embed_sum_fwd 0.080, embed_sum_bwd 0.067, lr_gather_bwd 0.064,
lr_memory_bwd 0.052 (lr_index, lr_gather_fwd and lr_memory_fwd are exact).
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import test_step_tail_contract as T
from test_step_tail_contract import E_BADARG, E_WORKSPACE, F32, F64, OK, U, _bf16_rne, _Leg

_REPORT = os.path.join(os.path.dirname(T._REPORT), "seq_contract.json")
E_UNSUPPORTED = -2
CAP_Y, CAP_GRAD_L2 = 2e-5, 1e-4  # tests/test_gpu_ops.py
RATIO_RECORDED = 8.644            # the float32 evaluation of the reference, see above
EXEMPT_RECORDED = 1
LN_EPS = 1e-6
BIG = 1e30                       # what rows at or after lens[b] hold
_FS_KS, _FS_CS = (1, 2, 3, 11, 40, 42, 41), (1, 63, 64, 65, 128, 129, 256, 300)
_FS_TS = (1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 161)
_V31, _V32 = 2 ** 31, 2 ** 32 + 3

_BRANCHES = [
    *["ln:C=%d" % c for c in (1, 63, 64, 65, 80, 257, 512, 1000, 1024)], *["ln:M=%d" % m for m in (1, 3, 4, 5)],
    "ln:constant-row", "ln:C=1025-unsupported",
    *["lnb:M=%d" % m for m in (1, 15, 16, 17, 33, 4097)], *["lnb:C=%d" % c for c in (80, 256, 257, 1024)], "lnb:accumulate",
    *["ln128:M=%d" % m for m in (1, 15, 16, 17, 40)], "ln128:y_bf16=0", "ln128:y_bf16=1", "ln128:constant-row",
    *["ln128b:M=%d" % m for m in (1, 17, 2048, 2049, 4100)], "ln128b:dy_bf16=0", "ln128b:dy_bf16=1", "ln128b:dres=NULL",
    "ln128b:dres", "ln128b:zero_rows=NULL", "ln128b:zero_rows-some", "ln128b:zero_rows-all", "ln128b:dy=0", "ln128b:bwd",
    "ln128b:bwd_rows",
    *["fsmn:K=%d" % k for k in _FS_KS], "fsmn:lp=0", "fsmn:lp=(K-1)/2", "fsmn:lp=K-1", *["fsmn:C=%d" % c for c in _FS_CS],
    *["fsmn:T=%d" % t for t in _FS_TS], "fsmn:lens=NULL", "fsmn:len=0", "fsmn:len=1", "fsmn:len<lp", "fsmn:len=T-1",
    "fsmn:len=T", "fsmn:len=T+2", "fsmn:res=NULL", "fsmn:res", "fsmn:dx-only", "fsmn:dw-only", "fsmn:dw-accumulate",
    "fsmn:xcd-81-blocks", "fsmn:reduce-34-rows", "fsmn:ws-short", "fsmn:ws-size", "fsmn:masked-rows-1e30",
    "rows:K=3", "rows:K=41", "rows:(0,T)", "rows:(5,5)", "rows:(7,8)", "rows:(16,33)", "rows:(T-1,T)", "rows:nan-tail",
    "rows:==whole",
    "slots:t0<0", "slots:t1<t0", "slots:t1>T", "slots:t1-t0>max_rows", *["slots:max_rows=%s" % m for m in (0, 1, 16, 17, "T+5")],
    "slots:==rows",
    *["emb:ntab=%d" % n for n in (1, 2, 3, 4)], *["emb:D=%d" % d for d in (1, 3, 64, 257)],
    *["emb:rows=%d" % r for r in (1, 31, 32, 33, 70)], "emb:rows>T", "emb:pos=NULL", "emb:scaled=NULL",
    "embb:eviction", "embb:all-ids-equal", "embb:rows%8", "embb:table=NULL", "embb:accumulate",
    *["lri:N=%d" % n for n in (1, 63, 64, 65, 130)], "lri:zero-between", "lri:all-zero", "lri:total<Tp", "lri:total=Tp",
    "lri:total>Tp", "lri:float-0.49999997", "lri:float-0.5", "lri:float-1.5", "lri:float-2.4999998",
    "lrg:ldo>C", "lrg:valid=NULL", "lrg:valid=0", "lrg:valid<total", "lrg:valid>Tp", "lrg:valid=2^31", "lrg:valid=2^32+3",
    "lrg:accumulate=0", "lrg:accumulate=1", "lrg:token-without-frame",
    "lrm:r=1", "lrm:r=3", "lrm:widths", "lrm:ldm>width", "lrm:lr_text", "lrm:lr_text=NULL", "lrm:lr_spk", "lrm:lr_spk=NULL",
    "lrm:lr_emo", "lrm:lr_emo=NULL", "lrm:valid=NULL", "lrm:valid=0", "lrm:valid<total", "lrm:valid>Tp", "lrm:valid=2^31",
    "lrm:valid=2^32+3", "lrm:refusals",
]


def a64(x):
    return np.abs(np.asarray(x, dtype=F64))


def ar(n):
    return np.arange(int(n), dtype=np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the arena and the case builder (test_step_tail_contract's, with the integer and bf16 blocks of these entry points)
class _Builder(T._Builder):
    def i32(self, vals):
        return self.raw(np.ascontiguousarray(vals, dtype=np.int32).tobytes())

    def u8(self, vals):
        return self.raw(np.ascontiguousarray(vals, dtype=np.uint8).tobytes())

    def bf16(self, vals):
        """a bf16 image of ``vals``; returns the offset in bf16 elements"""
        return 2 * self.raw(_bf16_rne(np.ascontiguousarray(vals, dtype=F32).reshape(-1)).tobytes())

    def lens(self, vals):
        return None if vals is None else self.i64(vals)


class _Case:
    def __init__(self, name, branches, build, emu=True):
        unknown = set(branches) - set(_BRANCHES)
        assert not unknown, (name, unknown)
        self.name, self.branches, self._build, self.emu = name, tuple(branches), build, emu
        self._built = self._ref = None

    def built(self):
        if self._built is None:
            b = _Builder(self.name)
            self._build(b)
            self._built = (b.finish(), b.calls)
        return self._built

    def reference(self):
        """the float64 evaluation, computed once and shared by every leg"""
        if self._ref is None:
            self._ref = _evaluate(self, F64)
        return self._ref


# ---------------------------------------------------------------------------------------------------------------------
# 2. the interpreter
class _Shadow(T._Shadow):
    """``val`` / ``S``: what the calls so far have written (inputs: the bytes the calls find); ``unc``: the S of LayerNorm
    statistics an earlier call of the case wrote (0 for statistics that are inputs); ``i32``: the arena as int32 words"""

    def __init__(self, raw, dt, rev):
        super().__init__(raw, dt, rev)
        self.i32 = raw.view(np.int32).copy()
        self.unc = np.zeros(raw.size)

    def cur(self, idx):
        return self.val[np.asarray(idx, dtype=np.int64)]

    def acc(self, idx, val, S):
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        self.put(idx, self.val[idx] + np.asarray(val, dtype=self.dt).reshape(-1), self.S[idx] + np.asarray(S, F64).reshape(-1))

    def bf16_in(self, off, n):
        u = self.raw.view(np.uint16)[off + ar(n)].astype(np.uint32) << 16
        return u.view(F32).astype(self.dt)

    def sum0(self, x):
        """sum over the first axis"""
        return self.sum(np.moveaxis(x, 0, -1))


def _ln_fwd(sh, c, C):
    """header: eps inside the sqrt, biased variance; mean, rstd (M) saved for backward"""
    if c["rc"] != OK or c["M"] == 0:
        return
    dt, M, ep = sh.dt, c["M"], c["ep"]
    x = sh.f(c["x"] + ar(M * C)).reshape(M, C)
    gam, bet = sh.f(c["gamma"] + ar(C)), sh.f(c["beta"] + ar(C))
    mu = sh.sum(x) / dt(C)
    d = x - mu[:, None]
    var = sh.sum(d * d) / dt(C)
    rs = dt(1) / np.sqrt(var + dt(F32(c["eps"])))
    y = d * rs[:, None] * gam + bet
    S_mu = a64(x).mean(1)
    S_d = a64(x) + S_mu[:, None]
    S_var = (a64(d) ** 2).mean(1) + (2 * a64(d) * S_d).mean(1)
    S_rs = a64(rs) + 0.5 * a64(rs) ** 3 * S_var
    S_y = a64(d * rs[:, None] * gam) + a64(bet) + a64(rs[:, None] * gam) * S_d + a64(d * gam) * S_rs[:, None]
    for k, v, S in (("mean", mu, S_mu), ("rstd", rs, S_rs)):
        i = c[k] + ar(M)
        sh.put(i, v, S)
        sh.unc[i] = S
        sh.region("%s@%d" % (k, c[k]), ep, "measured", i)
    if c.get("y_bf16"):
        sh.region("y(bf16)@%d" % c["y"], ep, "bf16", None, u16=c["y"] + ar(M * C), want=y.reshape(-1), S=S_y.reshape(-1))
    else:
        sh.put(c["y"] + ar(M * C), y, S_y)
        sh.region("y@%d" % c["y"], ep, "measured", c["y"] + ar(M * C), cap_abs=CAP_Y)


def _ln_bwd(sh, c, C):
    """the gradient of the forward expression at the saved statistics; dgamma / dbeta are ACCUMULATED; dres: dx = LN-gradient
    + dres; zero_rows: rows of dx written as 0"""
    if c["rc"] != OK or c["M"] == 0:
        return
    dt, M, ep = sh.dt, c["M"], c["ep"]
    x = sh.f(c["x"] + ar(M * C)).reshape(M, C)
    gam = sh.f(c["gamma"] + ar(C))
    dy = (sh.bf16_in(c["dy"], M * C) if c.get("dy_bf16") else sh.f(c["dy"] + ar(M * C))).reshape(M, C)
    i_mu, i_rs = c["mean"] + ar(M), c["rstd"] + ar(M)
    mu, rs, U_mu, U_rs = sh.cur(i_mu)[:, None], sh.cur(i_rs)[:, None], sh.unc[i_mu][:, None], sh.unc[i_rs][:, None]
    d = x - mu
    xh = d * rs
    S_xh = a64(rs) * (a64(x) + a64(mu) + U_mu) + a64(d) * U_rs
    g = dy * gam
    s1, s2 = (sh.sum(g) / dt(C))[:, None], (sh.sum(g * xh) / dt(C))[:, None]
    S_s1, S_s2 = a64(g).mean(1)[:, None], (a64(g) * S_xh).mean(1)[:, None]
    inner = g - s1 - xh * s2
    dx = rs * inner
    S_dx = a64(rs) * (a64(g) + S_s1 + S_xh * a64(s2) + a64(xh) * S_s2) + a64(inner) * U_rs
    if c.get("dres") is not None:
        dres = sh.f(c["dres"] + ar(M * C)).reshape(M, C)
        dx, S_dx = dx + dres, S_dx + a64(dres)
    zr = np.zeros(M, dtype=bool)
    if c.get("zero_rows") is not None:
        zr = sh.raw.view(np.uint8)[4 * c["zero_rows"] + ar(M)] != 0
    dx, S_dx = np.where(zr[:, None], dt(0), dx), np.where(zr[:, None], 0.0, S_dx)
    i_dx = (c["dx"] + ar(M * C)).reshape(M, C)
    sh.put(i_dx, dx, S_dx)
    if zr.any():
        sh.region("dx zeroed rows@%d" % c["dx"], ep, "exact", i_dx[zr])
    if (~zr).any():
        sh.region("dx@%d" % c["dx"], ep, "measured", i_dx[~zr], cap_l2=True)
    zero_dy = not dy.any()
    i_g, i_b = c["dgamma"] + ar(C), c["dbeta"] + ar(C)
    sh.acc(i_g, sh.sum0(dy * xh), (a64(dy) * S_xh).sum(0))
    sh.acc(i_b, sh.sum0(dy), a64(dy).sum(0))
    sh.region("dgamma@%d" % c["dgamma"], ep, "exact" if zero_dy else "measured", i_g, cap_l2=True)
    if zero_dy or c.get("exact"):
        sh.region("dbeta@%d" % c["dbeta"], ep, "exact", i_b, unit=None if zero_dy else 0.5)
    else:
        sh.region("dbeta@%d" % c["dbeta"], ep, "measured", i_b, cap_l2=True)


def _lens_of(sh, c, key="lens"):
    return None if c[key] is None else sh.ints(c[key], c["B"])


def _fir_terms(sh, c, src, flip, xlimit=None):
    """the terms of keep * (sum_k w[c,k] * xm[t + k - left_pad] + xm[t]), xm = src * keep (flip: t - k + left_pad): (B, T, C, K + 1)
    and keep (B, T).  Rows at or after ``xlimit`` are not read (kantts_fsmn_dwconv_fwd_rows)."""
    dt, (B, Tt, C, K, lp) = sh.dt, (c["B"], c["T"], c["C"], c["K"], c["left_pad"])
    lens = _lens_of(sh, c)
    keep = np.ones((B, Tt), dtype=bool) if lens is None else ar(Tt)[None, :] < lens[:, None]
    read = keep if xlimit is None else keep & (ar(Tt)[None, :] < xlimit)
    x = np.where(read[:, :, None], sh.raw[src + ar(B * Tt * C)].reshape(B, Tt, C), F32(0)).astype(dt)
    w = sh.f(c["w"] + ar(C * K)).reshape(C, K)
    front = (K - 1 - lp) if flip else lp
    pad = np.zeros((B, Tt + K - 1, C), dtype=dt)
    pad[:, front:front + Tt] = x
    terms = np.empty((B, Tt, C, K + 1), dtype=dt)
    for k in range(K):
        kk = (K - 1 - k) if flip else k
        terms[..., k] = w[:, k] * pad[:, kk:kk + Tt]
    terms[..., K] = x
    return np.where(keep[:, :, None, None], terms, dt(0)), keep, x


def _fsmn_out(sh, c, terms, keep, dst, what, res=None, rows=None, exact_kind="exact"):
    """store sum(terms) (+ res) at ``dst`` for the (b, t) of ``rows`` (a (B, T) mask; None: all): masked rows are exact (0 or res)"""
    B, Tt, C = c["B"], c["T"], c["C"]
    val, S = sh.sum(terms), a64(terms).sum(-1)
    if res is not None:
        r = sh.f(res + ar(B * Tt * C)).reshape(B, Tt, C)
        val, S = val + r, S + a64(r)
    idx = (dst + ar(B * Tt * C)).reshape(B, Tt, C)
    rows = np.ones((B, Tt), dtype=bool) if rows is None else rows
    sh.put(idx[rows], val[rows], S[rows])
    if c.get("exact"):
        sh.region(what, c["ep"], "exact", idx[rows], unit=0.25)
        return
    if (rows & ~keep).any():
        sh.region(what + " masked rows", c["ep"], "exact", idx[rows & ~keep])
    if (rows & keep).any():
        sh.region(what, c["ep"], "measured", idx[rows & keep], **({"cap_abs": CAP_Y} if what[0] == "y" else {"cap_l2": True}))


def _op_fsmn_fwd(sh, c):
    """header: xm = x*keep; y = keep*(sum_k w[c,k]*xm[t+k-left_pad] + xm[t]) (+ res); keep[b,t] = t < lens[b].  _rows: rows
    [t0, t1) only, reading no x row at or after t1 + (K - 1 - left_pad).  _slots: c0 = clamp(t0[b], 0, T),
    c1 = min(clamp(t1[b], c0, T), c0 + max_rows) per sequence."""
    if c["rc"] != OK or c["B"] == 0 or c["T"] == 0:
        return
    B, Tt, K, lp = c["B"], c["T"], c["K"], c["left_pad"]
    t = ar(Tt)[None, :]
    if c["ep"] == "kantts_fsmn_dwconv_fwd":
        terms, keep, _ = _fir_terms(sh, c, c["x"], False)
        rows = None
    elif c["ep"] == "kantts_fsmn_dwconv_fwd_rows":
        if c["t0"] == c["t1"]:
            return
        terms, keep, _ = _fir_terms(sh, c, c["x"], False, xlimit=c["t1"] + (K - 1 - lp))
        rows = np.broadcast_to((t >= c["t0"]) & (t < c["t1"]), (B, Tt))
    else:
        terms, keep, _ = _fir_terms(sh, c, c["x"], False)
        c0 = np.clip(sh.i32[c["t0"] + ar(B)].astype(np.int64), 0, Tt)
        c1 = np.minimum(np.clip(sh.i32[c["t1"] + ar(B)].astype(np.int64), c0, Tt), c0 + c["max_rows"])
        rows = (t >= c0[:, None]) & (t < c1[:, None])
    if rows is None or rows.any():
        _fsmn_out(sh, c, terms, keep, c["y"], "y@%d" % c["y"], res=c["res"], rows=rows)


def _op_fsmn_bwd(sh, c):
    """the gradients of the forward expression: dx = keep*(sum_k w[c,k]*dyk[t-k+left_pad] + dyk[t]), dyk = dy*keep;
    dw_accum[c,k] += sum_{b,t} dyk[b,t,c] * xm[b,t+k-left_pad,c]; either may be NULL"""
    if c["rc"] != OK or c["B"] == 0 or c["T"] == 0:
        return
    dt, (B, Tt, C, K, lp) = sh.dt, (c["B"], c["T"], c["C"], c["K"], c["left_pad"])
    if c["dx"] is not None:
        terms, keep, _ = _fir_terms(sh, c, c["dy"], True)
        _fsmn_out(sh, c, terms, keep, c["dx"], "dx@%d" % c["dx"])
    if c["dw"] is not None:
        _, keep, xm = _fir_terms(sh, c, c["x"], False)
        dyk = np.where(keep[:, :, None], sh.raw[c["dy"] + ar(B * Tt * C)].reshape(B, Tt, C), F32(0)).astype(dt)
        pad = np.zeros((B, Tt + K - 1, C), dtype=dt)
        pad[:, lp:lp + Tt] = xm
        prod = np.empty((C, K, B * Tt), dtype=dt)
        for k in range(K):
            prod[:, k, :] = (dyk * pad[:, k:k + Tt]).reshape(B * Tt, C).T
        i_dw = c["dw"] + ar(C * K)
        sh.acc(i_dw, sh.sum(prod), a64(prod).sum(-1))
        if c.get("exact"):
            sh.region("dw@%d" % c["dw"], c["ep"], "exact", i_dw, unit=0.25)
        else:
            sh.region("dw@%d" % c["dw"], c["ep"], "measured", i_dw, cap_l2=True)
        if K == 41 and c["ws_floats"]:
            sh.region("workspace@%d" % c["ws"], c["ep"], "scratch", c["ws"] + ar(c["ws_floats"]))


def _op_embed_fwd(sh, c):
    """header: out[row] = scale * sum_k table_k[ids[row,k]] (+ pos[row % T]); scaled_out: the value before the positional add"""
    if c["rc"] != OK or c["rows"] == 0:
        return
    dt, rows, D, nt = sh.dt, c["rows"], c["D"], len(c["tables"])
    ids = sh.ints(c["ids"], rows * nt).reshape(rows, nt)
    terms = np.stack([sh.f(c["tables"][k] + ids[:, k, None] * D + ar(D)[None, :]) for k in range(nt)], axis=-1)
    scale = dt(F32(c["scale"]))
    v, S = scale * sh.sum(terms), abs(float(scale)) * a64(terms).sum(-1)
    kind = dict(kind="exact", unit=0.5 * abs(float(scale))) if c.get("exact") else dict(kind="measured")
    if c["scaled"] is not None:
        sh.put(c["scaled"] + ar(rows * D), v, S)
        sh.region("scaled@%d" % c["scaled"], c["ep"], idx=c["scaled"] + ar(rows * D), **kind)
    if c["pos"] is not None:
        p = sh.f(c["pos"] + (ar(rows) % c["T"])[:, None] * D + ar(D)[None, :])
        v, S = v + p, S + a64(p)
    sh.put(c["out"] + ar(rows * D), v, S)
    sh.region("out@%d" % c["out"], c["ep"], idx=c["out"] + ar(rows * D), **kind)


def _op_embed_bwd(sh, c):
    """header: scatter-adds scale*dout into dtables (NULL entries skipped)"""
    if c["rc"] != OK or c["rows"] == 0:
        return
    dt, rows, D, nt = sh.dt, c["rows"], c["D"], len(c["tables"])
    ids = sh.ints(c["ids"], rows * nt).reshape(rows, nt)
    g = dt(F32(c["scale"])) * sh.f(c["dout"] + ar(rows * D)).reshape(rows, D)
    order = ar(rows)[::-1] if sh.rev else ar(rows)
    for k, tab in enumerate(c["tables"]):
        if tab is None:
            continue
        nrow = c["nrows"][k]
        idx = tab + ar(nrow * D)
        v, S = sh.cur(idx).reshape(nrow, D), sh.S[idx].reshape(nrow, D)
        np.add.at(v, ids[order, k], g[order])  # (unbuffered: one addition after the other, in this order)
        np.add.at(S, ids[order, k], a64(g[order]))
        sh.put(idx, v, S)
        if c.get("exact"):
            sh.region("dtable[%d]@%d" % (k, tab), c["ep"], "exact", idx, unit=0.5 * abs(float(F32(c["scale"]))))
        else:
            sh.region("dtable[%d]@%d" % (k, tab), c["ep"], "measured", idx, cap_l2=True)


def _op_lr_index(sh, c):
    """header: reps = trunc(dur + 0.5), formed in float32; idx (B,Tp) token per frame or -1; pos 1-based position inside the
    token (t+1 when uncovered); cs (B,N+1) exclusive prefix sums; lens (B) int64 totals"""
    if c["rc"] != OK or c["B"] == 0:
        return
    B, N, Tp, ep = c["B"], c["N"], c["Tp"], c["ep"]
    if c["dur_int"] is not None:
        reps = sh.ints(c["dur_int"], B * N).reshape(B, N)
    else:
        reps = np.trunc(sh.raw[c["dur_float"] + ar(B * N)] + F32(0.5)).astype(np.int64).reshape(B, N)
    cs = np.zeros((B, N + 1), dtype=np.int64)
    cs[:, 1:] = np.cumsum(reps, axis=1)
    idx = np.full((B, Tp), -1, dtype=np.int64)
    pos = np.tile(ar(Tp)[None, :] + 1, (B, 1))
    for b in range(B):
        for n in range(N):
            s, e = int(cs[b, n]), int(min(cs[b, n + 1], Tp))
            if s < e:
                idx[b, s:e] = n
                pos[b, s:e] = ar(e - s) + 1
    for k, v in (("idx", idx), ("cs", cs)):
        i = c[k] + ar(v.size)
        sh.i32[i] = v.reshape(-1)
        sh.region("%s@%d" % (k, c[k]), ep, "i32", i, want=v.reshape(-1).astype(np.int32))
    sh.put(c["pos"] + ar(B * Tp), pos, pos)
    sh.region("pos@%d" % c["pos"], ep, "exact", c["pos"] + ar(B * Tp))
    sh.region("lens@%d" % c["lens"], ep, "i64", c["lens"] + ar(2 * B), want=cs[:, N].copy())


def _live(sh, c):
    """kantts_lr_gather_fwd's rule: a frame is live when idx >= 0 and t < valid_lens[b]"""
    B, Tp = c["B"], c["Tp"]
    idx = sh.i32[c["idx"] + ar(B * Tp)].reshape(B, Tp).astype(np.int64)
    valid = _lens_of(sh, c, "valid")
    live = idx >= 0
    if valid is not None:
        assert (valid >= 0).all()
        live &= ar(Tp)[None, :] < valid[:, None]
    return idx, live


def _gathered(sh, c, src, width, idx, live):
    B, N = c["B"], c["N"]
    x = sh.f(src + ar(B * N * width)).reshape(B, N, width)
    return np.where(live[:, :, None], x[ar(B)[:, None], np.maximum(idx, 0)], sh.dt(0))


def _op_lr_gather_fwd(sh, c):
    """header: out[b,t, off:off+C] = x[b, idx[b,t], :] (0 when idx<0 or t >= valid_lens[b]); out rows have stride ldo"""
    if c["rc"] != OK or c["B"] * c["Tp"] == 0:
        return
    B, Tp, C = c["B"], c["Tp"], c["C"]
    idx, live = _live(sh, c)
    v = _gathered(sh, c, c["x"], C, idx, live)
    o = c["out"] + ar(B * Tp)[:, None] * c["ldo"] + c["off"] + ar(C)[None, :]
    sh.put(o, v, a64(v))
    sh.region("out@%d" % c["out"], c["ep"], "exact", o)


def _segments(sh, c):
    """per (b, n): the frames [cs[n], min(cs[n+1], Tp, valid_lens[b]))"""
    B, N, Tp = c["B"], c["N"], c["Tp"]
    cs = sh.i32[c["cs"] + ar(B * (N + 1))].reshape(B, N + 1).astype(np.int64)
    valid = _lens_of(sh, c, "valid")
    for b in range(B):
        for n in range(N):
            e = min(int(cs[b, n + 1]), Tp)
            if valid is not None:
                e = min(e, int(valid[b]))
            yield b, n, int(cs[b, n]), e


def _grad_kind(c):
    return dict(kind="exact", unit=0.5) if c.get("exact") else dict(kind="measured", cap_l2=True)


def _op_lr_gather_bwd(sh, c):
    """header: deterministic segment sum over [cs[n], cs[n+1]) (clipped to Tp and valid_lens[b]); accumulate: dx +="""
    if c["rc"] != OK or c["B"] == 0:
        return
    B, N, Tp, C = c["B"], c["N"], c["Tp"], c["C"]
    dout = sh.f(c["dout"] + ar(B * Tp)[:, None] * c["ldo"] + c["off"] + ar(C)[None, :]).reshape(B, Tp, C)
    v, S = np.zeros((B, N, C), dtype=sh.dt), np.zeros((B, N, C))
    for b, n, s, e in _segments(sh, c):
        if e > s:
            v[b, n], S[b, n] = sh.sum0(dout[b, s:e]), a64(dout[b, s:e]).sum(0)
    i = c["dx"] + ar(B * N * C)
    if c["accumulate"]:
        sh.acc(i, v, S)
    else:
        sh.put(i, v, S)
    sh.region("dx@%d" % c["dx"], c["ep"], idx=i, **_grad_kind(c))


def _op_lr_memory_fwd(sh, c):
    """header: memory (B, L, r*d_t + d_s + d_e): [b, l, j*d_t + c] = G(aug)[b, l*r + j, c] + pos_enc[b, l*r + j, c];
    [b, l, r*d_t + c] = G(spk)[b, l*r, c]; [b, l, r*d_t + d_s + c] = G(emo)[b, l*r, c]; lr_text / lr_spk / lr_emo: optional
    frame-level G(aug) + pos_enc, G(spk), G(emo)"""
    if c["rc"] != OK or c["B"] * c["Tp"] == 0:
        return
    B, Tp, r, dt_, ds, de, ep = c["B"], c["Tp"], c["r"], c["d_t"], c["d_s"], c["d_e"], c["ep"]
    L, W = Tp // r, r * dt_ + ds + de
    idx, live = _live(sh, c)
    text = _gathered(sh, c, c["aug"], dt_, idx, live) + sh.f(c["pos_enc"] + ar(B * Tp * dt_)).reshape(B, Tp, dt_)
    spk, emo = _gathered(sh, c, c["spk"], ds, idx, live), _gathered(sh, c, c["emo"], de, idx, live)
    row = c["memory"] + ar(B * L)[:, None] * W
    for what, v, cols, kind in (("text", text.reshape(B * L, r * dt_), ar(r * dt_), "round"),
                                ("spk", spk[:, ::r].reshape(B * L, ds), r * dt_ + ar(ds), "exact"),
                                ("emo", emo[:, ::r].reshape(B * L, de), r * dt_ + ds + ar(de), "exact")):
        sh.put(row + cols[None, :], v, a64(v))
        sh.region("memory %s@%d" % (what, c["memory"]), ep, kind, row + cols[None, :])
    for key, v, kind in (("lr_text", text, "round"), ("lr_spk", spk, "exact"), ("lr_emo", emo, "exact")):
        if c[key] is not None:
            sh.put(c[key] + ar(v.size), v, a64(v))
            sh.region("%s@%d" % (key, c[key]), ep, kind, c[key] + ar(v.size))


def _op_lr_memory_bwd(sh, c):
    """header: per token the sum over its frames [cs[n], min(cs[n+1], Tp, valid_lens[b])) in frame order of d_memory (row pitch
    ldm, batch pitch L * ldm); d_spk / d_emo: the frames with t % r == 0.  Every element of the three outputs is written."""
    if c["rc"] != OK or c["B"] == 0:
        return
    B, N, Tp, r, dt_, ds, de, ldm = c["B"], c["N"], c["Tp"], c["r"], c["d_t"], c["d_s"], c["d_e"], c["ldm"]
    L = Tp // r
    dm = sh.f(c["d_memory"] + ar(B * L * ldm)).reshape(B, L, ldm)
    outs = {"d_aug": (np.zeros((B, N, dt_), sh.dt), np.zeros((B, N, dt_))), "d_spk": (np.zeros((B, N, ds), sh.dt), np.zeros((B, N, ds))),
            "d_emo": (np.zeros((B, N, de), sh.dt), np.zeros((B, N, de)))}
    for b, n, s, e in _segments(sh, c):
        if e <= s:
            continue
        t = ar(e - s) + s
        fr = dm[b, t // r][ar(e - s)[:, None], (t % r)[:, None] * dt_ + ar(dt_)[None, :]]
        outs["d_aug"][0][b, n], outs["d_aug"][1][b, n] = sh.sum0(fr), a64(fr).sum(0)
        t = t[t % r == 0]
        if t.size:
            for key, lo, w in (("d_spk", r * dt_, ds), ("d_emo", r * dt_ + ds, de)):
                fr = dm[b, t // r, lo:lo + w]
                outs[key][0][b, n], outs[key][1][b, n] = sh.sum0(fr), a64(fr).sum(0)
    for key, (v, S) in outs.items():
        sh.put(c[key] + ar(v.size), v, S)
        sh.region("%s@%d" % (key, c[key]), c["ep"], idx=c[key] + ar(v.size), **_grad_kind(c))


def _op_check(sh, c):
    """not a call: two element lists that must hold the same bits afterwards (``finite``: and no NaN or infinity)"""
    sh.region("same %s" % c["what"], "-", "same", None, a=np.asarray(c["a"]).reshape(-1), b=np.asarray(c["b"]).reshape(-1),
              finite=c.get("finite", False))


_OPS = {"kantts_layernorm_fwd": lambda sh, c: _ln_fwd(sh, c, c["C"]), "kantts_layernorm_bwd": lambda sh, c: _ln_bwd(sh, c, c["C"]),
        "kantts_ln128_fwd": lambda sh, c: _ln_fwd(sh, c, 128), "kantts_ln128_bwd": lambda sh, c: _ln_bwd(sh, c, 128),
        "kantts_ln128_bwd_rows": lambda sh, c: _ln_bwd(sh, c, 128),
        "kantts_fsmn_dwconv_fwd": _op_fsmn_fwd, "kantts_fsmn_dwconv_fwd_rows": _op_fsmn_fwd, "kantts_fsmn_dwconv_fwd_slots": _op_fsmn_fwd,
        "kantts_fsmn_dwconv_bwd": _op_fsmn_bwd, "kantts_fsmn_dwconv_bwd_ws": lambda sh, c: None,
        "kantts_embed_sum_fwd": _op_embed_fwd, "kantts_embed_sum_bwd": _op_embed_bwd, "kantts_lr_index": _op_lr_index,
        "kantts_lr_gather_fwd": _op_lr_gather_fwd, "kantts_lr_gather_bwd": _op_lr_gather_bwd,
        "kantts_lr_memory_fwd": _op_lr_memory_fwd, "kantts_lr_memory_bwd": _op_lr_memory_bwd, "same": _op_check}
_ENTRY_POINTS = sorted(set(_OPS) - {"same"})
_NOT_EMULATED = {"kantts_lr_memory_fwd", "kantts_lr_memory_bwd", "kantts_fsmn_dwconv_fwd_rows", "kantts_fsmn_dwconv_fwd_slots"}


def _evaluate(case, dt, rev=False):
    raw, calls = case.built()
    sh = _Shadow(raw, dt, rev)
    with np.errstate(all="ignore"):
        for c in calls:
            _OPS[c["ep"]](sh, c)
    if dt is F64:  # the exact class: every partial sum in any order is a whole number of units below 2^24
        for r in sh.regions.values():
            if r["kind"] in ("exact", "round"):
                assert np.isfinite(sh.val[r["idx"]]).all(), (case.name, r["what"])
            if r["kind"] == "exact":
                assert np.array_equal(sh.val[r["idx"]].astype(F32).astype(F64), sh.val[r["idx"]]), (case.name, r["what"])
                if r.get("unit"):
                    units = sh.S[r["idx"]] / r["unit"]
                    assert np.array_equal(units, np.floor(units)) and (units < 2 ** 24).all(), (case.name, r["what"])
    return sh


# ---------------------------------------------------------------------------------------------------------------------
# 3. the case table
def _ln_cases():
    cs = []

    def data(b, M, C, const_row):
        x = b.randn(M * C).reshape(M, C) + F32(0.3)
        if const_row is not None:
            x[const_row] = 0.5  # variance 0; C * 0.5 and its quotient are exact in any order
        return dict(x=b.f32(x), gamma=b.f32(1 + b.randn(C, 0.3)), beta=b.f32(b.randn(C, 0.3)), mean=b.f32(n=M), rstd=b.f32(n=M), M=M)

    for i, C in enumerate((1, 63, 64, 65, 80, 257, 512, 1000, 1024)):
        for M in ((1, 3, 4, 5)[i % 4], (1, 3, 4, 5)[(i + 2) % 4]):
            def build(b, M=M, C=C):
                b.call("kantts_layernorm_fwd", y=b.f32(n=M * C), C=C, eps=LN_EPS, **data(b, M, C, 1 if M >= 3 else None))
            cs.append(_Case("ln_fwd_M%d_C%d" % (M, C), ["ln:C=%d" % C, "ln:M=%d" % M] + (["ln:constant-row"] if M >= 3 or C == 1 else []), build))

    def unsupported(b):
        d = data(b, 2, 1025, None)
        b.call("kantts_layernorm_fwd", rc=E_UNSUPPORTED, y=b.f32(n=2 * 1025), C=1025, eps=LN_EPS, **d)
        b.call("kantts_layernorm_bwd", rc=E_UNSUPPORTED, dy=b.f32(b.randn(2 * 1025)), dx=b.f32(n=2 * 1025), dgamma=b.f32(b.randn(1025)),
               dbeta=b.f32(b.randn(1025)), C=1025, **{k: d[k] for k in ("x", "gamma", "mean", "rstd", "M")})
    cs.append(_Case("ln_C1025", ["ln:C=1025-unsupported"], unsupported, emu=False))

    for M, C in ((1, 80), (15, 256), (16, 257), (17, 1024), (33, 80), (4097, 8), (33, 1024)):
        for exact in (False, True):
            def build(b, M=M, C=C, exact=exact):
                d = data(b, M, C, 1 if M > 1 else None)
                b.call("kantts_layernorm_fwd", y=b.f32(n=M * C), C=C, eps=LN_EPS, **d)
                b.call("kantts_layernorm_bwd", dy=b.f32(b.dyadic(M * C) if exact else b.randn(M * C)), dx=b.f32(n=M * C),
                       dgamma=b.f32(b.randn(C)), dbeta=b.f32(b.dyadic(C) if exact else b.randn(C)), C=C, exact=exact,
                       **{k: d[k] for k in ("x", "gamma", "mean", "rstd", "M")})
            cs.append(_Case("ln_bwd_M%d_C%d%s" % (M, C, "_exact" if exact else ""), ["lnb:M=%d" % M, "lnb:C=%d" % C, "lnb:accumulate"]
                            if C != 8 else ["lnb:M=%d" % M, "lnb:accumulate"], build))
    return cs, data


def _ln128_cases(data):
    cs = []
    for M in (1, 15, 16, 17, 40):
        for bf in (0, 1):
            def build(b, M=M, bf=bf):
                y = b.bf16(np.zeros(M * 128)) if bf else b.f32(n=M * 128)
                b.call("kantts_ln128_fwd", y=y, y_bf16=bf, eps=LN_EPS, **data(b, M, 128, M // 2 if M > 1 else None))
            cs.append(_Case("ln128_fwd_M%d_bf%d" % (M, bf), ["ln128:M=%d" % M, "ln128:y_bf16=%d" % bf] + (["ln128:constant-row"] if M > 1 else []), build))

    def bwd(name, M, bf, dres, zr, rows_ep, zero_dy=False, tag_m=True):
        for exact in (False, True):
            def build(b, exact=exact):
                d = data(b, M, 128, 0 if M > 1 else None)
                b.call("kantts_ln128_fwd", y=b.f32(n=M * 128), y_bf16=0, eps=LN_EPS, **d)
                dy = np.zeros(M * 128, F32) if zero_dy else (b.dyadic(M * 128) if exact else b.randn(M * 128))
                z = None
                if zr is not None:
                    z = np.ones(M, np.uint8) if zr == "all" else (b.rng.integers(0, 3, size=M) == 0).astype(np.uint8) * 7
                    if zr == "some":
                        z[0], z[-1] = 1, 0 if M > 1 else 1
                kw = dict(dy=b.bf16(dy) if bf else b.f32(dy), dy_bf16=bf, dres=b.f32(b.randn(M * 128)) if dres else None, dx=b.f32(n=M * 128),
                          dgamma=b.f32(b.randn(128)), dbeta=b.f32(b.dyadic(128) if exact else b.randn(128)), exact=exact,
                          **{k: d[k] for k in ("x", "gamma", "mean", "rstd", "M")})
                if rows_ep:
                    b.call("kantts_ln128_bwd_rows", zero_rows=None if z is None else b.u8(z), **kw)
                else:
                    b.call("kantts_ln128_bwd", **kw)
            br = ["ln128b:dy_bf16=%d" % bf, "ln128b:dres" if dres else "ln128b:dres=NULL", "ln128b:bwd_rows" if rows_ep else "ln128b:bwd",
                  {None: "ln128b:zero_rows=NULL", "some": "ln128b:zero_rows-some", "all": "ln128b:zero_rows-all"}[zr]]
            cs.append(_Case(name + ("_exact" if exact else ""), br + (["ln128b:M=%d" % M] if tag_m else []) + (["ln128b:dy=0"] if zero_dy else []), build))
            if zero_dy:
                break

    bwd("ln128_bwd_M1", 1, 0, False, None, False)
    bwd("ln128_bwd_M17", 17, 1, True, "some", True)
    bwd("ln128_bwd_M2048", 2048, 0, True, None, False)
    bwd("ln128_bwd_M2049", 2049, 1, False, "all", True)
    bwd("ln128_bwd_M4100_rows", 4100, 0, True, "some", True)
    bwd("ln128_bwd_M4100", 4100, 1, False, None, False)
    bwd("ln128_bwd_M17_all", 17, 0, False, "all", True)
    bwd("ln128_bwd_M1_rows_null", 1, 1, True, None, True)
    bwd("ln128_bwd_zero_dy", 40, 0, True, None, True, zero_dy=True, tag_m=False)
    bwd("ln128_bwd_zero_dy_bf16", 40, 1, False, "some", True, zero_dy=True, tag_m=False)
    return cs


def _ws_floats(B, Tt, C, K):
    """header: B * ceil(T / 128) * C * 41 floats of weight-gradient partials for K = 41, 0 otherwise"""
    return B * ((Tt + 127) // 128) * C * 41 if K == 41 else 0


def _fsmn_lens(kind, B, Tt, lp):
    if kind is None:
        return None, ["fsmn:lens=NULL"]
    pool = [(0, "fsmn:len=0"), (1, "fsmn:len=1"), (max(lp - 1, 0), "fsmn:len<lp"), (Tt - 1, "fsmn:len=T-1"), (Tt, "fsmn:len=T"),
            (Tt + 2, "fsmn:len=T+2"), ((Tt + 1) // 2, None)]
    pick = [pool[(kind + j) % 7] for j in range(B)] if B < 7 else pool + [pool[4]] * (B - 7)
    return [p[0] for p in pick], [p[1] for p in pick if p[1]] + ["fsmn:masked-rows-1e30"]


def _fsmn_tensors(b, B, Tt, C, K, lens, exact):
    n = B * Tt * C
    x, dy = (b.dyadic(n), b.dyadic(n)) if exact else (b.randn(n), b.randn(n))
    if lens is not None:  # rows at or after lens[b]: large finite values (the header writes x*keep)
        dead = (np.arange(Tt)[None, :] >= np.asarray(lens)[:, None])[:, :, None]
        x, dy = (np.where(dead, F32(BIG) * np.sign(v.reshape(B, Tt, C) + F32(0.1)), v.reshape(B, Tt, C)).astype(F32) for v in (x, dy))
    w = b.dyadic(C * K) if exact else b.randn(C * K, 0.2)
    return x, dy, w


def _fsmn_cases():
    cs = []

    def add(name, branches, B, Tt, C, K, lp, lens_kind, res, split=False):
        lens, lb = _fsmn_lens(lens_kind, B, Tt, lp)
        for exact in (True, False):
            def build(b, exact=exact):
                x, dy, w = _fsmn_tensors(b, B, Tt, C, K, lens, exact)
                n = B * Tt * C
                t = dict(x=b.f32(x), w=b.f32(w), lens=b.lens(lens), B=B, T=Tt, C=C, K=K, left_pad=lp, exact=exact)
                b.call("kantts_fsmn_dwconv_fwd", y=b.f32(n=n), res=b.f32(b.dyadic(n) if exact else b.randn(n)) if res else None, **t)
                ws_n = _ws_floats(B, Tt, C, K)
                b.call("kantts_fsmn_dwconv_bwd_ws", rc=ws_n, B=B, T=Tt, C=C, K=K)
                ws = b.f32(n=ws_n + 5) if ws_n else None
                dy_off, dw = b.f32(dy), b.f32(b.dyadic(C * K) if exact else b.randn(C * K))
                if split:
                    b.call("kantts_fsmn_dwconv_bwd", dy=dy_off, dx=b.f32(n=n), dw=None, ws=None, ws_floats=0, **t)
                    b.call("kantts_fsmn_dwconv_bwd", dy=dy_off, dx=None, dw=dw, ws=ws, ws_floats=ws_n, **t)
                else:
                    b.call("kantts_fsmn_dwconv_bwd", dy=dy_off, dx=b.f32(n=n), dw=dw, ws=ws, ws_floats=ws_n, **t)
            cs.append(_Case(name + ("_exact" if exact else ""), list(branches) + lb + ["fsmn:dw-accumulate", "fsmn:ws-size"]
                            + ["fsmn:res" if res else "fsmn:res=NULL"] + (["fsmn:dx-only", "fsmn:dw-only"] if split else []), build))

    lps = lambda K: (0, (K - 1) // 2, K - 1)
    lpn = ("fsmn:lp=0", "fsmn:lp=(K-1)/2", "fsmn:lp=K-1")
    for i, K in enumerate(_FS_KS):       # every K with every left_pad, seven sequences: every length of the list
        for j in range(3):
            add("fsmn_K%d_lp%d" % (K, j), ["fsmn:K=%d" % K, lpn[j]], 7, 33 + i, 5, K, lps(K)[j], 0, res=(i + j) % 2 == 0, split=j == 1)
    for i, C in enumerate(_FS_CS):       # every channel count, generic and 41-tap kernel
        for K in (3, 41):
            add("fsmn_C%d_K%d" % (C, K), ["fsmn:C=%d" % C, "fsmn:K=%d" % K], 3, 18, C, K, (K - 1) // 2, None if i % 3 == 2 else i,
                res=i % 2 == 1, split=i % 4 == 3)
    for i, Tt in enumerate(_FS_TS):      # every frame count, generic (K cycling) and 41-tap kernel
        for K in (_FS_KS[i % 6], 41):
            add("fsmn_T%d_K%d" % (Tt, K), ["fsmn:T=%d" % Tt, "fsmn:K=%d" % K, lpn[i % 3]], 4, Tt, (7, 66)[Tt < 40], K, lps(K)[i % 3],
                None if i % 4 == 1 else i, res=i % 2 == 0, split=i % 5 == 2)
    add("fsmn_xcd_bands", ["fsmn:xcd-81-blocks", "fsmn:K=41"], 9, 130, 3, 41, 20, 2, res=True)
    add("fsmn_xcd_bands_nolens", ["fsmn:xcd-81-blocks", "fsmn:K=41"], 9, 130, 3, 41, 40, None, res=False)
    add("fsmn_reduce_34", ["fsmn:reduce-34-rows", "fsmn:K=41"], 17, 129, 3, 41, 20, 3, res=False, split=True)
    return cs


def _rows_cases():
    cs = []
    Tt, B, C = 40, 2, 65
    for K, lp in ((3, 1), (41, 20), (3, 2), (41, 40)):
        for exact in (True, False):
            def build(b, K=K, lp=lp, exact=exact):
                lens = [Tt + 2, 35]
                x, _, w = _fsmn_tensors(b, B, Tt, C, K, lens, exact)
                n = B * Tt * C
                res = b.f32(b.dyadic(n) if exact else b.randn(n))
                t = dict(w=b.f32(w), res=res, lens=b.lens(lens), B=B, T=Tt, C=C, K=K, left_pad=lp, exact=exact)
                whole = b.f32(n=n)
                b.call("kantts_fsmn_dwconv_fwd", x=b.f32(x), y=whole, **t)
                for t0, t1 in ((0, Tt), (5, 5), (7, 8), (16, 33), (Tt - 1, Tt)):
                    xn = x.copy()
                    xn[:, t1 + (K - 1 - lp):] = np.nan  # rows the header says need not hold data yet
                    y = b.f32(n=n)
                    b.call("kantts_fsmn_dwconv_fwd_rows", x=b.f32(xn), y=y, t0=t0, t1=t1, **t)
                    if t1 > t0:
                        i = (ar(B)[:, None, None] * Tt + ar(t1 - t0)[None, :, None] + t0) * C + ar(C)[None, None, :]
                        b.call("same", what="rows (%d, %d)" % (t0, t1), a=whole + i, b=y + i, finite=True)
            cs.append(_Case("rows_K%d_lp%d%s" % (K, lp, "_exact" if exact else ""),
                            ["rows:K=%d" % K, "rows:(0,T)", "rows:(5,5)", "rows:(7,8)", "rows:(16,33)", "rows:(T-1,T)", "rows:nan-tail", "rows:==whole"],
                            build, emu=False))
    return cs


def _slots_cases():
    cs = []
    Tt, B, C = 40, 5, 20
    t0s, t1s = [-3, 20, 30, 2, 7], [10, 12, 45, 39, 8]
    for K, lp in ((3, 1), (41, 20)):
        for exact in (True, False):
            def build(b, K=K, lp=lp, exact=exact):
                lens = [Tt, 25, Tt + 2, 38, 3]
                x, _, w = _fsmn_tensors(b, B, Tt, C, K, lens, exact)
                n = B * Tt * C
                t = dict(x=b.f32(x), w=b.f32(w), res=b.f32(b.dyadic(n) if exact else b.randn(n)), lens=b.lens(lens), B=B, T=Tt, C=C, K=K,
                         left_pad=lp, exact=exact)
                d0, d1 = b.i32(t0s), b.i32(t1s)
                for mr in (0, 1, 16, 17, Tt + 5):
                    y = b.f32(n=n)
                    b.call("kantts_fsmn_dwconv_fwd_slots", y=y, t0=d0, t1=d1, max_rows=mr, **t)
                    for s in range(B):
                        c0 = min(max(t0s[s], 0), Tt)
                        c1 = min(min(max(t1s[s], c0), Tt), c0 + mr)
                        if c1 > c0:
                            y2 = b.f32(n=n)
                            b.call("kantts_fsmn_dwconv_fwd_rows", y=y2, t0=c0, t1=c1, **t)
                            i = (s * Tt + c0 + ar(c1 - c0)[:, None]) * C + ar(C)[None, :]
                            b.call("same", what="slot %d rows (%d, %d) max_rows %d" % (s, c0, c1, mr), a=y + i, b=y2 + i, finite=True)
            cs.append(_Case("slots_K%d%s" % (K, "_exact" if exact else ""),
                            ["slots:t0<0", "slots:t1<t0", "slots:t1>T", "slots:t1-t0>max_rows", "slots:==rows"]
                            + ["slots:max_rows=%s" % m for m in (0, 1, 16, 17, "T+5")], build, emu=False))
    return cs


def _embed_cases():
    cs = []
    nrows = (37, 20, 5, 3)

    def add(name, branches, ntab, D, rows, Tt, pos=True, scaled=True, ids_kind="random", null_tab=None, bwd=True):
        for exact in (True, False):
            def build(b, exact=exact):
                scale = 0.5 if exact else 11.313708
                mk = (lambda n: b.dyadic(n)) if exact else (lambda n: b.randn(n))
                if ids_kind == "random":
                    ids = np.stack([b.rng.integers(0, nrows[k], size=rows) for k in range(ntab)], axis=1)
                elif ids_kind == "equal":
                    ids = np.full((rows, ntab), 2)
                else:  # more than 8 distinct ids inside one 32-row chunk, each coming back after 8 others took its place
                    ids = np.stack([(ar(rows) * (k + 1)) % min(nrows[k], 11) for k in range(ntab)], axis=1)
                tabs = [b.f32(mk(nrows[k] * D)) for k in range(ntab)]
                i_off = b.i64(ids)
                b.call("kantts_embed_sum_fwd", tables=tabs, nrows=nrows, ids=i_off, pos=b.f32(mk(Tt * D)) if pos else None, out=b.f32(n=rows * D),
                       scaled=b.f32(n=rows * D) if scaled else None, rows=rows, T=Tt, D=D, scale=scale, exact=exact)
                if bwd:
                    dt = [None if k == null_tab else b.f32(mk(nrows[k] * D)) for k in range(ntab)]
                    b.call("kantts_embed_sum_bwd", tables=dt, nrows=nrows, ids=i_off, dout=b.f32(mk(rows * D)), rows=rows, D=D, scale=scale, exact=exact)
            cs.append(_Case(name + ("_exact" if exact else ""), branches + ["emb:ntab=%d" % ntab, "emb:D=%d" % D, "emb:rows=%d" % rows]
                            + (["embb:accumulate"] if bwd else []) + ([] if pos else ["emb:pos=NULL"]) + ([] if scaled else ["emb:scaled=NULL"])
                            + (["embb:rows%8"] if rows % 8 and bwd else []), build))

    add("emb_1tab", [], 1, 1, 1, 1)
    add("emb_2tab", ["emb:rows>T"], 2, 3, 31, 7, scaled=False)
    add("emb_3tab", ["embb:table=NULL"], 3, 64, 32, 32, pos=False, null_tab=1)
    add("emb_4tab", ["emb:rows>T", "embb:eviction"], 4, 257, 33, 11, ids_kind="evict")
    add("emb_70rows", ["emb:rows>T", "embb:eviction", "embb:table=NULL"], 4, 3, 70, 32, ids_kind="evict", null_tab=3)
    add("emb_equal_ids", ["embb:all-ids-equal"], 2, 64, 70, 70, ids_kind="equal")
    return cs


def _lr_durations(B, N, Tp):
    """(B, N) integer repetitions whose totals lie below, at and above Tp (by row), with zero durations between the others"""
    reps = np.zeros((B, N), dtype=np.int64)
    for r in range(B):
        want = max({0: Tp - 3, 1: Tp, 2: Tp + 5}[r % 3], 0)
        live = [n for n in range(N) if n % 3 != 1] or [0]
        for n in live:
            reps[r, n] = want // len(live)
        reps[r, live[-1]] += want - reps[r].sum()
        if r == 3:  # all durations zero
            reps[r] = 0
    return reps


def _lr_index_call(b, B, N, Tp, reps, as_float=False):
    t = dict(idx=b.f32(n=B * Tp), pos=b.f32(n=B * Tp), cs=b.f32(n=B * (N + 1)), lens=b.f32(n=2 * B), B=B, N=N, Tp=Tp)
    if as_float:
        b.call("kantts_lr_index", dur_int=None, dur_float=b.f32(reps), **t)
    else:
        b.call("kantts_lr_index", dur_int=b.i64(reps), dur_float=None, **t)
    return t


def _lr_cases():
    cs = []
    for N in (1, 63, 64, 65, 130):
        def build(b, N=N):
            _lr_index_call(b, 5, N, 2 * N + 7, _lr_durations(5, N, 2 * N + 7))
        cs.append(_Case("lr_index_N%d" % N, ["lri:N=%d" % N, "lri:total<Tp", "lri:total=Tp", "lri:total>Tp", "lri:all-zero"]
                        + (["lri:zero-between"] if N > 2 else []), build))

    def floats(b):
        dur = np.array([[0.49999997, 0.5, 1.5, 2.4999998, 0.0, 0.2, 3.7], [2.4999998, 0.0, 0.49999997, 1.5, 0.5, 0.0, 9.0]], dtype=F32)
        _lr_index_call(b, 2, 7, 12, dur, as_float=True)
    cs.append(_Case("lr_index_float", ["lri:float-0.49999997", "lri:float-0.5", "lri:float-1.5", "lri:float-2.4999998", "lri:zero-between"], floats))

    B, N, Tp = 7, 9, 24
    reps = np.array([[3, 0, 2, 4, 0, 1, 5, 2, 3]] * B, dtype=np.int64)  # total 20 < Tp; tokens 1 and 4 have no frame
    reps[5] = [6, 0, 5, 4, 0, 3, 5, 2, 3]                                # total 28 > Tp
    valids = [0, 11, Tp + 9, _V31, _V32, 26, 20]
    vb = ["valid=0", "valid<total", "valid>Tp", "valid=2^31", "valid=2^32+3"]

    for use_valid in (False, True):
        for exact in (True, False):
            def gather(b, use_valid=use_valid, exact=exact):
                t = _lr_index_call(b, B, N, Tp, reps)
                C, ldo, off = 5, 11, 3
                mk = (lambda n: b.dyadic(n)) if exact else (lambda n: b.randn(n))
                v = b.i64(valids) if use_valid else None
                g = dict(idx=t["idx"], cs=t["cs"], valid=v, B=B, N=N, Tp=Tp, C=C, ldo=ldo, off=off, exact=exact)
                b.call("kantts_lr_gather_fwd", x=b.f32(mk(B * N * C)), out=b.f32(n=B * Tp * ldo), **g)
                dout = b.f32(mk(B * Tp * ldo))
                b.call("kantts_lr_gather_bwd", dout=dout, dx=b.f32(n=B * N * C), accumulate=0, **g)
                b.call("kantts_lr_gather_bwd", dout=dout, dx=b.f32(mk(B * N * C)), accumulate=1, **g)
            cs.append(_Case("lr_gather%s%s" % ("_valid" if use_valid else "", "_exact" if exact else ""),
                            ["lrg:ldo>C", "lrg:accumulate=0", "lrg:accumulate=1", "lrg:token-without-frame"]
                            + (["lrg:" + v for v in vb] if use_valid else ["lrg:valid=NULL"]), gather))

    for r, (d_t, d_s, d_e), texts in ((1, (4, 8, 12), (1, 0, 1)), (3, (8, 4, 4), (0, 1, 0)), (3, (12, 12, 8), (1, 1, 1))):
        for use_valid in (False, True):
            for exact in (True, False):
                def memory(b, r=r, d_t=d_t, d_s=d_s, d_e=d_e, texts=texts, use_valid=use_valid, exact=exact):
                    t = _lr_index_call(b, B, N, Tp, reps)
                    mk = (lambda n: b.dyadic(n)) if exact else (lambda n: b.randn(n))
                    L, W = Tp // r, r * d_t + d_s + d_e
                    g = dict(idx=t["idx"], cs=t["cs"], valid=b.i64(valids) if use_valid else None, B=B, N=N, Tp=Tp, r=r, d_t=d_t, d_s=d_s, d_e=d_e,
                             exact=exact)
                    b.call("kantts_lr_memory_fwd", aug=b.f32(mk(B * N * d_t)), spk=b.f32(mk(B * N * d_s)), emo=b.f32(mk(B * N * d_e)),
                           pos_enc=b.f32(b.randn(B * Tp * d_t)), memory=b.f32(n=B * L * W), lr_text=b.f32(n=B * Tp * d_t) if texts[0] else None,
                           lr_spk=b.f32(n=B * Tp * d_s) if texts[1] else None, lr_emo=b.f32(n=B * Tp * d_e) if texts[2] else None, **g)
                    ldm = W + 8
                    b.call("kantts_lr_memory_bwd", d_memory=b.f32(mk(B * L * ldm)), ldm=ldm, d_aug=b.f32(n=B * N * d_t), d_spk=b.f32(n=B * N * d_s),
                           d_emo=b.f32(n=B * N * d_e), **g)
                cs.append(_Case("lr_memory_r%d_%d%s%s" % (r, d_t, "_valid" if use_valid else "", "_exact" if exact else ""),
                                ["lrm:r=%d" % r, "lrm:widths", "lrm:ldm>width"] + ["lrm:%s%s" % (k, "" if f else "=NULL") for k, f in
                                                                                    zip(("lr_text", "lr_spk", "lr_emo"), texts)]
                                + (["lrm:" + v for v in vb] if use_valid else ["lrm:valid=NULL"]), memory, emu=False))
    return cs


def _build_table():
    ln, data = _ln_cases()
    table = {"ln": ln, "ln128": _ln128_cases(data), "fsmn": _fsmn_cases(), "rows": _rows_cases(), "slots": _slots_cases(),
             "embed": _embed_cases(), "lr": _lr_cases()}
    names = [c.name for cs in table.values() for c in cs]
    assert len(set(names)) == len(names)
    return table


_TABLE = _build_table()
_GROUPS = list(_TABLE)
_MEASURED = {}


def _values(sh, r):
    return (r["want"], r["S"]) if r["kind"] == "bf16" else (sh.val[r["idx"]], sh.S[r["idx"]])


def _c():
    """c = 4 x the worst ratio of (float32, sequential sums in both directions) - (float64) to 2^-24 * S over the table"""
    if not _MEASURED:
        worst, where = 0.0, None
        for cases in _TABLE.values():
            for case in cases:
                ref = case.reference()
                for rev in (False, True):
                    low = _evaluate(case, F32, rev)
                    for key, r in ref.regions.items():
                        if r["kind"] not in ("measured", "bf16"):
                            continue
                        (want, S), got = _values(ref, r), np.asarray(_values(low, low.regions[key])[0], dtype=F64)
                        ok = np.isfinite(want) & (S > 0)
                        if ok.any():
                            ratio = float((np.abs(got - want)[ok] / (U * S[ok])).max())
                            if ratio > worst:
                                worst, where = ratio, "%s %s" % (case.name, r["what"])
        _MEASURED.update(ratio=worst, c=4.0 * worst, case=where)
        _record("fp32_reference", {"max_ratio_to_2^-24_S": worst, "c": 4.0 * worst, "case": where})
    return _MEASURED["c"]


def _record(key, val):
    try:
        os.makedirs(os.path.dirname(_REPORT), exist_ok=True)
        d = json.load(open(_REPORT)) if os.path.exists(_REPORT) else {}
        d[key] = val
        json.dump(d, open(_REPORT, "w"), indent=1)
    except (OSError, ValueError):  # (ValueError: another process is rewriting the report)
        pass


# ---------------------------------------------------------------------------------------------------------------------
# 4. back ends
def _leg_params(emu=True):
    ps = T._leg_params()
    return ps if emu else ps[1:]


class _Mem:
    """the arena on the leg's device, 16-byte aligned: p(off) = the address of float ``off``, h(off) of bf16 element ``off``"""

    def __init__(self, raw, leg):
        import kantts._hip as hip

        self.t = torch.empty(raw.size, dtype=torch.float32, device=leg.device)
        self.t.copy_(torch.from_numpy(raw))
        self.base, self.device = hip.ptr(self.t, torch.float32), leg.device
        assert self.base % 16 == 0

    def p(self, off):
        return None if off is None else self.base + 4 * int(off)

    def h(self, off):
        return None if off is None else self.base + 2 * int(off)

    def result(self):
        if self.device == "cuda":
            torch.cuda.synchronize()
        return self.t.cpu().numpy()


def _invoke(L_, m, c):
    """one call of the table through the C ABI"""
    import kantts._hip as hip

    ep, s, p = c["ep"], hip.stream(), m.p
    bs = c.get("byte_shift", {})
    q = lambda k: None if c[k] is None else p(c[k]) + bs.get(k, 0)
    if ep in ("kantts_ln128_fwd", "kantts_ln128_bwd", "kantts_ln128_bwd_rows", "kantts_lr_memory_fwd", "kantts_lr_memory_bwd") and c["rc"] == OK:
        for k in ("x", "gamma", "beta", "y", "dy", "dres", "dx", "aug", "spk", "emo", "pos_enc", "memory", "lr_text", "lr_spk", "lr_emo", "d_memory",
                  "d_aug", "d_spk", "d_emo"):
            if c.get(k) is not None:
                assert (m.h(c[k]) if k in ("y", "dy") and (c.get("y_bf16") or c.get("dy_bf16")) else p(c[k])) % 16 == 0, (ep, k)
    if ep == "kantts_layernorm_fwd":
        return L_.kantts_layernorm_fwd(q("x"), q("gamma"), q("beta"), q("y"), q("mean"), q("rstd"), c["M"], c["C"], c["eps"], s)
    if ep == "kantts_layernorm_bwd":
        return L_.kantts_layernorm_bwd(q("dy"), q("x"), q("gamma"), q("mean"), q("rstd"), q("dx"), q("dgamma"), q("dbeta"), c["M"], c["C"], s)
    if ep == "kantts_ln128_fwd":
        y = None if c["y"] is None else (m.h(c["y"]) if c["y_bf16"] else p(c["y"]))
        return L_.kantts_ln128_fwd(q("x"), q("gamma"), q("beta"), y, c["y_bf16"], q("mean"), q("rstd"), c["M"], c["eps"], s)
    if ep in ("kantts_ln128_bwd", "kantts_ln128_bwd_rows"):
        dy = None if c["dy"] is None else (m.h(c["dy"]) if c["dy_bf16"] else p(c["dy"]))
        a = (dy, c["dy_bf16"], q("x"), q("gamma"), q("mean"), q("rstd"), q("dres"), q("dx"), q("dgamma"), q("dbeta"))
        if ep == "kantts_ln128_bwd":
            return L_.kantts_ln128_bwd(*a, c["M"], s)
        return L_.kantts_ln128_bwd_rows(*a, q("zero_rows"), c["M"], s)
    if ep == "kantts_fsmn_dwconv_fwd":
        return L_.kantts_fsmn_dwconv_fwd(q("x"), q("w"), q("res"), q("lens"), q("y"), c["B"], c["T"], c["C"], c["K"], c["left_pad"], s)
    if ep == "kantts_fsmn_dwconv_fwd_rows":
        return L_.kantts_fsmn_dwconv_fwd_rows(q("x"), q("w"), q("res"), q("lens"), q("y"), c["B"], c["T"], c["C"], c["K"], c["left_pad"],
                                              c["t0"], c["t1"], s)
    if ep == "kantts_fsmn_dwconv_fwd_slots":
        return L_.kantts_fsmn_dwconv_fwd_slots(q("x"), q("w"), q("res"), q("lens"), q("y"), c["B"], c["T"], c["C"], c["K"], c["left_pad"],
                                               q("t0"), q("t1"), c["max_rows"], s)
    if ep == "kantts_fsmn_dwconv_bwd":
        return L_.kantts_fsmn_dwconv_bwd(q("dy"), q("x"), q("w"), q("lens"), q("dx"), q("dw"), q("ws"), c["ws_floats"], c["B"], c["T"], c["C"],
                                         c["K"], c["left_pad"], s)
    if ep == "kantts_fsmn_dwconv_bwd_ws":
        return int(L_.kantts_fsmn_dwconv_bwd_ws(c["B"], c["T"], c["C"], c["K"]))
    if ep in ("kantts_embed_sum_fwd", "kantts_embed_sum_bwd"):
        nt = c.get("ntab", len(c["tables"]))
        tabs = None if c.get("tables_null") else (ctypes.c_void_p * max(1, len(c["tables"])))(*[p(t) for t in c["tables"]])
        if ep == "kantts_embed_sum_fwd":
            return L_.kantts_embed_sum_fwd(tabs, nt, q("ids"), q("pos"), q("out"), q("scaled"), c["rows"], c["T"], c["D"], c["scale"], s)
        return L_.kantts_embed_sum_bwd(tabs, nt, q("ids"), q("dout"), c["rows"], c["D"], c["scale"], s)
    if ep == "kantts_lr_index":
        return L_.kantts_lr_index(q("dur_int"), q("dur_float"), q("idx"), q("pos"), q("cs"), q("lens"), c["B"], c["N"], c["Tp"], s)
    if ep == "kantts_lr_gather_fwd":
        return L_.kantts_lr_gather_fwd(q("x"), q("idx"), q("valid"), q("out"), c["B"], c["N"], c["Tp"], c["C"], c["ldo"], c["off"], s)
    if ep == "kantts_lr_gather_bwd":
        return L_.kantts_lr_gather_bwd(q("dout"), q("cs"), q("valid"), q("dx"), c["B"], c["N"], c["Tp"], c["C"], c["ldo"], c["off"],
                                       c["accumulate"], s)
    if ep == "kantts_lr_memory_fwd":
        return L_.kantts_lr_memory_fwd(q("aug"), q("spk"), q("emo"), q("idx"), q("valid"), q("pos_enc"), q("memory"), q("lr_text"), q("lr_spk"),
                                       q("lr_emo"), c["B"], c["N"], c["Tp"], c["r"], c["d_t"], c["d_s"], c["d_e"], s)
    if ep == "kantts_lr_memory_bwd":
        return L_.kantts_lr_memory_bwd(q("d_memory"), c["ldm"], q("cs"), q("valid"), q("d_aug"), q("d_spk"), q("d_emo"), c["B"], c["N"], c["Tp"],
                                       c["r"], c["d_t"], c["d_s"], c["d_e"], s)
    raise AssertionError(ep)


_WORST = {}


def _flush():
    """the worst ratio to the bound per leg and entry point so far, in one rewrite of the report"""
    try:
        os.makedirs(os.path.dirname(_REPORT), exist_ok=True)
        d = json.load(open(_REPORT)) if os.path.exists(_REPORT) else {}
        for (leg, ep), (w, where) in _WORST.items():
            d["%s_%s" % (leg, ep)] = {"max_ratio_to_bound": w, "case": where, "R": 2.0 if leg == "gpu" else 1.0, "c": _c()}
        json.dump(d, open(_REPORT, "w"), indent=1)
    except (OSError, ValueError):
        pass


def _inward(x, up):
    """the float32 next to ``x`` (float64) on the side of the reference: the smallest >= x (up) or the largest <= x"""
    f = x.astype(F32)
    bad = (f.astype(F64) < x) if up else (f.astype(F64) > x)
    return np.where(bad, np.nextafter(f, F32(np.inf if up else -np.inf)), f)


def _exempt(want, S):
    """exact cancellation over the whole tensor: ||ref|| <= 1e-9 ||S||; nothing may lie between 1e-9 and 1e-3"""
    nw, nS = float(np.linalg.norm(want)), float(np.linalg.norm(S))
    if nw <= 1e-9 * nS:
        return True
    assert nw > 1e-3 * nS, "||ref|| / ||S|| = %.3e lies between 1e-9 and 1e-3" % (nw / nS)
    return False


def _check(case, leg, got, raw):
    """the arena after the calls against the reference, region by region; what no region covers must hold its old bits"""
    ref = case.reference()
    g16, r16, g32 = got.view(np.uint16), raw.view(np.uint16), got.view(np.uint32)
    covered = np.zeros(g16.size, dtype=bool)  # in 2-byte units: a bf16 image is addressed in them
    c = _c()

    def ratio_of(err, S, what, ep):
        assert np.array_equal(err[S == 0], np.zeros(int((S == 0).sum()))), "%s: an element that must be exact is not" % what
        ratio = float((err[S > 0] / (U * S[S > 0])).max()) / c if (S > 0).any() else 0.0
        key = (leg.name, ep)
        if ratio >= _WORST.get(key, (-1.0, None))[0]:
            _WORST[key] = (ratio, case.name)
        print("%s %s: max |err| %.3e, ratio to c*2^-24*S %.4f (c = %.3f)" % (leg.name, what, float(err.max()) if err.size else 0.0, ratio, c))
        assert ratio <= leg.R, "%s: error %.3f x the bound c*2^-24*S (R = %g)" % (what, ratio, leg.R)

    for r in ref.regions.values():
        what, kind, idx = "%s %s %s" % (case.name, r["ep"], r["what"]), r["kind"], r["idx"]
        if kind == "same":
            assert np.array_equal(g32[r["a"]], g32[r["b"]]), "%s: the bits differ" % what
            assert not r["finite"] or np.isfinite(got[r["b"]]).all(), "%s: not finite" % what
            continue
        if kind == "bf16":
            covered[r["u16"]] = True
            have = (g16[r["u16"]].astype(np.uint32) << 16).view(F32)
            bound = leg.R * c * U * r["S"]
            lo = (_bf16_rne(_inward(r["want"] - bound, True)).astype(np.uint32) << 16).view(F32)
            hi = (_bf16_rne(_inward(r["want"] + bound, False)).astype(np.uint32) << 16).view(F32)
            bad = ~((have >= lo) & (have <= hi))
            print("%s %s: %d bf16 values, %d outside" % (leg.name, what, have.size, int(bad.sum())))
            assert not bad.any(), "%s: %d values are the bf16 of no float within the bound" % (what, int(bad.sum()))
            continue
        covered[2 * idx] = True
        covered[2 * idx + 1] = True
        if kind == "scratch":
            continue
        if kind == "i32":
            assert np.array_equal(got.view(np.int32)[idx], r["want"]), "%s: not the exact integers" % what
            continue
        if kind == "i64":
            assert np.array_equal(got.view(np.int64)[idx[::2] // 2], r["want"]), "%s: not the exact integers" % what
            continue
        have, want = got[idx], ref.val[idx]
        if kind == "exact":
            bad = have.astype(F64) != want
            assert not bad.any(), "%s: %d of %d differ from the exact value, first at %d: %r, expected %r" % (
                what, int(bad.sum()), bad.size, int(np.argmax(bad)), have[bad][:4], want[bad][:4])
        elif kind == "round":
            assert np.array_equal(have, want.astype(F32)), "%s: not float32(float64(a) + float64(b))" % what
        else:  # measured
            S = ref.S[idx]
            assert np.isfinite(have).all(), "%s: not finite" % what
            err = np.abs(have.astype(F64) - want)
            ratio_of(err, S, what, r["ep"])
            if r.get("cap_abs") is not None:
                assert err.size == 0 or float(err.max()) <= r["cap_abs"], "%s: max |err| %.3e > %.1e" % (what, float(err.max()), r["cap_abs"])
            if r.get("cap_l2"):
                if not _exempt(want, S):
                    l2 = float(np.linalg.norm(err) / np.linalg.norm(want))
                    assert l2 <= CAP_GRAD_L2, "%s: rel-L2 %.3e" % (what, l2)
    same = g16[~covered] == r16[~covered]
    assert same.all(), "%s: %d two-byte words outside the outputs were written, first at float %d" % (
        case.name, int((~same).sum()), int(np.flatnonzero(~covered)[np.argmax(~same)]) // 2)


def _run_case(case, leg):
    import kantts._hip as hip

    raw, calls = case.built()
    m = _Mem(raw, leg)
    for c in calls:
        if c["ep"] == "same" or (leg.name == "emu" and c["ep"] == "kantts_fsmn_dwconv_bwd_ws"):  # (the model needs no workspace)
            continue
        with np.errstate(all="ignore"):
            rc = _invoke(hip.lib(), m, c)
        assert rc == c["rc"], "%s %s: returned %d, expected %d" % (case.name, c["ep"], rc, c["rc"])
    _check(case, leg, m.result(), raw)


@pytest.mark.parametrize("group", _GROUPS)
@pytest.mark.parametrize("leg", T._leg_params())
def test_seq_kernels_match_the_fp64_interpreter(leg, group):
    leg = _Leg(leg)
    assert "KANTTS_LN_BWD_BLOCKS" not in os.environ, "the 128-block cap of kantts_ln128_bwd is part of what the table reaches"
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
    assert ran or (leg.name == "emu" and group in ("rows", "slots"))


def test_c_comes_from_the_fp32_evaluation_of_the_reference():
    """the measured ratio and c (recorded in seq_contract.json).  The ratio is pinned to the one recorded when the table was
    written: a case added later that is worse conditioned would otherwise loosen the bound of every other case"""
    c = _c()
    print("fp32 reference: worst ratio to 2^-24*S %.4f (%s), c = %.4f" % (_MEASURED["ratio"], _MEASURED["case"], c))
    assert c == 4.0 * _MEASURED["ratio"]
    assert 1.0 < _MEASURED["ratio"] <= 1.1 * RATIO_RECORDED, _MEASURED


def test_exempt_tensors_are_the_recorded_ones():
    """gradient tensors whose reference is exact cancellation (no relative cap): their number is stated, and no tensor lies in
    the gap between 1e-9 and 1e-3"""
    n = total = 0
    for cases in _TABLE.values():
        for case in cases:
            ref = case.reference()
            for r in ref.regions.values():
                if r["kind"] == "measured" and r.get("cap_l2"):
                    total += 1
                    n += _exempt(ref.val[r["idx"]], ref.S[r["idx"]])
    print("%d of %d gradient tensors are exempt from the relative cap" % (n, total))
    _record("exempt_from_rel_l2", {"tensors": n, "of": total})
    assert n == EXEMPT_RECORDED


def test_every_listed_branch_has_a_case():
    seen = {br for cs in _TABLE.values() for case in cs for br in case.branches} | {"fsmn:ws-short", "lrm:refusals"}
    assert seen == set(_BRANCHES), sorted(set(_BRANCHES) ^ seen)
    assert {"fsmn:ws-short", "lrm:refusals"} <= {br for _, br, _ in _REFUSALS}
    called = {c["ep"] for cs in _TABLE.values() for case in cs for c in case.built()[1]} - {"same"}
    assert called == set(_ENTRY_POINTS), sorted(set(_ENTRY_POINTS) ^ called)
    emulated = {c["ep"] for cs in _TABLE.values() for case in cs if case.emu for c in case.built()[1]} - {"same"}
    assert emulated == set(_ENTRY_POINTS) - _NOT_EMULATED
    _record("branches", sorted(seen))


# ---------------------------------------------------------------------------------------------------------------------
# 5. refusals: what the header or the entry point's own argument check documents
def _refusals():
    """(name, branch, build): each call returns its code and writes nothing"""
    out = []

    def add(name, build, branch=None):
        out.append((name, branch, build))

    def ln(b, ep, rc=E_BADARG, **kw):
        M, C = 3, 128
        c = dict(x=b.f32(b.randn(M * C)), gamma=b.f32(b.randn(C)), beta=b.f32(b.randn(C)), mean=b.f32(b.randn(M)), rstd=b.f32(b.randn(M) ** 2), M=M,
                 y=b.f32(n=M * C), y_bf16=0, eps=LN_EPS, dy=b.f32(b.randn(M * C)), dy_bf16=0, dres=None, dx=b.f32(n=M * C), dgamma=b.f32(b.randn(C)),
                 dbeta=b.f32(b.randn(C)), zero_rows=None, C=C)
        c.update(kw)
        b.call(ep, rc=rc, **c)

    for ep, nulls in (("kantts_layernorm_fwd", ("x", "gamma", "beta", "y", "mean", "rstd")), ("kantts_ln128_fwd", ("x", "gamma", "beta", "y", "mean", "rstd")),
                      ("kantts_layernorm_bwd", ("dy", "x", "gamma", "mean", "rstd", "dx", "dgamma", "dbeta")),
                      ("kantts_ln128_bwd", ("dy", "x", "gamma", "mean", "rstd", "dx", "dgamma", "dbeta")),
                      ("kantts_ln128_bwd_rows", ("dy", "x", "gamma", "mean", "rstd", "dx", "dgamma", "dbeta"))):
        for null in nulls:
            add("%s %s NULL" % (ep[7:], null), lambda b, ep=ep, null=null: ln(b, ep, **{null: None}))
        add("%s M < 0" % ep[7:], lambda b, ep=ep: ln(b, ep, M=-1))
    add("layernorm_fwd C < 1", lambda b: ln(b, "kantts_layernorm_fwd", C=0))
    add("layernorm_bwd C < 1", lambda b: ln(b, "kantts_layernorm_bwd", C=0))

    def fsmn(b, ep, rc=E_BADARG, K=41, **kw):
        B, Tt, C = 2, 20, 3
        n = B * Tt * C
        c = dict(x=b.f32(b.randn(n)), w=b.f32(b.randn(C * K)), res=None, lens=b.i64([20, 7]), y=b.f32(n=n), B=B, T=Tt, C=C, K=K, left_pad=1, t0=2, t1=9,
                 max_rows=5, dy=b.f32(b.randn(n)), dx=b.f32(n=n), dw=b.f32(b.randn(C * K)), ws=b.f32(n=_ws_floats(B, Tt, C, 41) + 4),
                 ws_floats=_ws_floats(B, Tt, C, 41))
        if ep == "kantts_fsmn_dwconv_fwd_slots":
            c.update(t0=b.i32([2, 3]), t1=b.i32([9, 4]))
        c.update(kw)
        b.call(ep, rc=rc, **c)

    for ep in ("kantts_fsmn_dwconv_fwd", "kantts_fsmn_dwconv_fwd_rows", "kantts_fsmn_dwconv_fwd_slots"):
        for null in ("x", "w", "y"):
            add("%s %s NULL" % (ep[7:], null), lambda b, ep=ep, null=null: fsmn(b, ep, **{null: None}))
        for dim in ("B", "T"):
            add("%s %s < 0" % (ep[7:], dim), lambda b, ep=ep, dim=dim: fsmn(b, ep, **{dim: -1}))
        add("%s C < 1" % ep[7:], lambda b, ep=ep: fsmn(b, ep, C=0))
        add("%s K < 1" % ep[7:], lambda b, ep=ep: fsmn(b, ep, K=0))
    for K in (3, 41):
        add("fsmn_dwconv_fwd_rows t0 < 0, K = %d" % K, lambda b, K=K: fsmn(b, "kantts_fsmn_dwconv_fwd_rows", K=K, t0=-1))
        add("fsmn_dwconv_fwd_rows t1 > T, K = %d" % K, lambda b, K=K: fsmn(b, "kantts_fsmn_dwconv_fwd_rows", K=K, t1=21))
        add("fsmn_dwconv_fwd_rows t0 > t1, K = %d" % K, lambda b, K=K: fsmn(b, "kantts_fsmn_dwconv_fwd_rows", K=K, t0=10))
    add("fsmn_dwconv_fwd_slots t0 NULL", lambda b: fsmn(b, "kantts_fsmn_dwconv_fwd_slots", t0=None))
    add("fsmn_dwconv_fwd_slots t1 NULL", lambda b: fsmn(b, "kantts_fsmn_dwconv_fwd_slots", t1=None))
    add("fsmn_dwconv_fwd_slots max_rows < 0", lambda b: fsmn(b, "kantts_fsmn_dwconv_fwd_slots", max_rows=-1))
    for null in ("dy", "x", "w"):
        add("fsmn_dwconv_bwd %s NULL" % null, lambda b, null=null: fsmn(b, "kantts_fsmn_dwconv_bwd", **{null: None}))
    add("fsmn_dwconv_bwd dx and dw NULL", lambda b: fsmn(b, "kantts_fsmn_dwconv_bwd", dx=None, dw=None))
    add("fsmn_dwconv_bwd workspace one float short", lambda b: fsmn(b, "kantts_fsmn_dwconv_bwd", rc=E_WORKSPACE, ws_floats=_ws_floats(2, 20, 3, 41) - 1),
        "fsmn:ws-short")
    add("fsmn_dwconv_bwd workspace one float short, dw only", lambda b: fsmn(b, "kantts_fsmn_dwconv_bwd", rc=E_WORKSPACE, dx=None,
                                                                         ws_floats=_ws_floats(2, 20, 3, 41) - 1), "fsmn:ws-short")
    add("fsmn_dwconv_bwd workspace NULL", lambda b: fsmn(b, "kantts_fsmn_dwconv_bwd", rc=E_WORKSPACE, ws=None), "fsmn:ws-short")

    def embed(b, ep, **kw):
        c = dict(tables=[b.f32(b.randn(12)), b.f32(b.randn(12))], nrows=(4, 4), ids=b.i64([[0, 1], [3, 2]]), pos=None, out=b.f32(n=6), scaled=None,
                 dout=b.f32(b.randn(6)), rows=2, T=2, D=3, scale=1.5)
        c.update(kw)
        b.call(ep, rc=E_BADARG, **c)

    for ep in ("kantts_embed_sum_fwd", "kantts_embed_sum_bwd"):
        add("%s tables NULL" % ep[7:], lambda b, ep=ep: embed(b, ep, tables_null=True))
        add("%s ntab 0" % ep[7:], lambda b, ep=ep: embed(b, ep, ntab=0))
        add("%s ntab 5" % ep[7:], lambda b, ep=ep: embed(b, ep, ntab=5))
        add("%s ids NULL" % ep[7:], lambda b, ep=ep: embed(b, ep, ids=None))
        add("%s rows < 0" % ep[7:], lambda b, ep=ep: embed(b, ep, rows=-1))
        add("%s D < 1" % ep[7:], lambda b, ep=ep: embed(b, ep, D=0))
    add("embed_sum_fwd out NULL", lambda b: embed(b, "kantts_embed_sum_fwd", out=None))
    add("embed_sum_bwd dout NULL", lambda b: embed(b, "kantts_embed_sum_bwd", dout=None))

    def lr(b, ep, rc=E_BADARG, **kw):
        B, N, Tp, r, d = 2, 3, 6, 3, 4
        cs_ = np.array([[0, 2, 2, 5], [0, 1, 4, 6]], dtype=np.int32)
        idx = np.array([[0, 0, 2, 2, 2, -1], [0, 1, 1, 1, 2, 2]], dtype=np.int32)
        c = dict(dur_int=b.i64([[2, 0, 3], [1, 3, 2]]), dur_float=None, idx=b.i32(idx), pos=b.f32(n=B * Tp), cs=b.i32(cs_), lens=b.f32(n=2 * B),
                 valid=b.i64([5, 6]), B=B, N=N, Tp=Tp, C=d, ldo=d, off=0, accumulate=0, x=b.f32(b.randn(B * N * d)), out=b.f32(n=B * Tp * d),
                 dout=b.f32(b.randn(B * Tp * d)), dx=b.f32(n=B * N * d), r=r, d_t=d, d_s=d, d_e=d, aug=b.f32(b.randn(B * N * d)),
                 spk=b.f32(b.randn(B * N * d)), emo=b.f32(b.randn(B * N * d)), pos_enc=b.f32(b.randn(B * Tp * d)), memory=b.f32(n=B * 2 * 5 * d),
                 lr_text=b.f32(n=B * Tp * d), lr_spk=None, lr_emo=b.f32(n=B * Tp * d), d_memory=b.f32(b.randn(B * 2 * 24)), ldm=24,
                 d_aug=b.f32(n=B * N * d), d_spk=b.f32(n=B * N * d), d_emo=b.f32(n=B * N * d))
        c.update(kw)
        b.call(ep, rc=rc, **c)

    add("lr_index both durations NULL", lambda b: lr(b, "kantts_lr_index", dur_int=None))
    for null in ("idx", "pos", "cs", "lens"):
        add("lr_index %s NULL" % null, lambda b, null=null: lr(b, "kantts_lr_index", **{null: None}))
    for ep, nulls in (("kantts_lr_gather_fwd", ("x", "idx", "out")), ("kantts_lr_gather_bwd", ("dout", "cs", "dx")),
                      ("kantts_lr_memory_fwd", ("aug", "spk", "emo", "idx", "pos_enc", "memory")),
                      ("kantts_lr_memory_bwd", ("d_memory", "cs", "d_aug", "d_spk", "d_emo"))):
        br = "lrm:refusals" if "memory" in ep else None
        for null in nulls:
            add("%s %s NULL" % (ep[7:], null), lambda b, ep=ep, null=null: lr(b, ep, **{null: None}), br)
        add("%s N < 1" % ep[7:], lambda b, ep=ep: lr(b, ep, N=0), br)
        add("%s B < 0" % ep[7:], lambda b, ep=ep: lr(b, ep, B=-1), br)
    add("lr_index N < 1", lambda b: lr(b, "kantts_lr_index", N=0))
    add("lr_gather_fwd ldo < C", lambda b: lr(b, "kantts_lr_gather_fwd", ldo=3))
    add("lr_gather_bwd ldo < C", lambda b: lr(b, "kantts_lr_gather_bwd", ldo=3))
    for ep in ("kantts_lr_memory_fwd", "kantts_lr_memory_bwd"):
        for w in ("d_t", "d_s", "d_e"):
            add("%s %s = 6" % (ep[7:], w), lambda b, ep=ep, w=w: lr(b, ep, rc=E_UNSUPPORTED, **{w: 6, "ldm": 32}), "lrm:refusals")
        add("%s Tp %% r != 0" % ep[7:], lambda b, ep=ep: lr(b, ep, r=4), "lrm:refusals")
    add("lr_memory_bwd ldm % 4 != 0", lambda b: lr(b, "kantts_lr_memory_bwd", rc=E_UNSUPPORTED, ldm=22), "lrm:refusals")
    add("lr_memory_bwd ldm below the row width", lambda b: lr(b, "kantts_lr_memory_bwd", ldm=16), "lrm:refusals")
    for k in ("aug", "spk", "emo", "pos_enc", "memory", "lr_text", "lr_emo"):  # refused by the host before any launch
        add("lr_memory_fwd %s + 4 bytes" % k, lambda b, k=k: lr(b, "kantts_lr_memory_fwd", rc=E_UNSUPPORTED, byte_shift={k: 4}), "lrm:refusals")
    for k in ("d_memory", "d_aug", "d_spk", "d_emo"):
        add("lr_memory_bwd %s + 4 bytes" % k, lambda b, k=k: lr(b, "kantts_lr_memory_bwd", rc=E_UNSUPPORTED, byte_shift={k: 4}), "lrm:refusals")
    return out


_REFUSALS = _refusals()


@pytest.mark.parametrize("leg", _leg_params(emu=False))
def test_refusals(leg):
    """each returns its code and leaves every byte of the arena as it was (the emulated ABI has no argument checks)"""
    import kantts._hip as hip

    leg = _Leg(leg)
    with leg.context():
        for name, _, build in _REFUSALS:
            b = _Builder(name)
            build(b)
            raw = b.finish()
            m = _Mem(raw, leg)
            for c in b.calls:
                rc = _invoke(hip.lib(), m, c)
                assert rc == c["rc"], "%s: returned %d, expected %d" % (name, rc, c["rc"])
            assert np.array_equal(m.result().view(np.uint32), raw.view(np.uint32)), "%s: a refused call wrote" % name
