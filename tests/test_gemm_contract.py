"""kantts_gemm_seg_launch against an fp64 interpreter of its descriptor (include/kantts_hip.h, "Segmented GEMM").

``_interpret`` is written from the header comment alone -- not from oracle/cabi_numpy.py, not from the kernels -- and
evaluates a descriptor in float64.  One table of descriptors (``_TABLE``) runs on three back ends: the emulated ABI, the
kernel sources on the CPU, and the device.  ``kantts_gemm_plan`` tells which kernel a descriptor gets; a module-level test
asserts that the table reaches all 4 instantiations of gemm_seg_mfma_kernel and all 64 of gemm_fast_kernel.

Bounds, for every element of C and of a_rowsum:
  * rel-L2 <= 2e-5 (the project's bound for this arithmetic: test_linear_fwd_bwd fp32 / ref,
    test_weight_gradient_contraction_with_both_output_tiles_gpu for bf16 MFMA against bf16-rounded operands);
  * |got - ref| <= R * (Ktot + 16) * 2^-24 * S, S = the same expression over absolute values: the forward bound of an fp32
    dot product of Ktot terms in any summation order (split-K atomics included) plus the few epilogue operations.  R = 1 where
    the arithmetic is IEEE round-to-nearest (emulated, kernel source on the CPU), R = 2 on the device (a faithfully rounding
    adder -- truncation at worst -- has unit roundoff 2^-23);
  * exactly: rows under rowmask are 0, memory outside C(i, j) is untouched, dropped elements are 0.
The largest ratio to the element-wise bound and the largest rel-L2 per leg and precision go to gemm_contract.json beside
the other parity reports.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cabi_numpy
import test_bench_config_parity as _bench_parity
import util

_REPORT = os.path.join(os.path.dirname(_bench_parity._REPORT), "gemm_contract.json")
_HAVE_CLANG = os.path.exists(os.environ.get("HIPEMU_CXX", "/opt/rocm/lib/llvm/bin/clang++"))
_NOFAST = os.environ.get("KANTTS_GEMM_NOFAST") is not None
E_BADARG = -1


def _record(key, val):
    try:
        os.makedirs(os.path.dirname(_REPORT), exist_ok=True)
        d = json.load(open(_REPORT)) if os.path.exists(_REPORT) else {}
        d[key] = val
        json.dump(d, open(_REPORT, "w"), indent=1)
    except OSError:
        pass


# ---------------------------------------------------------------------------------------------------------------------
# 1. the interpreter.  A descriptor is a dict with the header's field names; a pointer is a (flat fp32 tensor, element
#    offset) pair (uint8 tensors for the masks), absent = None.
def _bf16(x):
    """fp32 -> nearest bf16 (ties to even), as the (__bf16) cast does"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def _flat(p, absolute=False):
    t, off = p
    a = t.numpy()
    return (np.abs(a) if absolute else a), int(off)


def _token_rows(tok, shift, m, T):
    """header, 'Extended token map' (all zero = the plain map): source row and validity of token ``tok``"""
    inner, Tq, Tsrc = m.get("inner") or 1, m.get("Tq") or T, m.get("Tsrc") or T
    mul, div, up = m.get("mul") or 1, m.get("div") or 1, m.get("up") or 1
    pi, bq = tok % inner, tok // inner
    q, b = bq % Tq, bq // Tq
    t = q * mul + shift
    ok = np.ones(t.shape, dtype=bool)
    if div > 1:
        ok &= (t % div) == 0
        t = t // div
    ok &= (t >= 0) & (t < Tsrc * up)
    t = t // up
    return (b * Tsrc + t) * inner + pi, ok


def _gather(mem, base, offs, ok):
    lo, hi = (int(offs[ok].min()), int(offs[ok].max())) if ok.any() else (0, 0)
    assert base + lo >= 0 and base + hi < mem.size, "descriptor reads outside its buffer"
    return np.where(ok, mem[np.where(ok, base + offs, 0)], np.float32(0))


def _evaluate(g, absolute):
    M, N, T, prec = g["M"], g["N"], g["T"], g["precision"]
    ab = abs if absolute else (lambda x: x)
    f32 = np.float32
    groups = max(1, g["groups"])
    ztaps = g["z_taps"]
    i = np.arange(M, dtype=np.int64)[:, None]
    j = np.arange(N, dtype=np.int64)[:, None]
    jr = np.arange(N, dtype=np.int64)[None, :]
    cmem, coff = _flat(g["c"], absolute)
    C = cmem.astype(np.float64)
    touched = np.zeros(C.shape, dtype=bool)
    rowsum = None
    if g["a_rowsum"] is not None:
        rowsum = _flat(g["a_rowsum"], absolute)[0].astype(np.float64)
    kmask = None if g["kmask"] is None else g["kmask"][0].numpy() != 0
    for grp in range(groups):
        for slab in (range(ztaps) if ztaps > 0 else [None]):
            acc = np.zeros((M, N), dtype=np.float64)
            rs = np.zeros(M, dtype=np.float64)
            for si, s in enumerate(g["seg"]):
                K = s["klen"]
                kk = np.arange(K, dtype=np.int64)[None, :]
                for tap in range(s["ntaps"]):
                    if slab is not None and tap != slab:
                        continue
                    # ---- A(i, kk) = a[i*a_is + kk*a_ks], token shift s = shift0 + tap*step on the token axis
                    ai, ak = i + 0 * kk, kk + 0 * i
                    ok = np.ones((M, K), dtype=bool)
                    sh = s["a_shift0"] + tap * s["a_shift_step"]
                    if s["a_tok_axis"] == 1:
                        ai, ok = _token_rows(ai, sh, s["a_map"], T)
                    elif s["a_tok_axis"] == 2:
                        ak, ok = _token_rows(ak, sh, s["a_map"], T)
                    if kmask is not None:
                        ok = ok & ~kmask[:K][None, :]
                    offs = ai * s["a_is"] + ak * s["a_ks"] + grp * g["a_gs"]
                    amem, abase = _flat(s["a"], absolute)
                    A = _gather(amem, abase, offs, ok).astype(f32)
                    if s["a_act"]:
                        A = np.where(A > 0, A, A * f32(ab(s["a_slope"]))).astype(f32)
                    if s["a_gate"] is not None:
                        gmem, gbase = _flat(s["a_gate"])
                        gate = _gather(gmem, gbase, offs, ok)
                        A = np.where(ok & ~(gate > 0), A * f32(ab(s["a_gate_slope"])), A).astype(f32)
                    if s["a_drop_p"] > 0:
                        A = (A * cabi_numpy.dropout_scale(s["a_drop_p"], s["a_drop_seed"], np.where(ok, offs, 0))).astype(f32)
                    # ---- B(j, kk) = b[j*b_js + kk*b_ks + tap*b_tap]
                    bk = kk + 0 * j
                    okb = np.ones((N, K), dtype=bool)
                    if s["b_tok_axis"] == 2:
                        bk, okb = _token_rows(bk, s["b_shift0"] + tap * s["b_shift_step"], s["b_map"], T)
                    boffs = j * s["b_js"] + bk * s["b_ks"] + tap * s["b_tap"] + grp * g["b_gs"]
                    bmem, bbase = _flat(s["b"], absolute)
                    B = _gather(bmem, bbase, boffs, okb).astype(f32)
                    if s["b_act"]:
                        B = np.where(B > 0, B, B * f32(ab(s["b_slope"]))).astype(f32)
                    if prec == 1:
                        A, B = _bf16(A), _bf16(B)
                    A64 = A.astype(np.float64)
                    acc += A64 @ B.astype(np.float64).T
                    if si == 0 and (slab is None or slab == 0):
                        rs += A64.sum(axis=1)
            # ---- epilogue, in the header's order
            v = acc
            if g["bias"] is not None:
                mem, base = _flat(g["bias"], absolute)
                v = v + mem[base + jr + grp * g["bias_gs"]].astype(np.float64)
            if g["bias2"] is not None:
                mem, base = _flat(g["bias2"], absolute)
                v = v + mem[base + jr + grp * g["bias_gs"]].astype(np.float64)
            v = v * float(f32(ab(g["alpha"])))
            if g["relu"]:
                v = np.maximum(v, 0)
            if g["out_act"]:
                v = np.where(v > 0, v, v * float(f32(ab(g["out_slope"]))))
            if g["drop_p"] > 0:
                v = v * cabi_numpy.dropout_scale(g["drop_p"], g["drop_seed"], i * N + jr).astype(np.float64)
            if g["res"] is not None:
                mem, base = _flat(g["res"], absolute)
                roffs = base + i * g["r_is"] + jr * g["r_js"] + grp * g["r_gs"]
                assert roffs.min() >= 0 and roffs.max() < mem.size
                v = v + mem[roffs].astype(np.float64)
            coffs = coff + i * g["c_is"] + jr * g["c_js"] + grp * g["c_gs"]
            if g["gate"] is not None:
                mem, base = _flat(g["gate"])
                gv = mem[base + coffs - coff]
                v = v * np.where(gv > 0, 1.0, float(f32(ab(g["gate_slope"]))))
            if g["rowmask"] is not None:
                v = np.where(g["rowmask"][0].numpy()[:M, None] != 0, 0.0, v)
            if slab:
                coffs = coffs + slab * g["c_tap"]
            assert coffs.min() >= 0 and coffs.max() < C.size and not touched[coffs].any(), "C elements overlap / out of range"
            C[coffs] = v + (C[coffs] if g["accumulate"] else 0.0)
            touched[coffs] = True
            if rowsum is not None and (slab is None or slab == 0):
                rowsum[g["a_rowsum"][1] + np.arange(M) + grp * g["bias_gs"]] += rs
    return C, rowsum, touched


def _interpret(g):
    """(C, a_rowsum, S): the whole C buffer and the a_rowsum buffer after the launch, in float64, and S = (C, a_rowsum)
    of the same expression over absolute values; plus the mask of the C elements the launch writes."""
    C, rowsum, touched = _evaluate(g, False)
    SC, Srow, _ = _evaluate(g, True)
    return C, rowsum, (SC, Srow), touched


# ---------------------------------------------------------------------------------------------------------------------
# 2. the case table
_SEG_DEFAULTS = dict(a_gate=None, b_tap=0, ntaps=1, a_tok_axis=0, a_shift0=0, a_shift_step=0, b_tok_axis=0, b_shift0=0,
                     b_shift_step=0, a_drop_p=0.0, a_drop_seed=0, a_map={}, b_map={}, a_slope=0.0, a_act=0, b_slope=0.0,
                     b_act=0, a_gate_slope=0.0)
_ARG_DEFAULTS = dict(T=0, bias=None, bias2=None, res=None, r_is=0, r_js=0, rowmask=None, kmask=None, a_rowsum=None, alpha=1.0,
                     relu=0, accumulate=0, splitk=1, precision=0, drop_p=0.0, drop_seed=0, groups=1, a_gs=0, b_gs=0, c_gs=0,
                     bias_gs=0, r_gs=0, out_slope=0.0, out_act=0, gate=None, gate_slope=0.0, z_taps=0, c_tap=0)


class _Case:
    def __init__(self, name, g, expect=None):
        self.name, self.g, self.expect = name, g, expect
        self.ktot = sum(s["klen"] * s["ntaps"] for s in g["seg"])
        self._ref = {}

    def reference(self, precision):
        """computed once per arithmetic (fp32 for precision 0 and 2, bf16 operands for 1) and shared by every leg"""
        key = 1 if precision == 1 else 0
        if key not in self._ref:
            self._ref[key] = _interpret(dict(self.g, precision=key))
        return self._ref[key]


def _mk(name, M, N, segs, *, T=0, groups=1, c_pad=4, c_off=None, c_trans=False, bias=False, bias2=False, res=None,
        rowmask=False, kmask=False, rowsum=False, alpha=1.0, relu=False, out_leaky=None, gate=None, drop=None,
        accumulate=False, splitk=1, z_taps=False, expect=None):
    """Build a descriptor with random contents.  Each entry of ``segs``: dict(K, A='k'|'r', B='k'|'r', ...): 'k' = the
    reduction index has unit stride (rows with pitch > extent), 'r' = the row index has.  Group g of A / C / bias / res is
    the g-th column block; of B the g-th copy of the whole weight."""
    rng = torch.Generator().manual_seed(sum(ord(ch) * (k + 1) for k, ch in enumerate(name)) % (2 ** 31))

    def rand(n):
        return torch.randn(int(n), generator=rng)

    g = dict(_ARG_DEFAULTS, M=M, N=N, T=T, groups=groups, alpha=alpha, relu=int(relu), accumulate=int(accumulate), splitk=splitk)
    out = []
    for sp in segs:
        sp = dict(sp)
        K, ntaps = sp.pop("K"), sp.pop("ntaps", 1)
        s = dict(_SEG_DEFAULTS, klen=K, ntaps=ntaps)
        la, lb = sp.pop("A", "k"), sp.pop("B", "k")
        a_tok, b_tok = sp.pop("a_tok", None), sp.pop("b_tok", None)
        a_src, b_src = sp.pop("a_src", None), sp.pop("b_src", None)  # source length of the token axis under a map
        a_off, b_off = sp.pop("a_off", 0), sp.pop("b_off", 0)
        a_pad, b_pad = sp.pop("a_pad", 4), sp.pop("b_pad", 4)
        rows_a = (a_src if a_tok and a_tok[0] == 1 and a_src else M)
        ks_a = (a_src if a_tok and a_tok[0] == 2 and a_src else K)
        if la == "k":
            ld = groups * ks_a + a_pad
            s["a_is"], s["a_ks"], a_gs, size = ld, 1, ks_a, rows_a * ld
        else:
            ld = groups * rows_a + a_pad
            s["a_is"], s["a_ks"], a_gs, size = 1, ld, rows_a, ks_a * ld
        g["a_gs"] = a_gs if groups > 1 else 0
        s["a"] = (rand(a_off + size), a_off)
        if a_tok:
            s["a_tok_axis"], s["a_shift0"], s["a_shift_step"] = a_tok
        ks_b = b_src if b_src else K
        tap_pad = sp.pop("b_tap_pad", 0)
        if lb == "k":
            ld = ks_b + b_pad
            s["b_js"], s["b_ks"], blk = ld, 1, N * ld + tap_pad
        else:
            ld = N + b_pad
            s["b_js"], s["b_ks"], blk = 1, ld, ks_b * ld + tap_pad
        if b_tok:  # the taps read one tensor at shifted tokens
            s["b_tok_axis"], s["b_shift0"], s["b_shift_step"] = (2,) + tuple(b_tok)
            s["b_tap"], per_group = 0, blk
        else:
            s["b_tap"], per_group = blk, blk * ntaps
        g["b_gs"] = per_group if groups > 1 else 0
        s["b"] = (rand(b_off + per_group * groups), b_off)
        if "gate" in sp:
            s["a_gate"], s["a_gate_slope"] = (rand(a_off + size), a_off), sp.pop("gate")
        if "a_leaky" in sp:
            s["a_act"], s["a_slope"] = 1, sp.pop("a_leaky")
        if "b_leaky" in sp:
            s["b_act"], s["b_slope"] = 1, sp.pop("b_leaky")
        if "a_drop" in sp:
            s["a_drop_p"], s["a_drop_seed"] = sp.pop("a_drop")
        s["a_map"], s["b_map"] = sp.pop("a_map", {}), sp.pop("b_map", {})
        assert not sp, sp
        out.append(s)
    g["seg"] = out
    nt = out[0]["ntaps"] if z_taps else 1
    if c_trans:
        ldc = M + c_pad
        g["c_is"], g["c_js"], c_gs, span = 1, ldc, N * ldc, groups * N * ldc
    else:
        ldc = groups * N + c_pad
        g["c_is"], g["c_js"], c_gs, span = ldc, 1, N, M * ldc
    g["c_gs"] = c_gs if groups > 1 else 0
    if z_taps:
        g["z_taps"], g["c_tap"] = nt, span + 8
    c_off = 2 * ldc if c_off is None else c_off  # guard rows before C ...
    csize = c_off + (span + 8) * nt + 2 * ldc  # ... and after
    g["c"] = (rand(csize), c_off)
    if bias:
        g["bias"], g["bias_gs"] = (rand(groups * N), 0), (N if groups > 1 else 0)
    if bias2:
        g["bias2"], g["bias_gs"] = (rand(groups * N), 0), (N if groups > 1 else 0)
    if res == "plain" or res == "off1":
        ldr = groups * N + 8
        g["res"], g["r_is"], g["r_js"], r_gs = (rand(1 + M * ldr), int(res == "off1")), ldr, 1, N
    elif res == "trans":
        ldr = M + 3
        g["res"], g["r_is"], g["r_js"], r_gs = (rand(groups * N * ldr), 0), 1, ldr, N * ldr
    if res:
        g["r_gs"] = r_gs if groups > 1 else 0
    if rowmask:
        g["rowmask"] = ((torch.arange(M) % 5 == 2).to(torch.uint8), 0)
    if kmask:
        g["kmask"] = ((torch.arange(max(s["klen"] for s in out)) % 3 == 1).to(torch.uint8), 0)
    if rowsum:
        assert groups == 1
        g["a_rowsum"] = (rand(M + 2), 1)
    if out_leaky is not None:
        g["out_act"], g["out_slope"] = 1, out_leaky
    if gate is not None:
        g["gate"], g["gate_slope"] = (rand(csize), c_off), gate
    if drop:
        g["drop_p"], g["drop_seed"] = drop
    return _Case(name, g, expect)


def _fwd(K, ntaps=1, **kw):
    """forward: tokens x K against tap-major weights, the taps as a row shift"""
    return dict(dict(K=K, ntaps=ntaps, A="k", B="k", a_tok=(1, -(ntaps // 2), 1) if ntaps > 1 else None), **kw)


def _wgrad(K, ntaps=1, **kw):
    """weight gradient: both operands with unit row stride, the token on kk, a shift on B"""
    return dict(dict(K=K, ntaps=ntaps, A="r", B="r", b_tok=(-(ntaps // 2), 1)), **kw)


def _dgrad(K, **kw):
    """data gradient: A = dY with k contiguous, B = the transposed weight"""
    return dict(dict(K=K, A="k", B="r"), **kw)


def _mixed(K, **kw):
    """A with unit row stride (a transposed activation), B = a plain weight"""
    return dict(dict(K=K, A="r", B="k"), **kw)


def _instantiation_cases():
    """one fast-kernel case per (A_ROW, B_ROW, GATE, BIGK, BM): 32 cases x 2 precisions = the 64 instantiations.
    BM = 64 is reached the way production reaches it: cdiv(N,64)*cdiv(M,64)*splitk*groups*z_taps >= 512."""
    cases = []
    n = 0
    for lay, fam in (("fwd", _fwd), ("wgrad", _wgrad), ("dgrad", _dgrad), ("mixed", _mixed)):
        for gate in (None, 0.0, 0.2):
            for bigk in (False, True):
                for bm64 in (False, True):
                    if gate == 0.2 and (bigk != bm64):
                        continue  # the leaky gate: two of the four GATE = true shapes per family
                    n += 1
                    K = 512 if bigk else 72
                    M = 68 if lay in ("wgrad", "mixed") else 70
                    N = 68 if lay in ("wgrad", "dgrad") else 67
                    sp = {} if gate is None else {"gate": gate}
                    kw = {}
                    taps = 1
                    if lay == "fwd" and not bigk:
                        taps, kw["T"], M = 3, 35, 70
                    if lay == "wgrad":
                        taps, kw["T"] = (3 if not bigk else 2), K // 4
                        kw["z_taps"] = bool(n % 2)
                    if n % 3 == 0:
                        sp["a_leaky"] = 0.1
                    if n % 3 == 1:
                        sp["b_leaky"] = 0.3
                    if bm64:
                        groups = (1, 2, 4)[n % 3]
                        zt = taps if kw.get("z_taps") else 1
                        kw.update(groups=groups, splitk=-(-512 // (4 * groups * zt)), accumulate=True)
                    else:
                        kw.update(splitk=(1, 2, 7)[n % 3], accumulate=True)
                    kw.update(bias=bool(n % 2), res=(None, "plain", "trans")[n % 3], alpha=(1.0, 0.5)[n % 2],
                              rowsum=(kw.get("groups", 1) == 1 and n % 4 < 2 and (taps == 1 or bool(kw.get("z_taps")))))
                    seg = fam(K, taps, **sp) if lay in ("fwd", "wgrad") else fam(K, **sp)
                    name = "%s_g%s_%s_%s" % (lay, "n" if gate is None else ("h" if gate == 0 else "l"),
                                             "bigk" if bigk else "k72", "bm64" if bm64 else "bm32")
                    cases.append(_mk(name, M, N, [seg], expect=("fast", 64 if bm64 else 32, int(bigk)), **kw))
    return cases


def _edge_cases():
    c = []
    # tile edges of M, N, K (fast: K % 4 == 0; coalesced epilogue where N % 4 == 0)
    for M, N, K in ((31, 63, 28), (32, 64, 32), (33, 65, 36), (63, 1, 4), (64, 64, 64), (65, 68, 68), (1, 1, 4), (33, 64, 124),
                    (32, 60, 128), (31, 65, 132), (65, 33, 60)):
        c.append(_mk("edge_fast_%dx%dx%d" % (M, N, K), M, N, [_fwd(K)], bias=True, expect=("fast", 32, 0)))
    # the same in the generic kernel (K % 4 != 0: A and B staged with mode 0)
    for M, N, K in ((31, 63, 31), (32, 64, 33), (33, 65, 63), (63, 1, 65), (64, 64, 1), (65, 65, 127), (64, 32, 129)):
        c.append(_mk("edge_generic_%dx%dx%d" % (M, N, K), M, N, [_fwd(K, a_pad=3, b_pad=1)], bias=True, expect=("generic", 32)))
    # deep reduction tiles (BK 64 fp32 / 128 bf16): runs one below / at / above a tile, two and three segments
    c.append(_mk("bigk_two_segments", 40, 64, [_fwd(448), _fwd(132)], bias=True, expect=("fast", 32, 1)))
    c.append(_mk("bigk_three_segments", 40, 64, [_fwd(384), _fwd(124), _fwd(68)], res="plain"))
    c.append(_mk("bigk_exact_512", 33, 36, [_fwd(512)], expect=("fast", 32, 1)))
    c.append(_mk("bigk_taps_516", 34, 36, [_fwd(172, 3)], T=17, expect=("fast", 32, 1)))
    # klen no multiple of BK with several taps and two segments; four segments of different K
    c.append(_mk("taps_two_segments", 34, 65, [_fwd(36, 3), _fwd(44, 2, a_tok=(1, 0, 2))], T=17, bias=True, relu=True))
    c.append(_mk("four_segments", 37, 40, [_fwd(8), _fwd(100), _fwd(36, 3), _fwd(4)], T=37, bias=True, bias2=True))
    c.append(_mk("four_segments_generic", 37, 41, [_fwd(7, a_pad=1), _fwd(99), _fwd(35, 3), _fwd(1)], T=37, expect=("generic", 32)))
    # accumulate onto a non-zero C under split-K, more slices than reduction tiles: bias and residual exactly once
    for sk in (1, 2, 7):
        c.append(_mk("splitk%d_fast" % sk, 40, 64, [_fwd(64)], splitk=sk, accumulate=True, bias=True, res="plain", alpha=0.5,
                     rowsum=True, expect=("fast", 32, 0)))
        c.append(_mk("splitk%d_generic" % sk, 40, 63, [_fwd(66)], splitk=sk, accumulate=True, bias=True, res="trans",
                     rowsum=True, expect=("generic", 32)))
    # >= 64 tiles, not a multiple of 8, ragged M: the XCD remap visits every tile once (736 x 192: 23 x 3 = 69 tiles)
    c.append(_mk("xcd_69_tiles", 730, 192, [_fwd(8)], accumulate=True, bias=True, expect=("fast", 32, 0)))
    c.append(_mk("xcd_69_tiles_store", 730, 192, [_fwd(8)], res="plain", expect=("fast", 32, 0)))
    # 512 tiles by M x N alone: 64-row tiles with the coalesced epilogue, and the generic kernel's 64-row tiles
    c.append(_mk("bm64_by_shape", 8190, 256, [_fwd(8)], bias=True, relu=True, expect=("fast", 64, 0)))
    c.append(_mk("bm64_generic", 70, 67, [_fwd(66)], splitk=128, accumulate=True, bias=True, expect=("generic", 64)))
    c.append(_mk("bm64_generic_groups", 70, 67, [_dgrad(35)], groups=4, splitk=32, accumulate=True, res="plain",
                 expect=("generic", 64)))
    return c


def _epilogue_cases():
    c = []
    f = ("fast", 32, 0)
    c.append(_mk("epi_relu_bias2_alpha", 33, 64, [_fwd(64)], bias=True, bias2=True, alpha=-0.75, relu=True, expect=f))
    c.append(_mk("epi_out_act", 33, 64, [_fwd(64)], bias=True, out_leaky=0.1, res="plain", expect=f))
    c.append(_mk("epi_gate_hard", 33, 64, [_dgrad(64)], gate=0.0, res="plain", expect=f))
    c.append(_mk("epi_gate_leaky", 33, 68, [_dgrad(64)], gate=0.1, alpha=2.0, expect=f))
    c.append(_mk("epi_rowmask_vec", 33, 64, [_fwd(64)], bias=True, rowmask=True, res="plain", expect=f))
    c.append(_mk("epi_rowmask_direct", 33, 63, [_fwd(64)], bias=True, rowmask=True, res="trans", expect=f))
    c.append(_mk("epi_rowmask_generic", 33, 63, [_fwd(62)], bias=True, rowmask=True, res="trans", expect=("generic", 32)))
    c.append(_mk("epi_res_misaligned", 33, 64, [_fwd(64)], res="off1", expect=f))
    c.append(_mk("epi_res_n_mod4", 33, 62, [_fwd(64)], res="plain", out_leaky=0.2, expect=f))
    c.append(_mk("epi_res_groups", 33, 32, [_fwd(32)], groups=2, res="plain", bias=True, expect=f))
    c.append(_mk("epi_c_transposed", 36, 33, [_fwd(64)], c_trans=True, bias=True, res="trans", expect=f))
    c.append(_mk("epi_c_offset_one", 33, 64, [_fwd(64)], c_off=5, bias=True, expect=f))
    c.append(_mk("epi_generic_all", 35, 30, [_fwd(30, a_pad=1)], bias=True, bias2=True, alpha=0.5, out_leaky=0.3, res="trans",
                 gate=0.2, rowmask=True, expect=("generic", 32)))
    # dropout in the epilogue, and regenerated on a contiguous (M, N) A with the same seed (the backward of that epilogue)
    c.append(_mk("drop_epilogue_vec", 40, 64, [_fwd(64)], bias=True, relu=True, drop=(0.3, 1234), res="plain", expect=f))
    c.append(_mk("drop_epilogue_direct", 40, 63, [_fwd(64)], bias=True, drop=(0.3, 1234), expect=f))
    c.append(_mk("drop_epilogue_generic", 40, 63, [_fwd(63)], drop=(0.5, 99), res="plain", expect=("generic", 32)))
    c.append(_mk("drop_a_kvec", 40, 48, [_dgrad(64, a_pad=0, a_drop=(0.3, 1234))], expect=f))
    c.append(_mk("drop_a_kvec_gate", 40, 48, [_dgrad(64, a_pad=0, a_drop=(0.3, 1234), gate=0.0)], expect=f))
    c.append(_mk("drop_a_rowvec", 64, 48, [_wgrad(40, a_pad=0, a_drop=(0.3, 1234))], T=40, accumulate=True, splitk=2, expect=f))
    c.append(_mk("drop_a_generic", 40, 48, [_dgrad(63, a_pad=0, a_drop=(0.3, 1234))], expect=("generic", 32)))
    # a_leaky / b_leaky, a_gate in the generic kernel's layouts
    c.append(_mk("leaky_both", 33, 64, [_fwd(64, a_leaky=0.1, b_leaky=0.2)], expect=f))
    c.append(_mk("leaky_gate_generic", 33, 63, [_fwd(62, 3, a_leaky=0.1, b_leaky=0.2, gate=0.25)], T=11, expect=("generic", 32)))
    c.append(_mk("gate_generic_rows", 34, 48, [_wgrad(30, gate=0.0)], T=30, accumulate=True, expect=("generic", 32)))
    return c


def _group_cases():
    c = []
    for groups in (2, 4):
        c.append(_mk("groups%d_fast_fwd" % groups, 33, 32, [_fwd(32, 3)], T=11, groups=groups, bias=True, bias2=True, res="plain",
                     expect=("fast", 32, 0)))
        c.append(_mk("groups%d_fast_wgrad" % groups, 32, 36, [_wgrad(40, 3)], T=20, groups=groups, accumulate=True, splitk=2,
                     z_taps=True, expect=("fast", 32, 0)))
        c.append(_mk("groups%d_generic" % groups, 33, 30, [_fwd(30, 3)], T=11, groups=groups, bias=True, res="trans", gate=0.0,
                     expect=("generic", 32)))
        c.append(_mk("groups%d_generic_dgrad" % groups, 33, 31, [_dgrad(33)], groups=groups, res="plain", accumulate=True,
                     expect=("generic", 32)))
    # z_taps == ntaps writes C + tap * c_tap, a_rowsum once; a_rowsum under split-K
    c.append(_mk("ztaps_rowsum_fast", 64, 36, [_wgrad(44, 3)], T=22, z_taps=True, rowsum=True, accumulate=True, splitk=2,
                 expect=("fast", 32, 0)))
    c.append(_mk("ztaps_store_fast", 64, 36, [_wgrad(44, 3)], T=22, z_taps=True, rowsum=True, expect=("fast", 32, 0)))
    c.append(_mk("ztaps_rowsum_generic", 62, 35, [_wgrad(45, 3)], T=15, z_taps=True, rowsum=True, accumulate=True, splitk=7,
                 expect=("generic", 32)))
    c.append(_mk("wgrad_no_ztaps", 64, 36, [_wgrad(44, 3)], T=22, accumulate=True, alpha=0.5, expect=("fast", 32, 0)))
    return c


def _kmask_cases():
    """kmask with A in each staging mode (the a_mode == 2 descriptors are staged as mode 0 by the launcher)"""
    g = ("generic", 32)
    return [
        _mk("kmask_a_mode2", 40, 64, [_fwd(64)], kmask=True, rowsum=True, expect=g),
        _mk("kmask_a_mode2_taps", 34, 64, [_fwd(36, 3), _fwd(64)], T=17, kmask=True, bias=True, expect=g),
        _mk("kmask_a_mode0", 40, 64, [_fwd(66)], kmask=True, rowsum=True, expect=g),
        _mk("kmask_a_mode3", 40, 64, [_wgrad(64)], T=64, kmask=True, accumulate=True, rowsum=True, expect=("fast", 32, 0)),
        _mk("kmask_a_mode3_generic", 40, 62, [_wgrad(64)], T=64, kmask=True, accumulate=True, expect=g),
        _mk("kmask_a_mode1", 42, 64, [_wgrad(64)], T=64, kmask=True, accumulate=True, rowsum=True, expect=g),
    ]


def _map_cases():
    """extended token maps (generic kernel only) and every staging mode of the generic kernel"""
    g = ("generic", 32)
    Bt = 2
    c = [
        _mk("map_stride", Bt * 9, 40, [_fwd(32, 3, a_map=dict(Tq=9, Tsrc=19, mul=2), a_src=Bt * 19)], bias=True, expect=g),
        _mk("map_transposed", Bt * 16, 40, [_fwd(32, 4, a_tok=(1, -1, 1), a_map=dict(Tq=16, Tsrc=8, div=2), a_src=Bt * 8)], expect=g),
        _mk("map_upsample", Bt * 15, 40, [_fwd(32, 3, a_map=dict(Tq=15, Tsrc=5, up=3), a_src=Bt * 5)], out_leaky=0.1, expect=g),
        _mk("map_period_fold", Bt * 7 * 3, 40, [_fwd(32, 3, a_map=dict(inner=3, Tq=7, Tsrc=7), a_src=Bt * 7 * 3)], bias=True, expect=g),
        _mk("map_tsrc", Bt * 5, 40, [_fwd(32, 3, a_tok=(1, 0, 1), a_map=dict(Tq=5, Tsrc=7), a_src=Bt * 7)], expect=g),
        _mk("map_b_stride", 32, 36, [_wgrad(Bt * 9, 3, a_tok=(2, 0, 0), a_map=dict(Tq=9, Tsrc=9), b_map=dict(Tq=9, Tsrc=19, mul=2),
                                           b_src=Bt * 19)], accumulate=True, z_taps=True, expect=g),
        _mk("map_a_on_k", 33, 36, [_mixed(Bt * 9, ntaps=3, a_tok=(2, -1, 1), a_map=dict(Tq=9, Tsrc=19, mul=2), a_src=Bt * 19)], expect=g),
    ]
    # staging modes 0-3 of either operand in the generic kernel, reached by what the fast path declines
    c += [
        _mk("modes_a2_b0", 33, 64, [_fwd(64, b_pad=1)], bias=True, expect=g),                 # B pitch % 4 != 0
        _mk("modes_a0_b2", 33, 64, [_fwd(64, a_pad=3)], bias=True, expect=g),                 # A pitch % 4 != 0
        _mk("modes_a2_b1", 33, 63, [_dgrad(64)], res="plain", expect=g),                      # N % 4 != 0: rows of B
        _mk("modes_a1_b3", 34, 64, [_wgrad(40)], T=40, accumulate=True, expect=g),            # M % 4 != 0: rows of A
        _mk("modes_a3_b1", 36, 62, [_wgrad(40)], T=40, accumulate=True, expect=g),
        _mk("modes_a3_b0", 36, 64, [_mixed(64, b_off=1)], expect=g),                          # B base one element off
        _mk("modes_a0_b3", 33, 64, [_dgrad(64, a_off=1)], expect=g),                          # A base one element off
        _mk("modes_a0_b0_k", 33, 64, [_fwd(62)], expect=g),                                   # K % 4 != 0
        _mk("modes_b_tap_odd", 34, 64, [_fwd(64, 3, b_tap_pad=2)], T=17, expect=g),           # b_tap % 4 != 0, B k-vectors
        _mk("modes_b_tap_odd_rows", 34, 64, [dict(_dgrad(64), ntaps=3, a_tok=(1, -1, 1), b_tap_pad=2)], T=17, expect=g),
    ]
    return c


def _build_table():
    inst = _instantiation_cases()
    table = {}
    for lay in ("fwd", "wgrad", "dgrad", "mixed"):
        table["instantiations_" + lay] = [c for c in inst if c.name.startswith(lay + "_")]
    edges = _edge_cases()
    table["tile_edges"] = [c for c in edges if c.name.startswith("edge_")]
    table["segments_splitk"] = [c for c in edges if c.name.startswith(("bigk_", "taps_", "four_", "splitk"))]
    table["many_tiles"] = [c for c in edges if c.name.startswith(("xcd_", "bm64_"))]
    epi = _epilogue_cases()
    table["epilogue"] = [c for c in epi if c.name.startswith("epi_")]
    table["dropout_gates"] = [c for c in epi if not c.name.startswith("epi_")]
    table["groups_ztaps"] = _group_cases()
    table["kmask"] = _kmask_cases()
    table["token_maps_modes"] = _map_cases()
    names = [c.name for cs in table.values() for c in cs]
    assert len(set(names)) == len(names)
    return table


_TABLE = _build_table()
_GROUPS = list(_TABLE)


# ---------------------------------------------------------------------------------------------------------------------
# 3. back ends
class _Leg:
    def __init__(self, name):
        self.name = name
        self.device = "cuda" if name == "gpu" else "cpu"
        self.R = 2.0 if name == "gpu" else 1.0
        self.has_plan = name != "emu"

    def context(self):
        import contextlib

        return {"emu": util.emulation, "src": util.kernel_source_on_cpu, "gpu": contextlib.nullcontext}[self.name]()


def _leg_params():
    return [pytest.param("emu", id="emu"),
            pytest.param("src", id="src", marks=pytest.mark.skipif(not _HAVE_CLANG, reason="ROCm clang not installed")),
            pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]


def _plan_legs():
    return _leg_params()[1:]


def _descriptor(case, precision, device):
    """(GemmArgs, the tensors it points to) for one launch: fresh copies of every buffer on ``device``"""
    import kantts._hip as hip

    g = case.g
    keep = []

    def dev(p):
        if p is None:
            return None
        t = p[0].clone().to(device)
        keep.append(t)
        return (t, p[1])

    segs = []
    for s in g["seg"]:
        a = dev(s["a"])
        gate = None if s["a_gate"] is None else dev(s["a_gate"])
        segs.append(hip.make_seg(a, s["a_is"], s["a_ks"], dev(s["b"]), s["b_js"], s["b_ks"], s["klen"], ntaps=s["ntaps"],
                                 b_tap=s["b_tap"], a_tok_axis=s["a_tok_axis"], a_shift0=s["a_shift0"],
                                 a_shift_step=s["a_shift_step"], b_tok_axis=s["b_tok_axis"], b_shift0=s["b_shift0"],
                                 b_shift_step=s["b_shift_step"], a_gate=gate, a_drop_p=s["a_drop_p"],
                                 a_drop_seed=s["a_drop_seed"], a_map=s["a_map"], b_map=s["b_map"],
                                 a_leaky=s["a_slope"] if s["a_act"] else None, b_leaky=s["b_slope"] if s["b_act"] else None,
                                 a_gate_slope=s["a_gate_slope"]))
    c = dev(g["c"])
    one = lambda p: None if p is None else dev(p)[0]
    res = None if g["res"] is None else dev(g["res"])
    rowsum = None if g["a_rowsum"] is None else dev(g["a_rowsum"])
    gate = None if g["gate"] is None else dev((g["gate"][0], 0))
    args = hip.gemm_args(segs, g["M"], g["N"], c[0], g["c_is"], g["c_js"], bias=one(g["bias"]), bias2=one(g["bias2"]),
                         res=None if res is None else res[0], res_off=0 if res is None else res[1], r_is=g["r_is"],
                         r_js=g["r_js"], rowmask=one(g["rowmask"]), kmask=one(g["kmask"]), alpha=g["alpha"], relu=g["relu"],
                         accumulate=g["accumulate"], splitk=g["splitk"], T=g["T"], drop_p=g["drop_p"], drop_seed=g["drop_seed"],
                         precision=precision, c_off=c[1], groups=g["groups"], a_gs=g["a_gs"], b_gs=g["b_gs"], c_gs=g["c_gs"],
                         bias_gs=g["bias_gs"], r_gs=g["r_gs"], out_leaky=g["out_slope"] if g["out_act"] else None,
                         gate=None if gate is None else gate[0], gate_slope=g["gate_slope"], z_taps=g["z_taps"], c_tap=g["c_tap"])
    if rowsum is not None:
        args.a_rowsum = hip.ptr(rowsum[0], torch.float32) + 4 * rowsum[1]
    hip.rng_state(device).zero_()  # the device word added to every dropout seed
    return args, c[0], (None if rowsum is None else rowsum[0]), keep


def _launch(args, device):
    import kantts._hip as hip

    rc = hip.lib().kantts_gemm_seg_launch(ctypes.byref(args), hip.stream())
    if device == "cuda":
        torch.cuda.synchronize()
    return rc


_WORST = {}


def _note(leg, precision, ratio, rel):
    w = _WORST.setdefault((leg, precision), [0.0, 0.0])
    w[0], w[1] = max(w[0], ratio), max(w[1], rel)
    _record("%s_precision%d" % (leg, precision), {"max_elementwise_ratio_to_bound": w[0], "max_rel_l2": w[1], "R": 2.0 if leg == "gpu" else 1.0})


def _compare(case, leg, precision, got, ref, S, what, touched=None):
    got = got.double().cpu().numpy()
    if touched is not None:
        assert np.array_equal(got[~touched], ref[~touched]), "%s: memory outside C was written" % case.name
        got, ref, S = got[touched], ref[touched], S[touched]
    err = np.abs(got - ref)
    rel = float(np.linalg.norm(got - ref) / (np.linalg.norm(ref) + 1e-30))
    unit = (case.ktot + 16) * 2.0 ** -24 * S
    exact = unit == 0  # masked rows, dropped elements without a residual, k-masked / out-of-sequence products only
    assert np.array_equal(got[exact], ref[exact]), "%s %s: an element that must be exact is not" % (case.name, what)
    ratio = float((err[~exact] / unit[~exact]).max()) if (~exact).any() else 0.0
    print("%s %s %s precision %d: rel-L2 %.3e, element-wise ratio to (Ktot+16)*2^-24*S %.4f" % (leg.name, case.name, what,
                                                                                              precision, rel, ratio))
    _note(leg.name, precision, ratio, rel)
    assert rel <= 2e-5, "%s %s: rel-L2 %.3e" % (case.name, what, rel)
    assert ratio <= leg.R, "%s %s: element-wise error %.3f x the bound (R = %g)" % (case.name, what, ratio, leg.R)


def _expect_plan(case, plan, precision):
    if precision == 2:
        assert plan[0] == 3, (case.name, plan)
        return
    e = case.expect
    if e is None:
        assert plan[0] in (1, 2), (case.name, plan)
    elif e[0] == "generic" or _NOFAST:
        assert plan[0] == 1, (case.name, plan)
        if e[0] == "generic":
            assert plan[1] == e[1], (case.name, plan)
    else:
        assert plan[0] == 2 and plan[1] == e[1] and plan[2] == e[2], (case.name, plan)


def _run_case(case, leg, precision):
    import kantts._hip as hip

    ref, ref_rowsum, (S, S_rowsum), touched = case.reference(precision)
    args, c, rowsum, keep = _descriptor(case, precision, leg.device)
    if leg.has_plan:
        _expect_plan(case, hip.gemm_plan(args), precision)
    assert _launch(args, leg.device) == 0, case.name
    _compare(case, leg, precision, c, ref, S, "C", touched)
    g = case.g
    if g["rowmask"] is not None:  # masked rows are exactly zero (C is not accumulated onto in those cases)
        assert not g["accumulate"]
        M, N = g["M"], g["N"]
        view = c.cpu()[g["c"][1]:].as_strided((M, N), (g["c_is"], g["c_js"]))
        assert (view[g["rowmask"][0].bool()[:M]] == 0).all(), case.name
    if rowsum is not None:
        _compare(case, leg, precision, rowsum, ref_rowsum, S_rowsum, "a_rowsum")
        assert rowsum[0] == g["a_rowsum"][0][0] and rowsum[-1] == g["a_rowsum"][0][-1], "a_rowsum guards"
    del keep


@pytest.mark.parametrize("group", _GROUPS)
@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("leg", _leg_params())
def test_gemm_matches_the_fp64_interpreter(leg, precision, group):
    leg = _Leg(leg)
    with leg.context():
        for case in _TABLE[group]:
            _run_case(case, leg, precision)


@pytest.mark.parametrize("leg", _plan_legs())
def test_table_reaches_every_kernel_instantiation(leg):
    """the union of kantts_gemm_plan over the table: 4 x gemm_seg_mfma_kernel<BF16, BM>, 64 x
    gemm_fast_kernel<BF16, BM, BIGK, A_ROW, B_ROW, GATE>, the coalesced epilogue both on and off"""
    import kantts._hip as hip

    if _NOFAST:
        pytest.skip("KANTTS_GEMM_NOFAST is set: every descriptor takes the generic kernel")
    leg = _Leg(leg)
    generic, fast, vec = set(), set(), set()
    with leg.context():
        for cases in _TABLE.values():
            for case in cases:
                for precision in (0, 1):
                    args, _, _, keep = _descriptor(case, precision, leg.device)
                    plan = hip.gemm_plan(args)
                    if plan[0] == 1:
                        generic.add((precision, plan[1]))
                    elif plan[0] == 2:
                        fast.add((precision,) + tuple(plan[1:6]))
                        vec.add(plan[6])
                    else:
                        raise AssertionError((case.name, plan))
    want_fast = {(p, bm, bk, ar, br, gt) for p in (0, 1) for bm in (32, 64) for bk in (0, 1) for ar in (0, 1) for br in (0, 1)
                 for gt in (0, 1)}
    print("instantiations reached: %d/4 generic, %d/64 fast" % (len(generic), len(fast)))
    assert generic == {(p, bm) for p in (0, 1) for bm in (32, 64)}, sorted(generic)
    assert fast == want_fast, sorted(want_fast - fast)
    assert vec == {0, 1}
    _record("%s_instantiations" % leg.name, len(generic) + len(fast))


# ---------------------------------------------------------------------------------------------------------------------
# 5. refusals, the generic kernel on fast-eligible descriptors, the host-side selector
def _refusals():
    def base(**kw):
        return _mk("refusal", 16, 16, [_fwd(16)], **kw)

    def field(**kw):
        def f(args):
            for k, v in kw.items():
                setattr(args, k, v)
        return f

    def no_T(args):
        args.seg[0].a_tok_axis, args.seg[0].a_shift0, args.T = 1, 1, 0

    return [
        ("splitk_without_accumulate", base(), field(splitk=2)),
        ("splitk_relu", base(accumulate=True, relu=True), field(splitk=2)),
        ("splitk_out_act", base(accumulate=True, out_leaky=0.1), field(splitk=2)),
        ("splitk_gate", base(accumulate=True, gate=0.0), field(splitk=2)),
        ("splitk_drop", base(accumulate=True, drop=(0.5, 1)), field(splitk=2)),
        ("z_taps_two_segments", _mk("refusal", 16, 16, [_fwd(16), _fwd(16)]), field(z_taps=1)),
        ("z_taps_not_ntaps", _mk("refusal", 16, 16, [_fwd(16, 3)], T=8), field(z_taps=2)),
        ("token_axis_without_T", base(), no_T),
        ("grid_z_too_large", base(accumulate=True), field(groups=300, splitk=300)),
        ("precision_3", base(), field(precision=3)),
        ("nseg_0", base(), field(nseg=0)),
        ("nseg_5", base(), field(nseg=5)),
    ]


@pytest.mark.parametrize("leg", _plan_legs())
def test_refusals(leg):
    """each returns KANTTS_E_BADARG, leaves C untouched, and kantts_gemm_plan reports the same code"""
    import kantts._hip as hip

    leg = _Leg(leg)
    with leg.context():
        for name, case, spoil in _refusals():
            for precision in (0, 1, 2):
                args, c, _, keep = _descriptor(case, precision, leg.device)
                spoil(args)
                before = c.clone()
                assert hip.gemm_plan(args)[0] == E_BADARG, name
                assert _launch(args, leg.device) == E_BADARG, name
                assert torch.equal(c, before), name


@pytest.mark.skipif(not _HAVE_CLANG, reason="ROCm clang not installed")
def test_generic_kernel_on_fast_eligible_descriptors_in_a_fresh_process():
    """KANTTS_GEMM_NOFAST=1 sends every descriptor to gemm_seg_mfma_kernel; the launcher reads the switch once per process --
    the kernel-source leg of this file again, in a child process."""
    env = dict(os.environ, KANTTS_GEMM_NOFAST="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k",
                        "test_gemm_matches_the_fp64_interpreter and src"],
                       env=env, capture_output=True, text=True, timeout=900, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-2000:] + r.stderr[-1000:]


def _mode_preconditions_hold(mode, base, row_stride, k_stride, klen, rows, tok_axis, group_stride, gate, tap_stride, ntaps):
    """the header's a_mode / b_mode comment; every float4 of a vector mode must be 16-byte aligned"""
    aligned = base % 16 == 0 and (gate is None or gate % 16 == 0) and group_stride % 4 == 0 and (ntaps == 1 or tap_stride % 4 == 0)
    if mode == 2:
        return k_stride == 1 and klen % 4 == 0 and row_stride % 4 == 0 and aligned and tok_axis != 2
    if mode == 3:
        return row_stride == 1 and rows % 4 == 0 and k_stride % 4 == 0 and aligned and tok_axis != 1
    return mode in (0, 1)


def test_host_side_staging_mode_selector():
    import kantts._hip as hip

    sm = hip._staging_mode
    assert sm(4096, 64, 1, 64, 40, 0, 0) == 2 and sm(4096, 1, 64, 40, 64, 0, 0) == 3
    assert sm(4096 + 4, 64, 1, 64, 40, 0, 0) == 0 and sm(4096 + 4, 1, 64, 40, 64, 0, 0) == 1      # base not 16-byte aligned
    assert sm(4096, 64, 1, 64, 40, 0, 0, gate=8192 + 8) == 0 and sm(4096, 1, 64, 40, 64, 0, 0, gate=8192 + 8) == 1  # gate pointer
    assert sm(4096, 64, 1, 64, 40, 0, 30) == 0 and sm(4096, 1, 64, 40, 64, 0, 30) == 1              # group stride % 4 != 0
    assert sm(4096, 64, 1, 64, 40, 2, 0) == 0 and sm(4096, 1, 64, 40, 64, 1, 0) == 1                # token map on the vector axis
    assert sm(4096, 64, 1, 62, 40, 0, 0) == 0 and sm(4096, 1, 64, 40, 62, 0, 0) == 1                # extent % 4 != 0
    seen = set()
    with util.emulation():
        for cases in _TABLE.values():
            for case in cases:
                args, _, _, keep = _descriptor(case, 0, "cpu")
                for k in range(args.nseg):
                    s = args.seg[k]
                    seen.add((s.a_mode, s.b_mode))
                    assert _mode_preconditions_hold(s.a_mode, s.a, s.a_is, s.a_ks, s.klen, args.M, s.a_tok_axis, args.a_gs,
                                                    s.a_gate, 0, 1), (case.name, k, "A", s.a_mode)
                    assert _mode_preconditions_hold(s.b_mode, s.b, s.b_js, s.b_ks, s.klen, args.N, s.b_tok_axis,
                                                    args.b_gs, None, s.b_tap, s.ntaps), (case.name, k, "B", s.b_mode)
    assert {m for m, _ in seen} == {0, 1, 2, 3} and {m for _, m in seen} == {0, 1, 2, 3}
