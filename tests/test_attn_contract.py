"""kantts_attn_fwd / _bwd, the PNCA pair and kantts_attn_decode against an fp64 interpreter of their contract
(include/kantts_hip.h, "Range-limited multi-head attention").

``_evaluate`` is written from the header comment alone -- not from oracle/cabi_numpy.py, not from the kernels -- and
addresses memory as the ABI does: ptr[(b*L+t)*ld + h*16 + d] into one flat buffer.  One table of cases (``_TABLE``) runs on
three back ends through the C ABI itself: the emulated ABI, the kernel sources on the CPU, and the device.  The backward of a
case reads the o and lse the SAME leg's forward wrote.  ``kantts_attn_plan`` tells which kernels a case gets; every case
carries the path it expects, and a module-level test asserts that the table reaches every path.

Bounds:
  * exactly: every element outside the rows an entry point writes is bit-identical after the call; an element whose
    expression has no term (S = 0: context and lse of a skipped padded query row, dq of a padded query row -- or its old
    value under accumulate_dq --, dk / dv of a key no valid query sees, probs outside [lo, hi] and dropped probs) equals the
    reference exactly; return codes;
  * the project's caps (tests/test_gpu_ops.py) per element: context 2e-5, probs 2e-6, lse 2e-5; gradients rel-L2 <= 1e-4
    over each whole tensor.  The only tensors exempt are those whose reference is exact cancellation, |ref| <= 1e-9 * |S|
    over the whole tensor: with one key per interval dq and dk are differences of two equal terms, 0 up to the float64
    rounding of the reference (|ref| ~ 1e-16 * |S|), and a norm relative to that says nothing.  Every other gradient of
    the table (263 of 316) has |ref| >= 8e-3 * |S|; nothing lies between the two;
  * per element of the context, dq, dk, dv: |got - ref| <= R * c * 2^-24 * S, S = the interpreter's expression with every
    product replaced by its absolute value (the probabilities themselves are kept).  R = 1 where the arithmetic is IEEE
    round-to-nearest (emulated, kernel source on the CPU), R = 2 on the device, as in tests/test_gemm_contract.py.
    c comes from the reference, never from the kernels: the interpreter evaluated a second time in numpy float32 with the
    keys (queries, for dk / dv) summed in reversed order differs from the float64 evaluation by at most ``ratio`` * 2^-24 * S
    over the whole table, and c = 4 * ratio (the 4 covers the tree-shaped sums of the four-lanes-per-query kernels and a
    device expf that is not correctly rounded).  Measured when this file was written: ratio = 14.33 (attn_L391_mode2), c = 57.3
    (the test measures it again in every session and uses what it measures; both go to attn_contract.json).  The measured
    ratio may not exceed the recorded one by more than 10 % (the float32 matrix products run in the BLAS's own order), so a
    case added later cannot loosen the bound of every other case without a visible sign.
The largest ratio to the bound and the largest rel-L2 per leg and path go to attn_contract.json beside gemm_contract.json.
"""
import contextlib
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

_REPORT = os.path.join(os.path.dirname(_bench_parity._REPORT), "attn_contract.json")
_HAVE_CLANG = os.path.exists(os.environ.get("HIPEMU_CXX", "/opt/rocm/lib/llvm/bin/clang++"))
_NO_QUAD = os.environ.get("KANTTS_ATTN_NO_QUAD") is not None
_NO_DQ2 = os.environ.get("KANTTS_ATTN_NO_DQ2") is not None
_SWITCHES = "".join(s for s, on in (("_noquad", _NO_QUAD), ("_nodq2", _NO_DQ2),
                                    ("_headmajor", os.environ.get("KANTTS_ATTN_HEAD_MAJOR") is not None)) if on)
E_BADARG, E_UNSUPPORTED = -1, -2
DH = 16
U = 2.0 ** -24
CAP_CTX, CAP_PROBS, CAP_LSE, CAP_GRAD_REL = 2e-5, 2e-6, 2e-5, 1e-4  # tests/test_gpu_ops.py
CANCELLED = 1e-9        # |ref| <= CANCELLED * |S|: the reference tensor is exact cancellation (see above)
RATIO_RECORDED = 14.33  # the float32 evaluation of the reference, see above


def _record(key, val):
    try:
        os.makedirs(os.path.dirname(_REPORT), exist_ok=True)
        d = json.load(open(_REPORT)) if os.path.exists(_REPORT) else {}
        d[key] = val
        json.dump(d, open(_REPORT, "w"), indent=1)
    except (OSError, ValueError):  # (ValueError: another process is rewriting the report)
        pass


# ---------------------------------------------------------------------------------------------------------------------
# 1. the interpreter.  A problem is a dict: mem (flat fp32 array), q / k / v / d_o = (element offset, ld), B, H, L, mode,
#    bw (int, or B ints = bw_seq), lens (B ints or None), drop_p, seed (host seed + device word), probs (bool),
#    step (None, or the decoder position of kantts_attn_decode: q then holds B rows).
def _rows(mem, off, ld, B, nrow, H):
    """element (b, t, h, d) at off + (b*nrow + t)*ld + h*16 + d"""
    b = np.arange(B, dtype=np.int64)[:, None, None, None]
    t = np.arange(nrow, dtype=np.int64)[None, :, None, None]
    h = np.arange(H, dtype=np.int64)[None, None, :, None]
    d = np.arange(DH, dtype=np.int64)[None, None, None, :]
    idx = off + (b * nrow + t) * ld + h * DH + d
    assert idx.min() >= 0 and idx.max() < mem.size, "the problem reads or writes outside its buffer"
    return idx


def _interval(mode, i, ln, L, bw):
    """header: the keys [lo, hi] of the queries ``i`` of a sequence with ``ln`` valid positions"""
    if mode == 0:
        return np.zeros_like(i), np.full_like(i, ln - 1)
    if mode == 1:
        lo, hi = np.maximum(0, i - bw), i
    else:
        lo, hi = i, np.minimum(np.minimum(i + bw, L - 1), ln - 1)
    padded = i >= ln
    return np.where(padded, 0, lo), np.where(padded, L - 1, hi)


def _qk(a, b):
    """(H, I, 16) x (H, J, 16) -> (H, I, J): the sum over d"""
    return a @ np.ascontiguousarray(b.transpose(0, 2, 1))


def _over_keys(w, x, flip):
    """(H, I, J) x (H, J, 16) -> (H, I, 16): the sum over the keys j"""
    return np.ascontiguousarray(flip(w, axis=2)) @ np.ascontiguousarray(flip(x, axis=1))


def _over_queries(w, x, flip):
    """(H, I, J) x (H, I, 16) -> (H, J, 16): the sum over the queries i"""
    return np.ascontiguousarray(flip(w, axis=1).transpose(0, 2, 1)) @ np.ascontiguousarray(flip(x, axis=1))


def _evaluate(pr, dt=np.float64, reverse=False):
    """Context, lse, post-dropout probs, dq / dk / dv of one problem in ``dt``, and S_* = the same sums over absolute
    values.  ``reverse``: every sum over keys (over queries for dk / dv) runs in reversed order."""
    mem, B, H, L, mode = pr["mem"], pr["B"], pr["H"], pr["L"], pr["mode"]
    step, want_probs = pr.get("step"), pr["probs"]
    qi = np.arange(L, dtype=np.int64) if step is None else np.array([step], dtype=np.int64)
    nq = qi.size
    Q = mem[_rows(mem, *pr["q"], B, nq, H)].astype(dt)
    K = mem[_rows(mem, *pr["k"], B, L, H)].astype(dt)
    V = mem[_rows(mem, *pr["v"], B, L, H)].astype(dt)
    G = mem[_rows(mem, *pr["d_o"], B, nq, H)].astype(dt) if pr.get("d_o") is not None else None
    flip = np.flip if reverse else (lambda a, axis: a)
    quarter = dt(0.25)
    r = {"o": np.zeros((B, nq, H, DH), dt), "S_o": np.zeros((B, nq, H, DH), dt), "lse": np.zeros((B, H, nq), dt),
         "probs": np.zeros((H, B, L, L), dt) if want_probs else None}
    if G is not None:
        for n in ("dq", "dk", "dv", "S_dq", "S_dk", "S_dv"):
            r[n] = np.zeros((B, L, H, DH), dt)
    j = np.arange(L, dtype=np.int64)
    hh = np.arange(H, dtype=np.int64)[:, None, None]
    for b in range(B):
        ln = L if pr["lens"] is None else int(pr["lens"][b])
        bw = int(pr["bw"]) if np.ndim(pr["bw"]) == 0 else int(pr["bw"][b])
        lo, hi = _interval(mode, qi, ln, L, bw)
        allow = (j[None, :] >= lo[:, None]) & (j[None, :] <= hi[:, None])
        padded = (qi >= ln) & (mode != 0)  # band modes: computed only when probs is requested, never in the backward
        if not want_probs:
            allow = allow & ~padded[:, None]
        q, k, v = (np.ascontiguousarray(x[b].transpose(1, 0, 2)) for x in (Q, K, V))  # (H, rows, 16)
        s = (quarter * _qk(q, k)).astype(dt)
        live = allow.any(axis=1)
        A = allow[None]
        m = np.where(live[None], np.where(A, s, -np.inf).max(axis=2), 0).astype(dt)
        e = np.where(A, np.exp(np.where(A, s - m[..., None], 0)), 0).astype(dt)
        l = flip(e, axis=2).sum(axis=2, dtype=dt)
        lse = np.where(live[None], m + np.log(np.where(live[None], l, 1)), 0).astype(dt)
        p = (e / np.where(live[None], l, 1)[..., None]).astype(dt)
        drop = cabi_numpy.dropout_scale(pr["drop_p"], pr["seed"], ((hh * B + b) * L + qi[None, :, None]) * L + j[None, None, :])
        drop = drop.astype(dt)
        pd = p * drop
        o = _over_keys(pd, v, flip)
        S_o = _over_keys(pd, np.abs(v), flip)
        r["o"][b], r["S_o"][b], r["lse"][b] = o.transpose(1, 0, 2), S_o.transpose(1, 0, 2), lse
        if want_probs:
            r["probs"][:, b] = pd
        if G is None:
            continue
        g = np.ascontiguousarray(G[b].transpose(1, 0, 2))
        Ab = (allow & ~padded[:, None])[None]
        pb = np.where(Ab, np.exp(np.where(Ab, s - lse[..., None], 0)), 0).astype(dt)
        D, D_abs = (g * o).sum(axis=2, dtype=dt), (np.abs(g) * S_o).sum(axis=2, dtype=dt)
        dp = _qk(g, v) * drop
        dp_abs = _qk(np.abs(g), np.abs(v)) * drop
        ds = (quarter * pb * (dp - D[..., None])).astype(dt)
        ds_abs = (quarter * pb * (dp_abs + D_abs[..., None])).astype(dt)
        pbd = pb * drop
        for n, val in (("dq", _over_keys(ds, k, flip)),
                       ("S_dq", _over_keys(ds_abs, np.abs(k), flip)),
                       ("dk", _over_queries(ds, q, flip)),
                       ("S_dk", _over_queries(ds_abs, np.abs(q), flip)),
                       ("dv", _over_queries(pbd, g, flip)),
                       ("S_dv", _over_queries(pbd, np.abs(g), flip))):
            r[n][b] = val.transpose(1, 0, 2)
    return r


# ---------------------------------------------------------------------------------------------------------------------
# 2. the case table
def _expected(which, L, mode=1):
    """the path the header promises (409 / 390 / 256), under this process's switches"""
    quad = mode == 0 and not _NO_QUAD
    if which == "fwd":
        return "fwd_direct" if L >= 410 else ("fwd_lds_quad" if quad else "fwd_lds")
    if which == "bwd":
        return "bwd_direct" if L >= 391 else ("bwd_lds_quad" if quad else "bwd_lds")
    if which == "pnca_fwd":
        return "unsupported" if L >= 410 else "pnca_fwd_lds"
    return "unsupported" if L >= 391 else ("pnca_bwd_dq2" if L <= 256 and not _NO_DQ2 else "pnca_bwd_split")


class _Arena:
    """offsets into one flat buffer: guard elements before the first block, after every block, and whatever the rows of
    a block leave between them (ld > width).  Every offset is a multiple of 4 (16-byte aligned rows)."""

    def __init__(self):
        self.n = 8

    def block(self, floats, tail=8):
        off = self.n
        self.n = off + (int(floats) + 3) // 4 * 4 + tail
        return off


def _lens(pat, B, L):
    """'none'; 'ragged': len = L, a len that is no multiple of 4, len = 1; 'zero': one empty sequence"""
    odd = max(1, (2 * L) // 3)
    odd += 1 if odd % 4 == 0 and odd < L else 0
    return {"none": None, "ragged": [L, odd, 1][:B] if B > 2 else [odd, L], "zero": [odd, 0, L][:B]}[pat]


class _Case:
    def __init__(self, name, kind, **kw):
        self.name, self.kind = name, kind
        self.__dict__.update(dict(B=3, H=3, mode=1, bw=3, bw_dev=None, lens=None, drop_p=0.0, seed=0, seed_dev=None,
                                  layout="packed", probs=False, acc=0, bwd=True, bw_x=3, bw_h=5, seed_h=0, ldh_extra=0,
                                  dqh_null=False, bw_seq=None), **kw)
        self.D = self.H * DH
        self._built = self._ref = None
        L, mode = self.L, self.mode
        if kind == "attn":
            self.expect = {"fwd": _expected("fwd", L, mode), "bwd": _expected("bwd", L, mode)}
        elif kind == "pnca":
            self.expect = {"pnca_fwd": _expected("pnca_fwd", L), "pnca_bwd": _expected("pnca_bwd", L)}
        else:
            self.expect = {}

    # -- memory: (flat input tensor, flat output tensor as it is before the call, offsets)
    def built(self):
        if self._built is not None:
            return self._built
        rng = torch.Generator().manual_seed(sum(ord(ch) * (k + 1) for k, ch in enumerate(self.name)) % (2 ** 31))
        B, L, D, M = self.B, self.L, self.D, self.B * self.L
        ai, ao, f = _Arena(), _Arena(), {}
        if self.kind == "attn":
            if self.layout == "fused":  # q | k | v columns of one (B*L, 3D) projection, dq | dk | dv likewise
                base, gbase = ai.block(M * 3 * D), None
                f.update(q=(base, 3 * D), k=(base + D, 3 * D), v=(base + 2 * D, 3 * D))
                f["d_o"] = (ai.block(M * D), D)
                f["o"] = (ao.block(M * D), D)
                gbase = ao.block(M * 3 * D)
                f.update(dq=(gbase, 3 * D), dk=(gbase + D, 3 * D), dv=(gbase + 2 * D, 3 * D))
            else:
                pads = (4, 8, 12, 4) if self.layout == "guard" else (0, 0, 0, 0)
                for n, pad in zip(("q", "k", "v", "d_o"), pads):
                    f[n] = (ai.block(M * (D + pad)), D + pad)
                f["o"] = (ao.block(M * (D + pads[1])), D + pads[1])
                for n, pad in zip(("dq", "dk", "dv"), pads):
                    f[n] = (ao.block(M * (D + pad)), D + pad)
            f["lse"], f["dvec"] = ao.block(B * self.H * L), ao.block(B * self.H * L)
            if self.probs:
                f["probs"] = ao.block(self.H * B * L * L)
        elif self.kind == "pnca":
            f["qkv"] = ai.block(M * 3 * D)
            f["ldh"] = 2 * D + self.ldh_extra  # hkv: a column block of a wider projection
            f["hkv"] = ai.block(M * f["ldh"]) + (4 if self.ldh_extra else 0)
            f["d_ox"], f["d_oh"] = ai.block(M * D), ai.block(M * D)
            f["ox"], f["oh"] = ao.block(M * D), ao.block(M * D)
            f["lse_x"], f["lse_h"] = ao.block(B * self.H * L), ao.block(B * self.H * L)
            f["dqkv"], f["dqh"], f["dhkv"] = ao.block(M * 3 * D), ao.block(M * D), ao.block(M * 2 * D)
        else:  # decode: one q / o row block per step
            pad = 4 if self.layout == "guard" else 0
            f["q"], f["k"], f["v"] = (ai.block(L * B * (D + pad)), D + pad), (ai.block(M * (D + 2 * pad)), D + 2 * pad), \
                (ai.block(M * (D + pad)), D + pad)
            f["o"] = (ao.block(L * B * (D + 2 * pad)), D + 2 * pad)
        self._built = (torch.randn(ai.n, generator=rng), torch.randn(ao.n, generator=rng), f)
        self._check_extents(ai.n, ao.n)
        return self._built

    def _check_extents(self, n_in, n_out):
        """no pointer the entry points get reaches past its arena (the kernels are handed raw addresses)"""
        f, M, D, BHL = self._built[2], self.B * self.L, self.D, self.B * self.H * self.L
        last = lambda off, rows, ld, width: off + (rows - 1) * ld + width
        if self.kind == "attn":
            assert all(last(f[n][0], M, f[n][1], D) <= n_in for n in ("q", "k", "v", "d_o"))
            assert all(last(f[n][0], M, f[n][1], D) <= n_out for n in ("o", "dq", "dk", "dv"))
            assert f["lse"] + BHL <= n_out and f["dvec"] + BHL <= n_out
            assert not self.probs or f["probs"] + self.H * self.B * self.L * self.L <= n_out
        elif self.kind == "pnca":
            assert last(f["qkv"], M, 3 * D, 3 * D) <= n_in and last(f["hkv"], M, f["ldh"], 2 * D) <= n_in
            assert all(f[n] + M * D <= n_in for n in ("d_ox", "d_oh")) and all(f[n] + M * D <= n_out for n in ("ox", "oh", "dqh"))
            assert f["dqkv"] + M * 3 * D <= n_out and f["dhkv"] + M * 2 * D <= n_out
            assert f["lse_x"] + BHL <= n_out and f["lse_h"] + BHL <= n_out
        else:
            assert last(f["q"][0], self.L * self.B, f["q"][1], D) <= n_in and last(f["o"][0], self.L * self.B, f["o"][1], D) <= n_out
            assert all(last(f[n][0], M, f[n][1], D) <= n_in for n in ("k", "v"))

    def band(self, which=None, step=None):
        """the interpreter's problem(s): an attention call, band 'x' / 'h' of a PNCA call, or one decode step"""
        inp, _, f = self.built()
        bw = self.bw if self.bw_dev is None else self.bw_dev
        pr = dict(mem=inp.numpy(), B=self.B, H=self.H, L=self.L, lens=self.lens, drop_p=self.drop_p, probs=self.probs)
        sd = self.seed_dev or 0
        if self.kind == "attn":
            pr.update(q=f["q"], k=f["k"], v=f["v"], d_o=f["d_o"] if self.bwd else None, mode=self.mode, bw=bw,
                      seed=self.seed + sd)
        elif self.kind == "pnca":
            D = self.D
            pr.update(q=(f["qkv"], 3 * D), probs=False)
            if which == "x":
                pr.update(k=(f["qkv"] + D, 3 * D), v=(f["qkv"] + 2 * D, 3 * D), d_o=(f["d_ox"], D), mode=1,
                          bw=self.bw_x if self.bw_dev is None else self.bw_dev, seed=self.seed + sd)
            else:
                pr.update(k=(f["hkv"], f["ldh"]), v=(f["hkv"] + D, f["ldh"]), d_o=(f["d_oh"], D), mode=2,
                          bw=self.bw_h if self.bw_dev is None else self.bw_dev, seed=self.seed_h + sd)
            if not self.bwd:
                pr["d_o"] = None
        else:
            pr.update(q=(f["q"][0] + step * self.B * f["q"][1], f["q"][1]), k=f["k"], v=f["v"], mode=self.mode, step=step,
                      bw=self.bw if self.bw_seq is None else self.bw_seq, drop_p=0.0, seed=0)
        return pr

    def problems(self):
        if self.kind == "attn":
            return {"": self.band()}
        if self.kind == "pnca":
            return {"x": self.band("x"), "h": self.band("h")}
        return {step: self.band(step=step) for step in range(self.L)}

    def reference(self):
        """computed once and shared by every leg"""
        if self._ref is None:
            self._ref = {key: _evaluate(pr) for key, pr in self.problems().items()}
        return self._ref


def _attn_cases():
    """every sequence length of the seams x every mode, the other features dealt round; then the features crossed at two
    short lengths (13: one round of 64 queries, fewer keys than lanes for some sequences; 70: two rounds)"""
    small, mid, large = [], [], []
    for iL, L in enumerate((1, 3, 5, 63, 64, 65, 129, 256, 257, 390, 391, 409, 410)):
        for mode in (0, 1, 2):
            n = iL + mode
            B, H = ((3, 3) if L <= 129 else (2, 2)) if iL % 2 == 0 else ((3, 2) if L <= 129 else (2, 3 if L < 390 else 2))
            bw = (0, 3, L + 5)[(iL + 2 * mode) % 3]
            c = _Case("attn_L%d_mode%d" % (L, mode), "attn", B=B, H=H, L=L, mode=mode, bw=bw,
                      lens=_lens(("none", "ragged", "zero")[n % 3], B, L), drop_p=(0.0, 0.1)[n % 2], seed=1000 + n,
                      seed_dev=77 if iL % 2 or L == 410 else None, layout=("packed", "fused", "guard")[(n + 1) % 3],
                      probs=L in (1, 5, 64, 257), acc=(iL + mode // 2) % 2, bw_dev=None if (iL + mode) % 4 else bw)
            if c.bw_dev is not None:
                c.bw = 1 if bw != 1 else 2  # a deliberately wrong host value: the device word decides
            (small if L <= 129 else mid if L <= 257 else large).append(c)
    feats = []
    n = 0
    for L in (13, 70):
        for mode in (0, 1, 2):
            for pat in ("none", "ragged", "zero"):
                for probs in (False, True):
                    n += 1
                    bw = (0, 3, L + 5)[n % 3]
                    feats.append(_Case("feat_L%d_mode%d_%s_%s" % (L, mode, pat, "probs" if probs else "noprobs"), "attn", B=3,
                                       H=(3, 2)[n % 2], L=L, mode=mode, bw=1 if n % 5 == 0 else bw, bw_dev=bw if n % 5 == 0 else None,
                                       lens=_lens(pat, 3, L), drop_p=(0.1, 0.0)[(n // 2) % 2], seed=n, seed_dev=(5, None)[(n // 3) % 2],
                                       layout=("guard", "packed", "fused")[n % 3], probs=probs, acc=(n // 2) % 2))
    return {"attn_small": small, "attn_mid": mid, "attn_large": large, "attn_features": feats}


def _pnca_cases():
    small, mid, large = [], [], []
    for iL, L in enumerate((1, 3, 5, 63, 64, 65, 129, 256, 257, 390, 391, 409, 410)):
        B, H = (3, 3 if iL % 2 == 0 else 2) if L <= 129 else (2, 2)
        bws = ((3, 5), (0, L + 5), (L + 5, 0), (5, 3))[iL % 4]
        c = _Case("pnca_L%d" % L, "pnca", B=B, H=H, L=L, bw_x=bws[0], bw_h=bws[1], bwd=L <= 391,
                  lens=_lens(("ragged", "zero", "none")[iL % 3], B, L), drop_p=(0.1, 0.0)[iL % 2], seed=31 + iL, seed_h=977 + iL,
                  seed_dev=(None, 9)[(iL // 2) % 2], ldh_extra=(0, 8)[iL % 2], dqh_null=iL % 2 == 0,
                  bw_dev=4 if iL % 5 == 2 else None)
        (small if L <= 129 else mid if L <= 257 else large).append(c)
    # the same dropout seed for both bands would hide swapped seeds: every case above has seed_x != seed_h
    small.append(_Case("pnca_L37_drop", "pnca", B=3, H=3, L=37, bw_x=2, bw_h=6, lens=[37, 23, 0], drop_p=0.1, seed=5, seed_h=6,
                       seed_dev=3, ldh_extra=8))
    # dropout with a device seed word on the four-role backward (the loop above gives it to the three-role one)
    mid.append(_Case("pnca_L300_drop", "pnca", B=2, H=2, L=300, bw_x=4, bw_h=2, lens=[211, 300], drop_p=0.1, seed=8, seed_h=9,
                     seed_dev=11))
    return {"pnca_small": small, "pnca_mid": mid, "pnca_large": large}


def _decode_cases():
    c = []
    for mode in (0, 1, 2):
        c.append(_Case("decode_mode%d" % mode, "decode", B=3, H=3, L=9, mode=mode, bw=2, lens=[9, 4, 0], layout="guard"))
        c.append(_Case("decode_mode%d_bwseq" % mode, "decode", B=3, H=2, L=9, mode=mode, bw=100, bw_seq=[0, 2, 14],
                       lens=[5, 9, 1]))
        c.append(_Case("decode_mode%d_nolens" % mode, "decode", B=2, H=3, L=9, mode=mode, bw=(0, 3, 14)[mode]))
    return {"decode": c}


def _build_table():
    table = {}
    for part in (_attn_cases(), _pnca_cases(), _decode_cases()):
        table.update(part)
    names = [c.name for cs in table.values() for c in cs]
    assert len(set(names)) == len(names)
    return table


_TABLE = _build_table()
_GROUPS = list(_TABLE)
_PAIRS = (("o", "S_o"), ("dq", "S_dq"), ("dk", "S_dk"), ("dv", "S_dv"))
_MEASURED = {}


def _c():
    """c = 4 x the worst ratio of (float32, reversed sums) - (float64) to 2^-24 * S over the whole table"""
    if not _MEASURED:
        worst, where = 0.0, None
        for cases in _TABLE.values():
            for case in cases:
                ref = case.reference()
                low = {key: _evaluate(pr, np.float32, reverse=True) for key, pr in case.problems().items()}
                pairs = [(low[key][n].astype(np.float64), ref[key][n], ref[key][s]) for key in ref for n, s in _PAIRS if n in ref[key]]
                if case.kind == "pnca" and case.bwd:  # the summed query gradient of the two bands
                    pairs.append((low["x"]["dq"].astype(np.float64) + low["h"]["dq"], ref["x"]["dq"] + ref["h"]["dq"],
                                  ref["x"]["S_dq"] + ref["h"]["S_dq"]))
                for got, want, S in pairs:
                    ok = S > 0
                    if ok.any():
                        ratio = float((np.abs(got - want)[ok] / (U * S[ok])).max())
                        if ratio > worst:
                            worst, where = ratio, case.name
        _MEASURED.update(ratio=worst, c=4.0 * worst, case=where)
        _record("fp32_reference", {"max_ratio_to_2^-24_S": worst, "c": 4.0 * worst, "case": where})
    return _MEASURED["c"]


# ---------------------------------------------------------------------------------------------------------------------
# 3. back ends
class _Leg:
    def __init__(self, name):
        self.name = name
        self.device = "cuda" if name == "gpu" else "cpu"
        self.R = 2.0 if name == "gpu" else 1.0
        self.has_plan = name != "emu"

    def context(self):
        return {"emu": util.emulation, "src": util.kernel_source_on_cpu, "gpu": contextlib.nullcontext}[self.name]()


def _leg_params():
    return [pytest.param("emu", id="emu"),
            pytest.param("src", id="src", marks=pytest.mark.skipif(not _HAVE_CLANG, reason="ROCm clang not installed")),
            pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]


def _plan_legs():
    return _leg_params()[1:]


class _Mem:
    """a case's buffers on the leg's device: p(off) = pointer to element ``off`` of the input / output arena"""

    def __init__(self, case, leg):
        import kantts._hip as hip

        inp, out0, self.f = case.built()
        self.inp, self.out = inp.clone().to(leg.device), out0.clone().to(leg.device)
        self.out0 = out0.numpy()
        self.device = leg.device
        i32 = lambda v: None if v is None else torch.tensor(v, dtype=torch.int32).reshape(-1).to(leg.device)
        self.lens, self.bw_dev, self.bw_seq = i32(case.lens), i32(case.bw_dev), i32(case.bw_seq)
        self.seed_dev = None if case.seed_dev is None else torch.tensor([case.seed_dev], dtype=torch.int64).to(leg.device)
        self._in, self._out = hip.ptr(self.inp, torch.float32), hip.ptr(self.out, torch.float32)
        self.ptr = hip.ptr

    def i(self, off):
        return self._in + 4 * int(off)

    def o(self, off):
        return None if off is None else self._out + 4 * int(off)

    def sync(self):
        if self.device == "cuda":
            torch.cuda.synchronize()

    def result(self):
        self.sync()
        return self.out.cpu().numpy()


_WORST = {}


def _note(leg, path, ratio, rel):
    w = _WORST.setdefault((leg, path), [0.0, 0.0])
    w[0], w[1] = max(w[0], ratio), max(w[1], rel)


def _flush():
    """the worst figures so far into the report, in one rewrite of the file"""
    try:
        os.makedirs(os.path.dirname(_REPORT), exist_ok=True)
        d = json.load(open(_REPORT)) if os.path.exists(_REPORT) else {}
        for (leg, path), w in _WORST.items():
            d["%s%s_%s" % (leg, _SWITCHES, path)] = {"max_ratio_to_bound": w[0], "max_rel_l2": w[1],
                                                     "R": 2.0 if leg == "gpu" else 1.0, "c": _c()}
        json.dump(d, open(_REPORT, "w"), indent=1)
    except (OSError, ValueError):
        pass


class _Checker:
    """compares the output arena after the calls with the reference, region by region; what no region covers is a guard"""

    def __init__(self, case, leg, mem):
        self.case, self.leg, self.raw, self.raw0 = case, leg, mem.result(), mem.out0
        self.got, self.init = self.raw.astype(np.float64), self.raw0.astype(np.float64)
        self.covered = np.zeros(self.got.size, dtype=bool)

    def region(self, what, path, idx, ref, S=None, cap=None, rel_cap=None, accumulate=False):
        case, leg = self.case, self.leg
        assert not self.covered[idx].any(), "%s %s: regions overlap" % (case.name, what)
        self.covered[idx] = True
        got, base = self.got[idx], (self.init[idx] if accumulate else 0.0)
        want = ref + base
        err = np.abs(got - want)
        rel = float(np.linalg.norm((got - base) - ref) / (np.linalg.norm(ref) + 1e-30))
        ratio = 0.0
        if S is None:  # probs, lse: exactly 0 where the reference is (outside [lo, hi], dropped, skipped rows)
            exact = ref == 0
        else:
            exact = S == 0
            if (~exact).any():
                ratio = float((err[~exact] / (U * (S + np.abs(base))[~exact])).max()) / _c()
        assert np.array_equal(got[exact], want[exact]), "%s %s: an element that must be exact is not" % (case.name, what)
        print("%s%s %s %s [%s]: max |err| %.3e, rel-L2 %.3e, ratio to c*2^-24*S %.4f (c = %.3f)" % (
            leg.name, _SWITCHES, case.name, what, path, float(err.max()) if err.size else 0.0, rel, ratio, _c()))
        # (a single-key interval has dq = dk = 0 exactly, as a difference of two equal terms: the float64 reference is
        #  then its own rounding error, and a norm relative to it says nothing.  Nothing else is exempt.)
        cancelled = S is not None and np.linalg.norm(ref) <= CANCELLED * np.linalg.norm(S)
        if S is not None:
            _note(leg.name, path, ratio, 0.0 if cancelled else rel)  # (the context's rel-L2 is recorded, not capped)
        if cap is not None:
            assert err.size == 0 or float(err.max()) <= cap, "%s %s: max |err| %.3e > %.1e" % (case.name, what, float(err.max()), cap)
        if rel_cap is not None and not cancelled:
            assert rel <= rel_cap, "%s %s: rel-L2 %.3e" % (case.name, what, rel)
        if S is not None:
            assert ratio <= leg.R, "%s %s: error %.3f x the bound c*2^-24*S (R = %g)" % (case.name, what, ratio, leg.R)

    def scratch(self, off, n):
        self.covered[off:off + n] = True

    def guards(self):
        same = self.raw.view(np.uint32)[~self.covered] == self.raw0.view(np.uint32)[~self.covered]
        assert same.all(), "%s: %d elements outside the outputs were written" % (self.case.name, int((~same).sum()))


def _plan(case, leg, which):
    """the plan of this case's pass, asserted against the path the case expects (no plan on the emulated ABI)"""
    import kantts._hip as hip

    want = case.expect[which]
    if leg.has_plan:
        got = hip.attn_plan(case.L, case.mode, which)
        assert got == want, "%s %s: plan %s, expected %s" % (case.name, which, got, want)
        assert not (_NO_QUAD and "quad" in got) and not (_NO_DQ2 and "dq2" in got), (case.name, got)
    return want


def _run_attn(case, leg):
    import kantts._hip as hip

    L_, m = hip.lib(), _Mem(case, leg)
    f, B, H, L, D = m.f, case.B, case.H, case.L, case.D
    ref = case.reference()[""]
    fpath, bpath = _plan(case, leg, "fwd"), _plan(case, leg, "bwd")
    (q, ldq), (k, ldk), (v, ldv), (o, ldo) = f["q"], f["k"], f["v"], f["o"]
    rc = L_.kantts_attn_fwd(m.i(q), m.i(k), m.i(v), ldq, ldk, ldv, m.o(o), ldo, m.o(f["lse"]), m.o(f.get("probs")),
                            m.ptr(m.lens), m.ptr(m.bw_dev), case.bw, B, H, L, DH, case.mode, case.drop_p, case.seed,
                            m.ptr(m.seed_dev), hip.stream())
    assert rc == 0, (case.name, rc)
    if case.bwd:  # reads the o and lse this leg's forward just wrote
        (go, lddo), (dq, lddq), (dk, lddk), (dv, lddv) = f["d_o"], f["dq"], f["dk"], f["dv"]
        rc = L_.kantts_attn_bwd(m.i(q), m.i(k), m.i(v), ldq, ldk, ldv, m.o(o), ldo, m.i(go), lddo, m.o(f["lse"]),
                                m.o(f["dvec"]), m.o(dq), m.o(dk), m.o(dv), lddq, lddk, lddv, case.acc, m.ptr(m.lens),
                                m.ptr(m.bw_dev), case.bw, B, H, L, DH, case.mode, case.drop_p, case.seed, m.ptr(m.seed_dev),
                                hip.stream())
        assert rc == 0, (case.name, rc)
    ck = _Checker(case, leg, m)
    ck.region("context", fpath, _rows(ck.got, o, ldo, B, L, H), ref["o"], ref["S_o"], cap=CAP_CTX)
    ck.region("lse", fpath, f["lse"] + np.arange(B * H * L).reshape(B, H, L), ref["lse"], cap=CAP_LSE)
    if case.probs:
        ck.region("probs", fpath, f["probs"] + np.arange(H * B * L * L).reshape(H, B, L, L), ref["probs"], cap=CAP_PROBS)
    if case.bwd:
        ck.scratch(f["dvec"], B * H * L)
        ck.region("dq", bpath, _rows(ck.got, dq, lddq, B, L, H), ref["dq"], ref["S_dq"], rel_cap=CAP_GRAD_REL, accumulate=bool(case.acc))
        ck.region("dk", bpath, _rows(ck.got, dk, lddk, B, L, H), ref["dk"], ref["S_dk"], rel_cap=CAP_GRAD_REL)
        ck.region("dv", bpath, _rows(ck.got, dv, lddv, B, L, H), ref["dv"], ref["S_dv"], rel_cap=CAP_GRAD_REL)
    ck.guards()


def _pnca_fwd(L_, m, case, d_head=DH):
    import kantts._hip as hip

    f = m.f
    return L_.kantts_pnca_attn_fwd(m.i(f["qkv"]), m.i(f["hkv"]), f["ldh"], m.o(f["ox"]), m.o(f["oh"]), m.o(f["lse_x"]),
                                   m.o(f["lse_h"]), m.ptr(m.lens), m.ptr(m.bw_dev), case.bw_x, case.bw_h, case.B, case.H, case.L,
                                   d_head, case.drop_p, case.seed, case.seed_h, m.ptr(m.seed_dev), hip.stream())


def _pnca_bwd(L_, m, case, dqh, d_head=DH):
    import kantts._hip as hip

    f = m.f
    return L_.kantts_pnca_attn_bwd(m.i(f["qkv"]), m.i(f["hkv"]), f["ldh"], m.o(f["ox"]), m.o(f["oh"]), m.i(f["d_ox"]),
                                   m.i(f["d_oh"]), m.o(f["lse_x"]), m.o(f["lse_h"]), m.o(f["dqkv"]), m.o(dqh), m.o(f["dhkv"]),
                                   m.ptr(m.lens), m.ptr(m.bw_dev), case.bw_x, case.bw_h, case.B, case.H, case.L, d_head,
                                   case.drop_p, case.seed, case.seed_h, m.ptr(m.seed_dev), hip.stream())


def _run_pnca(case, leg):
    import kantts._hip as hip

    L_, m = hip.lib(), _Mem(case, leg)
    f, B, H, L, D = m.f, case.B, case.H, case.L, case.D
    fpath, bpath = _plan(case, leg, "pnca_fwd"), _plan(case, leg, "pnca_bwd")
    if not leg.has_plan and fpath == "unsupported":
        return  # the emulated ABI has no kernels, hence no refusals
    rc = _pnca_fwd(L_, m, case)
    if fpath == "unsupported":  # L >= 410: refused, nothing written
        assert rc == E_UNSUPPORTED, (case.name, rc)
        _Checker(case, leg, m).guards()
        return
    assert rc == 0, (case.name, rc)
    ref = case.reference()
    x, h = ref["x"], ref["h"]
    split = None
    if case.bwd and (leg.has_plan or bpath != "unsupported"):  # (no refusals on the emulated ABI: forward only)
        dq2 = bpath == "pnca_bwd_dq2"
        rc = _pnca_bwd(L_, m, case, None if (case.dqh_null and dq2) else f["dqh"])
        if bpath == "unsupported":  # L >= 391: refused, the gradients untouched
            assert rc == E_UNSUPPORTED, (case.name, rc)
        elif leg.has_plan:
            assert rc == (0 if dq2 else 1), "%s: return code %d on path %s" % (case.name, rc, bpath)
        else:
            assert rc in (0, 1), (case.name, rc)
        split = None if bpath == "unsupported" else rc == 1
    ck = _Checker(case, leg, m)
    ck.region("x context", fpath, _rows(ck.got, f["ox"], D, B, L, H), x["o"], x["S_o"], cap=CAP_CTX)
    ck.region("h context", fpath, _rows(ck.got, f["oh"], D, B, L, H), h["o"], h["S_o"], cap=CAP_CTX)
    lse_idx = np.arange(B * H * L).reshape(B, H, L)
    ck.region("x lse", fpath, f["lse_x"] + lse_idx, x["lse"], cap=CAP_LSE)
    ck.region("h lse", fpath, f["lse_h"] + lse_idx, h["lse"], cap=CAP_LSE)
    if split is not None:
        kw = dict(rel_cap=CAP_GRAD_REL)
        if split:  # the bands' query gradients side by side
            ck.region("dq x", bpath, _rows(ck.got, f["dqkv"], 3 * D, B, L, H), x["dq"], x["S_dq"], **kw)
            ck.region("dq h", bpath, _rows(ck.got, f["dqh"], D, B, L, H), h["dq"], h["S_dq"], **kw)
        else:      # summed; dqh keeps its sentinel (checked with the guards)
            ck.region("dq", bpath, _rows(ck.got, f["dqkv"], 3 * D, B, L, H), x["dq"] + h["dq"], x["S_dq"] + h["S_dq"], **kw)
        ck.region("dk x", bpath, _rows(ck.got, f["dqkv"] + D, 3 * D, B, L, H), x["dk"], x["S_dk"], **kw)
        ck.region("dv x", bpath, _rows(ck.got, f["dqkv"] + 2 * D, 3 * D, B, L, H), x["dv"], x["S_dv"], **kw)
        ck.region("dk h", bpath, _rows(ck.got, f["dhkv"], 2 * D, B, L, H), h["dk"], h["S_dk"], **kw)
        ck.region("dv h", bpath, _rows(ck.got, f["dhkv"] + D, 2 * D, B, L, H), h["dv"], h["S_dv"], **kw)
    ck.guards()


def _decode(L_, m, case, step, d_head=DH, block=None, ld_add=(0, 0, 0, 0)):
    """step ``step`` on the q / o row block ``block`` (default: the step's own); ``ld_add``: added to ldq, ldk, ldv, ldo"""
    import kantts._hip as hip

    f, B = m.f, case.B
    (q, ldq), (k, ldk), (v, ldv), (o, ldo) = f["q"], f["k"], f["v"], f["o"]
    block = step if block is None else block
    assert 0 <= block < case.L
    aq, ak, av, ao = ld_add
    return L_.kantts_attn_decode(m.i(q + block * B * ldq), m.i(k), m.i(v), ldq + aq, ldk + ak, ldv + av,
                                 m.o(o + block * B * ldo), ldo + ao,
                                 m.ptr(m.lens), m.ptr(m.bw_seq), B, case.H, case.L, d_head, case.mode, step, case.bw, hip.stream())


def _run_decode(case, leg):
    import kantts._hip as hip

    L_, m = hip.lib(), _Mem(case, leg)
    for step in range(case.L):
        assert _decode(L_, m, case, step) == 0, (case.name, step)
    ck = _Checker(case, leg, m)
    o, ldo = m.f["o"]
    for step, r in case.reference().items():
        ck.region("context of step %d" % step, "decode", _rows(ck.got, o + step * case.B * ldo, ldo, case.B, 1, case.H), r["o"],
                  r["S_o"], cap=CAP_CTX)
    ck.guards()


@pytest.mark.parametrize("group", _GROUPS)
@pytest.mark.parametrize("leg", _leg_params())
def test_attn_matches_the_fp64_interpreter(leg, group):
    leg = _Leg(leg)
    try:
        with leg.context():
            for case in _TABLE[group]:
                {"attn": _run_attn, "pnca": _run_pnca, "decode": _run_decode}[case.kind](case, leg)
    finally:
        _flush()


def test_c_comes_from_the_fp32_evaluation_of_the_reference():
    """the measured ratio and c (recorded in attn_contract.json).  The ratio is pinned to the one recorded when the table
    was written: a case added later that is worse conditioned would otherwise loosen the bound of every other case"""
    c = _c()
    print("fp32 reference: worst ratio to 2^-24*S %.4f (%s), c = %.4f" % (_MEASURED["ratio"], _MEASURED["case"], c))
    assert c == 4.0 * _MEASURED["ratio"]
    assert 1.0 < _MEASURED["ratio"] <= 1.1 * RATIO_RECORDED, _MEASURED


@pytest.mark.parametrize("leg", _plan_legs())
def test_table_reaches_every_path(leg):
    """the union of kantts_attn_plan over the table: three forward, three backward, the PNCA forward, both PNCA backward
    forms and both PNCA refusals; decode has one kernel and its own group"""
    import kantts._hip as hip

    if _NO_QUAD or _NO_DQ2:
        pytest.skip("KANTTS_ATTN_NO_QUAD / KANTTS_ATTN_NO_DQ2 is set: the quad / dq2 paths are switched off")
    leg = _Leg(leg)
    seen = set()
    with leg.context():
        for cases in _TABLE.values():
            for case in cases:
                for which in case.expect:
                    seen.add((which, hip.attn_plan(case.L, case.mode, which)))
        assert hip.lib().kantts_attn_plan(5, 3, 0) == E_BADARG and hip.lib().kantts_attn_plan(5, 0, 4) == E_BADARG
        assert hip.lib().kantts_attn_plan(-1, 0, 0) == E_BADARG
    want = {("fwd", "fwd_lds_quad"), ("fwd", "fwd_lds"), ("fwd", "fwd_direct"), ("bwd", "bwd_lds_quad"), ("bwd", "bwd_lds"),
            ("bwd", "bwd_direct"), ("pnca_fwd", "pnca_fwd_lds"), ("pnca_fwd", "unsupported"), ("pnca_bwd", "pnca_bwd_dq2"),
            ("pnca_bwd", "pnca_bwd_split"), ("pnca_bwd", "unsupported")}
    assert seen == want, sorted(want ^ seen)
    assert any(c.kind == "decode" for c in _TABLE["decode"])
    _record("%s_paths" % leg.name, sorted("%s:%s" % p for p in seen))


def test_every_path_has_a_dropout_case_with_a_device_seed_word():
    cases = [c for cs in _TABLE.values() for c in cs if c.kind != "decode" and c.drop_p > 0 and c.seed_dev]
    seen = {p for c in cases for which, p in c.expect.items() if c.bwd or which in ("fwd", "pnca_fwd")}
    want = {_expected(w, L, mode) for w in ("fwd", "bwd", "pnca_fwd", "pnca_bwd") for L in (5, 257, 390, 410) for mode in (0, 1)}
    assert seen >= want - {"unsupported"}, sorted(want - seen)


# ---------------------------------------------------------------------------------------------------------------------
# 4. refusals
@pytest.mark.parametrize("leg", _plan_legs())
def test_refusals(leg):
    """each returns its code and writes nothing"""
    import kantts._hip as hip

    leg = _Leg(leg)
    with leg.context():
        L_ = hip.lib()
        case = _Case("refusal_attn", "attn", L=7, layout="guard")
        f = case.built()[2]
        (q, ldq), (k, ldk), (v, ldv), (o, ldo) = f["q"], f["k"], f["v"], f["o"]
        (go, lddo), (dq, lddq), (dk, lddk), (dv, lddv) = f["d_o"], f["dq"], f["dk"], f["dv"]

        def fwd(m, d_head=DH, **ld):
            g = dict(dict(ldq=ldq, ldk=ldk, ldv=ldv, ldo=ldo), **ld)
            return L_.kantts_attn_fwd(m.i(q), m.i(k), m.i(v), g["ldq"], g["ldk"], g["ldv"], m.o(o), g["ldo"], m.o(f["lse"]), None,
                                      None, None, 3, case.B, case.H, case.L, d_head, 1, 0.0, 0, None, hip.stream())

        def bwd(m, d_head=DH, **ld):
            g = dict(dict(ldq=ldq, ldk=ldk, ldv=ldv, ldo=ldo, lddo=lddo, lddq=lddq, lddk=lddk, lddv=lddv), **ld)
            return L_.kantts_attn_bwd(m.i(q), m.i(k), m.i(v), g["ldq"], g["ldk"], g["ldv"], m.o(o), g["ldo"], m.i(go), g["lddo"],
                                      m.o(f["lse"]), m.o(f["dvec"]), m.o(dq), m.o(dk), m.o(dv), g["lddq"], g["lddk"], g["lddv"],
                                      0, None, None, 3, case.B, case.H, case.L, d_head, 1, 0.0, 0, None, hip.stream())

        calls = [("fwd d_head 8", case, lambda m: fwd(m, d_head=8), E_UNSUPPORTED),
                 ("bwd d_head 8", case, lambda m: bwd(m, d_head=8), E_UNSUPPORTED)]
        for n in ("ldq", "ldk", "ldv", "ldo"):
            calls.append(("fwd %s %% 4" % n, case, lambda m, n=n: fwd(m, **{n: case.D + 2}), E_BADARG))
        for n in ("ldq", "ldk", "ldv", "ldo", "lddo", "lddq", "lddk", "lddv"):
            calls.append(("bwd %s %% 4" % n, case, lambda m, n=n: bwd(m, **{n: case.D + 2}), E_BADARG))
        pn = _Case("refusal_pnca", "pnca", L=7)
        calls += [("pnca fwd d_head 8", pn, lambda m: _pnca_fwd(L_, m, pn, d_head=8), E_UNSUPPORTED),
                  ("pnca bwd d_head 8", pn, lambda m: _pnca_bwd(L_, m, pn, pn.built()[2]["dqh"], d_head=8), E_UNSUPPORTED)]
        for L, call, name in ((410, lambda m, c: _pnca_fwd(L_, m, c), "pnca fwd L 410"),
                              (391, lambda m, c: _pnca_bwd(L_, m, c, c.built()[2]["dqh"]), "pnca bwd L 391")):
            big = _Case("refusal_pnca_L%d" % L, "pnca", B=2, H=2, L=L)
            calls.append((name, big, lambda m, call=call, big=big: call(m, big), E_UNSUPPORTED))
        dec = _Case("refusal_decode", "decode", L=9, mode=1)
        calls += [("decode step L", dec, None, E_BADARG),
                  ("decode d_head 8", dec, lambda m: _decode(L_, m, dec, 0, d_head=8), E_UNSUPPORTED)]
        for n in range(4):
            calls.append(("decode %s %% 4" % ("ldq", "ldk", "ldv", "ldo")[n], dec,
                          lambda m, n=n: _decode(L_, m, dec, 0, ld_add=tuple(2 * (k == n) for k in range(4))), E_BADARG))
        for name, c, call, code in calls:
            m = _Mem(c, leg)
            if name == "decode step L":  # the last valid step first (it writes its rows), then step = L on the same buffers
                assert _decode(L_, m, c, c.L - 1) == 0
                before = m.result().copy()
                rc = _decode(L_, m, c, c.L, block=c.L - 1)
            else:
                before = m.result().copy()
                rc = call(m)
            assert rc == code, "%s: return code %d, expected %d" % (name, rc, code)
            assert np.array_equal(m.result().view(np.uint32), before.view(np.uint32)), "%s: a refused call wrote" % name


# ---------------------------------------------------------------------------------------------------------------------
# 5. the per-process switches: the launchers read them once, so each setting gets a fresh child process
def _child(leg, **switches):
    """this file's ``leg`` again under the switches, without the L >= 390 groups; the parent reads the result only"""
    env = dict(os.environ, **switches)
    keep = "test_attn_matches_the_fp64_interpreter and %s and not large" % leg
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-k", keep],
                       env=env, capture_output=True, text=True, timeout=240,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]


@pytest.mark.skipif(not _HAVE_CLANG, reason="ROCm clang not installed")
def test_non_quad_and_split_paths_in_a_fresh_process():
    """KANTTS_ATTN_NO_QUAD sends mode 0 to the one-thread-per-query LDS bodies, KANTTS_ATTN_NO_DQ2 every PNCA backward to the
    four-role launch (return code 1 at L <= 256 too): the plan never reports a quad or dq2 path there"""
    _child("src", KANTTS_ATTN_NO_QUAD="1", KANTTS_ATTN_NO_DQ2="1")


@pytest.mark.skipif(not _HAVE_CLANG, reason="ROCm clang not installed")
def test_head_major_grid_in_a_fresh_process():
    _child("src", KANTTS_ATTN_HEAD_MAJOR="1")


@pytest.mark.gpu
def test_non_quad_and_split_paths_in_a_fresh_process_gpu():
    _child("gpu", KANTTS_ATTN_NO_QUAD="1", KANTTS_ATTN_NO_DQ2="1")


@pytest.mark.gpu
def test_head_major_grid_in_a_fresh_process_gpu():
    _child("gpu", KANTTS_ATTN_HEAD_MAJOR="1")
