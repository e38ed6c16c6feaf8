"""The kernels that close a training step -- the loss reductions, the gradient norm, the clip scale, Adam and the weight-norm
reparametrisation -- against an fp64 interpreter of their contract (include/kantts_hip.h).

``_evaluate`` (the ``_op_*`` functions) is written from the header alone -- not from oracle/cabi_numpy.py, not from the kernels -- and addresses ONE flat
arena as the ABI does: element offsets, the strides rs / cs / ks, the offsets of a kantts_wn_desc table.  The arena carries
guard elements before the first block and after every block; what a strided layout leaves between rows is guard too.  int64
lengths / targets, bf16 images and descriptor tables live in the same arena (viewed as int64 / uint16 / bytes).  One table of
cases (``_TABLE``) runs through the C ABI on three legs: the emulated ABI, the kernel sources on the CPU, and the device.
Every case names the branches it is there for (``_BRANCHES``); a module-level test asserts that each branch has a case.

Exactly, on every leg:
  * every element no call of the case writes is bit-identical afterwards (guards, inputs, a NULL gradient's neighbours, the
    accumulators of calls that return early); return codes;
  * kantts_scale_many: float32(float64(x) * float64(s));
  * the sign and zero pattern of every L1 gradient; its magnitude is ONE value, ``inv`` or ``scale``: the float32 chain
    1 / (f32(rows) * f32(C)) bit for bit on the emulated ABI and the kernel sources, within one ulp on the device, and exact
    on every leg when the denominator is a power of two;  mode-1 gradients of kantts_elem_loss equal
    fl(fl(2 * scale) * fl(a - target));
  * exact sums: with inputs from {+-0.5, +-1}, sum(rows) * C and every scale a power of two, every partial sum in any order
    is representable (the case builder asserts the total stays below 2^24 units), so kantts_sumsq, kantts_sumsq_det, every
    L1 loss, component and total and kantts_elem_loss equal the fp64 value bit for bit.  This class alone carries the large
    sizes of the grid-stride seams: a dropped, doubled or mis-masked element moves the result by at least one unit;
  * bf16 images: wf is the round-to-nearest-even bf16 of the w THE SAME LAUNCH wrote, wd the header's permutation of it; the
    table equals the per-layer call bit for bit;  kantts_sumsq_det gives the same bits twice, also with a call of another
    n on the same workspace in between, and leaves the ticket word 0 after every call;
  * a zero row of v: NaN in that row's outputs and nowhere else.
Measured, per element: |got - ref| <= R * c * 2^-24 * S with S = the interpreter's expression over absolute values (sums:
sum |term|; Adam m': |b1 m| + |(1 - b1) g'|, v' alike (|g'| = |clip g| + |wd p|: under weight decay its two terms may cancel), p': |p| + |delta| with the m' inside delta replaced by its S (the two terms
of m' may cancel; delta = m' where they do not), under dyn_lr_step + |delta| (k1 + k2 / 2) with
k = beta^t / (1 - beta^t): the bias corrections are formed in float32 and cancel; weight norm w: |w|, dg: sum |dw v| / ||v||,
dv: |g / ||v||| (|dw| + |v| S_dg / ||v||)).  R = 1 on the emulated ABI and the kernel sources, 2 on the device.  c is not
chosen: the interpreter is evaluated again in numpy float32 with every sum strictly left-to-right and right-to-left
(np.cumsum); ``ratio`` is its largest distance from the float64 evaluation in units of 2^-24 * S over the whole table and
c = 4 * ratio (tree-shaped block sums, FMA contraction, the device's logf / powf).  Measured when this file was written:
ratio = 25.80 (det_same_bits), c = 103.2; the test measures it again in every session, uses what it measures and refuses a
ratio more than 10 % above the recorded one.  Real-valued sums stay at n <= 8193 so that a sequential float32 sum is a tight
yardstick.  The project's caps hold as well: loss values 2e-5 relative, Adam parameters 1e-6 absolute.
The measured ratio, c and the worst ratio to the bound per leg and entry point go to step_tail_contract.json beside
gemm_contract.json.
"""
import contextlib
import ctypes
import json
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import test_bench_config_parity as _bench_parity
import util

_REPORT = os.path.join(os.path.dirname(_bench_parity._REPORT), "step_tail_contract.json")
_HAVE_CLANG = os.path.exists(os.environ.get("HIPEMU_CXX", "/opt/rocm/lib/llvm/bin/clang++"))
OK, E_BADARG, E_WORKSPACE = 0, -1, -3
U = 2.0 ** -24
CAP_LOSS_REL, CAP_ADAM_ABS = 2e-5, 1e-6  # tests/test_gpu_ops.py
RATIO_RECORDED = 25.80                   # the float32 evaluation of the reference, see above
F32, F64 = np.float32, np.float64
LOSS_MAX_TERMS, ELOSS_MAX_TERMS, WN_BWD_MAX, DET_WS = 5, 64, 64, 1025
_KEEP = 1 << 18                         # arenas up to this many floats, and their references, are kept for the other legs

_BRANCHES = [
    # masked_l1 / _many
    "l1:C=1", "l1:C=3", "l1:C=4", "l1:C=80", "l1:T=1", "l1:B=1", "l1:len=0", "l1:len=T", "l1:len>T",
    "l1:vec4+len=0", "l1:vec4+len>T", "l1:pred+1", "l1:target+1", "l1:grad+1", "l1:grad=NULL", "l1:all-zero-lengths",
    "l1:empty-call", "l1:seam-scalar-262143", "l1:seam-scalar-262145", "l1:seam-scalar-262144+257", "l1:seam-vec4-262145",
    "l1many:1-term", "l1many:5-terms", "l1many:log1p", "l1many:seam-8192", "l1many:seam-8193",
    "l1many:seam-256-blocks", "l1many:pred+1", "l1many:all-zero-lengths", "l1:single==many",
    # elem_loss / _many
    "eloss:mode0", "eloss:mode1", "eloss:ties", "eloss:-0.0", "eloss:grad=NULL", "eloss:n=1", "eloss:n=255", "eloss:n=256",
    "eloss:n=257", "eloss:n=1024", "eloss:n=1025", "eloss:seam-1048577", "elossmany:seam-524289", "elossmany:64-terms",
    "elossmany:shared-out", "elossmany:n=0-NULL", "elossmany:1-term",
    # scale_many
    "scale:1", "scale:2", "scale:64", "scale:n=0", "scale:seam-524289",
    # sumsq / sumsq_det
    *["sumsq:n=%d" % n for n in (0, 1, 3, 4, 5, 1023, 1024, 1025, 2 ** 21 + 5)],
    *["det:n=%d" % n for n in (0, 1, 5, 4095, 4096, 4097, 16384 + 3, 4096 * 256, 4096 * 256 + 5, 2 ** 21 + 5)],
    "det:workspace-reuse", "det:same-bits",
    # adam
    "adam:n=1", "adam:n=255", "adam:n=257", "adam:n=1048579", "adam:betas=0.9,0.98", "adam:betas=0.9,0.999",
    "adam:betas=0.8,0.99", "adam:eps=1e-09", "adam:eps=1e-08", "adam:wd=0", "adam:wd=0.01", "adam:max_norm=0",
    "adam:gnorm=NULL", "adam:clip=1", "adam:clip<1", "adam:clip-1e-6-decides", "adam:step=1", "adam:step=2", "adam:step=10",
    "adam:step=1000", "adam:host-args", "adam:dyn", "adam:g=0,v=0", "adam:p=0",
    # weight norm
    *["wn:layer%d" % i for i in range(7)],
    "wn:plain", "wn:strided-tap-major", "wn:strided-gapped", "wn:images", "wn:images-wf=NULL", "wn:images-wd=NULL",
    "wn:table-1", "wn:table-2", "wn:table-7", "wn:table-off=-1", "wn:table==per-layer", "wn:bwd-sublist", "wn:bwd-twice",
    "wn:bwd-nl=1", "wn:bwd-nl=64", "wn:zero-row",
]
# (rows, cin, K, groups): rows at the 8-row tile seam (7, 8, 9); rows / groups a multiple of 8 (the 16-byte wd store: layers
# 1, 3, 5) and not (element stores, a tile straddling groups: 0, 2); cols below, at and above 256
_LAYERS = [(12, 3, 5, 3), (16, 8, 3, 1), (9, 1, 7, 9), (24, 4, 1, 3), (1, 300, 2, 1), (8, 64, 4, 1), (7, 257, 1, 1)]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the arena and the case builder
class _Arena:
    """offsets (in floats) into one flat buffer: guard elements before the first block and after every block.  Every
    block starts 16-byte aligned; ``shift`` moves its first element by that many floats (a misaligned pointer)."""

    def __init__(self):
        self.n = 8

    def block(self, floats, tail=8, shift=0):
        off = self.n + shift
        self.n = self.n + (int(floats) + shift + 3) // 4 * 4 + tail
        return off


class _Builder:
    def __init__(self, name):
        self.rng = np.random.default_rng(zlib.crc32(name.encode()))
        self.arena, self.fills, self.calls = _Arena(), [], []

    def f32(self, vals=None, n=None, shift=0):
        """a float block: ``vals``, or n elements of the arena's own noise"""
        if vals is not None:
            vals = np.ascontiguousarray(vals, dtype=F32).reshape(-1)
            n = vals.size
        off = self.arena.block(n, shift=shift)
        if vals is not None and n:
            self.fills.append((off, vals.view(np.uint8)))
        return off

    def i64(self, vals):
        vals = np.ascontiguousarray(vals, dtype=np.int64).reshape(-1)
        off = self.arena.block(2 * vals.size)
        if vals.size:
            self.fills.append((off, vals.view(np.uint8)))
        return off

    def raw(self, data):
        off = self.arena.block((len(data) + 3) // 4)
        self.fills.append((off, np.frombuffer(data, dtype=np.uint8)))
        return off

    def randn(self, n, scale=1.0):
        return (self.rng.standard_normal(int(n)) * scale).astype(F32)

    def dyadic(self, n, zero=False):
        """values from {+-0.5, +-1}: every sum of them, of their differences and of their squares is representable"""
        return self.rng.choice(np.array([-1.0, -0.5, 0.5, 1.0] + ([0.0] if zero else []), dtype=F32), size=int(n))

    def call(self, ep, rc=OK, **kw):
        self.calls.append(dict(kw, ep=ep, rc=rc))

    def finish(self):
        mem = self.rng.standard_normal(self.arena.n).astype(F32)
        b = mem.view(np.uint8)
        for off, data in self.fills:
            assert 4 * off + data.size <= b.size
            b[4 * off:4 * off + data.size] = data
        return mem


class _Case:
    def __init__(self, name, branches, build, exact=False):
        unknown = set(branches) - set(_BRANCHES)
        assert not unknown, (name, unknown)
        self.name, self.branches, self._build, self.exact = name, tuple(branches), build, exact
        self._built = self._ref = None

    def built(self):
        """(arena as the calls find it, the calls)"""
        if self._built is not None:
            return self._built
        b = _Builder(self.name)
        self._build(b)
        built = (b.finish(), b.calls)
        if built[0].size < _KEEP:  # (the arenas of the seam sizes are rebuilt on demand: the same seed, the same bytes)
            self._built = built
        return built

    def reference(self):
        """the float64 evaluation, computed once and shared by every leg"""
        if self._ref is not None:
            return self._ref
        ref = _evaluate(self, F64)
        if ref.raw.size < _KEEP:
            self._ref = ref
        return ref


# ---------------------------------------------------------------------------------------------------------------------
# 2. the interpreter
class _Shadow:
    """the arena as the interpreter sees it: inputs are read from the bytes the calls find (``raw``); ``val`` / ``S`` hold
    what the calls so far have written or accumulated, and S the same expression over absolute values"""

    def __init__(self, raw, dt, rev):
        self.raw, self.dt, self.rev = raw, dt, rev
        self.i64 = raw.view(np.int64)
        self.val = raw.astype(dt)
        self.S = np.abs(raw.astype(F64))
        self.regions = {}

    def f(self, idx):
        idx = np.asarray(idx, dtype=np.int64)
        assert idx.size == 0 or (idx.min() >= 0 and idx.max() < self.raw.size), "the case reads outside its arena"
        return self.raw[idx].astype(self.dt)

    def ints(self, off, n):
        assert off % 2 == 0 and off // 2 + n <= self.i64.size
        return self.i64[off // 2:off // 2 + n]

    def sum(self, x, axis=-1):
        """float64: numpy's sum; float32: strictly sequential, left-to-right or right-to-left"""
        if self.dt is F64:
            return x.sum(axis=axis)
        if x.shape[axis] == 0:
            return np.zeros(x.shape[:axis] + x.shape[axis:][1:], dtype=F32)
        x = np.flip(x, axis) if self.rev else x
        return np.cumsum(x, axis=axis, dtype=F32).take(-1, axis=axis)

    def put(self, idx, val, S):
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        assert idx.size == 0 or (idx.min() >= 0 and idx.max() < self.raw.size), "the case writes outside its arena"
        self.val[idx] = np.asarray(val, dtype=self.dt).reshape(-1)
        self.S[idx] = np.asarray(S, dtype=F64).reshape(-1)

    def add(self, off, val, S):
        self.val[off] = self.val[off] + self.dt(val)
        self.S[off] += float(S)

    def region(self, what, ep, kind, idx=None, **extra):
        self.regions[what] = dict(extra, what=what, ep=ep, kind=kind,
                                  idx=None if idx is None else np.asarray(idx, dtype=np.int64).reshape(-1))


def _l1_term(sh, t):
    """header: rows_b = min(lens[b], T), lens[b] >= 0; sum_{t < rows_b} |target - pred| / (sum(rows) * C); the duration targets are
    int64 values v read as log(v + 1).  Returns (value, S, sign (n), rows, unit) or None for an empty term."""
    dt, (B, T, C) = sh.dt, (t["B"], t["T"], t["C"])
    n = B * T * C
    if n == 0:
        return None
    assert (sh.ints(t["lens"], B) >= 0).all(), "the header leaves a negative length undefined"
    rows = np.minimum(sh.ints(t["lens"], B), T)
    pred = sh.f(t["pred"] + np.arange(n)).reshape(B, T, C)
    if t["log1p"]:
        y = np.log(sh.ints(t["target"], n).astype(dt) + dt(1)).astype(dt).reshape(B, T, C)
    else:
        y = sh.f(t["target"] + np.arange(n)).reshape(B, T, C)
    valid = (np.arange(T)[None, :] < rows[:, None])[:, :, None]
    d = pred - y
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = dt(1) / (dt(rows.sum()) * dt(C))
        val = sh.sum(np.where(valid, np.abs(d), dt(0)).reshape(-1)) * inv
        S = float(np.where(valid, np.abs(pred.astype(F64)) + np.abs(y.astype(F64)), 0.0).sum()) * float(inv)
    return val, S, np.where(valid, np.sign(d), 0).reshape(-1).astype(np.int8), int(rows.sum()), 0.5 * float(inv)


def _l1_grad_region(sh, what, ep, t, sign, rows):
    if t["grad"] is not None:
        den = rows * t["C"]
        sh.region(what, ep, "sign", t["grad"] + np.arange(sign.size), sign=sign, pow2=den > 0 and den & (den - 1) == 0,
                  mag=(F32(1) / (F32(rows) * F32(t["C"]))) if den else F32(0), one_ulp_on_device=True)


def _loss_region(sh, what, ep, off, exact, unit):
    if exact:
        sh.region(what, ep, "exact", [off], unit=unit)
    else:
        sh.region(what, ep, "measured", [off], cap_rel=CAP_LOSS_REL)


def _op_masked_l1(sh, c):
    if c["rc"] != OK:
        return
    r = _l1_term(sh, c)
    if r is None:
        return
    val, S, sign, rows, unit = r
    sh.add(c["loss"], val, S)
    _loss_region(sh, "loss@%d" % c["loss"], c["ep"], c["loss"], c.get("exact"), unit)
    _l1_grad_region(sh, "grad@%s" % c["grad"], c["ep"], c, sign, rows)


def _op_masked_l1_many(sh, c):
    if c["rc"] != OK:
        return
    units = []
    for k, t in enumerate(c["terms"]):
        r = _l1_term(sh, t)
        if r is None:
            continue
        val, S, sign, rows, unit = r
        units.append(unit)
        sh.add(c["losses"] + k, val, S)
        sh.add(c["losses"] + LOSS_MAX_TERMS, val, S)
        _loss_region(sh, "losses[%d]@%d" % (k, c["losses"]), c["ep"], c["losses"] + k, c.get("exact"), unit)
        _l1_grad_region(sh, "grad[%d]@%s" % (k, t["grad"]), c["ep"], t, sign, rows)
    if units:
        _loss_region(sh, "total@%d" % c["losses"], c["ep"], c["losses"] + LOSS_MAX_TERMS, c.get("exact"), min(units))


def _eloss_term(sh, t, ep, what):
    """header: mode 0: scale * sum |a - b|, grad = scale * sign(a - b); mode 1: scale * sum (a - target)^2,
    grad = 2 * scale * (a - target).  Returns (value, S, unit)."""
    dt, n = sh.dt, t["n"]
    a = sh.f(t["a"] + np.arange(n))
    scale = dt(F32(t["scale"]))
    if t["mode"] == 0:
        b = sh.f(t["b"] + np.arange(n))
        d = a - b
        val = scale * sh.sum(np.abs(d))
        S = abs(float(scale)) * float((np.abs(a.astype(F64)) + np.abs(b.astype(F64))).sum())
        if t["grad"] is not None:
            sh.region(what, ep, "sign", t["grad"] + np.arange(n), sign=np.sign(d).astype(np.int8), pow2=True,
                      mag=F32(t["scale"]), one_ulp_on_device=False)
        return val, S, 0.5 * abs(float(scale))
    tg = dt(F32(t["target"]))
    d = a - tg
    val = scale * sh.sum(d * d)
    S = abs(float(scale)) * float(((np.abs(a.astype(F64)) + abs(float(tg))) ** 2).sum())
    if t["grad"] is not None:  # fl(fl(2 * scale) * fl(a - target)): exact on every leg
        d32 = (a.astype(F64) - float(F32(t["target"]))).astype(F32)
        want = ((F32(2) * F32(t["scale"])).astype(F64) * d32.astype(F64)).astype(F32)
        sh.region(what, ep, "bits", t["grad"] + np.arange(n), want=want)
    return val, S, 0.25 * abs(float(scale))


def _op_elem_loss(sh, c):
    if c["rc"] != OK or c["n"] == 0:
        return
    val, S, unit = _eloss_term(sh, c, c["ep"], "grad@%s" % c["grad"])
    sh.add(c["loss"], val, S)
    _loss_region(sh, "loss@%d" % c["loss"], c["ep"], c["loss"], c.get("exact"), unit)


def _op_elem_loss_many(sh, c):
    if c["rc"] != OK:
        return
    units = {}
    for k, t in enumerate(c["terms"]):
        if t["n"] == 0:
            continue
        val, S, unit = _eloss_term(sh, t, c["ep"], "grad[%d]@%s" % (k, t["grad"]))
        sh.add(c["losses"] + t["out"], val, S)
        units[t["out"]] = min(unit, units.get(t["out"], unit))
    for out, unit in units.items():
        _loss_region(sh, "losses[%d]@%d" % (out, c["losses"]), c["ep"], c["losses"] + out, c.get("exact"), unit)


def _op_scale_many(sh, c):
    if c["rc"] != OK:
        return
    s = float(sh.raw[c["scale"]])
    for k, (x, n) in enumerate(zip(c["x"], c["n"])):
        if n:
            idx = x + np.arange(n)
            want = (sh.raw[idx].astype(F64) * s).astype(F32)
            sh.put(idx, want, np.abs(want))
            sh.region("x[%d]@%d" % (k, x), c["ep"], "bits", idx, want=want)


def _op_sumsq(sh, c):
    if c["rc"] != OK:
        return
    det, n = c["ep"] == "kantts_sumsq_det", c["n"]
    if det:
        sh.region("ticket@%d" % c["ws"], c["ep"], "bits", [c["ws"]], want=np.zeros(1, F32))
        sh.region("partials@%d" % c["ws"], c["ep"], "scratch", c["ws"] + 1 + np.arange(DET_WS - 1))
    elif n == 0:
        return
    x = sh.f(c["x"] + np.arange(n))
    val = sh.sum(x * x)
    S = float((x.astype(F64) ** 2).sum())
    if det:
        sh.put([c["out"]], val, S)
    else:
        sh.add(c["out"], val, S)
    if c.get("exact"):
        sh.region("out@%d" % c["out"], c["ep"], "exact", [c["out"]], unit=0.25)
    elif c.get("unchecked"):  # (a real-valued sum above n = 8193: only what the case says about its bits)
        sh.region("out@%d" % c["out"], c["ep"], "scratch", [c["out"]])
    else:
        sh.region("out@%d" % c["out"], c["ep"], "measured", [c["out"]], cap_rel=CAP_LOSS_REL)


def _op_adam(sh, c):
    """torch.optim.Adam on flat arenas; clip = min(1, max_norm / (sqrt(gnorm_sq) + 1e-6)) when max_norm > 0 and gnorm_sq is
    given (clip_grad_norm_); g' = clip g + wd p; m' = b1 m + (1 - b1) g'; v' = b2 v + (1 - b2) g'^2;
    p' = p - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps); dyn_lr_step {lr, step}: lr and bc = 1 - beta^step from memory."""
    if c["rc"] != OK or c["n"] == 0:
        return
    dt, n = sh.dt, c["n"]
    lr, b1, b2, eps, wd, bc1, bc2, mn = (dt(F32(c[k])) for k in ("lr", "b1", "b2", "eps", "wd", "bc1", "bc2", "max_norm"))
    extra = 0.0
    if c["dyn"] is not None:
        lr, t = sh.f(c["dyn"]), sh.f(c["dyn"] + 1)
        bc1, bc2 = dt(1) - b1 ** t, dt(1) - b2 ** t
        k1, k2 = (float(b) ** float(t) / (1.0 - float(b) ** float(t)) for b in (b1, b2))
        extra = k1 + k2 / 2
    clip = dt(1)
    if mn > 0 and c["gnorm"] is not None:
        clip = min(dt(1), dt(mn / (np.sqrt(sh.f(c["gnorm"])) + dt(F32(1e-6)))))
    i = np.arange(n)
    P, G, M, V = (sh.f(c[k] + i) for k in "pgmv")
    gp = G * clip
    a64 = lambda x: np.abs(x.astype(F64))
    S_gp = a64(gp)
    if wd != 0:  # the two terms of g' may cancel: S carries |clip g| + |wd p| wherever g' appears
        S_gp = S_gp + a64(wd * P)
        gp = gp + wd * P
    ta, tb = b1 * M, (dt(1) - b1) * gp
    m1 = ta + tb
    ua, ub = b2 * V, (dt(1) - b2) * gp * gp
    v1 = ua + ub
    delta = (lr / bc1) * m1 / (np.sqrt(v1) / np.sqrt(bc2) + eps)
    p1 = P - delta
    S_m = a64(ta) + float(dt(1) - b1) * S_gp
    sh.put(c["m"] + i, m1, S_m)
    sh.put(c["v"] + i, v1, a64(ua) + float(dt(1) - b2) * S_gp * S_gp)
    # |delta| over absolute values: its numerator m' is the sum of two terms that may cancel
    S_delta = float(lr / bc1) * S_m / (np.sqrt(v1.astype(F64)) / float(np.sqrt(bc2)) + float(eps))
    sh.put(c["p"] + i, p1, a64(P) + S_delta * (1.0 + extra))
    sh.region("m@%d" % c["m"], c["ep"], "measured", c["m"] + i)
    sh.region("v@%d" % c["v"], c["ep"], "measured", c["v"] + i)
    sh.region("p@%d" % c["p"], c["ep"], "measured", c["p"] + i, cap_abs=CAP_ADAM_ABS)


def _wn_index(c, layout):
    """flat indices (rows, cin, K) of the weight-side tensor of a call"""
    rows, cin, K = c["rows"], c["cin"], c["K"]
    r, ci, k = np.arange(rows)[:, None, None], np.arange(cin)[None, :, None], np.arange(K)[None, None, :]
    if layout == "param":     # (rows, cin, K), the layout of v / dv
        return (r * cin + ci) * K + k
    if layout == "strided":
        return r * c["rs"] + ci * c["cs"] + k * c["ks"]
    if layout == "tap":       # (K, rows, cin)
        return (k * rows + r) * cin + ci
    rg = rows // c["groups"]  # "wd": (K, groups, cin, rows / groups)
    return ((k * c["groups"] + r // rg) * cin + ci) * rg + r % rg


def _wn_rows(sh, v_off, g_off, c):
    dt = sh.dt
    V = sh.f(v_off + _wn_index(c, "param"))
    g = sh.f(g_off + np.arange(c["rows"]))
    nrm = np.sqrt(sh.sum((V * V).reshape(c["rows"], -1))).astype(dt)
    return V, g, nrm


def _wn_fwd(sh, c, v_off, g_off, w_idx, what):
    V, g, nrm = _wn_rows(sh, v_off, g_off, c)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = (g[:, None, None] * V / nrm[:, None, None]).astype(sh.dt)
    sh.put(w_idx, w, np.abs(w.astype(F64)))
    sh.region(what, c["ep"], "measured", w_idx)


def _wn_bwd(sh, c, v_off, g_off, dw_idx, dv_off, dg_off, what):
    V, g, nrm = _wn_rows(sh, v_off, g_off, c)
    DW = sh.f(dw_idx)
    with np.errstate(divide="ignore", invalid="ignore"):
        dg = sh.sum((DW * V).reshape(c["rows"], -1)) / nrm
        dv = (g / nrm)[:, None, None] * (DW - V * (dg / nrm)[:, None, None])
        n64, a64 = nrm.astype(F64), lambda x: np.abs(x.astype(F64))
        S_dg = (a64(DW) * a64(V)).reshape(c["rows"], -1).sum(axis=1) / n64
        S_dv = (a64(g) / n64)[:, None, None] * (a64(DW) + a64(V) * (S_dg / n64)[:, None, None])
    sh.put(dg_off + np.arange(c["rows"]), dg, S_dg)
    sh.put(dv_off + _wn_index(c, "param"), dv, S_dv)
    sh.region("dg " + what, c["ep"], "measured", dg_off + np.arange(c["rows"]))
    sh.region("dv " + what, c["ep"], "measured", dv_off + _wn_index(c, "param"))


def _wn_images(sh, c, w_off, wf, wd, what):
    """wf / wd: offsets in bf16 elements, or None"""
    _wn_fwd(sh, c, c["v"], c["g"], w_off + _wn_index(c, "tap"), "w " + what)
    if wf is not None:
        sh.region("wf " + what, c["ep"], "bf16", None, u16=(wf + _wn_index(c, "tap")).reshape(-1),
                  src=(w_off + _wn_index(c, "tap")).reshape(-1))
    if wd is not None:
        sh.region("wd " + what, c["ep"], "bf16", None, u16=(wd + _wn_index(c, "wd")).reshape(-1),
                  src=(w_off + _wn_index(c, "tap")).reshape(-1))


def _op_wn(sh, c):
    if c["rc"] != OK or c.get("rows") == 0:
        return
    ep = c["ep"]
    if ep == "kantts_weight_norm_fwd":
        _wn_fwd(sh, c, c["v"], c["g"], c["w"] + _wn_index(c, "param"), "w@%d" % c["w"])
    elif ep == "kantts_weight_norm_bwd":
        _wn_bwd(sh, c, c["v"], c["g"], c["dw"] + _wn_index(c, "param"), c["dv"], c["dg"], "@%d" % c["dv"])
    elif ep == "kantts_weight_norm_strided_fwd":
        _wn_fwd(sh, c, c["v"], c["g"], c["w"] + _wn_index(c, "strided"), "w@%d" % c["w"])
    elif ep == "kantts_weight_norm_strided_bwd":
        _wn_bwd(sh, c, c["v"], c["g"], c["dw"] + _wn_index(c, "strided"), c["dv"], c["dg"], "@%d" % c["dv"])
    elif ep == "kantts_weight_norm_tap_images":
        _wn_images(sh, c, c["w"], c["wf"], c["wd"], "@%d" % c["w"])
    elif ep == "kantts_weight_norm_table":  # flat, w, wf, wd are the arena itself: the table's offsets are absolute
        for d in c["table"]:
            _wn_images(sh, dict(d, ep=ep), d["w_off"], d["wf_off"] if d["wf_off"] >= 0 else None,
                       d["wd_off"] if d["wd_off"] >= 0 else None, "@%d" % d["w_off"])
    else:  # table_bwd: dv / dg at grad_flat + the entry's v_off / g_off
        for l, e in enumerate(c["desc"]):
            d = dict(c["table"][e], ep=ep)
            _wn_bwd(sh, d, d["v"], d["g"], c["dw"][l] + _wn_index(d, "tap"), c["grad"] + d["v"], c["grad"] + d["g"],
                    "of entry %d" % e)


def _op_check(sh, c):
    """not a call: ``same`` = two element lists that must hold the same bits afterwards"""
    sh.region("same %s" % c["what"], "-", "same", None, a=np.asarray(c["a"]).reshape(-1), b=np.asarray(c["b"]).reshape(-1),
              u16=c.get("u16", False))


_OPS = {"kantts_masked_l1": _op_masked_l1, "kantts_masked_l1_many": _op_masked_l1_many, "kantts_elem_loss": _op_elem_loss,
        "kantts_elem_loss_many": _op_elem_loss_many, "kantts_scale_many": _op_scale_many, "kantts_sumsq": _op_sumsq,
        "kantts_sumsq_det": _op_sumsq, "kantts_adam_step": _op_adam, "same": _op_check, "ticket": lambda sh, c: None}
_WN_EPS = ("kantts_weight_norm_fwd", "kantts_weight_norm_bwd", "kantts_weight_norm_strided_fwd", "kantts_weight_norm_strided_bwd",
           "kantts_weight_norm_tap_images", "kantts_weight_norm_table", "kantts_weight_norm_table_bwd")
_OPS.update({ep: _op_wn for ep in _WN_EPS})
_ENTRY_POINTS = sorted(set(_OPS) - {"same", "ticket"})


def _evaluate(case, dt, rev=False):
    raw, calls = case.built()
    sh = _Shadow(raw, dt, rev)
    for c in calls:
        _OPS[c["ep"]](sh, c)
    if dt is F64:  # the exact class: every partial sum in any order is a whole number of units below 2^24
        for r in sh.regions.values():
            if r["kind"] == "exact" and np.isfinite(sh.val[r["idx"][0]]):
                units = sh.S[r["idx"][0]] / r["unit"]
                assert units == np.floor(units) and units < 2 ** 24, (case.name, r["what"], units)
                assert float(F32(sh.val[r["idx"][0]])) == sh.val[r["idx"][0]], (case.name, r["what"])
    return sh


# ---------------------------------------------------------------------------------------------------------------------
# 3. the case table
def _l1_data(b, B, T, C, lens, grad=True, log1p=False, exact=False, shift=None):
    n = B * T * C
    if log1p:
        pred, target = b.randn(n), None
        t_off = b.i64(b.rng.integers(0, 40, size=n))
    else:
        pred, target = (b.dyadic(n), b.dyadic(n)) if exact else (b.randn(n), b.randn(n))
        if n and not exact:
            pred[::7] = target[::7]  # ties: gradient 0
        t_off = b.f32(target, shift=int(shift == "target"))
    return dict(pred=b.f32(pred, shift=int(shift == "pred")), target=t_off, lens=b.i64(lens),
                grad=b.f32(n=n, shift=int(shift == "grad")) if grad else None, B=B, T=T, C=C, log1p=int(log1p))


def _spread(total, B, T):
    """B lengths: the last is T + 2 (more than T), one is 0 when there is room, the valid rows sum to ``total``"""
    rest, lens = total - T, []
    assert rest >= 0
    for _ in range(B - 1):
        take = min(T, rest) if len(lens) % 2 == 0 else min(T, rest // 2)
        lens.append(take)
        rest -= take
    assert rest == 0, "cannot spread %d rows over (%d, %d)" % (total, B, T)
    return lens + [T + 2]


def _l1_cases():
    cs = []

    def single(name, branches, B, T, C, lens, exact=False, acc0=None, **kw):
        def build(b):
            t = _l1_data(b, B, T, C, lens, exact=exact, **kw)
            loss = b.f32([0.5 if acc0 is None else acc0])
            b.call("kantts_masked_l1", loss=loss, exact=exact, **t)
        cs.append(_Case(name, branches, build, exact=exact))

    def many(name, branches, specs, exact=False):
        def build(b):
            terms = [_l1_data(b, exact=exact, **s) for s in specs]
            b.call("kantts_masked_l1_many", terms=terms, losses=b.f32(np.zeros(LOSS_MAX_TERMS + 1)), exact=exact)
        cs.append(_Case(name, branches, build, exact=exact))

    single("l1_C1", ["l1:C=1", "l1:len=0", "l1:len=T", "l1:len>T"], 3, 7, 1, [7, 0, 9])
    single("l1_C3", ["l1:C=3", "l1:len=T"], 2, 5, 3, [3, 5])
    single("l1_C4", ["l1:C=4", "l1:vec4+len=0", "l1:vec4+len>T", "l1:len=0", "l1:len>T"], 3, 6, 4, [0, 6, 8])
    single("l1_C80", ["l1:C=80", "l1:len=T"], 2, 9, 80, [9, 4])
    single("l1_T1", ["l1:T=1", "l1:vec4+len=0", "l1:vec4+len>T"], 3, 1, 4, [1, 0, 2])
    single("l1_B1", ["l1:B=1"], 1, 5, 3, [4])
    single("l1_C4_two_blocks", ["l1:C=4", "l1:vec4+len=0", "l1:vec4+len>T"], 3, 40, 8, [0, 47, 13])  # 240 float4 + a second block
    for which in ("pred", "target", "grad"):
        single("l1_C4_%s_plus_1" % which, ["l1:%s+1" % which], 3, 6, 4, [5, 0, 9], shift=which)
    single("l1_C4_nograd", ["l1:grad=NULL", "l1:C=4"], 2, 6, 4, [6, 2], grad=False)
    single("l1_C3_nograd", ["l1:grad=NULL", "l1:C=3"], 2, 6, 3, [1, 8], grad=False)
    single("l1_C4_zero_lengths", ["l1:all-zero-lengths", "l1:vec4+len=0"], 2, 4, 4, [0, 0])
    single("l1_C3_zero_lengths", ["l1:all-zero-lengths"], 2, 4, 3, [0, 0])
    single("l1_empty_B0", ["l1:empty-call"], 0, 4, 4, [])
    single("l1_empty_T0", ["l1:empty-call"], 2, 0, 3, [1, 2])
    # the grid-stride seams, exact class (1024 blocks x 256 threads = 262144 elements / float4 groups per trip)
    single("l1_seam_262143", ["l1:seam-scalar-262143"], 3, 87381, 1, _spread(2 ** 17, 3, 87381), exact=True)
    single("l1_seam_262145", ["l1:seam-scalar-262145"], 5, 52429, 1, _spread(2 ** 17, 5, 52429), exact=True)
    single("l1_seam_262401", ["l1:seam-scalar-262144+257"], 3, 87467, 1, _spread(2 ** 17, 3, 87467), exact=True)
    single("l1_seam_vec4_262145", ["l1:seam-vec4-262145"], 5, 52429, 4, _spread(2 ** 17, 5, 52429), exact=True)
    single("l1_exact_small_C4", ["l1:C=4"], 2, 5, 4, [3, 5], exact=True)

    many("l1many_1", ["l1many:1-term", "l1:C=80"], [dict(B=2, T=9, C=80, lens=[9, 4])])
    five = [dict(B=3, T=6, C=80, lens=[6, 0, 8]), dict(B=2, T=7, C=4, lens=[7, 3]),
            dict(B=3, T=5, C=1, lens=[5, 2, 0], log1p=True), dict(B=3, T=5, C=1, lens=[4, 5, 9]),
            dict(B=1, T=11, C=3, lens=[10], grad=False)]
    many("l1many_5", ["l1many:5-terms", "l1many:log1p", "l1:grad=NULL", "l1:vec4+len=0", "l1:vec4+len>T"], five)
    many("l1many_pred_plus_1", ["l1many:pred+1"],
         [dict(B=3, T=6, C=4, lens=[5, 0, 9], shift="pred"), dict(B=3, T=6, C=4, lens=[5, 0, 9], shift="grad"),
          dict(B=3, T=6, C=4, lens=[5, 0, 9], shift="target")])
    many("l1many_zero_lengths", ["l1many:all-zero-lengths"], [dict(B=2, T=4, C=4, lens=[0, 0]), dict(B=2, T=4, C=3, lens=[4, 1])])
    many("l1many_seam_8192", ["l1many:seam-8192"], [dict(B=2, T=1024, C=4, lens=[1026, 1024])], exact=True)
    many("l1many_seam_8193", ["l1many:seam-8193"],
         [dict(B=3, T=2731, C=1, lens=[1365, 0, 2731]), dict(B=2, T=4, C=4, lens=[4, 4])], exact=True)
    many("l1many_seam_256_blocks", ["l1many:seam-256-blocks"],
         [dict(B=2, T=4, C=4, lens=[4, 4]), dict(B=5, T=52429, C=8, lens=_spread(2 ** 17, 5, 52429))], exact=True)

    # the single and the _many call give the same bits on the same data (one block each: one order of summation)
    for C in (3, 4):
        def build(b, C=C):
            t = _l1_data(b, 2, 4, C, [0, 2])
            t2 = dict(t, grad=b.f32(n=2 * 4 * C))
            loss, losses = b.f32([0.0]), b.f32(np.zeros(LOSS_MAX_TERMS + 1))
            b.call("kantts_masked_l1", loss=loss, **t)
            b.call("kantts_masked_l1_many", terms=[t2], losses=losses)
            n = np.arange(2 * 4 * C)
            b.call("same", what="loss", a=[loss, loss], b=[losses, losses + LOSS_MAX_TERMS])
            b.call("same", what="grad", a=t["grad"] + n, b=t2["grad"] + n)
        cs.append(_Case("l1_single_equals_many_C%d" % C, ["l1:single==many", "l1:len=0"], build))
    return cs


def _eloss_cases():
    cs = []

    def data(b, n, mode, exact, grad=True, scale=None):
        if exact:
            a, bb, target = b.dyadic(n), b.dyadic(n), 0.5
            scale = 2.0 ** -20 if scale is None else scale
        else:
            a, bb, target = b.randn(n), b.randn(n), 1.0
            a[::5] = bb[::5]  # ties
            if n > 2:
                a[1], bb[1] = -0.0, 0.0  # a - b = -0.0: gradient 0
                a[2], bb[2] = 0.0, -0.0
            scale = 0.37 / n if scale is None else scale
        return dict(a=b.f32(a), b=b.f32(bb) if mode == 0 else None, grad=b.f32(n=n) if grad else None, n=n, target=target,
                    scale=scale, mode=mode)

    def single(name, branches, n, mode, exact=False, **kw):
        def build(b):
            b.call("kantts_elem_loss", loss=b.f32([0.25]), exact=exact, **data(b, n, mode, exact, **kw))
        cs.append(_Case(name, branches, build, exact=exact))

    for i, n in enumerate((1, 255, 256, 257, 1024, 1025)):
        for mode in (0, 1):
            single("eloss_n%d_mode%d" % (n, mode), ["eloss:n=%d" % n, "eloss:mode%d" % mode, "eloss:ties", "eloss:-0.0"], n, mode)
            single("eloss_exact_n%d_mode%d" % (n, mode), ["eloss:n=%d" % n, "eloss:mode%d" % mode], n, mode, exact=True,
                   grad=(i + mode) % 2 == 0)
    single("eloss_nograd_mode0", ["eloss:grad=NULL"], 300, 0, grad=False)
    single("eloss_nograd_mode1", ["eloss:grad=NULL"], 300, 1, grad=False)
    single("eloss_seam_mode0", ["eloss:seam-1048577"], 2 ** 20 + 1, 0, exact=True)
    single("eloss_seam_mode1", ["eloss:seam-1048577"], 2 ** 20 + 1, 1, exact=True, grad=False)

    def many(name, branches, specs, n_out, exact=False):
        def build(b):
            terms = []
            for s in specs:
                if s["n"] == 0:  # an empty tensor: NULL pointers
                    terms.append(dict(a=None, b=None, grad=None, n=0, target=0.0, scale=1.0, mode=s["mode"], out=s["out"]))
                else:
                    terms.append(dict(data(b, s["n"], s["mode"], exact, grad=s.get("grad", True), scale=s.get("scale")), out=s["out"]))
            b.call("kantts_elem_loss_many", terms=terms, losses=b.f32(np.zeros(n_out)), exact=exact)
        cs.append(_Case(name, branches, build, exact=exact))

    many("elossmany_1", ["elossmany:1-term"], [dict(n=700, mode=0, out=0)], 1)
    # 64 terms of unequal sizes (1 .. 3 blocks), four accumulators shared, empty terms with NULL pointers in between: the
    # bisection over first_block sees every split
    specs = [dict(n=0 if k % 7 == 3 else (1 + 37 * k if k % 5 else 1025 + 300 * (k % 3)), mode=k % 2, out=k % 4, grad=k % 3 != 0)
             for k in range(ELOSS_MAX_TERMS)]
    many("elossmany_64", ["elossmany:64-terms", "elossmany:shared-out", "elossmany:n=0-NULL", "eloss:grad=NULL"], specs, 4)
    many("elossmany_64_exact", ["elossmany:64-terms", "elossmany:shared-out", "elossmany:n=0-NULL"],
         [dict(s, scale=2.0 ** -(8 + k % 3)) for k, s in enumerate(specs)], 4, exact=True)
    many("elossmany_seam", ["elossmany:seam-524289"],
         [dict(n=5, mode=1, out=1), dict(n=2 ** 19 + 1, mode=0, out=0), dict(n=0, mode=0, out=0), dict(n=1030, mode=1, out=1)], 2,
         exact=True)
    return cs


def _scale_cases():
    cs = []

    def case(name, branches, sizes):
        def build(b):
            b.call("kantts_scale_many", x=[b.f32(b.randn(n)) for n in sizes], n=list(sizes), scale=b.f32([0.7310585975646973]))
        cs.append(_Case(name, branches, build))

    case("scale_1", ["scale:1"], [301])
    case("scale_2", ["scale:2", "scale:n=0"], [0, 1030])
    case("scale_64", ["scale:64", "scale:n=0"], [0 if k == 9 else 1 + 53 * k + (2049 if k % 11 == 0 else 0) for k in range(64)])
    case("scale_seam", ["scale:seam-524289", "scale:2"], [7, 1024 * 512 + 1])
    return cs


def _sumsq_cases():
    cs = []
    for n in (0, 1, 3, 4, 5, 1023, 1024, 1025, 2 ** 21 + 5):
        def build(b, n=n, exact=True):
            b.call("kantts_sumsq", x=b.f32(b.dyadic(n) if exact else b.randn(n)), out=b.f32([0.75 if exact else 0.3]), n=n,
                   exact=exact)
        cs.append(_Case("sumsq_exact_n%d" % n, ["sumsq:n=%d" % n], build, exact=True))
        if 0 < n <= 1025:
            cs.append(_Case("sumsq_real_n%d" % n, ["sumsq:n=%d" % n], lambda b, build=build: build(b, exact=False)))
    det_n = (0, 1, 5, 4095, 4096, 4097, 16384 + 3, 4096 * 256, 4096 * 256 + 5, 2 ** 21 + 5)
    for n in det_n:
        def build(b, n=n, exact=True):
            b.call("kantts_sumsq_det", x=b.f32(b.dyadic(n) if exact else b.randn(n)), out=b.f32(n=1), n=n,
                   ws=b.f32(np.zeros(DET_WS)), ws_floats=DET_WS, exact=exact)
        cs.append(_Case("det_exact_n%d" % n, ["det:n=%d" % n], build, exact=True))
        if 0 < n <= 4097:
            cs.append(_Case("det_real_n%d" % n, ["det:n=%d" % n], lambda b, build=build: build(b, exact=False)))

    def reuse(b):  # one workspace, consecutive calls of different n (grids of 1 .. 256 blocks); the ticket reads 0 after each
        ws = b.f32(np.zeros(DET_WS + 3))
        for n in (4097, 2 ** 21 + 5, 0, 16387, 4096 * 256, 5, 4096 * 256 + 5, 1, 4096):
            b.call("kantts_sumsq_det", x=b.f32(b.dyadic(n)), out=b.f32(n=1), n=n, ws=ws, ws_floats=DET_WS + 3, exact=True)
            b.call("ticket", off=ws)
    cs.append(_Case("det_workspace_reuse", ["det:workspace-reuse"], reuse, exact=True))

    def same_bits(b):  # random real data: the same bits twice, and with a call of another n (another grid) in between
        ws, xa, xb = b.f32(np.zeros(DET_WS)), b.f32(b.randn(8193)), b.f32(b.randn(4096 * 37 + 2))
        outs = [b.f32(n=1) for _ in range(4)]
        for out, (x, n) in zip(outs, ((xa, 8193), (xa, 8193), (xb, 4096 * 37 + 2), (xa, 8193))):
            b.call("kantts_sumsq_det", x=x, out=out, n=n, ws=ws, ws_floats=DET_WS, unchecked=n > 8193)
            b.call("ticket", off=ws)
        b.call("same", what="twice", a=[outs[0], outs[0]], b=[outs[1], outs[3]])
    cs.append(_Case("det_same_bits", ["det:same-bits", "det:workspace-reuse"], same_bits))
    return cs


def _adam_cases():
    cs = []
    betas = ((0.9, 0.98), (0.9, 0.999), (0.8, 0.99))
    clips = ("max_norm=0", "gnorm=NULL", "clip=1", "clip<1", "clip-1e-6-decides")

    def case(name, n, bt, eps, wd, clip, step, dyn, p0=False, extra=()):
        def build(b):
            p, g = (np.zeros(n, F32) if p0 else b.randn(n, 0.1)), b.randn(n, 0.05)
            # moments as three earlier gradients leave them (|m| <~ sqrt(v), as in any run of the optimizer: independent m and
            # v put elements with v ~ 0 under a large m, an update of 1e3 that no training step takes)
            past = b.rng.standard_normal((3, n)) * 0.05
            m = sum((1 - bt[0]) * bt[0] ** i * past[i] for i in range(3)).astype(F32)
            v = sum((1 - bt[1]) * bt[1] ** i * past[i] ** 2 for i in range(3)).astype(F32)
            z = np.arange(n) % 9 == 4  # elements the optimizer has never seen a gradient for
            g[z], m[z], v[z] = 0, 0, 0
            gsq = float((g.astype(F64) ** 2).sum())
            gnorm, max_norm = {"max_norm=0": (gsq, 0.0), "gnorm=NULL": (None, 1.0), "clip=1": (gsq, 10.0 * gsq ** 0.5 + 1.0),
                               "clip<1": (gsq + 100.0, 1.0), "clip-1e-6-decides": (1e-12, 1e-6)}[clip]
            lr = 1e-3
            bc1, bc2 = 1.0 - bt[0] ** step, 1.0 - bt[1] ** step
            if dyn:  # deliberately wrong host values: the device words decide
                d_off, lr, bc1, bc2 = b.f32([1e-3, float(step)]), 0.5, 0.25, 0.125
            b.call("kantts_adam_step", p=b.f32(p), g=b.f32(g), m=b.f32(m), v=b.f32(v), n=n, lr=lr, b1=bt[0], b2=bt[1], eps=eps,
                   wd=wd, bc1=bc1, bc2=bc2, gnorm=None if gnorm is None else b.f32([gnorm]), max_norm=max_norm,
                   dyn=d_off if dyn else None)
        br = ["adam:n=%d" % n, "adam:betas=%g,%g" % bt, "adam:eps=%g" % eps, "adam:wd=%g" % wd, "adam:" + clip,
              "adam:step=%d" % step, "adam:dyn" if dyn else "adam:host-args", "adam:g=0,v=0"] + (["adam:p=0"] if p0 else [])
        cs.append(_Case(name, br + list(extra), build))

    k = 0
    for step in (1, 2, 10, 1000):
        for dyn in (False, True):
            for clip in clips:  # every step x form x clip regime; the other features dealt round
                case("adam_step%d_%s_%s" % (step, "dyn" if dyn else "host", clip), (1, 255, 257)[k % 3], betas[(k // 2) % 3],
                     (1e-9, 1e-8)[k % 2], (0.0, 0.01)[(k // 3) % 2], clip, step, dyn)
                k += 1
    for j, bt in enumerate(betas):  # p = 0 everywhere: the new p IS the update
        for dyn in (False, True):
            case("adam_p0_betas%d_%s" % (j, "dyn" if dyn else "host"), 257, bt, (1e-9, 1e-8)[j % 2], 0.0,
                 clips[(2 * j + dyn) % 5], (1, 2, 10)[j], dyn, p0=True)
    case("adam_big_host", 2 ** 20 + 3, betas[0], 1e-9, 0.01, "clip<1", 10, False)
    case("adam_big_dyn", 2 ** 20 + 3, betas[1], 1e-8, 0.0, "clip=1", 2, True)
    return cs


def _wn_tensors(b, layer, zero_row=None):
    rows, cin, K, groups = layer
    v = b.randn(rows * cin * K).reshape(rows, -1)
    if zero_row is not None:
        v[zero_row] = 0
    return dict(v=b.f32(v), g=b.f32(b.randn(rows)), rows=rows, cin=cin, K=K, groups=groups)


def _desc_bytes(d, row0):
    """kantts_wn_desc: 5 int64 + 6 int32"""
    return struct.pack("<5q6i", d["v"], d["g"], d["w_off"], d["wf_off"], d["wd_off"], d["rows"], d["cin"], d["K"], d["groups"], row0, 0)


def _wn_cases():
    cs = []
    for i, layer in enumerate(_LAYERS):
        rows, cin, K, groups = layer
        cols, tag = cin * K, ["wn:layer%d" % i]

        def plain(b, layer=layer, cols=cols):
            t = _wn_tensors(b, layer)
            b.call("kantts_weight_norm_fwd", w=b.f32(n=t["rows"] * cols), cols=cols, **t)
            b.call("kantts_weight_norm_bwd", dw=b.f32(b.randn(t["rows"] * cols)), dv=b.f32(n=t["rows"] * cols),
                   dg=b.f32(n=t["rows"]), cols=cols, **t)
        cs.append(_Case("wn_plain_%d" % i, tag + ["wn:plain"], plain))
        for lay in ("tap-major", "gapped"):
            def strided(b, layer=layer, lay=lay):
                t = _wn_tensors(b, layer)
                rows, cin, K = t["rows"], t["cin"], t["K"]
                rs, cs_, ks = (cin, 1, rows * cin) if lay == "tap-major" else (2 * cin + 3, 2, rows * (2 * cin + 3) + 5)
                size = (rows - 1) * rs + (cin - 1) * cs_ + (K - 1) * ks + 1
                b.call("kantts_weight_norm_strided_fwd", w=b.f32(n=size), rs=rs, cs=cs_, ks=ks, **t)
                b.call("kantts_weight_norm_strided_bwd", dw=b.f32(b.randn(size)), dv=b.f32(n=rows * cin * K), dg=b.f32(n=rows),
                       rs=rs, cs=cs_, ks=ks, **t)
            cs.append(_Case("wn_strided_%s_%d" % (lay, i), tag + ["wn:strided-" + lay], strided))
        for wf, wd in ((True, True), (False, True), (True, False)):
            def images(b, layer=layer, wf=wf, wd=wd):
                t = _wn_tensors(b, layer)
                n = t["rows"] * t["cin"] * t["K"]
                b.call("kantts_weight_norm_tap_images", w=b.f32(n=n), wf=2 * b.f32(n=(n + 1) // 2) if wf else None,
                       wd=2 * b.f32(n=(n + 1) // 2) if wd else None, **t)
            cs.append(_Case("wn_images_%d%s%s" % (i, "" if wf else "_nowf", "" if wd else "_nowd"),
                            tag + ["wn:images"] + ([] if wf else ["wn:images-wf=NULL"]) + ([] if wd else ["wn:images-wd=NULL"]), images))

    def table_case(name, branches, layers, no_wf=(), no_wd=(), zero_row=None, bwd=None):
        def build(b):
            table, row0, tiles = [], [], 0
            for j, i in enumerate(layers):
                t = _wn_tensors(b, _LAYERS[i], zero_row=zero_row if j == 0 else None)
                n = t["rows"] * t["cin"] * t["K"]
                t.update(w_off=b.f32(n=n), wf_off=-1 if j in no_wf else 2 * b.f32(n=(n + 1) // 2),
                         wd_off=-1 if j in no_wd else 2 * b.f32(n=(n + 1) // 2))
                table.append(t)
                row0.append(tiles)
                tiles += (t["rows"] + 7) // 8
            params = b.arena.n  # everything so far is the parameter arena; the gradient arena mirrors it
            b.f32(n=params)
            tab = b.raw(b"".join(_desc_bytes(d, r) for d, r in zip(table, row0)))
            b.call("kantts_weight_norm_table", table=table, tab=tab, tiles=tiles)
            for d in table:  # the per-layer call on the same v / g: the same bits
                n = d["rows"] * d["cin"] * d["K"]
                w2, wf2, wd2 = b.f32(n=n), 2 * b.f32(n=(n + 1) // 2), 2 * b.f32(n=(n + 1) // 2)
                b.call("kantts_weight_norm_tap_images", w=w2, wf=wf2, wd=wd2, **{k: d[k] for k in ("v", "g", "rows", "cin", "K", "groups")})
                i_n = np.arange(n)
                b.call("same", what="w of %d" % d["w_off"], a=d["w_off"] + i_n, b=w2 + i_n)
                if d["wf_off"] >= 0:
                    b.call("same", what="wf of %d" % d["w_off"], a=d["wf_off"] + i_n, b=wf2 + i_n, u16=True)
                if d["wd_off"] >= 0:
                    b.call("same", what="wd of %d" % d["w_off"], a=d["wd_off"] + i_n, b=wd2 + i_n, u16=True)
            if bwd is not None:
                dws, dw_of, tile0, t0 = [], {}, [], 0
                for e in bwd:  # a layer listed twice gets the same gradient twice (the launch ASSIGNS the slot)
                    d = table[e]
                    if e not in dw_of:
                        dw_of[e] = b.f32(b.randn(d["rows"] * d["cin"] * d["K"]))
                    dws.append(dw_of[e])
                    tile0.append(t0)
                    t0 += (d["rows"] + 7) // 8
                b.call("kantts_weight_norm_table_bwd", table=table, tab=tab, desc=list(bwd), dw=dws, tile0=tile0 + [t0], grad=params)
        cs.append(_Case(name, branches, build))

    table_case("wn_table_1", ["wn:table-1", "wn:table==per-layer", "wn:bwd-nl=1", "wn:layer0"], [0], bwd=[0])
    table_case("wn_table_2", ["wn:table-2", "wn:table-off=-1", "wn:table==per-layer", "wn:bwd-nl=1"], [5, 2], no_wf=[0], no_wd=[1], bwd=[1])
    table_case("wn_table_7", ["wn:table-7", "wn:table-off=-1", "wn:table==per-layer", "wn:bwd-sublist", "wn:bwd-twice"]
               + ["wn:layer%d" % i for i in range(7)], list(range(7)), no_wf=[2, 6], no_wd=[0, 6], bwd=[5, 1, 6, 1, 0])
    table_case("wn_table_7_reversed", ["wn:table-7", "wn:bwd-nl=64", "wn:bwd-twice"], list(range(6, -1, -1)), no_wd=[3],
               bwd=[(5 * l + 3) % 7 for l in range(WN_BWD_MAX)])
    table_case("wn_table_zero_row", ["wn:zero-row", "wn:table-2"], [0, 3], zero_row=5, bwd=[1, 0])
    table_case("wn_table_zero_row_vec", ["wn:zero-row", "wn:table-1"], [1], zero_row=11, bwd=[0])

    def zero_row(b):
        t = _wn_tensors(b, _LAYERS[0], zero_row=5)
        n, cols = 12 * 15, 15
        b.call("kantts_weight_norm_fwd", w=b.f32(n=n), cols=cols, **t)
        b.call("kantts_weight_norm_bwd", dw=b.f32(b.randn(n)), dv=b.f32(n=n), dg=b.f32(n=12), cols=cols, **t)
        b.call("kantts_weight_norm_strided_fwd", w=b.f32(n=n), rs=3, cs=1, ks=36, **t)
        b.call("kantts_weight_norm_strided_bwd", dw=b.f32(b.randn(n)), dv=b.f32(n=n), dg=b.f32(n=12), rs=3, cs=1, ks=36, **t)
        b.call("kantts_weight_norm_tap_images", w=b.f32(n=n), wf=2 * b.f32(n=n // 2), wd=2 * b.f32(n=n // 2), **t)
    cs.append(_Case("wn_zero_row", ["wn:zero-row", "wn:plain", "wn:strided-tap-major", "wn:images"], zero_row))
    return cs


def _build_table():
    table = {"l1": _l1_cases(), "eloss": _eloss_cases(), "scale": _scale_cases(), "sumsq": _sumsq_cases(), "adam": _adam_cases(),
             "wn": _wn_cases()}
    names = [c.name for cs in table.values() for c in cs]
    assert len(set(names)) == len(names)
    return table


_TABLE = _build_table()
_GROUPS = list(_TABLE)
_MEASURED = {}


def _c():
    """c = 4 x the worst ratio of (float32, sequential sums in both directions) - (float64) to 2^-24 * S over the table"""
    if not _MEASURED:
        worst, where = 0.0, None
        for cases in _TABLE.values():
            for case in cases:
                if case.exact:
                    continue
                ref = case.reference()
                for rev in (False, True):
                    low = _evaluate(case, F32, rev)
                    for r in ref.regions.values():
                        if r["kind"] != "measured":
                            continue
                        want, S, got = ref.val[r["idx"]], ref.S[r["idx"]], low.val[r["idx"]].astype(F64)
                        ok = np.isfinite(want) & (S > 0)
                        if ok.any():
                            ratio = float((np.abs(got - want)[ok] / (U * S[ok])).max())
                            if ratio > worst:
                                worst, where = ratio, case.name
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
class _Leg:
    def __init__(self, name):
        self.name = name
        self.device = "cuda" if name == "gpu" else "cpu"
        self.R = 2.0 if name == "gpu" else 1.0

    def context(self):
        return {"emu": util.emulation, "src": util.kernel_source_on_cpu, "gpu": contextlib.nullcontext}[self.name]()


def _leg_params():
    return [pytest.param("emu", id="emu"),
            pytest.param("src", id="src", marks=pytest.mark.skipif(not _HAVE_CLANG, reason="ROCm clang not installed")),
            pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]


class _Mem:
    """the arena on the leg's device: p(off) = the address of float ``off``, h(off) of bf16 element ``off``"""

    def __init__(self, raw, leg):
        import kantts._hip as hip

        self.t = torch.from_numpy(raw.copy()).to(leg.device)
        self.base, self.device = hip.ptr(self.t, torch.float32), leg.device

    def p(self, off):
        return None if off is None else self.base + 4 * int(off)

    def h(self, off):
        return None if off is None else self.base + 2 * int(off)

    def result(self):
        if self.device == "cuda":
            torch.cuda.synchronize()
        return self.t.cpu().numpy()


def _loss_terms(m, terms):
    import kantts._hip as hip

    arr = (hip.LossTerm * max(1, len(terms)))()
    for q, t in zip(arr, terms):
        q.pred, q.target, q.lens, q.grad = m.p(t["pred"]), m.p(t["target"]), m.p(t["lens"]), m.p(t["grad"])
        q.B, q.T, q.C, q.target_log1p = t["B"], t["T"], t["C"], t["log1p"]
    return arr


def _eloss_terms(m, terms):
    import kantts._hip as hip

    arr = (hip.ElossTerm * max(1, len(terms)))()
    for q, t in zip(arr, terms):
        q.a, q.b, q.grad, q.n = m.p(t["a"]), m.p(t["b"]), m.p(t["grad"]), t["n"]
        q.target, q.scale, q.mode, q.out = t["target"], t["scale"], t["mode"], t["out"]
    return arr


def _wn_bwd_args(m, c):
    import kantts._hip as hip

    a = hip.WnBwdArgs()
    for l in range(min(len(c["desc"]), WN_BWD_MAX)):
        a.dw[l], a.desc[l] = m.p(c["dw"][l]), c["desc"][l]
    for l, t in enumerate(c["tile0"][:WN_BWD_MAX + 1]):
        a.tile0[l] = t
    a.nl = c.get("nl", len(c["desc"]))
    return a


def _invoke(L_, m, c):
    """one call of the table through the C ABI"""
    import kantts._hip as hip

    ep, s, p = c["ep"], hip.stream(), m.p
    if ep == "kantts_masked_l1":
        return L_.kantts_masked_l1(p(c["pred"]), p(c["target"]), p(c["lens"]), p(c["loss"]), p(c["grad"]), c["B"], c["T"], c["C"], s)
    if ep == "kantts_masked_l1_many":
        return L_.kantts_masked_l1_many(_loss_terms(m, c["terms"]) if c["terms"] is not None else None,
                                        c.get("nterms", len(c["terms"] or ())), p(c["losses"]), s)
    if ep == "kantts_elem_loss":
        return L_.kantts_elem_loss(p(c["a"]), p(c["b"]), c["target"], c["mode"], c["scale"], p(c["loss"]), p(c["grad"]), c["n"], s)
    if ep == "kantts_elem_loss_many":
        return L_.kantts_elem_loss_many(_eloss_terms(m, c["terms"]) if c["terms"] is not None else None,
                                        c.get("nterms", len(c["terms"] or ())), p(c["losses"]), s)
    if ep == "kantts_scale_many":
        count = c.get("count", len(c["x"]))
        xs = (ctypes.c_void_p * max(1, len(c["x"])))(*[p(x) for x in c["x"]])
        ns = (ctypes.c_longlong * max(1, len(c["n"])))(*c["n"])
        return L_.kantts_scale_many(None if c.get("x_null") else xs, ns, count, p(c["scale"]), s)
    if ep == "kantts_sumsq":
        return L_.kantts_sumsq(None if c["x"] is None else p(c["x"]) + c.get("byte_shift", 0), p(c["out"]), c["n"], s)
    if ep == "kantts_sumsq_det":
        return L_.kantts_sumsq_det(None if c["x"] is None else p(c["x"]) + c.get("byte_shift", 0), p(c["out"]), p(c["ws"]),
                                   c["ws_floats"], c["n"], s)
    if ep == "kantts_adam_step":
        return L_.kantts_adam_step(p(c["p"]), p(c["g"]), p(c["m"]), p(c["v"]), c["n"], c["lr"], c["b1"], c["b2"], c["eps"], c["wd"],
                                   c["bc1"], c["bc2"], p(c["gnorm"]), c["max_norm"], p(c["dyn"]), s)
    if ep == "kantts_weight_norm_fwd":
        return L_.kantts_weight_norm_fwd(p(c["v"]), p(c["g"]), p(c["w"]), c["rows"], c["cols"], s)
    if ep == "kantts_weight_norm_bwd":
        return L_.kantts_weight_norm_bwd(p(c["dw"]), p(c["v"]), p(c["g"]), p(c["dv"]), p(c["dg"]), c["rows"], c["cols"], s)
    if ep == "kantts_weight_norm_strided_fwd":
        return L_.kantts_weight_norm_strided_fwd(p(c["v"]), p(c["g"]), p(c["w"]), c["rows"], c["cin"], c["K"], c["rs"], c["cs"], c["ks"], s)
    if ep == "kantts_weight_norm_strided_bwd":
        return L_.kantts_weight_norm_strided_bwd(p(c["dw"]), p(c["v"]), p(c["g"]), p(c["dv"]), p(c["dg"]), c["rows"], c["cin"], c["K"],
                                                 c["rs"], c["cs"], c["ks"], s)
    if ep == "kantts_weight_norm_tap_images":
        return L_.kantts_weight_norm_tap_images(p(c["v"]), p(c["g"]), p(c["w"]), m.h(c["wf"]), m.h(c["wd"]), c["rows"], c["cin"], c["K"],
                                                c["groups"], s)
    if ep == "kantts_weight_norm_table":
        return L_.kantts_weight_norm_table(p(0), p(0), p(0), p(0), p(c["tab"]), len(c["table"]), c["tiles"], s)
    if ep == "kantts_weight_norm_table_bwd":
        return L_.kantts_weight_norm_table_bwd(p(0), p(c["grad"]), p(c["tab"]), ctypes.byref(_wn_bwd_args(m, c)), s)
    raise AssertionError(ep)


def _run_calls(L_, m, case, calls):
    for c in calls:
        if c["ep"] == "same":
            continue
        if c["ep"] == "ticket":
            word = m.result().view(np.uint32)[c["off"]]
            assert word == 0, "%s: the ticket word reads %d after the call" % (case.name, word)
            continue
        with np.errstate(all="ignore"):
            rc = _invoke(L_, m, c)
        assert rc == c["rc"], "%s %s: return code %d, expected %d" % (case.name, c["ep"], rc, c["rc"])


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


def _bf16_rne(x):
    """float32 array -> its round-to-nearest-even bf16 bit patterns (uint16)"""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def _ulps(a, b):
    return abs(int(np.asarray(a, F32).view(np.int32)) - int(np.asarray(b, F32).view(np.int32)))


def _check(case, leg, got, raw):
    """the arena after the calls against the reference, region by region; what no region covers must hold its old bits"""
    ref = case.reference()
    g16, r16 = got.view(np.uint16), raw.view(np.uint16)
    covered = np.zeros(g16.size, dtype=bool)  # in 2-byte units: a bf16 image may end inside a float
    c = _c()

    def cover(idx):
        covered[2 * idx] = True
        covered[2 * idx + 1] = True

    for r in ref.regions.values():
        what, kind, idx = "%s %s %s" % (case.name, r["ep"], r["what"]), r["kind"], r["idx"]
        if kind == "same":
            src = g16 if r["u16"] else got.view(np.uint32)
            assert np.array_equal(src[r["a"]], src[r["b"]]), "%s: the bits differ" % what
            continue
        if kind == "bf16":
            covered[r["u16"]] = True
            w = got[r["src"]]
            have, want = g16[r["u16"]], _bf16_rne(w)
            nan = np.isnan(w)
            assert np.array_equal(have[~nan], want[~nan]), "%s: not the bf16 of the w this launch wrote" % what
            assert ((have[nan] & 0x7F80) == 0x7F80).all() and ((have[nan] & 0x7F) != 0).all(), "%s: NaN lost" % what
            continue
        cover(idx)
        if kind == "scratch":
            continue
        have = got[idx]
        if kind == "bits":
            assert np.array_equal(have, r["want"]) and not np.isnan(r["want"]).any(), "%s: not the exact value" % what
        elif kind == "exact":
            want = ref.val[idx]
            if np.isnan(want).any():
                assert np.isnan(have).all(), "%s: %r, expected NaN" % (what, have)
            else:
                assert np.array_equal(have.astype(F64), want), "%s: %r, expected exactly %r" % (what, have, want)
        elif kind == "sign":
            sg = r["sign"]
            assert np.array_equal(np.sign(have).astype(np.int8), sg), "%s: sign / zero pattern" % what
            if (sg != 0).any():
                mags = np.unique(np.abs(have[sg != 0]))
                assert mags.size == 1, "%s: %d different magnitudes" % (what, mags.size)
                slack = 1 if (leg.name == "gpu" and r["one_ulp_on_device"] and not r["pow2"]) else 0
                assert _ulps(mags[0], r["mag"]) <= slack, "%s: magnitude %r, expected %r (%d ulp allowed)" % (what, mags[0], r["mag"], slack)
        else:  # measured
            want, S = ref.val[idx], ref.S[idx]
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(have), nan), "%s: NaN where the reference has none, or none where it has one" % what
            err = np.abs(have.astype(F64) - want)[~nan]
            S, want = S[~nan], want[~nan]
            assert np.array_equal(err[S == 0], np.zeros(int((S == 0).sum()))), "%s: an element that must be exact is not" % what
            ratio = float((err[S > 0] / (U * S[S > 0])).max()) / c if (S > 0).any() else 0.0
            key = (leg.name, r["ep"])
            if ratio >= _WORST.get(key, (-1.0, None))[0]:
                _WORST[key] = (ratio, case.name)
            print("%s %s: max |err| %.3e, ratio to c*2^-24*S %.4f (c = %.3f)" % (leg.name, what, float(err.max()) if err.size else 0.0, ratio, c))
            assert ratio <= leg.R, "%s: error %.3f x the bound c*2^-24*S (R = %g)" % (what, ratio, leg.R)
            if r.get("cap_abs") is not None:
                assert err.size == 0 or float(err.max()) <= r["cap_abs"], "%s: max |err| %.3e > %.1e" % (what, float(err.max()), r["cap_abs"])
            if r.get("cap_rel") is not None:
                assert (err <= r["cap_rel"] * np.abs(want)).all(), "%s: relative error %.3e" % (what, float((err / np.abs(want)).max()))
    same = g16[~covered] == r16[~covered]
    assert same.all(), "%s: %d two-byte words outside the outputs were written" % (case.name, int((~same).sum()))


def _run_case(case, leg):
    import kantts._hip as hip

    raw, calls = case.built()
    m = _Mem(raw, leg)
    _run_calls(hip.lib(), m, case, calls)
    _check(case, leg, m.result(), raw)


@pytest.mark.parametrize("group", _GROUPS)
@pytest.mark.parametrize("leg", _leg_params())
def test_step_tail_matches_the_fp64_interpreter(leg, group):
    leg = _Leg(leg)
    try:
        with leg.context():
            for case in _TABLE[group]:
                _run_case(case, leg)
    finally:
        _flush()


def test_c_comes_from_the_fp32_evaluation_of_the_reference():
    """the measured ratio and c (recorded in step_tail_contract.json).  The ratio is pinned to the one recorded when the
    table was written: a case added later that is worse conditioned would otherwise loosen the bound of every other case"""
    c = _c()
    print("fp32 reference: worst ratio to 2^-24*S %.4f (%s), c = %.4f" % (_MEASURED["ratio"], _MEASURED["case"], c))
    assert c == 4.0 * _MEASURED["ratio"]
    assert 1.0 < _MEASURED["ratio"] <= 1.1 * RATIO_RECORDED, _MEASURED


def test_every_listed_branch_has_a_case():
    seen = {br for cs in _TABLE.values() for case in cs for br in case.branches}
    assert seen == set(_BRANCHES), sorted(set(_BRANCHES) ^ seen)
    called = {c["ep"] for cs in _TABLE.values() for case in cs for c in case.built()[1]} - {"same", "ticket"}
    assert called == set(_ENTRY_POINTS), sorted(set(_ENTRY_POINTS) ^ called)
    _record("branches", sorted(seen))


# ---------------------------------------------------------------------------------------------------------------------
# 5. refusals
def _refusals():
    """(name, the model implements it, build): each call returns its code and writes nothing"""
    out = []

    def add(name, build, emu=False):
        out.append((name, emu, build))

    def l1(b, rc=E_BADARG, null=None, **kw):
        t = _l1_data(b, 2, 3, 4, [3, 1])
        t.update(kw)
        c = dict(t, loss=b.f32([0.5]))
        if null:
            c[null] = None
        b.call("kantts_masked_l1", rc=rc, **c)

    for null in ("pred", "target", "lens", "loss"):
        add("masked_l1 %s NULL" % null, lambda b, null=null: l1(b, null=null))
    add("masked_l1 B < 0", lambda b: l1(b, B=-1))
    add("masked_l1 T < 0", lambda b: l1(b, T=-1))
    add("masked_l1 C < 1", lambda b: l1(b, C=0))

    def l1many(b, nterms=None, terms_null=False, losses_null=False, **kw):
        terms = [_l1_data(b, 2, 3, 4, [3, 1]) for _ in range(6 if nterms == 6 else 2)]
        terms[1].update(kw)
        b.call("kantts_masked_l1_many", rc=E_BADARG, terms=None if terms_null else terms, nterms=len(terms) if nterms is None else nterms,
               losses=None if losses_null else b.f32(np.zeros(6)))

    add("masked_l1_many nterms 0", lambda b: l1many(b, nterms=0))
    add("masked_l1_many nterms 6", lambda b: l1many(b, nterms=6))
    add("masked_l1_many terms NULL", lambda b: l1many(b, terms_null=True, nterms=2))
    add("masked_l1_many losses NULL", lambda b: l1many(b, losses_null=True))
    add("masked_l1_many pred NULL", lambda b: l1many(b, pred=None))
    add("masked_l1_many lens NULL", lambda b: l1many(b, lens=None))
    add("masked_l1_many C < 1", lambda b: l1many(b, C=0))
    add("masked_l1_many B < 0", lambda b: l1many(b, B=-2))

    def eloss(bd, **kw):
        c = dict(a=bd.f32(bd.randn(9)), b=bd.f32(bd.randn(9)), grad=bd.f32(n=9), n=9, target=1.0, scale=0.1, mode=0, loss=bd.f32([0.5]))
        c.update(kw)
        bd.call("kantts_elem_loss", rc=E_BADARG, **c)

    add("elem_loss a NULL", lambda bd: eloss(bd, a=None))
    add("elem_loss b NULL in mode 0", lambda bd: eloss(bd, b=None))
    add("elem_loss loss NULL", lambda bd: eloss(bd, loss=None))
    add("elem_loss n < 0", lambda bd: eloss(bd, n=-1))
    add("elem_loss mode 2", lambda bd: eloss(bd, mode=2))

    def elossmany(bd, nterms=None, terms_null=False, losses_null=False, **kw):
        mk = lambda: dict(a=bd.f32(bd.randn(9)), b=bd.f32(bd.randn(9)), grad=bd.f32(n=9), n=9, target=1.0, scale=0.1, mode=0, out=0)
        terms = [mk() for _ in range(65 if nterms == 65 else 2)]
        terms[1].update(kw)
        bd.call("kantts_elem_loss_many", rc=E_BADARG, terms=None if terms_null else terms, nterms=len(terms) if nterms is None else nterms,
               losses=None if losses_null else bd.f32(np.zeros(2)))

    add("elem_loss_many nterms 0", lambda bd: elossmany(bd, nterms=0))
    add("elem_loss_many nterms 65", lambda bd: elossmany(bd, nterms=65))
    add("elem_loss_many terms NULL", lambda bd: elossmany(bd, terms_null=True, nterms=2))
    add("elem_loss_many losses NULL", lambda bd: elossmany(bd, losses_null=True))
    add("elem_loss_many mode 2", lambda bd: elossmany(bd, mode=2))
    add("elem_loss_many out < 0", lambda bd: elossmany(bd, out=-1))
    add("elem_loss_many n < 0", lambda bd: elossmany(bd, n=-1))
    add("elem_loss_many a NULL", lambda bd: elossmany(bd, a=None))
    add("elem_loss_many b NULL in mode 0", lambda bd: elossmany(bd, b=None))

    def scale(b, count=None, n=(5, 9), null_k=None, **kw):
        xs = [b.f32(b.randn(max(1, k))) for k in n]
        if null_k is not None:
            xs[null_k] = None
        c = dict(x=xs, n=list(n), scale=b.f32([0.5]), count=len(n) if count is None else count)
        c.update(kw)
        b.call("kantts_scale_many", rc=E_BADARG, **c)

    add("scale_many count 65", lambda b: scale(b, n=(3,) * 65, count=65))
    add("scale_many count < 0", lambda b: scale(b, count=-1))
    add("scale_many a NULL x[k]", lambda b: scale(b, null_k=1))
    add("scale_many n[k] < 0", lambda b: scale(b, n=(5, -1)))
    add("scale_many x NULL", lambda b: scale(b, x_null=True))
    add("scale_many scale NULL", lambda b: scale(b, scale=None))

    def sumsq(b, det, rc=E_BADARG, **kw):
        c = dict(x=b.f32(b.randn(40)), out=b.f32([0.5]), n=33)
        if det:
            c.update(ws=b.f32(np.zeros(DET_WS)), ws_floats=DET_WS)
        c.update(kw)
        b.call("kantts_sumsq_det" if det else "kantts_sumsq", rc=rc, **c)

    for det in (False, True):
        nm = "sumsq_det" if det else "sumsq"
        add("%s pointer + 4 bytes" % nm, lambda b, det=det: sumsq(b, det, byte_shift=4))
        add("%s x NULL" % nm, lambda b, det=det: sumsq(b, det, x=None))
        add("%s out NULL" % nm, lambda b, det=det: sumsq(b, det, out=None))
        add("%s n < 0" % nm, lambda b, det=det: sumsq(b, det, n=-1))
    add("sumsq_det ws_floats 1024", lambda b: sumsq(b, True, rc=E_WORKSPACE, ws_floats=1024), emu=True)
    add("sumsq_det workspace NULL", lambda b: sumsq(b, True, ws=None))

    def adam(b, **kw):
        c = dict(p=b.f32(b.randn(9)), g=b.f32(b.randn(9)), m=b.f32(b.randn(9)), v=b.f32(b.randn(9) ** 2), n=9, lr=1e-3, b1=0.9, b2=0.98,
                 eps=1e-9, wd=0.0, bc1=0.1, bc2=0.02, gnorm=None, max_norm=0.0, dyn=None)
        c.update(kw)
        b.call("kantts_adam_step", rc=E_BADARG, **c)

    for null in "pgmv":
        add("adam_step %s NULL" % null, lambda b, null=null: adam(b, **{null: None}))
    add("adam_step n < 0", lambda b: adam(b, n=-1))

    def wn(b, ep, **kw):
        t = _wn_tensors(b, (12, 3, 5, 3))
        n = 180
        c = dict(t, w=b.f32(n=n), dw=b.f32(b.randn(n)), dv=b.f32(n=n), dg=b.f32(n=12), cols=15, rs=3, cs=1, ks=36, wf=2 * b.f32(n=n // 2),
                 wd=2 * b.f32(n=n // 2))
        c.update(kw)
        b.call(ep, rc=E_BADARG, **c)

    for ep, nulls in (("kantts_weight_norm_fwd", "vgw"), ("kantts_weight_norm_strided_fwd", "vgw"), ("kantts_weight_norm_tap_images", "vgw"),
                      ("kantts_weight_norm_bwd", ("dw", "v", "g", "dv", "dg")), ("kantts_weight_norm_strided_bwd", ("dw", "v", "g", "dv", "dg"))):
        for null in nulls:
            add("%s %s NULL" % (ep[7:], null), lambda b, ep=ep, null=null: wn(b, ep, **{null: None}))
        add("%s rows < 0" % ep[7:], lambda b, ep=ep: wn(b, ep, rows=-1))
    add("weight_norm_fwd cols < 1", lambda b: wn(b, "kantts_weight_norm_fwd", cols=0))
    add("weight_norm_bwd cols < 1", lambda b: wn(b, "kantts_weight_norm_bwd", cols=0))
    add("weight_norm_strided_fwd cin < 1", lambda b: wn(b, "kantts_weight_norm_strided_fwd", cin=0))
    add("weight_norm_strided_bwd K < 1", lambda b: wn(b, "kantts_weight_norm_strided_bwd", K=0))
    add("weight_norm_tap_images rows % groups", lambda b: wn(b, "kantts_weight_norm_tap_images", groups=5))
    add("weight_norm_tap_images groups < 1", lambda b: wn(b, "kantts_weight_norm_tap_images", groups=0))

    def table_bwd(b, nl=None, null_l=None):
        t = _wn_tensors(b, (12, 3, 5, 3))
        t.update(w_off=b.f32(n=180), wf_off=-1, wd_off=-1)
        params = b.arena.n
        b.f32(n=params)
        tab, dw = b.raw(_desc_bytes(t, 0)), b.f32(b.randn(180))
        desc = [0] * (WN_BWD_MAX if nl else 2)
        dws = [dw] * len(desc)
        if null_l is not None:
            dws[null_l] = None
        b.call("kantts_weight_norm_table_bwd", rc=E_BADARG, table=[t], tab=tab, desc=desc, dw=dws, tile0=[2 * l for l in range(len(desc) + 1)],
               grad=params, nl=nl if nl else len(desc))

    add("weight_norm_table_bwd nl 65", lambda b: table_bwd(b, nl=65))
    add("weight_norm_table_bwd a NULL dw[l]", lambda b: table_bwd(b, null_l=1))
    return out


_REFUSALS = _refusals()


@pytest.mark.parametrize("leg", _leg_params())
def test_refusals(leg):
    """each returns its code and leaves every byte of the arena as it was.  The emulated ABI has no argument checks: only
    the refusals its model implements run there"""
    import kantts._hip as hip

    leg = _Leg(leg)
    ran = 0
    with leg.context():
        for name, emu, build in _REFUSALS:
            if leg.name == "emu" and not emu:
                continue
            b = _Builder(name)
            build(b)
            raw = b.finish()
            m = _Mem(raw, leg)
            for c in b.calls:
                rc = _invoke(hip.lib(), m, c)
                assert rc == c["rc"], "%s: return code %d, expected %d" % (name, rc, c["rc"])
            assert np.array_equal(m.result().view(np.uint32), raw.view(np.uint32)), "%s: a refused call wrote" % name
            ran += 1
    assert ran == (sum(emu for _, emu, _ in _REFUSALS) if leg.name == "emu" else len(_REFUSALS))
