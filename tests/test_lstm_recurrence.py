"""The LSTM recurrence kernels of kan-tts_amd/csrc/lstm.hip, step by step against a float64 time loop.

kantts_lstm_fwd / kantts_lstm_bwd / kantts_lstm_cell are driven through the raw C ABI: no GEMM sits between the inputs and
what is compared.  Every case runs on two back ends: ``kernel_source`` (the kernel sources compiled for the host,
tests/hipemu; part of the CPU suite) and ``gpu`` (the device library).

References (both plain torch, written below):
  R32  the time loop in float64 with ``lengths`` / ``reverse`` semantics; its autograd gradient with respect to ``gx`` is the
       expected ``dgates`` (gate-major (ndir, B, T, 4H)).  Expected values of the fp32 form (precision 0).
  Rbf  the same loop with the operand rounding of the bf16 forms (precision 1): W_hh and h_{t-1} rounded to bf16 inside
       the recurrent product only, and the gradient that flows from a step's pre-activations into h_{t-1} through W_hh^T
       rounded to bf16 (the stored dgates are not).  Cell state, gates and outputs stay unrounded.

Compared per case: ``out``, ``c_save`` at t < len, and the ``dgates`` of a backward call that is fed the kernel's own saved
state and a random ``dout``.  The error is taken per row (dir, b, t) as max-abs over the row and the worst row is held
against the bound; ``out`` and ``dgates`` at t >= len must be exactly 0.0.  ``out`` / ``dgates`` / the saved state start as
NaN, so an unwritten cell shows, and all four live inside larger buffers with 8 guard rows of a sentinel on either side,
so a stray write shows as an assertion.

Bounds (from the references, never from the kernels): ``floor`` = max over rows |reference in float32 - reference in
float64|, evaluated inside the test.
  fp32 form        max(4 floor, 2e-5 max(1, max|ref|))     (4: tests/test_ctc.py; 2e-5: tests/test_ops_sweep.py)
  bf16 forms / Rbf max(4 floor_bf, one_flip), one_flip = 2^-7 max|W_hh| max|rounded operand| (|h| <= 1 forward,
                   max|dgates_ref| backward): what ONE bf16 operand landing on the other side of a rounding tie moves a
                   pre-activation by -- neither the kernel nor the reference controls that.
Every check prints the worst row error beside its bound and floor (pytest -s shows them)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

H, G = 128, 512
GUARD = 8  # guard rows before and after every output buffer
SENTINEL = 12345.0
_HAS_CLANG = os.path.exists(os.environ.get("HIPEMU_CXX", "/opt/rocm/lib/llvm/bin/clang++"))

RESIDUE_T = [1, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 24, 31, 33]
DIR_FORMS = [(2, 0), (1, 0), (1, 1)]  # (ndir, reverse_first)


# ------------------------------------------------------------------------------------------------ back ends
class _Backend:
    def __init__(self, name):
        self.name = name
        self.device = "cuda" if name == "gpu" else "cpu"

    def __enter__(self):
        import kantts._hip as hip
        import util

        if self.name == "gpu":
            hip.lib()  # fails loudly when the device library is missing
            self._ctx = None
        else:
            self._ctx = util.kernel_source_on_cpu()
            self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self._ctx is not None:
            self._ctx.__exit__(*exc)
        return False


@pytest.fixture(params=[
    pytest.param("kernel_source", marks=pytest.mark.skipif(not _HAS_CLANG, reason="the host build of the kernel sources "
                                                                                  "needs the ROCm clang")),
    pytest.param("gpu", marks=pytest.mark.gpu)])
def be(request):
    with _Backend(request.param) as b:
        yield b


# ------------------------------------------------------------------------------------------------ references
def _bf(x):
    """Round to bf16 (nearest even), keep the dtype.  A float64 value passes through float32 first, as the kernels'
    operands do."""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


class _RoundValue(torch.autograd.Function):
    """bf16-rounded value, straight-through gradient: the h_{t-1} operand of the recurrent product."""

    @staticmethod
    def forward(ctx, x):
        return _bf(x)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundGrad(torch.autograd.Function):
    """Identity whose incoming gradient is rounded to bf16: the d(pre-activation) operand of the product with W_hh^T."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return _bf(g)


def _reference(gx, whh, bhh, lens, dout, ndir, rev_first, bf, dtype):
    """The time loop.  gx (B, T, ndir 4H), whh (ndir, 4H, H), bhh (ndir, 4H) or None, lens (B,) or None, dout (B, T, ndir H).
    Returns out (ndir, B, T, H), c (ndir, B, T, H), dgates (ndir, B, T, 4H) in ``dtype``; rows at t >= len are zero."""
    B, T = gx.shape[:2]
    gx = gx.to(dtype).clone().requires_grad_(True)
    whh, dout = whh.to(dtype), dout.to(dtype)
    ln = torch.full((B,), T, dtype=torch.int64) if lens is None else lens.to(torch.int64)
    outs, cs = [], []
    for d in range(ndir):
        rev = bool(rev_first) or d == 1
        w = _bf(whh[d]) if bf else whh[d]
        bias = gx.new_zeros(G) if bhh is None else bhh[d].to(dtype)
        h, c = gx.new_zeros(B, H), gx.new_zeros(B, H)
        o_t, c_t = [None] * T, [None] * T
        for t in (range(T - 1, -1, -1) if rev else range(T)):
            rec = F.linear(_RoundValue.apply(h), w) if bf else F.linear(h, w)
            pre = gx[:, t, d * G:(d + 1) * G] + bias + (_RoundGrad.apply(rec) if bf else rec)
            i, f, g, o = pre.chunk(4, -1)
            c_new = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h_new = torch.sigmoid(o) * torch.tanh(c_new)
            live = (t < ln)[:, None]
            c, h = torch.where(live, c_new, c), torch.where(live, h_new, h)
            o_t[t] = torch.where(live, h_new, torch.zeros_like(h_new))
            c_t[t] = torch.where(live, c_new, torch.zeros_like(c_new))
        outs.append(torch.stack(o_t, 1))
        cs.append(torch.stack(c_t, 1))
    out = torch.stack(outs, 0)  # (ndir, B, T, H)
    loss = (out * dout.view(B, T, ndir, H).permute(2, 0, 1, 3)).sum()
    (dgx,) = torch.autograd.grad(loss, gx)
    return out.detach(), torch.stack(cs, 0).detach(), dgx.view(B, T, ndir, G).permute(2, 0, 1, 3).contiguous()


# ------------------------------------------------------------------------------------------------ the kernels
def _guarded(shape, row, fill, device):
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD * row,), SENTINEL, device=device)
    inner = buf[GUARD * row:GUARD * row + n]
    inner.fill_(fill)
    return buf, inner.view(shape)


def _guards_intact(buf, row):
    return bool((buf[:GUARD * row] == SENTINEL).all()) and bool((buf[-GUARD * row:] == SENTINEL).all())


def _run_kernels(be, gx, whh, bhh, lens, dout, ndir, rev_first, precision):
    """kantts_lstm_fwd, then kantts_lstm_bwd on the saved state it left.  Returns out (ndir, B, T, H), c_save, dgates on
    the host.  All four output buffers are interior slices of larger ones; the guards are checked here."""
    import kantts._hip as hip

    B, T = gx.shape[:2]
    nan = float("nan")

    def dev(t):
        return None if t is None else t.contiguous().to(be.device)

    gx, whh, bhh, dout = dev(gx), dev(whh), dev(bhh), dev(dout)
    lens = None if lens is None else dev(lens.to(torch.int32))
    bufs = {"out": _guarded((B, T, ndir * H), ndir * H, nan, be.device) + (ndir * H,),
            "gates_save": _guarded((ndir, B, T, G), G, nan, be.device) + (G,),
            "c_save": _guarded((ndir, B, T, H), H, nan, be.device) + (H,),
            "dgates": _guarded((ndir, B, T, G), G, nan, be.device) + (G,)}
    out, gates, cst, dg = (bufs[k][1] for k in ("out", "gates_save", "c_save", "dgates"))
    L, p, s = hip.lib(), hip.ptr, hip.stream()
    assert L.kantts_lstm_fwd(p(gx), p(whh), p(bhh), p(lens), p(out), p(gates), p(cst), B, T, H, ndir, rev_first, precision,
                             s) == 0
    assert L.kantts_lstm_bwd(p(dout), p(whh), p(lens), p(gates), p(cst), p(dg), B, T, H, ndir, rev_first, precision, s) == 0
    if be.device == "cuda":
        torch.cuda.synchronize()
    for name, (buf, _, row) in bufs.items():
        assert _guards_intact(buf, row), "%s: a guard row around the buffer was written" % name
    return out.cpu().view(B, T, ndir, H).permute(2, 0, 1, 3).contiguous(), cst.cpu(), dg.cpu()


def _worst(err, valid):
    """err (ndir, B, T) row errors; the worst row among ``valid`` (B, T) and where it is."""
    e = torch.where(valid[None].expand_as(err), err, torch.zeros_like(err))
    if not e.numel():
        return 0.0, None
    i = int(torch.nan_to_num(e, nan=float("inf")).argmax())
    return float(e.reshape(-1)[i]), tuple(int(v) for v in np.unravel_index(i, tuple(e.shape)))


def _check(be, tag, gx, whh, bhh, lens, dout, ndir, rev_first, precision, finite=False):
    """One case: kernels against the reference of their precision, row by row.  Returns {quantity: (worst, bound, floor)}."""
    B, T = gx.shape[:2]
    bf = precision == 1
    got = _run_kernels(be, gx, whh, bhh, lens, dout, ndir, rev_first, precision)
    r64 = _reference(gx, whh, bhh, lens, dout, ndir, rev_first, bf, torch.float64)
    r32 = _reference(gx, whh, bhh, lens, dout, ndir, rev_first, bf, torch.float32)
    ln = torch.full((B,), T) if lens is None else lens.to(torch.int64).clamp(0, T)
    valid = torch.arange(T)[None, :] < ln[:, None]  # (B, T)
    everywhere = torch.ones_like(valid)
    pad = (~valid)[None, :, :, None]
    wmax = float(whh[:ndir].abs().max())
    figures = {}
    for name, a, r, f32, rows in (("out", got[0], r64[0], r32[0], everywhere), ("c_save", got[1], r64[1], r32[1], valid),
                                  ("dgates", got[2], r64[2], r32[2], everywhere)):
        if name != "c_save":  # the padded tail: exactly zero, every cell written
            tail = a.masked_select(pad.expand_as(a))
            assert bool((tail == 0).all()), "%s %s: %d cells at t >= len are not exactly 0.0" % (
                tag, name, int((tail != 0).sum()))
        if finite:
            assert bool(torch.isfinite(a.masked_select(rows[None, :, :, None].expand_as(a))).all()), \
                "%s %s: NaN or Inf" % (tag, name)
        floor, _ = _worst((f32.double() - r).abs().amax(-1), rows)
        rmax = float(r.abs().max()) if r.numel() else 0.0
        if bf:
            bound = max(4 * floor, 2.0 ** -7 * wmax * (rmax if name == "dgates" else 1.0))
        else:
            bound = max(4 * floor, 2e-5 * max(1.0, rmax))
        worst, where = _worst((a.double() - r).abs().amax(-1), rows)
        figures[name] = (worst, bound, floor)
        print("lstm-recurrence %-13s prec=%d %-34s %-7s worst row %.3e  bound %.3e  floor %.3e  at (dir,b,t)=%s" % (
            be.name, precision, tag, name, worst, bound, floor, where))
        assert worst <= bound, "%s %s: worst row error %.3e at (dir, b, t) = %s beyond %.3e (floor %.3e)" % (
            tag, name, worst, where, bound, floor)
    return figures


def _inputs(seed, B, T, ndir, gx_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    gx = torch.randn(B, T, ndir * G, generator=g) * gx_scale
    whh = torch.randn(ndir, G, H, generator=g) * 0.08
    bhh = torch.randn(ndir, G, generator=g) * 0.1
    dout = torch.randn(B, T, ndir * H, generator=g)
    return gx, whh, bhh, dout


def _residue_lengths(T):
    """T, 1, 0, T + 5 (behaves as T), and for every residue r the largest length <= T with len % 8 == r."""
    ln = [T, 1, 0, T + 5]
    for r in range(8):
        v = T - ((T - r) % 8)
        if 0 <= v <= T and v not in ln:
            ln.append(v)
    return torch.tensor(ln, dtype=torch.int32)


# ------------------------------------------------------------------------------------------------ the cases
def _case_residues(be, precision, T):
    """Case 1: lengths on every residue of the prefetch chunks (8 forward, 4 + 4 backward), both directions, with and
    without the recurrent bias, with and without lengths."""
    lens = _residue_lengths(T)
    B = len(lens)
    for ndir, rev in DIR_FORMS:
        gx, whh, bhh, dout = _inputs(1000 * T + 10 * ndir + rev, B, T, ndir)
        for with_bias, with_lens in ((True, True), (False, True), (True, False), (False, False)):
            tag = "residues T=%d ndir=%d rev=%d%s%s" % (T, ndir, rev, "" if with_bias else " nobias", "" if with_lens else " nolens")
            _check(be, tag, gx, whh, bhh if with_bias else None, lens if with_lens else None, dout, ndir, rev, precision)


def _case_long(be, precision):
    """Case 3: the postnet's regime (about 600 steps), where error compounds."""
    gx, whh, bhh, dout = _inputs(640, 2, 640, 2)
    return _check(be, "long T=640", gx, whh, bhh, torch.tensor([640, 613], dtype=torch.int32), dout, 2, 0, precision)


@pytest.mark.parametrize("T", RESIDUE_T)
@pytest.mark.parametrize("precision", [0, 1])
def test_chunk_residues(be, precision, T):
    _case_residues(be, precision, T)


@pytest.mark.parametrize("precision", [0, 1])
def test_lone_reversed_direction_is_direction_1_of_a_pair(be, precision):
    """Case 2: reverse_first = 1 with one direction is direction 1 of a two-direction call with the same weights, bit for
    bit (same arithmetic, same order)."""
    B, T = 3, 11
    lens = torch.tensor([T, 4, 1], dtype=torch.int32)
    gx, whh, bhh, dout = _inputs(41 + precision, B, T, 2, gx_scale=0.5)
    for b in (bhh, None):
        both = _run_kernels(be, gx, whh, b, lens, dout, 2, 0, precision)
        lone = _run_kernels(be, gx[..., G:], whh[1:], None if b is None else b[1:], lens, dout[..., H:], 1, 1, precision)
        valid = (torch.arange(T)[None, :] < lens[:, None])[None, :, :, None]
        assert torch.equal(lone[0], both[0][1:])
        assert torch.equal(lone[2], both[2][1:])
        assert torch.equal(torch.where(valid, lone[1], torch.zeros(())), torch.where(valid, both[1][1:], torch.zeros(())))


@pytest.mark.parametrize("precision", [0, 1])
def test_long_sequence(be, precision):
    """Case 3.  On the kernel-source back end the 640 steps were measured at 5 s (fp32 form) and 3 s (bf16 pair form) under
    the fibre scheduler, references included, so that back end runs them without the KANTTS_HOSTSIM_FULL switch."""
    _case_long(be, precision)


@pytest.mark.parametrize("precision", [0, 1])
def test_every_workgroup_of_a_wide_grid(be, precision):
    """Case 4: B = 33, both directions, random lengths -- all 66 (b, dir) workgroups are compared."""
    B, T = 33, 9
    gx, whh, bhh, dout = _inputs(33, B, T, 2)
    lens = torch.randint(0, T + 1, (B,), generator=torch.Generator().manual_seed(9), dtype=torch.int32)
    _check(be, "grid B=33 T=9", gx, whh, bhh, lens, dout, 2, 0, precision)


@pytest.mark.parametrize("precision", [0, 1])
def test_saturated_gates(be, precision):
    """Case 5: pre-activations of +-30, +-90 and +-1e4 beside ordinary ones -- the expf overflow path of
    lstm_sigmoid<false> and the v_exp / v_rcp path of the fast form.  Nothing may become NaN or Inf."""
    B, T = 4, 19
    gx, whh, bhh, dout = _inputs(5, B, T, 2)
    g = torch.Generator().manual_seed(55)
    big = torch.tensor([30.0, -30.0, 90.0, -90.0, 1e4, -1e4])[torch.randint(0, 6, gx.shape, generator=g)]
    gx = torch.where(torch.rand(gx.shape, generator=g) < 0.15, big, gx)
    lens = torch.tensor([T, 13, 8, 1], dtype=torch.int32)
    for ndir, rev in DIR_FORMS:
        _check(be, "saturated ndir=%d rev=%d" % (ndir, rev), gx[..., :ndir * G].contiguous(), whh[:ndir], bhh[:ndir], lens,
               dout[..., :ndir * H].contiguous(), ndir, rev, precision, finite=True)


@pytest.mark.parametrize("precision", [0, 1])
def test_negative_lengths_behave_as_zero(be, precision):
    """Case 6: a negative length is an empty sequence (lengths are clamped into [0, T]).  Without the lower clamp the tail
    loops of all four kernels start at a negative row: the guard rows in front of ``out`` / ``dgates`` catch it."""
    T = 5
    lens = torch.tensor([-3, 4, -1], dtype=torch.int32)
    for ndir, rev in DIR_FORMS:
        gx, whh, bhh, dout = _inputs(600 + 10 * ndir + rev, 3, T, ndir)
        _check(be, "negative lens ndir=%d rev=%d" % (ndir, rev), gx, whh, bhh, lens, dout, ndir, rev, precision)


def test_bf16_quad_kernels_in_a_fresh_process(be):
    """Case 7: lstm_fwd_kernel<true> / lstm_bwd_kernel<true> are selected by KANTTS_LSTM_PAIR=0 / KANTTS_LSTM_PAIR_BWD=0,
    which the launchers (device and host build alike) read once per process: one child process runs the residue cases
    and the long case at precision 1 and exits non-zero on a mismatch."""
    env = dict(os.environ, KANTTS_LSTM_PAIR="0", KANTTS_LSTM_PAIR_BWD="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), be.name], env=env, capture_output=True, text=True,
                       timeout=1500, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(r.stdout)
    assert r.returncode == 0 and "bf16 quad kernels ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.parametrize("with_c", [True, False])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("Hc", [1, 128, 130])
def test_lstm_cell(be, Hc, B, with_c):
    """Case 8: kantts_lstm_cell against the float64 cell update.  2e-6 absolute: libm expf / tanhf and a handful of fp32
    roundings on gates in (0, 1) / (-1, 1) and |c| of a few units (half an ulp of 4.0 is 2.4e-7)."""
    import kantts._hip as hip

    g = torch.Generator().manual_seed(100 * Hc + 10 * B + with_c)
    gates = torch.randn(B, 4 * Hc, generator=g) * 1.5
    c_prev = torch.randn(B, Hc, generator=g) if with_c else None
    hb, h = _guarded((B, Hc), Hc, float("nan"), be.device)
    cb, c = _guarded((B, Hc), Hc, float("nan"), be.device)
    gd, cd = gates.to(be.device), None if c_prev is None else c_prev.to(be.device)
    assert hip.lib().kantts_lstm_cell(hip.ptr(gd), hip.ptr(cd), hip.ptr(h), hip.ptr(c), B, Hc, hip.stream()) == 0
    if be.device == "cuda":
        torch.cuda.synchronize()
    assert _guards_intact(hb, Hc) and _guards_intact(cb, Hc)
    i, f, gg, o = gates.double().chunk(4, -1)
    c_ref = torch.sigmoid(i) * torch.tanh(gg) + (torch.sigmoid(f) * c_prev.double() if with_c else 0.0)
    h_ref = torch.sigmoid(o) * torch.tanh(c_ref)
    ec, eh = float((c.cpu().double() - c_ref).abs().max()), float((h.cpu().double() - h_ref).abs().max())
    print("lstm-recurrence %-13s cell H=%d B=%d c_prev=%d  c %.3e  h %.3e  bound 2e-6" % (be.name, Hc, B, with_c, ec, eh))
    assert ec <= 2e-6 and eh <= 2e-6


# ------------------------------------------------------------------------------------------------ the child of case 7
if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (os.path.join(_root, "kan-tts_amd"), os.path.join(_root, "oracle"), _root, os.path.join(_root, "tests")):
        if _p not in sys.path:
            sys.path.insert(0, _p)
    assert os.environ.get("KANTTS_LSTM_PAIR") == "0" and os.environ.get("KANTTS_LSTM_PAIR_BWD") == "0"
    with _Backend(sys.argv[1]) as _be:
        for _T in RESIDUE_T:
            _case_residues(_be, 1, _T)
        _case_long(_be, 1)
    print("bf16 quad kernels ok")
