"""Per-slot row counts of the chunked vocoder (csrc/sconv.hip kantts_sconv_rows_launch, ChunkedVocoder.step(rows=...),
play_many, infer_hifigan --slots, sambert live_rows).

CPU leg: the kernel SOURCE on the host build (util.kernel_source_on_cpu), graph=False.  GPU leg: the same checks on the
device, graph both True and False.

Bounds.  Wherever two plays run the same arithmetic the assertion is torch.equal: an output element of sconv.hip is summed
chunk-major, tap-inner whatever the tile shape, and a row of a causal layer depends on rows before it only -- so a live row
of a ragged call, the same row of a plain call on the truncated input, and the same row of a lockstep play are the same
sum.  Against fp64 torch: 2e-5 for fp32 and max-abs <= 4e-2 * max(1, |ref|max) for bf16, the bounds of
test_chunked_vocoder.py for the same arithmetic.  Dead rows are checked exactly (a sentinel, or 0.0)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

from test_chunked_vocoder import _CONV_CASES, _G64, _POLY_CASES, _g64
from util import ROOT, assert_close, kernel_source_on_cpu

S = 3
SENTINEL = -1234.5  # what `out` and the state half to be written hold before a call
GUARD = 7.0
NAN = float("nan")


# ---------------------------------------------------------------------------------------------------------------------
# layer level
class _Layer:
    """One layer with seeded weights, a NON-zero carried state and S slots; `call` is one launch on fresh buffers."""

    def __init__(self, kind, case, prec, device, seed=3):
        g = torch.Generator().manual_seed(seed)
        if kind == "conv":
            Cin, N, K, step = case
            W = torch.randn(N, Cin, K, generator=g) / (Cin * K) ** 0.5
            b = torch.randn(N, generator=g)
            self.torch_w, self.torch_b = W, b
            w_knc = W.permute(2, 0, 1).flip(0)
        else:
            Cin, s, Cout, J = case
            step, K, N = 1, J, s * Cout
            W = torch.randn(Cin, Cout, J * s, generator=g) / (Cin * J) ** 0.5
            b = torch.randn(Cout, generator=g)
            self.torch_w, self.torch_b = W, b
            b = b.repeat(s)
            w_knc = W.view(Cin, Cout, J, s).permute(2, 3, 1, 0).reshape(J, N, Cin)
        self.Cin, self.N, self.K, self.step, self.H = Cin, N, K, step, (K - 1) * step
        self.prec, self.device, self.gen = prec, device, g
        self.ss = self.H * Cin + 8  # slot stride with guard floats behind every slot's state
        bf = prec == "bf16" and N > 1
        self.w = w_knc.to(torch.bfloat16 if bf else torch.float32).contiguous().to(device)
        self.b = b.to(device)
        self.hist = torch.randn(S, self.H, Cin, generator=g)

    def call(self, x, hist=None, rows=None, row_mul=1, zero_tail=False, res=None):
        """x (S, Tc, Cin) [, res (S, Tc, N)] -> out (S, Tc, N), state (S, H, Cin); asserts every guard float."""
        import kantts._hip as hip

        Tc, N, H, Cin = x.shape[1], self.N, self.H, self.Cin
        hist = self.hist if hist is None else hist
        arena = torch.full((2, S, self.ss), GUARD)
        arena[0, :, :H * Cin] = hist.reshape(S, H * Cin)
        arena[1, :, :H * Cin] = SENTINEL
        arena = arena.to(self.device)
        pad = 4 * N  # guard rows in front of and behind `out`
        flat = torch.full((S * Tc * N + 2 * pad,), GUARD).to(self.device)
        out = flat[pad:pad + S * Tc * N].view(S, Tc, N)
        out.fill_(SENTINEL)
        kw = {}
        if rows is not None:
            kw = dict(rows=torch.tensor(rows, dtype=torch.int32).to(self.device), row_mul=row_mul, zero_tail=zero_tail)
        ok = hip.sconv(x.contiguous().to(self.device), arena[0, 0], arena[1, 0], self.w, out, S=S, Tc=Tc, Cin=Cin, N=N,
                       K=self.K, step=self.step, hist_ss=self.ss,
                       precision=hip.PREC_BF16 if self.prec == "bf16" else hip.PREC_FP32, bias=self.b,
                       res=None if res is None else res.contiguous().to(self.device), **kw)
        assert ok
        assert bool((arena[:, :, H * Cin:] == GUARD).all()), "guard floats behind a slot's state were written"
        assert torch.equal(arena[0, :, :H * Cin].cpu(), hist.reshape(S, H * Cin)), "hist_in was written"
        assert bool((flat[:pad] == GUARD).all()) and bool((flat[-pad:] == GUARD).all()), "guard rows around out were written"
        return out.cpu().clone(), arena[1, :, :H * Cin].cpu().view(S, H, Cin).clone()


def _check_full_counts(kind, case, prec, device):
    """rows = [Tc] * S is the plain call, bit for bit, in out and in the state."""
    L = _Layer(kind, case, prec, device)
    for Tc in (8, 40):
        x = torch.randn(S, Tc, L.Cin, generator=L.gen)
        res = torch.randn(S, Tc, L.N, generator=L.gen)
        o0, h0 = L.call(x, res=res)
        o1, h1 = L.call(x, res=res, rows=[Tc] * S, zero_tail=L.N == 1)
        assert torch.equal(o0, o1) and torch.equal(h0, h1), (kind, case, prec, Tc)
        assert not bool((o0 == SENTINEL).any()) and not bool((h0 == SENTINEL).any())


# live rows per slot (row_mul = 1) / frame counts (row_mul = 2) for every row-tile shape of the launcher (Tc <= 16: one
# 16-row tile; <= 64: 64 rows; beyond: 128 rows): 0, 1, H - 1 = 29 and H + 1 = 31 for the (16, 16, 11, 3) case, the tile
# boundaries 16 / 64 / 128 and their neighbours, and Tc itself
_RAGGED = {
    (8, 1): [[0, 1, 8], [7, 3, 0]],
    (40, 1): [[0, 1, 40], [15, 16, 17], [29, 31, 39]],
    (130, 1): [[0, 1, 130], [15, 16, 17], [29, 31, 63], [64, 65, 129], [127, 128, 130]],
    (8, 2): [[0, 1, 4], [3, 2, 0]],
    (40, 2): [[0, 8, 20], [15, 7, 9]],
    (130, 2): [[0, 32, 65], [8, 31, 33], [1, 15, 64]],
}


def _check_ragged(case, prec, Tc, row_mul, device):
    L = _Layer("conv", case, prec, device)
    x = torch.randn(S, Tc, L.Cin, generator=L.gen)
    res = torch.randn(S, Tc, L.N, generator=L.gen)
    plain = {}  # n -> (out, state) of the plain call on the first n rows, all S slots

    def plain_call(n):
        if n not in plain:
            plain[n] = L.call(x[:, :n], res=res[:, :n])
        return plain[n]

    for counts in _RAGGED[(Tc, row_mul)]:
        live = [c * row_mul for c in counts]
        xn, rn = x.clone(), res.clone()
        for s, n in enumerate(live):
            xn[s, n:] = NAN  # rows the call must not load
            rn[s, n:] = NAN
        for zero_tail in ([False, True] if L.N == 1 else [False]):
            out, st = L.call(xn, res=rn, rows=counts, row_mul=row_mul, zero_tail=zero_tail)
            for s, n in enumerate(live):
                what = (case, prec, Tc, row_mul, counts, s, zero_tail)
                assert not bool(torch.isnan(out[s, :n]).any()) and not bool(torch.isnan(st[s]).any()), what
                want_state = torch.cat([L.hist[s], x[s, :n]], dim=0)[n:]
                assert torch.equal(st[s], want_state), ("state", what)
                if n == 0:
                    assert torch.equal(st[s], L.hist[s]), ("held state", what)
                else:
                    po, ps = plain_call(n)
                    assert torch.equal(out[s, :n], po[s]), ("live rows", what)
                    assert torch.equal(st[s], ps[s]), ("state against the plain call", what)
                tail = out[s, n:]
                assert bool((tail == (0.0 if zero_tail else SENTINEL)).all()), ("dead rows", what)


def _check_clamping(case, device):
    """Counts below 0 and above Tc / row_mul behave as 0 and Tc / row_mul (guards are asserted inside every call)."""
    L = _Layer("conv", case, "fp32", device)
    for Tc, row_mul in ((40, 1), (40, 2), (8, 1)):
        cap = Tc // row_mul
        x = torch.randn(S, Tc, L.Cin, generator=L.gen)
        o0, h0 = L.call(x, rows=[0, cap, 3], row_mul=row_mul, zero_tail=L.N == 1)
        o1, h1 = L.call(x, rows=[-5, cap + 9, 3], row_mul=row_mul, zero_tail=L.N == 1)
        assert torch.equal(o0, o1) and torch.equal(h0, h1), (case, Tc, row_mul)
        assert torch.equal(h1[0], L.hist[0])
        assert bool((o1[0] == (0.0 if L.N == 1 else SENTINEL)).all())
        assert not bool((o1[1] == SENTINEL).any())
        o2, h2 = L.call(x, rows=[-(2 ** 31), 2 ** 31 - 1, 3], row_mul=row_mul, zero_tail=L.N == 1)
        assert torch.equal(o0, o2) and torch.equal(h0, h2), (case, Tc, row_mul, "int32 extremes")


def _check_schedule(kind, case, prec, device):
    """Three slots play sequences of 40, 17 and 29 rows with a seeded random count per step (zeros included); the
    concatenated live output of every slot against torch in fp64."""
    L = _Layer(kind, case, prec, device)
    lens, Tc = [40, 17, 29], 8
    xs = [torch.randn(n, L.Cin, generator=L.gen) for n in lens]
    refs = []
    for x in xs:
        xd = x.double().t()[None]
        if kind == "conv":
            r = F.conv1d(F.pad(xd, (L.H, 0)), L.torch_w.double(), L.torch_b.double(), dilation=L.step)[0].t()
        else:
            Cin, s, Cout, J = case
            r = F.conv_transpose1d(xd, L.torch_w.double(), L.torch_b.double(), stride=s)[0, :, :x.shape[0] * s]
            r = r.t().reshape(x.shape[0], L.N)
        refs.append(r)
    rng = np.random.default_rng(11)
    pos, got = [0, 0, 0], [[], [], []]
    hist = torch.zeros(S, L.H, L.Cin)
    steps = 0
    while any(p < n for p, n in zip(pos, lens)):
        steps += 1
        assert steps < 200
        counts = [int(rng.integers(0, min(Tc, n - p) + 1)) for p, n in zip(pos, lens)]
        x = torch.full((S, Tc, L.Cin), NAN)
        for s in range(S):
            x[s, :counts[s]] = xs[s][pos[s]:pos[s] + counts[s]]
        out, hist = L.call(x, hist=hist, rows=counts, zero_tail=L.N == 1)
        for s in range(S):
            got[s].append(out[s, :counts[s]])
            pos[s] += counts[s]
    for s in range(S):
        y = torch.cat(got[s], dim=0)
        assert y.shape == refs[s].shape
        if prec == "fp32" or L.N == 1:
            assert_close(y, refs[s].float(), 2e-5, what="%s %s slot %d" % (kind, case, s))
        else:
            err = float((y.double() - refs[s]).abs().max())
            assert err <= 4e-2 * max(1.0, float(refs[s].abs().max())), (kind, case, s, err)


_FULL = [("conv", c) for c in _CONV_CASES] + [("poly", _POLY_CASES[0])]
_H30 = (16, 16, 11, 3)  # H = 30: the state straddles hist_in and the new rows at 29 / 31 live rows
_N1 = (32, 1, 7, 1)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("kind,case", _FULL, ids=lambda v: v if isinstance(v, str) else "_".join(map(str, v)))
def test_sconv_rows_full_counts_equal_the_plain_call(kind, case, prec):
    with kernel_source_on_cpu():
        _check_full_counts(kind, case, prec, "cpu")


@pytest.mark.parametrize("row_mul", [1, 2])
@pytest.mark.parametrize("Tc", [8, 40, 130])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_sconv_rows_ragged_counts(prec, Tc, row_mul):
    with kernel_source_on_cpu():
        _check_ragged(_H30, prec, Tc, row_mul, "cpu")


@pytest.mark.parametrize("row_mul", [1, 2])
@pytest.mark.parametrize("Tc", [8, 130])
def test_sconv_rows_ragged_counts_n1_zero_tail(Tc, row_mul):
    with kernel_source_on_cpu():
        _check_ragged(_N1, "fp32", Tc, row_mul, "cpu")


@pytest.mark.parametrize("case", [_H30, _N1], ids=["n16", "n1"])
def test_sconv_rows_counts_are_clamped_from_both_sides(case):
    with kernel_source_on_cpu():
        _check_clamping(case, "cpu")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("kind,case", [("conv", (80, 32, 7, 1)), ("conv", _H30), ("conv", _N1), ("poly", _POLY_CASES[1])],
                         ids=lambda v: v if isinstance(v, str) else "_".join(map(str, v)))
def test_sconv_rows_random_schedule_matches_torch(kind, case, prec):
    with kernel_source_on_cpu():
        _check_schedule(kind, case, prec, "cpu")


def _check_refusals(device):
    import kantts._hip as hip

    x, out, st = torch.zeros(1, 4, 16, device=device), torch.zeros(1, 4, 16, device=device), torch.zeros(2, 1, 64, device=device)
    w = torch.zeros(3, 16, 16, device=device)
    rows = torch.zeros(1, dtype=torch.int32, device=device)
    kw = dict(S=1, Tc=4, Cin=16, N=16, K=3, step=1, hist_ss=64, precision=hip.PREC_FP32)
    assert hip.sconv(x, st[0], st[1], w, out, rows=rows, row_mul=2, **kw) is True
    with pytest.raises(RuntimeError):
        hip.sconv(x, st[0], st[1], w, out, rows=rows, row_mul=0, **kw)
    with pytest.raises(RuntimeError):
        hip.sconv(x, st[0], st[1], w, out, rows=rows, row_mul=3, **kw)  # Tc % row_mul != 0
    with pytest.raises(ValueError):
        hip.sconv(x, st[0], st[1], w, out, rows=torch.zeros(2, dtype=torch.int32, device=device), **kw)
    # outside the shape contract of kantts_sconv_launch: declined, not an error
    for Cin, N, K, step in [(12, 16, 3, 1), (16, 8, 3, 1), (16, 16, 13, 1), (16, 16, 3, 8)]:
        kw2 = dict(kw, Cin=Cin, N=N, K=K, step=step)
        assert hip.sconv(x, st[0], st[1], torch.zeros(K, N, Cin, device=device), out, rows=rows, **kw2) is False
    # the zero tail exists for N == 1 only (include/kantts_hip.h)
    assert hip.sconv(x, st[0], st[1], w, out, rows=rows, zero_tail=True, **kw) is False


def test_sconv_rows_refusals():
    with kernel_source_on_cpu():
        _check_refusals("cpu")


def test_sconv_rows_struct_layout_matches_the_header(tmp_path):
    """SConvRowsArgs against gcc's view of kantts_sconv_rows_args; its leading fields sit where kantts_sconv_args has them."""
    import kantts._hip as hip

    pairs = [(hip.SConvRowsArgs, "kantts_sconv_rows_args"), (hip.SConvArgs, "kantts_sconv_args")]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "kantts_hip.h"', 'int main(void) {']
    for cls, cname in pairs:
        lines.append('  printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname.rstrip("_")))
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    c_layout = {}
    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        cname, field, val = ln.split()
        c_layout[(cname, field)] = int(val)
    for cls, cname in pairs:
        assert ctypes.sizeof(cls) == c_layout[(cname, "sizeof")], cname
        for fname, _ in cls._fields_:
            assert getattr(cls, fname).offset == c_layout[(cname, fname)], (cname, fname)
    for fname, _ in hip.SConvArgs._fields_:
        assert c_layout[("kantts_sconv_rows_args", fname)] == c_layout[("kantts_sconv_args", fname)], fname
    assert [f for f, _ in hip.SConvRowsArgs._fields_][-3:] == ["rows", "row_mul", "zero_tail"]


# ---------------------------------------------------------------------------------------------------------------------
# class level: the 64-channel generator of test_chunked_vocoder.py (scales 4 x 2, hop 8, 40 layers), 2 slots
def _vocoder(device, graph, mode="fp32"):
    import kantts._hip as hip
    from kantts.models.hifigan.chunked import ChunkedVocoder

    hip.set_precision(mode)
    return ChunkedVocoder(_g64().to(device), slots=2, graph=graph)


def _check_class_full_counts(device, graph, mode="fp32"):
    import kantts._hip as hip

    try:
        v, w = _vocoder(device, graph, mode), _vocoder(device, graph, mode)
        g = torch.Generator().manual_seed(2)
        for Tc in (8, 1, 5, 8):
            mel = torch.randn(2, 80, Tc, generator=g).to(device)
            a, b = v.step(mel, rows=[Tc, Tc]), w.step(mel)
            assert torch.equal(a, b), Tc
            assert torch.equal(v.arena, w.arena), Tc
    finally:
        hip.set_precision("fp32")


def _check_pause(device, graph, mode="fp32"):
    import kantts._hip as hip

    try:
        g = torch.Generator().manual_seed(5)
        A, B = torch.randn(80, 32, generator=g), torch.randn(80, 24, generator=g)
        hop = 8
        v = _vocoder(device, graph, mode)
        got, pa, pb = ([], []), 0, 0
        for ca, cb in zip([8, 8, 8, 8, 0, 0], [0, 3, 8, 0, 5, 8]):
            mel = torch.full((2, 80, 8), NAN)
            mel[0, :, :ca] = A[:, pa:pa + ca]
            mel[1, :, :cb] = B[:, pb:pb + cb]
            before = v.arena[v._parity].clone()
            wav = v.step(mel.to(device), rows=[ca, cb]).cpu()
            assert wav.shape == (2, 1, 8 * hop)
            for s, c in enumerate((ca, cb)):
                assert bool((wav[s, :, c * hop:] == 0.0).all()), "samples behind a slot's count must be exactly 0"
                assert not bool(torch.isnan(wav[s]).any())
                got[s].append(wav[s, :, :c * hop])
                if c == 0:  # a held slot: its state moves to the other half bit for bit
                    assert torch.equal(v.arena[v._parity, s], before[s])
            assert not bool(torch.isnan(v.arena).any()), "NaN reached the state"
            pa, pb = pa + ca, pb + cb
            if graph:
                assert v.captures == 1, "changing the counts must not capture again"
        assert (pa, pb) == (32, 24)
        # B in lockstep steps of 3, 8, 5, 8 on a fresh 2-slot object (slot 0 fed zeros)
        w = _vocoder(device, graph, mode)
        lock, p = [], 0
        for c in (3, 8, 5, 8):
            mel = torch.zeros(2, 80, c)
            mel[1] = B[:, p:p + c]
            lock.append(w.step(mel.to(device))[1].cpu())
            p += c
        assert torch.equal(torch.cat(got[1], dim=1), torch.cat(lock, dim=1)), "the paused slot differs from a lockstep play"
        # A alone
        w = _vocoder(device, graph, mode)
        alone = []
        for i in range(4):
            mel = torch.zeros(2, 80, 8)
            mel[0] = A[:, 8 * i:8 * i + 8]
            alone.append(w.step(mel.to(device))[0].cpu())
        assert torch.equal(torch.cat(got[0], dim=1), torch.cat(alone, dim=1)), "the steady slot differs from playing alone"
    finally:
        hip.set_precision("fp32")


_LENGTHS = (21, 8, 1, 40, 13)


def _schedule(lengths, slots, n):
    """The (index, frames) sequence play_many must yield, from the rule in its docstring."""
    cur, pos, nxt, out = [None] * slots, [0] * slots, 0, []
    while True:
        for s in range(slots):
            if cur[s] is None and nxt < len(lengths):
                cur[s], pos[s], nxt = nxt, 0, nxt + 1
        if all(c is None for c in cur):
            return out
        fed = [0 if c is None else min(n, lengths[c] - pos[s]) for s, c in enumerate(cur)]
        out += [(c, fed[s]) for s, c in enumerate(cur) if c is not None]
        for s, c in enumerate(cur):
            if c is not None:
                pos[s] += fed[s]
                if pos[s] >= lengths[c]:
                    cur[s] = None


def test_the_schedule_of_this_file_is_the_documented_one():
    assert _schedule((21, 8, 1), 2, 8) == [(0, 8), (1, 8), (0, 8), (2, 1), (0, 5)]


def _check_play_many(device, graph, mode="fp32"):
    import kantts._hip as hip

    try:
        g = torch.Generator().manual_seed(9)
        mels = [torch.randn(80, n, generator=g).to(device) for n in _LENGTHS]
        v = _vocoder(device, graph, mode)
        order, parts = [], {}
        for i, wav in v.play_many(mels, chunk_frames=8):
            assert wav.dim() == 2 and wav.shape[0] == 1 and wav.shape[1] % v.hop == 0
            order.append((i, wav.shape[1] // v.hop))
            parts.setdefault(i, []).append(wav.cpu())
        assert order == _schedule(_LENGTHS, 2, 8)
        w = _vocoder(device, graph, mode)
        for i, mel in enumerate(mels):
            want = torch.cat([c.cpu() for c in w.synthesize(mel, chunk_frames=8, slot=i % 2)], dim=1)
            have = torch.cat(parts[i], dim=1)
            assert have.shape == want.shape == (1, _LENGTHS[i] * v.hop)
            assert torch.equal(have, want), "utterance %d differs from synthesize" % i
    finally:
        hip.set_precision("fp32")


def test_step_rows_full_counts_equal_the_plain_step():
    with kernel_source_on_cpu():
        _check_class_full_counts("cpu", False)


def test_step_rows_pause_and_resume():
    with kernel_source_on_cpu():
        _check_pause("cpu", False)


def test_play_many_matches_synthesize_and_its_schedule():
    with kernel_source_on_cpu():
        _check_play_many("cpu", False)


def test_step_rows_validation():
    with kernel_source_on_cpu():
        v = _vocoder("cpu", False)
        mel = torch.zeros(2, 80, 4)
        for bad in ([1], [1, 2, 3], torch.zeros(3, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32)):
            with pytest.raises(ValueError):
                v.step(mel, rows=bad)
        for bad in (torch.ones(2), torch.ones(2, dtype=torch.float64), [1.0, 2.0], torch.ones(2, dtype=torch.bool)):
            with pytest.raises(ValueError):
                v.step(mel, rows=bad)
        for bad in ([0, 5], [-1, 2], torch.tensor([4, 5]), torch.tensor([-1, 0], dtype=torch.int32)):
            with pytest.raises(ValueError):
                v.step(mel, rows=bad)
        assert v._parity == 0 and not bool(v.arena.any()), "a refused step must not advance anything"
        assert v.step(mel, rows=torch.tensor([4, 0], dtype=torch.int64)).shape == (2, 1, 32)
        with pytest.raises(ValueError):
            list(v.play_many([torch.zeros(80, 0)]))
        with pytest.raises(ValueError):
            list(v.play_many([torch.zeros(80, 3)], chunk_frames=0))


def test_infer_hifigan_slots_need_chunk_frames(tmp_path):
    from kantts.bin import infer_hifigan

    with pytest.raises(ValueError):
        infer_hifigan.hifigan_infer(str(tmp_path), "unused.pth", str(tmp_path / "out"), config={}, slots=2)
    with pytest.raises(SystemExit) as e:
        infer_hifigan.main(["--ckpt", "c.pth", "--input_mel", str(tmp_path), "--output_dir", str(tmp_path / "out"),
                            "--slots", "2"])
    assert e.value.code == 2
    assert not (tmp_path / "out").exists()


def test_live_rows():
    from kantts.models.sambert.chunked import live_rows

    r = live_rows([5, 12, 30], 8, 16)
    assert r.dtype == torch.int32 and r.tolist() == [0, 4, 8]
    r = live_rows(torch.tensor([5, 12, 30]), lo=8, hi=16)
    assert r.dtype == torch.int32 and r.tolist() == [0, 4, 8]
    assert live_rows([3, 40], 0, 12).tolist() == [3, 12] and live_rows([3], 16, 16).tolist() == [0]


# ---------------------------------------------------------------------------------------------------------------------
# GPU
@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_sconv_rows_layer_gpu(prec):
    for kind, case in _FULL:
        _check_full_counts(kind, case, prec, "cuda")
    for Tc, row_mul in sorted(_RAGGED):
        _check_ragged(_H30, prec, Tc, row_mul, "cuda")
    for kind, case in [("conv", (80, 32, 7, 1)), ("conv", _H30), ("conv", _N1), ("poly", _POLY_CASES[1])]:
        _check_schedule(kind, case, prec, "cuda")


@pytest.mark.gpu
def test_sconv_rows_n1_clamping_and_refusals_gpu():
    for Tc, row_mul in sorted(_RAGGED):
        _check_ragged(_N1, "fp32", Tc, row_mul, "cuda")
    for case in (_H30, _N1):
        _check_clamping(case, "cuda")
    _check_refusals("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [True, False])
def test_step_rows_full_counts_equal_the_plain_step_gpu(graph):
    _check_class_full_counts("cuda", graph)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("graph", [True, False])
def test_step_rows_pause_and_resume_gpu(graph, mode):
    _check_pause("cuda", graph, mode)


@pytest.mark.gpu
def test_step_rows_graph_replays_with_changing_counts_gpu():
    """One capture serves every count vector of a chunk size (a device tensor of counts included), and graph replay and
    eager launches give identical bits."""
    import kantts._hip as hip

    hip.set_precision("fp32")
    vg, ve = _vocoder("cuda", True), _vocoder("cuda", False)
    g = torch.Generator().manual_seed(4)
    for i, counts in enumerate([[8, 8], [0, 5], [3, 0], [8, 1], [0, 0], [7, 8]]):
        mel = torch.randn(2, 80, 8, generator=g).cuda()
        rows = torch.tensor(counts, device="cuda") if i % 2 else counts
        a, b = vg.step(mel, rows=rows), ve.step(mel, rows=rows)
        assert torch.equal(a, b), counts
        assert torch.equal(vg.arena, ve.arena), counts
        assert vg.captures == 1 and len(vg._graphs) == 1
    mel = torch.randn(2, 80, 8, generator=g).cuda()
    assert torch.equal(vg.step(mel), ve.step(mel))  # the plain form keeps graphs of its own
    assert vg.captures == 2
    assert torch.equal(vg.step(mel, rows=[2, 2]), ve.step(mel, rows=[2, 2]))
    assert vg.captures == 2
    # a device count outside [0, Tc] is not read back: the kernel clamps it
    a, b = vg.step(mel, rows=torch.tensor([-3, 99], device="cuda")), ve.step(mel, rows=[0, 8])
    assert torch.equal(a, b) and torch.equal(vg.arena, ve.arena)
    assert not bool(a[0].any()) and bool(a[1].any())
    assert vg.captures == 2


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [True, False])
def test_play_many_matches_synthesize_and_its_schedule_gpu(graph):
    _check_play_many("cuda", graph)


@pytest.mark.gpu
def test_infer_hifigan_slots_cli_gpu(tmp_path):
    import kantts._hip as hip
    from kantts.bin.infer_hifigan import hifigan_infer
    from scipy.io import wavfile

    hip.set_precision("fp32")
    voc_dir = tmp_path / "voc" / "ckpt"
    voc_dir.mkdir(parents=True)
    (tmp_path / "voc" / "config.yaml").write_text(yaml.dump(
        {"Model": {"Generator": {"params": _G64}}, "audio_config": {"sampling_rate": 16000}}))
    torch.save({"model": {"generator": _g64().state_dict()}}, voc_dir / "checkpoint_1.pth")
    mel_dir = tmp_path / "mels"
    mel_dir.mkdir()
    rng = np.random.default_rng(0)
    lengths = {"utt_a": 21, "utt_b": 5, "utt_c": 34}
    for name, n in lengths.items():
        np.save(mel_dir / (name + ".npy"), rng.standard_normal((n, 80)).astype(np.float32))
    ck = str(voc_dir / "checkpoint_1.pth")
    hifigan_infer(str(mel_dir), ck, str(tmp_path / "one"), chunk_frames=8, slots=1)
    hifigan_infer(str(mel_dir), ck, str(tmp_path / "two"), chunk_frames=8, slots=2)
    for name, n in lengths.items():
        _, a = wavfile.read(tmp_path / "one" / (name + "_gen.wav"))
        _, b = wavfile.read(tmp_path / "two" / (name + "_gen.wav"))
        assert a.dtype == b.dtype == np.int16 and a.shape == b.shape == (n * 8,)
        assert np.array_equal(a, b), name
