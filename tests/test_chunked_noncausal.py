"""The layer of chunked inference for symmetric (non-causal) networks: csrc/sconv_sym.hip, kantts_sconv_sym_rows_launch,
kantts._hip.sconv_sym / nc_emit; and the non-causal ConvTranspose1d whose kernel is no multiple of its stride.

CPU leg: the kernel SOURCE on the host build (util.kernel_source_on_cpu).  GPU leg: the same checks on the device.

Bounds.  Against torch in fp64: 2e-5 for fp32 and max-abs <= 4e-2 * max(1, |ref|max) for bf16, the bounds of
test_chunked_vocoder.py for the same arithmetic (the kernel is sconv.hip's contraction: same tiles, same summation order).
Everything the rule defines exactly is asserted exactly: rows outside the utterance are 0.0, rows the call does not own keep
their sentinel, the state is a copy, guard floats and read-only buffers are untouched."""
import ctypes
import itertools
import json
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

import hifigan_oracle as H
import test_bench_config_parity as _bench_parity
import test_chunked_acoustic as _ca
from util import ROOT, assert_close, assert_grads_close, emulation, kernel_source_on_cpu

S = 3
LENS = [40, 17, 3]  # rows per slot; 3 is shorter than every padding below but the first
SENTINEL = -1234.5
GUARD = 7.0
NAN = float("nan")
SLOPE = 0.1
EXTRA = 4  # rows every slot keeps stepping after its last true row came out: they must be zeros

_CASES = [(16, 16, 3, 1), (32, 32, 3, 7), (16, 16, 11, 3), (32, 1, 7, 1)]  # (Cin, N, K, dilation)
_SCHEDULES = {"eights": [8], "ones": [1], "mixed": [5, 11, 3, 13, 8]}


def _prec(hip, prec):
    return hip.PREC_BF16 if prec == "bf16" else hip.PREC_FP32


def _assert_bound(y, ref, prec, n1, what):
    if prec == "fp32" or n1:
        assert_close(y, ref.float(), 2e-5, what=str(what))
    else:
        err = float((y.double() - ref).abs().max())
        assert err <= 4e-2 * max(1.0, float(ref.abs().max())), (what, err)


class _SymLayer:
    """One symmetric convolution (padding (K - 1) d / 2) played as a stream on S slots: seeded weights, a ping-pong state
    arena with guard floats behind every slot, the per-slot position in a ping-pong int32 buffer of its own."""

    def __init__(self, case, prec, device, lag=0, with_res=False, seed=5, stage=False):
        import kantts._hip as hip

        self.hip = hip
        g = torch.Generator().manual_seed(seed)
        self.sub = 1
        if stage:  # both paths of an upsampling stage as one polyphase layer: row q holds the s samples of token q
            from kantts.models.hifigan.chunked_nc import fused_stage_weight, stage_geometry

            Cin, Cout, s, K_T = case
            self.Wt = torch.randn(Cin, Cout, K_T, generator=g) / (Cin * K_T / s) ** 0.5
            self.W7 = torch.randn(Cout, Cin, 7, generator=g) / (Cin * 7) ** 0.5
            self.bt, self.b7 = torch.randn(Cout, generator=g), torch.randn(Cout, generator=g)
            self.P, E, K = stage_geometry(K_T, s, 7)
            N, d, self.sub = s * Cout, 1, s
            w_knc = fused_stage_weight(self.Wt, self.W7, s).reshape(Cin, Cout, K, s).permute(2, 3, 1, 0).reshape(K, N, Cin)
            self.b = (self.bt + self.b7).repeat(s)
            self.delay = E  # in output samples
        else:
            Cin, N, K, d = case
            self.W = torch.randn(N, Cin, K, generator=g) / (Cin * K) ** 0.5
            self.b = torch.randn(N, generator=g)
            w_knc = self.W.permute(2, 0, 1).flip(0)
            self.p = (K - 1) * d // 2
            self.delay = self.p + lag
        self.Cin, self.N, self.K, self.d, self.lag, self.gen = Cin, N, K, d, lag, g
        self.Hs = (K - 1) * d + lag
        self.prec, self.device = prec, device
        bf = prec == "bf16" and N > 1
        self.w = w_knc.to(torch.bfloat16 if bf else torch.float32).contiguous().to(device)
        self.bias = self.b.to(device)
        self.ss = self.Hs * Cin + 8
        self.arena = torch.full((2, S, self.ss), GUARD)
        self.arena[:, :, :self.Hs * Cin] = 0.0  # a zeroed state is a fresh slot
        self.arena = self.arena.to(device)
        self.pos = torch.full((2, S, 2), 77, dtype=torch.int32)
        self.pos[:, :, 0] = 0
        self.pos = self.pos.to(device)
        self.parity = 0
        self.with_res = with_res
        self.res_lag = self.delay if with_res else 0  # x + conv(x): the residual is as late as the output
        self.rh = torch.zeros(S, self.res_lag, N)  # the state of the layer the residual comes from, kept by the test

    def step(self, x, counts, end, res=None):
        """x (S, Tc, Cin), counts / end: S ints -> out (S, Tc, N), state (S, Hs, Cin), pos (S)."""
        hip, dev = self.hip, self.device
        Tc, N, Cin, Hs, p = x.shape[1], self.N, self.Cin, self.Hs, self.parity
        pad = 4 * N
        flat = torch.full((S * Tc * N + 2 * pad,), GUARD).to(dev)
        out = flat[pad:pad + S * Tc * N].view(S, Tc, N)
        out.fill_(SENTINEL)
        self.arena[1 - p, :, :Hs * Cin] = SENTINEL
        before = self.arena[p].clone()
        kw = {}
        if self.with_res:
            rss = self.res_lag * N + 8
            rha = torch.full((S, rss), GUARD)
            rha[:, :self.res_lag * N] = self.rh.reshape(S, -1)
            rha_dev = rha.to(dev)
            kw = dict(res=res.contiguous().to(dev), res_hist=rha_dev, res_hist_ss=rss, res_hist_rows=self.res_lag,
                      res_lag=self.res_lag)
        ok = hip.sconv_sym(x.contiguous().to(dev), self.arena[p, 0], self.arena[1 - p, 0], self.w, out, S=S, Tc=Tc, Cin=Cin,
                           N=N, K=self.K, step=self.d, hist_ss=self.ss, precision=_prec(hip, self.prec), bias=self.bias,
                           rows=torch.tensor(counts, dtype=torch.int32).to(dev),
                           end=torch.tensor(end, dtype=torch.int32).to(dev), pos_in=self.pos[p, 0], pos_out=self.pos[1 - p, 0],
                           pos_ss=2, delay=self.delay, sub=self.sub, lag=self.lag, in_end=True, in_leaky=SLOPE, zero_tail=N == 1, **kw)
        assert ok
        assert bool((self.arena[:, :, Hs * Cin:] == GUARD).all()), "guard floats behind a slot's state were written"
        assert torch.equal(self.arena[p], before), "hist_in was written"
        assert bool((self.pos[:, :, 1] == 77).all()), "guard words behind a slot's position were written"
        assert bool((flat[:pad] == GUARD).all()) and bool((flat[-pad:] == GUARD).all()), "guard rows around out were written"
        if self.with_res:
            assert torch.equal(rha_dev.cpu().view(torch.int32), rha.view(torch.int32)), "res_hist was written"  # NaN rows too
            for s, n in enumerate(counts):
                self.rh[s] = torch.cat([self.rh[s], res[s, :n]], dim=0)[n:]
        self.parity ^= 1
        return (out.cpu().clone(), self.arena[1 - p, :, :Hs * Cin].cpu().view(S, Hs, Cin).clone(),
                self.pos[1 - p, :, 0].cpu().clone())


def _check_neutral(device, prec, slots, Tc, case):
    """kantts_sconv_sym_rows_launch with neutral settings (lag = delay = res_lag = 0, sub = 1, every end open, pos = 0)
    against kantts_sconv_rows_launch on the same buffers: the two kernels include ONE tile loop (csrc/sconv_body.inc) and
    the two entry points ask ONE tile picker (csrc/sconv_common.inc), so the live rows of out and the state are the same
    bits -- no tolerance."""
    import kantts._hip as hip

    Cin, N, K, d = case
    Hn = (K - 1) * d
    g = torch.Generator().manual_seed(11)
    bf = prec == "bf16" and N > 1
    w = (torch.randn(K, N, Cin, generator=g) / (Cin * K) ** 0.5).to(torch.bfloat16 if bf else torch.float32).to(device)
    bias = torch.randn(N, generator=g).to(device)
    x = torch.randn(slots, Tc, Cin, generator=g).to(device)
    res = torch.randn(slots, Tc, N, generator=g).to(device)
    hist = torch.randn(slots, Hn, Cin, generator=g).to(device)
    counts = [[Tc, Tc // 2, 0][s % 3] for s in range(slots)]
    rows = torch.tensor(counts, dtype=torch.int32).to(device)
    end = torch.full((slots,), -1, dtype=torch.int32).to(device)
    pos = torch.zeros(slots, dtype=torch.int32).to(device)
    kw = dict(S=slots, Tc=Tc, Cin=Cin, N=N, K=K, step=d, hist_ss=Hn * Cin, precision=_prec(hip, prec), bias=bias, res=res,
              in_leaky=SLOPE, out_leaky=SLOPE, rows=rows, row_mul=1, zero_tail=N == 1)
    got = []
    for sym in (False, True):
        out = torch.full((slots, Tc, N), SENTINEL).to(device)
        st = torch.full((slots, Hn, Cin), SENTINEL).to(device)
        if sym:
            assert hip.sconv_sym(x, hist, st, w, out, end=end, pos_in=pos, lag=0, delay=0, sub=1, res_lag=0, **kw)
        else:
            assert hip.sconv(x, hist, st, w, out, **kw)
        got.append((out.cpu(), st.cpu()))
    (out_c, st_c), (out_s, st_s) = got
    what = (case, prec, slots, Tc)
    for s, n in enumerate(counts):
        assert not bool((out_c[s, :n] == SENTINEL).any()), ("live rows were not written", what, s)
        assert torch.equal(out_s[s, :n], out_c[s, :n]), ("live rows of out", what, s)
    assert torch.equal(st_s, st_c), ("hist_out", what)


# (Cin, N, K, dilation): the smallest; a partial 32-channel chunk, a second fp32 slab and a partial column fragment; a second
# bf16 slab and the longest tap count; N == 1 (with zero_tail)
_NEUTRAL = [(16, 16, 3, 1), (72, 40, 3, 7), (136, 48, 11, 3), (32, 1, 7, 1)]
# (S, Tc, (Cin, N, K, dilation)): the wider column tiles.  At Tc = 8 the four waves sit side by side (WN = 4), so the
# picker's blocks(nfr) = S * ceil(N / (64 * nfr)): S = 96, N = 512 gives blocks(4) = 192 < 384 <= blocks(2) = 384 (NFR = 2),
# and S = 96, N = 1024 gives blocks(4) = 384 (NFR = 4)
_NEUTRAL_WIDE = [(96, 8, (16, 512, 3, 1)), (96, 8, (16, 1024, 3, 1))]


@pytest.mark.parametrize("Tc", [8, 40, 130])  # the three row-tile classes of the dispatcher
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", _NEUTRAL, ids=lambda c: "_".join(map(str, c)))
def test_sconv_sym_neutral_is_sconv_rows(case, prec, Tc):
    with kernel_source_on_cpu():
        _check_neutral("cpu", prec, S, Tc, case)


def _check_layer(case, prec, sched, device, lag=0, with_res=False, late_end=False, stage=False):
    L = _SymLayer(case, prec, device, lag=lag, with_res=with_res, stage=stage)
    xs = [torch.randn(T, L.Cin, generator=L.gen) for T in LENS]
    rs = [torch.randn(T, L.N, generator=L.gen) for T in LENS]
    refs = []
    for x, r in zip(xs, rs):
        a = F.leaky_relu(x.double(), SLOPE).t()[None]
        if stage:
            y = (F.conv_transpose1d(a, L.Wt.double(), L.bt.double(), stride=L.sub, padding=L.P)
                 + F.conv1d(a.repeat_interleave(L.sub, dim=2), L.W7.double(), L.b7.double(), padding=3))[0].t()
        else:
            y = F.conv1d(a, L.W.double(), L.b.double(), padding=L.p, dilation=L.d)[0].t()
        refs.append(y + r.double() if with_res else y)
    total = [T + -(-L.delay // L.sub) + EXTRA for T in LENS]
    pos, got = [0] * S, [[] for _ in range(S)]
    fed = [torch.zeros(0, L.Cin) for _ in range(S)]  # what the state must copy: flush rows count as zeros
    sizes = itertools.cycle(_SCHEDULES[sched])
    steps = 0
    while any(p < n for p, n in zip(pos, total)):
        steps += 1
        assert steps < 400
        Tc = next(sizes)
        counts = [min(Tc, n - p) for p, n in zip(pos, total)]
        x = torch.full((S, Tc, L.Cin), NAN)  # rows beyond counts[s] and beyond the end stay NaN: they must not be loaded
        r = torch.full((S, Tc, L.N), NAN)
        end = []
        for s in range(S):
            live = max(0, min(counts[s], LENS[s] - pos[s]))
            x[s, :live] = xs[s][pos[s]:pos[s] + live]
            r[s, :live] = rs[s][pos[s]:pos[s] + live]
            fed[s] = torch.cat([fed[s], x[s, :live], torch.zeros(counts[s] - live, L.Cin)], dim=0)
            # the end may stay open until the first step that feeds a row at or beyond it
            end.append(-1 if late_end and pos[s] + counts[s] <= LENS[s] else LENS[s])
        out, st, newpos = L.step(x, counts, end, res=r)
        for s in range(S):
            what = (case, prec, sched, lag, with_res, "step", steps, "slot", s)
            got[s].append(out[s, :counts[s]])
            assert bool((out[s, counts[s]:] == (0.0 if L.N == 1 else SENTINEL)).all()), ("dead rows", what)
            pos[s] += counts[s]
            assert int(newpos[s]) == pos[s], ("pos", what)
            want = torch.cat([torch.zeros(L.Hs, L.Cin), fed[s]], dim=0)[-L.Hs:]
            assert torch.equal(st[s], want), ("state", what)
    for s, T in enumerate(LENS):
        what = (case, prec, sched, lag, with_res, "slot", s)
        y = torch.cat(got[s], dim=0)
        assert y.shape[0] == total[s]
        y = y.reshape(total[s] * L.sub, L.N // L.sub)  # a polyphase row is `sub` samples: the window is checked per sample
        T = T * L.sub
        assert not bool(torch.isnan(y).any()), what
        assert bool((y[:L.delay] == 0.0).all()), ("samples before the utterance", what)
        assert bool((y[L.delay + T:] == 0.0).all()), ("samples behind the utterance", what)
        _assert_bound(y[L.delay:L.delay + T], refs[s], prec, L.N == 1, what)


@pytest.mark.parametrize("sched", list(_SCHEDULES))
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", _CASES, ids=lambda c: "_".join(map(str, c)))
def test_sconv_sym_layer_matches_torch(case, prec, sched):
    with kernel_source_on_cpu():
        _check_layer(case, prec, sched, "cpu", late_end=sched == "ones")


@pytest.mark.parametrize("with_res", [False, True], ids=["lag", "lag_res"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", _CASES, ids=lambda c: "_".join(map(str, c)))
def test_sconv_sym_layer_lag_and_lagged_residual(case, prec, with_res):
    with kernel_source_on_cpu():
        _check_layer(case, prec, "mixed", "cpu", lag=5, with_res=with_res)
        if with_res:
            _check_layer(case, prec, "ones", "cpu", lag=0, with_res=True)


_STAGES = [(32, 16, 2, 4), (32, 16, 4, 8), (32, 16, 5, 11)]  # (Cin, Cout, s, K_T)


@pytest.mark.parametrize("sched", list(_SCHEDULES))
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", _STAGES, ids=lambda c: "_".join(map(str, c)))
def test_sconv_sym_stage_matches_torch(case, prec, sched):
    """Transposed convolution (padding (K_T - s) // 2) plus nearest-repeat and a symmetric k7 convolution, both zero-padded
    at the utterance's edges, as one polyphase layer of J taps."""
    with kernel_source_on_cpu():
        _check_layer(case, prec, sched, "cpu", stage=True, late_end=sched == "mixed")


def test_nc_emit_is_the_window_of_the_kernel():
    """nc_emit against the rule written out: the true samples a step holds are a contiguous run; over an utterance they add
    up to end * hop, also when the end is learnt late and when the utterance is shorter than the delay."""
    import kantts._hip as hip

    for hop, delay, T, n in [(8, 27, 23, 4), (8, 27, 2, 1), (10, 31, 9, 8), (200, 3424, 5, 8), (4, 0, 6, 4)]:
        flush = -(-delay // hop)
        pos, total, nxt = 0, 0, 0
        while pos < T + flush:
            m = min(n, T + flush - pos)
            end = T if pos + m > T else -1
            off, cnt = hip.nc_emit(pos, m, end, delay, hop)
            lo = max(0, pos * hop - delay)
            hi = (pos + m) * hop - delay if end < 0 else min((pos + m) * hop - delay, T * hop)
            assert cnt == max(0, hi - lo) and (cnt == 0 or (off == lo + delay - pos * hop and lo == nxt))
            assert 0 <= off and off + cnt <= m * hop
            nxt, total, pos = nxt + cnt, total + cnt, pos + m
        assert total == T * hop, (hop, delay, T, n)


def _check_refusals(device):
    import kantts._hip as hip

    z = lambda *shape, **kw: torch.zeros(*shape, device=device, **kw)
    x, out, st, w = z(1, 4, 16), z(1, 4, 16), z(2, 1, 128), z(3, 16, 16)
    i32 = lambda: z(1, dtype=torch.int32)
    rows, end, pos = i32(), i32(), z(2, 1, dtype=torch.int32)
    kw = dict(S=1, Tc=4, Cin=16, N=16, K=3, step=1, hist_ss=128, precision=hip.PREC_FP32, rows=rows, end=end, pos_in=pos[0])
    assert hip.sconv_sym_entry_points()
    assert hip.sconv_sym(x, st[0], st[1], w, out, pos_out=pos[1], row_mul=2, lag=3, **kw) is True
    assert hip.sconv_sym(x, st[0], st[1], z(3, 32, 16), z(1, 4, 32), sub=2, **dict(kw, N=32)) is True
    for bad in (dict(row_mul=0), dict(row_mul=3), dict(lag=-1), dict(res_lag=-1), dict(delay=-1), dict(sub=0), dict(sub=3),
                dict(res=out.clone(), res_lag=2),                                          # no res_hist
                dict(res=out.clone(), res_hist=z(64), res_hist_rows=1, res_lag=2),         # beyond the residual history
                dict(res_hist=z(64), res_hist_rows=2),                                     # res_hist without res
                dict(pos_out=pos[0])):
        with pytest.raises(RuntimeError):
            hip.sconv_sym(x, st[0], st[1], w, out, **dict(kw, **bad))
    for missing in ("rows", "end", "pos_in"):
        with pytest.raises(RuntimeError):
            hip.sconv_sym(x, st[0], st[1], w, out, **dict(kw, **{missing: None}))
    with pytest.raises(RuntimeError):
        hip.sconv_sym(x, None, None, w, out, **kw)  # K > 1 without a state
    with pytest.raises(RuntimeError):
        hip.sconv_sym(x, None, None, z(1, 16, 16), out, lag=2, **dict(kw, K=1))  # a lag needs a state too
    with pytest.raises(ValueError):
        hip.sconv_sym(x, st[0], st[1], w, out, **dict(kw, end=z(2, dtype=torch.int32)))
    # outside the shape contract of kantts_sconv_launch: declined, not an error
    for Cin, N, K, step in [(12, 16, 3, 1), (16, 8, 3, 1), (16, 16, 13, 1), (16, 16, 3, 8)]:
        kw2 = dict(kw, Cin=Cin, N=N, K=K, step=step)
        assert hip.sconv_sym(x, st[0], st[1], z(K, N, Cin), out, **kw2) is False
    assert hip.sconv_sym(x, st[0], st[1], w, out, zero_tail=True, **kw) is False  # the zero tail exists for N == 1 only


def test_sconv_sym_refusals():
    with kernel_source_on_cpu():
        _check_refusals("cpu")


def test_sconv_sym_struct_layout_matches_the_header(tmp_path):
    """SConvSymArgs against gcc's view of kantts_sconv_sym_args."""
    import kantts._hip as hip

    cls, cname = hip.SConvSymArgs, "kantts_sconv_sym_args"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "kantts_hip.h"', 'int main(void) {',
             '  printf("sizeof %%zu\\n", sizeof(%s));' % cname]
    for fname, _ in cls._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(%s, %s));' % (fname, cname, fname.rstrip("_")))
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    c_layout = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert ctypes.sizeof(cls) == int(c_layout["sizeof"])
    for fname, _ in cls._fields_:
        assert getattr(cls, fname).offset == int(c_layout[fname]), fname


# ---------------------------------------------------------------------------------------------------------------------
# non-causal ConvTranspose1d with kernel % stride != 0 (the shipped non-causal configurations: kernel 11 at stride 5)
_G32_NC = dict(channels=32, upsample_scales=[5, 2], upsample_kernal_sizes=[11, 4])


def _check_conv_transpose(device):
    """Forward and the gradients of input, weight_g, weight_v and bias against torch autograd in fp64, at the 2e-5 of the
    layer tests; (K - s) odd gives the reference module's T s + 1 samples."""
    from kantts.models.hifigan.layers import ConvTranspose1d

    for Cin, Cout, K, s, T in [(16, 8, 11, 5, 9), (16, 8, 11, 5, 1), (16, 16, 7, 2, 6), (16, 8, 3, 5, 4), (16, 8, 8, 4, 5)]:
        pad = (K - s) // 2 if K >= s else 0
        torch.manual_seed(K * 10 + s)
        m = ConvTranspose1d(Cin, Cout, K, s, padding=pad)
        g = torch.Generator().manual_seed(4)
        x = torch.randn(2, Cin, T, generator=g)
        P = {k: v.detach().double().requires_grad_(True) for k, v in m.state_dict().items()}
        xr = x.double().requires_grad_(True)
        yr = F.conv_transpose1d(xr, H.wn(P, "deconv"), P["deconv.bias"], stride=s, padding=pad)
        m = m.to(device)
        xd = x.to(device).requires_grad_(True)
        y = m(xd)
        what = "ConvTranspose1d K %d s %d" % (K, s)
        assert y.shape == yr.shape == (2, Cout, (T - 1) * s - 2 * pad + K), what
        assert_close(y.detach().cpu(), yr.detach().float(), 2e-5, what=what)
        cot = torch.randn(yr.shape, generator=g)
        (y * cot.to(device)).sum().backward()
        (yr * cot.double()).sum().backward()
        assert_close(xd.grad.cpu(), xr.grad.float(), 2e-5, what=what + " dx")
        for n, prm in m.named_parameters():
            assert_close(prm.grad.cpu(), P[n].grad.float(), 2e-5, what="%s d%s" % (what, n))
    with pytest.raises(NotImplementedError, match="output_padding"):
        ConvTranspose1d(16, 8, 11, 5, padding=3, output_padding=1)


def _check_generator_k11_s5(device):
    from kantts.models.hifigan.hifigan import Generator

    torch.manual_seed(3)
    G = Generator(causal=False, **_G32_NC)
    PG = {k: v.detach().clone().requires_grad_(True) for k, v in G.state_dict().items()}
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 80, 7, generator=g)
    G = G.to(device)
    yo = G(x.to(device))
    yr = H.generator(PG, x, scales=(5, 2), causal=False)
    assert yo.shape == yr.shape == (2, 1, 70)
    assert_close(yo.detach().cpu(), yr.detach(), 2e-5, what="non-causal generator, kernel 11 stride 5")
    cot = torch.randn(yr.shape, generator=g)
    (yo * cot.to(device)).sum().backward()
    (yr * cot).sum().backward()
    assert_grads_close([(n, p.grad, PG[n].grad) for n, p in G.named_parameters()], 2e-3, "non-causal G k11 s5")


def test_conv_transpose_kernel_no_multiple_of_stride_emulated():
    with emulation():
        _check_conv_transpose("cpu")


def test_noncausal_generator_k11_s5_emulated():
    with emulation():
        _check_generator_k11_s5("cpu")


# ---------------------------------------------------------------------------------------------------------------------
# GPU legs
@pytest.mark.gpu
def test_conv_transpose_kernel_no_multiple_of_stride_gpu():
    import kantts._hip as hip

    hip.set_precision("fp32")
    _check_conv_transpose("cuda")
    _check_generator_k11_s5("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_sconv_sym_layer_gpu(prec):
    for case in _CASES:
        for sched in _SCHEDULES:
            _check_layer(case, prec, sched, "cuda", late_end=sched == "ones")
        _check_layer(case, prec, "mixed", "cuda", lag=5)
        _check_layer(case, prec, "mixed", "cuda", lag=5, with_res=True)
        _check_layer(case, prec, "ones", "cuda", with_res=True)
    for case in _STAGES:
        for sched in _SCHEDULES:
            _check_layer(case, prec, sched, "cuda", stage=True, late_end=sched == "mixed")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_sconv_sym_neutral_is_sconv_rows_gpu(prec):
    for case in _NEUTRAL:
        for Tc in (8, 40, 130):
            _check_neutral("cuda", prec, S, Tc, case)
    for slots, Tc, case in _NEUTRAL_WIDE:
        _check_neutral("cuda", prec, slots, Tc, case)


@pytest.mark.gpu
def test_sconv_sym_refusals_gpu():
    _check_refusals("cuda")


# ---------------------------------------------------------------------------------------------------------------------
# class level: ChunkedNCVocoder against Generator.forward on the same device
# Two 64-channel generators (narrower ones end below the 16 input channels the layer contract needs): scales 4 x 2 with
# kernels 8 / 4 (hop 8) and scales 5 x 2 with kernels 11 / 4 (hop 10).  Delays by the rule, with the stacks' 60 rows
# (kernel 11, dilations 1, 3, 5): ((3 * 4 + 3 + 60) * 2 + 3 + 60) + 3 = 216 samples = 27 frames, and
# ((3 * 5 + 3 + 60) * 2 + 3 + 60) + 3 = 222 samples = 23 frames.
_DELAYS = {"s4x2": (216, 27), "s5x2": (222, 23)}
_GNC = {"s4x2": dict(channels=64, upsample_scales=[4, 2], upsample_kernal_sizes=[8, 4]),
        "s5x2": dict(channels=64, upsample_scales=[5, 2], upsample_kernal_sizes=[11, 4])}
_FRAMES = [23, 9, 2]  # 2 is fewer than flush_frames
_REPORT = os.path.join(os.path.dirname(_bench_parity._REPORT), "chunked_noncausal_parity.json")


def _record(key, val):
    try:
        os.makedirs(os.path.dirname(_REPORT), exist_ok=True)
        d = json.load(open(_REPORT)) if os.path.exists(_REPORT) else {}
        d[key] = val
        json.dump(d, open(_REPORT, "w"), indent=1)
    except OSError:
        pass


def _gnc(name, device="cpu"):
    from kantts.models.hifigan.hifigan import Generator

    torch.manual_seed(0)
    return Generator(causal=False, **_GNC[name]).eval().to(device)


def _mels(device, frames=_FRAMES):
    g = torch.Generator().manual_seed(21)
    return [torch.randn(80, T, generator=g).to(device) for T in frames]


def _one_shot(G, mels):
    with torch.no_grad():
        return [G(m[None])[0] for m in mels]


def _chunked(v, mels, n):
    """Every utterance through synthesize (alone) and all of them through play_many; both must have T * hop samples."""
    syn = [torch.cat(list(v.synthesize(m, chunk_frames=n)), dim=1) for m in mels]
    many = [[] for _ in mels]
    for i, w in v.play_many(mels, chunk_frames=n):
        many[i].append(w)
    many = [torch.cat(ws, dim=1) for ws in many]
    for m, a, b in zip(mels, syn, many):
        assert a.shape == b.shape == (1, m.shape[1] * v.hop), (a.shape, b.shape, m.shape)
    return syn, many


def _check_generator_fp32(name, n, device, graph=False):
    import kantts._hip as hip
    from kantts.models.hifigan.chunked_nc import ChunkedNCVocoder

    hip.set_precision("fp32")
    G, mels = _gnc(name, device), _mels(device)
    ref = _one_shot(G, mels)
    v = ChunkedNCVocoder(G, slots=2, graph=graph)
    assert v.delay_samples == ChunkedNCVocoder.delay_of(G) == _DELAYS[name][0] and v.flush_frames == _DELAYS[name][1]
    for kind, got in zip(("synthesize", "play_many"), _chunked(v, mels, n)):
        for T, y, r in zip(_FRAMES, got, ref):
            err = float((y - r).abs().mean())
            print("chunked non-causal", name, kind, "chunk", n, "frames", T, "mean-abs", err)
            assert err <= 1e-5, (name, kind, n, T, err)


@pytest.mark.parametrize("n", [1, 4, 8])
@pytest.mark.parametrize("name", list(_GNC))
def test_chunked_noncausal_generator_kernel_source(name, n):
    with kernel_source_on_cpu():
        _check_generator_fp32(name, n, "cpu")


def _refusal_cases():
    from kantts.models.hifigan.hifigan import Generator

    torch.manual_seed(0)
    g64 = _GNC["s4x2"]
    return [
        (Generator(causal=True, **g64).eval(), ValueError, "ChunkedVocoder"),
        (Generator(causal=False, nsf_params={"nb_harmonics": 7, "sampling_rate": 16000}, in_channels=80, **g64).eval(),
         NotImplementedError, "NSF"),
        (Generator(causal=False, out_channels=4, **g64).eval(), NotImplementedError, "out_channels"),
        (Generator(causal=False, **g64).train(), ValueError, "eval"),
        (Generator(causal=False, channels=32).eval(), NotImplementedError, "outside what"),  # 2-channel last stage
        (Generator(causal=False, channels=64, upsample_scales=[2, 2], upsample_kernal_sizes=[5, 4]).eval(),
         NotImplementedError, "even"),  # (kernel - stride) odd
    ]


def test_chunked_noncausal_refusals():
    from kantts.models.hifigan.chunked import ChunkedVocoder
    from kantts.models.hifigan.chunked_nc import ChunkedNCVocoder

    with kernel_source_on_cpu():
        for G, exc, pat in _refusal_cases():
            with pytest.raises(exc, match=pat):
                ChunkedNCVocoder(G, slots=1, graph=False)
        with pytest.raises(ValueError, match="causal"):
            ChunkedVocoder(_gnc("s4x2"), slots=1, graph=False)
        v = ChunkedNCVocoder(_gnc("s4x2"), slots=2, graph=False)
        mel = torch.zeros(2, 80, 4)
        for bad in ([1], [1, 2, 3], [1.5, 2], torch.zeros(2), torch.zeros(3, dtype=torch.int32)):
            with pytest.raises(ValueError):
                v.step(mel, end=bad)
        with pytest.raises(ValueError):
            v.step(mel, rows=[5, 0])


def test_delay_of_the_shipped_noncausal_geometry():
    """hifigan_noncausal_v1_16k: channels 256, scales 10 x 5 x 2 x 2 with kernels 20 / 11 / 4 / 4, residual kernels 3 / 7 / 11
    with dilations (1, 3, 5, 7): 3424 samples = 18 frames of 200 samples, layer by layer as DESIGN.md has it."""
    from kantts.models.hifigan.chunked_nc import ChunkedNCVocoder, plan_delays
    from kantts.models.hifigan.hifigan import Generator

    G = Generator(causal=False, channels=256, upsample_scales=[10, 5, 2, 2], upsample_kernal_sizes=[20, 11, 4, 4],
                  resblock_kernel_sizes=[3, 7, 11], resblock_dilations=[[1, 3, 5, 7]] * 3).eval()
    assert ChunkedNCVocoder.delay_of(G) == 3424
    assert [d for _, _, d in plan_delays(G)] == [3, 35, 135, 678, 778, 1559, 1659, 3321, 3421, 3424]
    with kernel_source_on_cpu():
        v = ChunkedNCVocoder(G, slots=1, graph=False)
    assert v.delay_samples == 3424 and v.flush_frames == 18 and v.hop == 200
    lags = sorted({L.lag for L in v.layers})
    assert lags == [0, 40, 80]  # stacks of 20, 60 and 100 rows aligned at their first convolution


def _manual(v, mel, n, slot, late_end=False, pause=(), others=None):
    """One utterance on ``slot`` by hand-made steps of room ``n``: ``pause`` lists steps in which the slot gets rows = 0,
    ``others`` maps other slots to utterances that play beside it.  Returns the slot's waveform."""
    import kantts._hip as hip

    v.reset()
    T, S = int(mel.shape[1]), v.slots
    plays = dict(others or {})
    plays[slot] = mel
    pos, out, i = {s: 0 for s in plays}, [], 0
    while pos[slot] < T + v.flush_frames:
        buf = torch.full((S, 80, n), NAN, device=mel.device)  # what is not fed must not be read
        counts, end = [0] * S, [-1] * S
        for s, m in plays.items():
            Ts = int(m.shape[1])
            if s == slot and i in pause:
                end[s] = -1 if late_end and pos[s] <= Ts else Ts
                continue
            counts[s] = max(0, min(n, Ts + v.flush_frames - pos[s]))
            live = max(0, min(counts[s], Ts - pos[s]))
            buf[s, :, :live] = m[:, pos[s]:pos[s] + live]
            end[s] = -1 if late_end and pos[s] + counts[s] <= Ts else Ts
        before = v.arena[v._parity, slot].clone()
        wav = v.step(buf, rows=counts, end=end)
        if counts[slot] == 0:
            assert torch.equal(v.arena[v._parity, slot].view(torch.int32), before.view(torch.int32)), "a held slot's state moved"
            assert bool((wav[slot] == 0.0).all())
        off, cnt = hip.nc_emit(pos[slot], counts[slot], T, v.delay_samples, v.hop)
        keep = torch.zeros(wav.shape[2], dtype=torch.bool, device=wav.device)
        keep[off:off + cnt] = True
        assert bool((wav[slot, 0][~keep] == 0.0).all()), "samples outside the emitted run must be 0.0"
        out.append(wav[slot, :, off:off + cnt])
        for s in plays:
            pos[s] += counts[s]
        i += 1
        assert i < 500
    return torch.cat(out, dim=1)


def _check_bits(device, graphs=(False,)):
    """torch.equal at equal chunk size: alone in slot 0 / in slot 2 among other utterances / with held steps / with the end
    learnt late / (GPU) graph replay against eager launches."""
    import kantts._hip as hip
    from kantts.models.hifigan.chunked_nc import ChunkedNCVocoder

    hip.set_precision("fp32")
    G = _gnc("s4x2", device)
    mels = _mels(device, [11, 23, 2])
    base = None
    for graph in graphs:
        v = ChunkedNCVocoder(G, slots=3, graph=graph)
        for n in (4, 5):
            a = _manual(v, mels[0], n, 0)
            assert a.shape == (1, 11 * v.hop)
            assert torch.equal(a, torch.cat(list(v.synthesize(mels[0], chunk_frames=n)), dim=1)), ("synthesize", n)
            assert torch.equal(a, _manual(v, mels[0], n, 2, others={0: mels[1], 1: mels[2]})), ("slot 2 among others", n)
            assert torch.equal(a, _manual(v, mels[0], n, 0, pause=(0, 2, 3, 7), others={1: mels[1]})), ("held steps", n)
            assert torch.equal(a, _manual(v, mels[0], n, 0, late_end=True)), ("late end", n)
            assert torch.equal(a, _manual(v, mels[0], n, 1, late_end=True, pause=(1, 4), others={2: mels[1]})), ("all", n)
            if base is None:
                base = {}
            assert torch.equal(base.setdefault(n, a), a), ("graph against eager", n)


def test_chunked_noncausal_bits_kernel_source():
    with kernel_source_on_cpu():
        _check_bits("cpu")


# ---------------------------------------------------------------------------------------------------------------------
# GPU legs of the class tests
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(_GNC))
def test_chunked_noncausal_generator_gpu(name):
    for n in (1, 4, 8):
        _check_generator_fp32(name, n, "cuda", graph=n == 8)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(_GNC))
def test_chunked_noncausal_generator_bf16_gpu(name):
    """bf16: the chunked path against the fp32 one-shot output errs at most twice as much (max-abs over the three
    utterances) as the bf16 one-shot path does against it, measured in the same run -- the yardstick of the chunk-boundary
    check of test_chunked_vocoder.py.  Both figures go to the parity report."""
    import kantts._hip as hip
    from kantts.models.hifigan.chunked_nc import ChunkedNCVocoder

    G, mels = _gnc(name, "cuda"), _mels("cuda")
    try:
        hip.set_precision("fp32")
        ref = torch.cat(_one_shot(G, mels), dim=1)
        hip.set_precision("bf16")
        one = float((torch.cat(_one_shot(G, mels), dim=1) - ref).abs().max())
        v = ChunkedNCVocoder(G, slots=2, graph=False)
        for n in (1, 4, 8):
            for kind, got in zip(("synthesize", "play_many"), _chunked(v, mels, n)):
                err = float((torch.cat(got, dim=1) - ref).abs().max())
                print("chunked non-causal bf16", name, kind, "chunk", n, "max-abs", err, "one-shot bf16", one)
                _record("bf16_%s_%s_chunk%d" % (name, kind, n), {"chunked_max_abs": err, "one_shot_bf16_max_abs": one})
                assert err <= 2 * one, (name, kind, n, err, one)
    finally:
        hip.set_precision("fp32")


@pytest.mark.gpu
def test_chunked_noncausal_bits_gpu():
    _check_bits("cuda", graphs=(False, True))


def _check_synthesize_leaves_the_other_slots_alone(device, graph):
    """Slot 1 is in the middle of an utterance whose ``end`` was given with its first step; ``synthesize`` on slot 0 runs
    in between; slot 1's remaining bare steps (no ``end``) give the bits of an undisturbed run."""
    import kantts._hip as hip
    from kantts.models.hifigan.chunked_nc import ChunkedNCVocoder

    hip.set_precision("fp32")
    v = ChunkedNCVocoder(_gnc("s4x2", device), slots=2, graph=graph)
    other, mine = _mels(device, [6, 9])
    T, n = 9, 4

    def play(disturb):
        v.reset()
        outs, pos = [], 0
        while pos < T + v.flush_frames:
            m = min(n, T + v.flush_frames - pos)
            live = max(0, min(m, T - pos))
            buf = torch.zeros(2, 80, n, device=device)
            buf[1, :, :live] = mine[:, pos:pos + live]
            wav = v.step(buf, rows=[0, m], end=[-1, T] if pos == 0 else None)
            off, cnt = hip.nc_emit(pos, m, T, v.delay_samples, v.hop)
            outs.append(wav[1, :, off:off + cnt].clone())
            pos += m
            if disturb and pos in (n, T + 3):  # once among the live frames, once among the flush frames
                assert torch.cat(list(v.synthesize(other, chunk_frames=n, slot=0)), dim=1).shape == (1, 6 * v.hop)
                assert v._end.tolist() == [6, T]
        return torch.cat(outs, dim=1)

    a, b = play(False), play(True)
    assert a.shape == (1, T * v.hop) and torch.equal(a, b)


def test_synthesize_leaves_the_other_slots_alone_kernel_source():
    with kernel_source_on_cpu():
        _check_synthesize_leaves_the_other_slots_alone("cpu", False)


@pytest.mark.gpu
def test_synthesize_leaves_the_other_slots_alone_gpu():
    _check_synthesize_leaves_the_other_slots_alone("cuda", True)


def test_end_as_a_tensor_is_copied_as_a_sequence_is_clamped():
    from kantts.models.hifigan.chunked_nc import ChunkedNCVocoder

    with kernel_source_on_cpu():
        v = ChunkedNCVocoder(_gnc("s4x2"), slots=2, graph=False)
        mel = torch.zeros(2, 80, 4)
        v.step(mel, rows=[0, 0], end=[-5, 3])
        assert v._end.tolist() == [-1, 3]
        v.step(mel, rows=[0, 0], end=torch.tensor([-5, 3]))
        assert v._end.tolist() == [-5, 3]


def _check_play_many_bits(device, graph):
    """More utterances than slots, one shorter than a chunk and than ``flush_frames``: play_many equals synthesize bit for
    bit."""
    import kantts._hip as hip
    from kantts.models.hifigan.chunked_nc import ChunkedNCVocoder

    hip.set_precision("fp32")
    v = ChunkedNCVocoder(_gnc("s4x2", device), slots=2, graph=graph)
    assert v.flush_frames > 1
    syn, many = _chunked(v, _mels(device, [1, 5, 9]), 4)
    for i, (a, b) in enumerate(zip(syn, many)):
        assert torch.equal(a, b), "play_many utterance %d differs from synthesize" % i


def test_chunked_noncausal_play_many_bits_kernel_source():
    with kernel_source_on_cpu():
        _check_play_many_bits("cpu", False)


@pytest.mark.gpu
def test_chunked_noncausal_play_many_bits_gpu():
    _check_play_many_bits("cuda", True)


@pytest.mark.gpu
def test_chunked_noncausal_refusals_gpu():
    from kantts.models.hifigan.chunked_nc import ChunkedNCVocoder

    for G, exc, pat in _refusal_cases():
        with pytest.raises(exc, match=pat):
            ChunkedNCVocoder(G.cuda(), slots=1, graph=True)


# ---------------------------------------------------------------------------------------------------------------------
# StreamingTTS(lookahead=True): the fixtures of tests/test_streaming_tts.py (imported, not edited)
def _check_streaming_lookahead(leg, dev, Tc):
    """Four utterances (96, 45, 6 frames and a free-running one) through two slots.  The pipeline runs in bf16 mode (the rule
    of AcousticSlots), so the audio is held to the bf16 bound of the generator test: against the fp32 one-shot output of the
    mel the pool produced, the streamed audio errs at most twice as much (max-abs over all utterances) as the bf16 one-shot
    path, measured in the same run."""
    import kantts._hip as hip
    import test_streaming_tts as _st
    from kantts.models.streaming import StreamingTTS

    m, _, utts, refs = _st._as._utterances(leg, dev)
    G = _gnc("s4x2", dev)
    with pytest.raises(ValueError, match="causal"):  # the default keeps the refusal
        StreamingTTS(m, G, slots=2, max_steps=32, chunk_frames=Tc, graph=False)
    tts = StreamingTTS(m, G, slots=2, max_steps=32, chunk_frames=Tc, graph=dev == "cuda", lookahead=True)
    assert tts.nc and tts.flush_frames == tts.vocoder.flush_frames == 27 and tts.hop == 8
    released = {}
    release = tts.release

    def rec_release(s, results=None):
        released[tts.index[s]] = (tts.frames[s], tts.vocoded[s], tts.flushed[s], tts.samples[s])
        return release(s, results)

    tts.release = rec_release
    results, chunks = {}, {}
    for index, first, wav in tts.play_many(utts, results=results):
        assert first == sum(w.shape[-1] for w in chunks.get(index, [])), (index, first)
        chunks.setdefault(index, []).append(wav.clone())
    assert sorted(results) == sorted(released) == [0, 1, 2, 3] and tts.index == [None, None]
    got, mels = [], []
    for i, r in enumerate(refs):
        frames = int(r["LR_length_rounded"][0])
        y = torch.cat(chunks[i], dim=1)
        assert y.shape == (1, frames * tts.hop), (i, y.shape, frames)
        # released only after the flush: every frame vocoded, every flush frame taken, every sample out
        assert released[i] == (frames, frames, tts.flush_frames, frames * tts.hop), (i, released[i])
        got.append(y)
        mels.append(results[i]["postnet_outputs"][0, :frames].t().contiguous().float())
    one = torch.cat(_one_shot(G, mels), dim=1)
    hip.set_precision("fp32")
    ref = torch.cat(_one_shot(G, mels), dim=1)
    hip.set_precision("bf16")
    e_one, e_chunked = float((one - ref).abs().max()), float((torch.cat(got, dim=1) - ref).abs().max())
    print("streaming lookahead", leg, "chunk", Tc, "max-abs", e_chunked, "one-shot bf16", e_one)
    _record("streaming_%s_chunk%d" % (leg, Tc), {"chunked_max_abs": e_chunked, "one_shot_bf16_max_abs": e_one})
    assert e_chunked <= 2 * e_one, (Tc, e_chunked, e_one)


@pytest.mark.parametrize("leg", _ca.LEGS)
@pytest.mark.parametrize("Tc", [15])
def test_streaming_tts_lookahead_plays_a_noncausal_generator(Tc, leg):
    import kantts._hip as hip

    ctx, dev = _ca._leg(leg)
    hip.set_precision("bf16")
    try:
        with ctx:
            _check_streaming_lookahead(leg, dev, Tc)
    finally:
        hip.set_precision("fp32")
