"""Chunked inference of NSF generators: the streamed sine source and the excitation down-convolutions
(csrc/nsf_source.hip: kantts_nsf_source_rows, kantts_nsf_downs_rows), SourceModule.excitation_from,
kantts.models.hifigan.chunked_nsf.ChunkedNSFVocoder and infer_hifigan --chunk_frames on an NSF checkpoint.

CPU leg: the kernel SOURCE on the host build (util.kernel_source_on_cpu), graph=False.  GPU leg: the same checks on the
device, graph both True and False.  Inputs that a call must not read hold NaN; outputs and the state half to be written
hold a sentinel and have guard cells around them.

Bounds.  Against fp64 formulas: max-abs <= 2e-5, the project's fp32 single-layer bound (the fixed-point phase is within
2^-24 cycles * 2 pi * alpha < 1e-7 of the fp64 running sum here).  Wherever two plays run the same arithmetic the assertion
is torch.equal: a sample of the source depends on the integer phase, the absolute sample index and its frame's inputs only,
an output row of a down-convolution on its window only.  Whole generator: fp32 mean-abs <= 1e-5, bf16 mean-abs <= 2e-3
against Generator.forward in the same precision mode, the bounds of test_chunked_vocoder.py for this comparison."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

from util import ROOT, assert_close, kernel_source_on_cpu

S, H1, SR = 3, 8, 16000
ALPHA, SIGMA = 0.1, 0.003
SENT = -1234.5
NAN = float("nan")
GUARD = 7


def _source_module(hop):
    from kantts.models.hifigan.layers import SourceModule

    return SourceModule(nb_harmonics=H1 - 1, upsample_ratio=hop, sampling_rate=SR)


class _Inputs:
    """Seeded inputs of S utterances of T frames: f0 in 60..400 Hz, voiced frames, frames with uv = 0, one with uv = 0.5."""

    def __init__(self, hop, T=24, seed=1):
        g = torch.Generator().manual_seed(seed)
        self.hop, self.T = hop, T
        self.f0 = 60.0 + 340.0 * torch.rand(S, T, generator=g)
        self.uv = torch.ones(S, T)
        self.uv[0, 5:9] = 0.0
        self.uv[1, :3] = 0.0
        self.uv[2, 20:] = 0.0
        self.uv[1, 11] = 0.5
        self.noise = SIGMA * torch.randn(S, T * hop, H1, generator=g)
        self.phase0 = (torch.rand(S, H1, generator=g) * 2 - 1) * math.pi
        self.phase0[:, 0] = 0.0
        self.w = torch.randn(H1, generator=g) * 0.6
        self.b = torch.randn(1, generator=g) * 0.1

    def states(self, given, seed=0):
        from kantts.models.hifigan.chunked_nsf import initial_state

        return torch.stack([initial_state(seed, 10 + s, H1, self.phase0[s] if given else None) for s in range(S)])


def _source_call(device, inp, state, f0, uv, noise=None, rows=None, harm=False, w=None, b=None):
    """One launch on fresh buffers: f0 / uv (S, Tc), state (S, 36) int32 -> e (S, Tc * hop), state_out, harm or None."""
    import kantts._hip as hip

    nS, Tc = f0.shape
    hop, W = inp.hop, hip.NSF_STATE_WORDS
    ss = W + 2
    arena = torch.full((2, nS, ss), GUARD, dtype=torch.int32)
    arena[0, :, :W] = state
    arena[1, :, :W] = -99
    arena = arena.to(device)
    n = nS * Tc * hop
    flat = torch.full((n + 32,), float(GUARD)).to(device)
    e = flat[16:16 + n].view(nS, Tc * hop)
    e.fill_(SENT)
    hm = torch.full((nS, Tc * hop, H1), SENT).to(device) if harm else None
    ok = hip.nsf_source(f0.contiguous().to(device), uv.contiguous().to(device), arena[0, 0], arena[1, 0],
                        (inp.w if w is None else w).to(device), e, S=nS, Tc=Tc, hop=hop, H1=H1, sr=SR, alpha=ALPHA, sigma=SIGMA,
                        state_ss=ss, bias=(inp.b if b is None else b).to(device),
                        noise=None if noise is None else noise.contiguous().to(device), harm=hm,
                        rows=None if rows is None else torch.tensor(rows, dtype=torch.int32).to(device))
    assert ok
    assert bool((arena[:, :, W:] == GUARD).all()), "guard words behind a slot's state were written"
    assert torch.equal(arena[0, :, :W].cpu(), state), "state_in was written"
    assert bool((flat[:16] == GUARD).all()) and bool((flat[-16:] == GUARD).all()), "guard cells around e were written"
    return e.cpu().clone(), arena[1, :, :W].cpu().clone(), None if hm is None else hm.cpu()


def _formula64(inp, hop, exact_index):
    """The excitation of the module's formula in fp64, projected: (S, T * hop).  ``exact_index``: frames are repeated
    sample-exactly (n // hop) instead of going through interpolate."""
    sm = _source_module(hop)
    pitch, uv = inp.f0.double()[:, None, :], inp.uv.double()[:, None, :]
    phase, noise = inp.phase0.double()[:, :, None], inp.noise.double().transpose(1, 2)
    if exact_index:
        ps, us = pitch.repeat_interleave(hop, dim=-1), uv.repeat_interleave(hop, dim=-1)
        harm = torch.arange(1, H1 + 1, dtype=torch.float64).view(1, -1, 1)
        theta = 2 * np.pi * (torch.cumsum(ps * harm / SR, dim=-1) % 1)
        x = (ALPHA * torch.sin(theta + phase) + noise) * us + (ALPHA / 3 / SIGMA * noise) * (1 - us)
    else:
        x = sm.excitation_from(pitch, uv, phase, noise)
    assert x.dtype == torch.float64 and tuple(x.shape) == (S, H1, inp.T * hop)
    return torch.tanh(inp.b.double() + (x * inp.w.double().view(1, -1, 1)).sum(1)), x


def _check_source_formula(device, hop):
    inp = _Inputs(hop)
    ref, x64 = _formula64(inp, hop, exact_index=hop != 8)
    if hop == 8:  # a power of two: interpolate's index is exact too, and the two forms of the formula agree
        assert_close(ref, _formula64(inp, hop, True)[0], 1e-12, what="formula")
    e, st, hm = _source_call(device, inp, inp.states(True), inp.f0, inp.uv, noise=inp.noise, harm=True)
    err = float((e.double() - ref).abs().max())
    print("nsf source vs fp64 formula: hop", hop, "max-abs", err)
    assert err <= 2e-5, err
    assert_close(hm.double(), x64.transpose(1, 2), 2e-5, what="harmonics before the projection")
    cur = st[:, 32:34].contiguous().view(torch.int64).reshape(-1)
    assert cur.tolist() == [inp.T * hop] * S
    assert torch.equal(st[:, 16:32], inp.states(True)[:, 16:32]) and torch.equal(st[:, 34:], inp.states(True)[:, 34:])


# ---------------------------------------------------------------------------------------------------------------------
# down-convolutions
_DOWN_CASES = {
    "u2_1": (4, (2, 1), (24, 10)),
    "u6_2_1": (12, (6, 2, 1), (33, 16, 5)),
    "u30_6_2_1": (60, (30, 6, 2, 1), (32, 16, 16, 16)),
}


class _Downs:
    def __init__(self, hop, us, Cs, seed=2):
        g = torch.Generator().manual_seed(seed)
        self.hop, self.us, self.Cs = hop, us, Cs
        self.ks = [2 * u if u > 1 else 1 for u in us]
        self.W = [torch.randn(C, 1, k, generator=g) / k ** 0.5 for C, k in zip(Cs, self.ks)]
        self.B = [torch.randn(C, generator=g) for C in Cs]
        self.Hh = max(self.ks) - 1

    def stages(self, device):
        return [(u, k, C, W[:, 0, :].t().contiguous().to(device), B.to(device))
                for u, k, C, W, B in zip(self.us, self.ks, self.Cs, self.W, self.B)]

    def torch64(self, e):
        """e (n,) -> [d_i (n / u_i, C_i)] by conv1d in fp64 on the left-padded signal."""
        x = e.double()[None, None, :]
        return [F.conv1d(F.pad(x, (k - 1, 0)), W.double(), B.double(), stride=u)[0].t()
                for u, k, W, B in zip(self.us, self.ks, self.W, self.B)]

    def call(self, device, e, hist, rows=None):
        """e (S, Tc * hop), hist (S, Hh) -> [d_i], hist_out."""
        import kantts._hip as hip

        nS, n = e.shape
        Tc = n // self.hop
        ss = self.Hh + 3
        arena = torch.full((2, nS, ss), float(GUARD))
        arena[0, :, :self.Hh] = hist
        arena[1, :, :self.Hh] = SENT
        arena = arena.to(device)
        flats, outs = [], []
        for u, C in zip(self.us, self.Cs):
            m = nS * (n // u) * C
            fl = torch.full((m + 32,), float(GUARD)).to(device)
            o = fl[16:16 + m].view(nS, n // u, C)
            o.fill_(SENT)
            flats.append(fl)
            outs.append(o)
        ok = hip.nsf_downs(e.contiguous().to(device), arena[0, 0], arena[1, 0], self.stages(device), outs, S=nS, Tc=Tc,
                           hop=self.hop, hist_ss=ss, rows=None if rows is None else torch.tensor(rows, dtype=torch.int32).to(device))
        assert ok
        assert bool((arena[:, :, self.Hh:] == GUARD).all()), "guard floats behind a slot's history were written"
        assert torch.equal(arena[0, :, :self.Hh].cpu(), hist), "hist_in was written"
        for fl in flats:
            assert bool((fl[:16] == GUARD).all()) and bool((fl[-16:] == GUARD).all()), "guard cells around an output were written"
        return [o.cpu().clone() for o in outs], arena[1, :, :self.Hh].cpu().clone()


def _check_downs(device, name):
    hop, us, Cs = _DOWN_CASES[name]
    D = _Downs(hop, us, Cs)
    T = 10
    e = torch.rand(S, T * hop, generator=torch.Generator().manual_seed(4)) * 2 - 1
    outs, hist = D.call(device, e, torch.zeros(S, D.Hh))
    for s in range(S):
        for i, (o, r) in enumerate(zip(outs, D.torch64(e[s]))):
            assert_close(o[s].double(), r, 2e-5, what="%s stage %d slot %d" % (name, i, s))
    assert torch.equal(hist, e[:, T * hop - D.Hh:])
    # ragged: dead rows untouched, dead inputs not read, the state of a paused slot copied
    rows = [3, 0, T]
    en = e.clone()
    h0 = torch.randn(S, D.Hh, generator=torch.Generator().manual_seed(6))
    for s, n in enumerate(rows):
        en[s, n * hop:] = NAN
    outs2, hist2 = D.call(device, en, h0, rows=rows)
    full, _ = D.call(device, e, h0)
    for s, n in enumerate(rows):
        for i, u in enumerate(us):
            live = n * hop // u
            assert torch.equal(outs2[i][s, :live], full[i][s, :live]), (name, i, s)
            assert bool((outs2[i][s, live:] == SENT).all()), ("dead rows", name, i, s)
        assert torch.equal(hist2[s], torch.cat([h0[s], e[s, :n * hop]])[n * hop:]), (name, s)
    assert torch.equal(hist2[1], h0[1])


# ---------------------------------------------------------------------------------------------------------------------
# cut invariance: the source and the down-convolutions of a hop-8 generator (u = 2, 1) through four schedules
_RAGGED = [[5, 0, 8], [0, 3, 8], [8, 8, 8], [8, 5, 0], [3, 8, 0]]
_SCHEDULES = {"one": [24], "8x3": [8, 8, 8], "3_5_1_7_8": [3, 5, 1, 7, 8], "ragged": _RAGGED}


def _play_kernels(device, inp, D, sched, given):
    """-> e (S, T * hop), [d_i (S, T * hop / u_i, C_i)], final source state, final history."""
    hop, T = inp.hop, inp.T
    state, hist = inp.states(given), torch.zeros(S, D.Hh)
    pos = [0] * S
    es, ds = [[] for _ in range(S)], [[[] for _ in D.us] for _ in range(S)]
    for item in sched:
        ragged = isinstance(item, list)
        Tc = 8 if ragged else item
        counts = item if ragged else [Tc] * S
        f0, uv = torch.full((S, Tc), NAN), torch.full((S, Tc), NAN)
        nz = torch.full((S, Tc * hop, H1), NAN)
        for s, c in enumerate(counts):
            f0[s, :c], uv[s, :c] = inp.f0[s, pos[s]:pos[s] + c], inp.uv[s, pos[s]:pos[s] + c]
            nz[s, :c * hop] = inp.noise[s, pos[s] * hop:(pos[s] + c) * hop]
        rows = counts if ragged else None
        e, state2, _ = _source_call(device, inp, state, f0, uv, noise=nz if given else None, rows=rows)
        d, hist2 = D.call(device, e, hist, rows=rows)
        for s, c in enumerate(counts):
            assert bool((e[s, c * hop:] == SENT).all()), "samples behind a slot's count were written"
            if c == 0:
                assert torch.equal(state2[s], state[s]) and torch.equal(hist2[s], hist[s]), "a paused slot's state changed"
            es[s].append(e[s, :c * hop])
            for i, u in enumerate(D.us):
                ds[s][i].append(d[i][s, :c * hop // u])
            pos[s] += c
        state, hist = state2, hist2
    assert pos == [T] * S
    e = torch.stack([torch.cat(x) for x in es])
    d = [torch.stack([torch.cat(ds[s][i]) for s in range(S)]) for i in range(len(D.us))]
    assert not bool(torch.isnan(e).any()) and not any(bool(torch.isnan(x).any()) for x in d)
    return e, d, state, hist


def _check_cut_invariance(device, given):
    inp, D = _Inputs(8), _Downs(8, (2, 1), (32, 16))
    want = None
    for name, sched in _SCHEDULES.items():
        got = _play_kernels(device, inp, D, sched, given)
        if want is None:
            want = got
            continue
        assert torch.equal(got[0], want[0]), ("e", name)
        for i in range(len(D.us)):
            assert torch.equal(got[1][i], want[1][i]), ("d", i, name)
        assert torch.equal(got[2], want[2]), ("state", name)
        assert torch.equal(got[3], want[3]), ("history", name)
    if given:  # and the one call is the formula
        assert float((want[0].double() - _formula64(inp, 8, True)[0]).abs().max()) <= 2e-5


# ---------------------------------------------------------------------------------------------------------------------
# generated noise
def _generated(device, key, voiced):
    """50 frames of hop 64 at 200 Hz in chunks of 7 frames -> the excitation before its projection (3200, 8)."""
    from kantts.models.hifigan.chunked_nsf import initial_state

    inp = _Inputs(64, T=50)
    state = initial_state(0, key, H1)[None]
    parts = []
    for t0 in range(0, 50, 7):
        n = min(7, 50 - t0)
        f0 = torch.full((1, n), 200.0 if voiced else 0.0)
        _, state, hm = _source_call(device, inp, state, f0, torch.full((1, n), 1.0 if voiced else 0.0), harm=True)
        parts.append(hm[0])
    return torch.cat(parts)


def _check_generated_noise(device):
    x = _generated(device, 3, voiced=False)
    assert tuple(x.shape) == (3200, 8)
    std, mean = float(x.std()), float(x.mean())
    r1 = float((x[1:] * x[:-1]).sum() / (x * x).sum())
    print("generated noise: std", std, "mean", mean, "lag-1 autocorrelation", r1)
    assert abs(std - ALPHA / 3) < 2e-3
    assert abs(mean) < 1e-3
    assert abs(r1) < 0.05
    assert torch.equal(x, _generated(device, 3, voiced=False)), "the same key must give the same bits"
    assert not torch.equal(x, _generated(device, 4, voiced=False)), "two keys must give different noise"
    v = _generated(device, 3, voiced=True)[:, 0]
    assert abs(float(v.pow(2).mean().sqrt()) - ALPHA / 2 ** 0.5) < 3e-3
    assert float((v[:1600] - v[80:1680]).abs().mean()) < 0.01  # 200 Hz at 16 kHz: a period of 80 samples


# ---------------------------------------------------------------------------------------------------------------------
# argument errors and refusals: the return codes of include/kantts_hip.h, and nothing written
def _check_codes(device):
    import kantts._hip as hip

    L = hip.lib()
    W = hip.NSF_STATE_WORDS
    bufs = dict(f0=torch.full((2, 4), 100.0), uv=torch.ones(2, 4), w=torch.ones(16), st=torch.zeros(2, 2, W, dtype=torch.int32),
                e=torch.full((2, 32), SENT), hist=torch.zeros(2, 2, 8), w0=torch.ones(4, 3), w1=torch.ones(1, 3),
                o0=torch.full((2, 16, 3), SENT), o1=torch.full((2, 32, 3), SENT))
    bufs = {k: v.to(device) for k, v in bufs.items()}
    st = bufs["st"]
    st[1] = -99

    def source(**over):
        g = hip.NsfSourceArgs()
        g.f0, g.uv, g.w, g.e = (hip.ptr(bufs[k]) for k in ("f0", "uv", "w", "e"))
        g.state_in, g.state_out, g.state_ss = hip.ptr(st[0]), hip.ptr(st[1]), W
        g.S, g.Tc, g.hop, g.H1, g.sr, g.alpha, g.sigma = 2, 4, 8, 8, SR, ALPHA, SIGMA
        for k, v in over.items():
            setattr(g, k, v)
        return L.kantts_nsf_source_rows(ctypes.byref(g), hip.stream())

    def downs(**over):
        g = hip.NsfDownsArgs()
        g.e, g.hist_in, g.hist_out, g.hist_ss = hip.ptr(bufs["e"]), hip.ptr(bufs["hist"][0]), hip.ptr(bufs["hist"][1]), 8
        g.S, g.Tc, g.hop, g.nstages = 2, 4, 8, 2
        g.u[0], g.k[0], g.C[0], g.w[0], g.out[0] = 2, 4, 3, hip.ptr(bufs["w0"]), hip.ptr(bufs["o0"])
        g.u[1], g.k[1], g.C[1], g.w[1], g.out[1] = 1, 1, 3, hip.ptr(bufs["w1"]), hip.ptr(bufs["o1"])
        for k, v in over.items():
            if isinstance(v, tuple):
                getattr(g, k)[v[0]] = v[1]
            else:
                setattr(g, k, v)
        return L.kantts_nsf_downs_rows(ctypes.byref(g), hip.stream())

    BAD, UNS = -1, hip.E_UNSUPPORTED
    assert L.kantts_nsf_source_rows(None, hip.stream()) == BAD and L.kantts_nsf_downs_rows(None, hip.stream()) == BAD
    for name in ("f0", "uv", "w", "state_in", "state_out", "e"):
        assert source(**{name: None}) == BAD, name
    assert source(Tc=0) == BAD and source(hop=0) == BAD and source(H1=0) == BAD and source(sr=0.0) == BAD
    assert source(state_out=hip.ptr(st[0])) == BAD and source(state_ss=W - 2) == BAD
    assert source(H1=17) == UNS and source(state_ss=W + 1) == UNS
    assert downs(e=None) == BAD and downs(Tc=0) == BAD and downs(nstages=0) == BAD and downs(hop=0) == BAD
    assert downs(w=(1, None)) == BAD and downs(out=(0, None)) == BAD and downs(C=(0, 0)) == BAD
    assert downs(hist_in=None) == BAD and downs(hist_out=hip.ptr(bufs["hist"][0])) == BAD and downs(hist_ss=2) == BAD
    assert downs(nstages=9) == UNS and downs(u=(0, 3)) == UNS and downs(k=(0, 8193)) == UNS
    assert bool((bufs["e"] == SENT).all()) and bool((bufs["o0"] == SENT).all()) and bool((bufs["o1"] == SENT).all())
    assert bool((st[1] == -99).all()) and not bool(bufs["hist"].any()), "a refused call wrote its state"
    assert source() == 0 and downs() == 0
    assert not bool((bufs["o0"] == SENT).any()) and not bool((bufs["o1"] == SENT).any())
    # the wrappers: declined shapes are False, bad arguments raise
    kw = dict(S=2, Tc=4, hop=8, sr=SR, alpha=ALPHA, sigma=SIGMA)
    assert hip.nsf_source(bufs["f0"], bufs["uv"], st[0], st[1], torch.ones(17).to(device), bufs["e"], H1=17, **kw) is False
    with pytest.raises(RuntimeError):
        hip.nsf_source(bufs["f0"], bufs["uv"], st[0], st[0], bufs["w"], bufs["e"], H1=8, **kw)
    with pytest.raises(ValueError):
        hip.nsf_source(bufs["f0"], bufs["uv"], st[0], st[1], bufs["w"], bufs["e"], H1=8,
                       rows=torch.zeros(3, dtype=torch.int32).to(device), **kw)
    nine = [(1, 1, 3, bufs["w1"], None)] * 9
    assert hip.nsf_downs(bufs["e"], bufs["hist"][0], bufs["hist"][1], nine, [bufs["o1"]] * 9, S=2, Tc=4, hop=8, hist_ss=8) is False


def test_nsf_struct_layouts_match_the_header(tmp_path):
    """NsfSourceArgs / NsfDownsArgs and the state size against gcc's view of include/kantts_hip.h."""
    import kantts._hip as hip

    pairs = [(hip.NsfSourceArgs, "kantts_nsf_source_args"), (hip.NsfDownsArgs, "kantts_nsf_downs_args")]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "kantts_hip.h"', 'int main(void) {',
             '  printf("state words %d\\n", KANTTS_NSF_STATE_WORDS);']
    for cls, cname in pairs:
        lines.append('  printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in cls._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    c_layout = {}
    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        cname, field, val = ln.split()
        c_layout[(cname, field)] = int(val)
    assert c_layout[("state", "words")] == hip.NSF_STATE_WORDS
    for cls, cname in pairs:
        assert ctypes.sizeof(cls) == c_layout[(cname, "sizeof")], cname
        for fname, _ in cls._fields_:
            assert getattr(cls, fname).offset == c_layout[(cname, fname)], (cname, fname)


def test_excitation_draws_are_unchanged():
    """excitation == the same draws handed to excitation_from, and excitation_from keeps the dtype of its inputs."""
    from torch.distributions.normal import Normal
    from torch.distributions.uniform import Uniform

    sm = _source_module(6)
    pitch, uv = torch.rand(2, 1, 5) * 300 + 60, (torch.rand(2, 1, 5) > 0.3).float()
    torch.manual_seed(7)
    e = sm.excitation(pitch, uv)
    torch.manual_seed(7)
    one = torch.ones(())
    phase = Uniform(low=-np.pi * one, high=np.pi * one).sample(sample_shape=(2, H1, 1))
    phase[:, 0, :] = 0
    noise = Normal(loc=0.0 * one, scale=SIGMA * one).sample(sample_shape=(2, H1, 30))
    assert torch.equal(e, sm.excitation_from(pitch, uv, phase, noise)) and e.dtype == torch.float32
    assert sm.excitation_from(pitch.double(), uv.double(), phase.double(), noise.double()).dtype == torch.float64


@pytest.mark.parametrize("hop", [8, 6])
def test_nsf_source_matches_the_fp64_formula(hop):
    with kernel_source_on_cpu():
        _check_source_formula("cpu", hop)


@pytest.mark.parametrize("name", sorted(_DOWN_CASES))
def test_nsf_downs_match_torch(name):
    with kernel_source_on_cpu():
        _check_downs("cpu", name)


@pytest.mark.parametrize("given", [True, False], ids=["given", "generated"])
def test_nsf_kernels_do_not_depend_on_the_cuts(given):
    with kernel_source_on_cpu():
        _check_cut_invariance("cpu", given)


def test_nsf_generated_noise():
    with kernel_source_on_cpu():
        _check_generated_noise("cpu")


def test_nsf_return_codes():
    with kernel_source_on_cpu():
        _check_codes("cpu")


# ---------------------------------------------------------------------------------------------------------------------
# model level
_GNSF = dict(in_channels=80, channels=64, upsample_scales=[4, 2], upsample_kernal_sizes=[8, 4],
             nsf_params={"nb_harmonics": 7, "sampling_rate": 16000})
_SHIPPED_NSF = dict(in_channels=80, channels=512, upsample_scales=[8, 5, 3, 2], upsample_kernal_sizes=[16, 10, 6, 4],
                    nsf_params={"nb_harmonics": 7, "sampling_rate": 24000})


def _gnsf(params=_GNSF):
    from kantts.models.hifigan.hifigan import Generator

    torch.manual_seed(0)
    G = Generator(**params).eval()
    G.remove_weight_norm()
    return G


def _feats(T, seed, C=80):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(C + 2, T, generator=g)
    x[-2] = 60.0 + 340.0 * torch.rand(T, generator=g)
    x[-1] = (torch.rand(T, generator=g) > 0.25).float()
    x[-2] *= x[-1]  # unvoiced frames carry f0 = 0, as the acoustic model's features do
    return x


def _yardstick(G, v, feats, key):
    """Generator.forward of the whole utterance with SourceModule.excitation returning what the source kernel produces in
    ONE call over the whole utterance (before its projection)."""
    import kantts._hip as hip
    from kantts.models.hifigan.chunked_nsf import initial_state
    from kantts.models.hifigan.layers import SourceModule

    dev = feats.device
    T = feats.shape[1]
    st = torch.zeros(2, 1, hip.NSF_STATE_WORDS, dtype=torch.int32)
    st[0, 0] = initial_state(v.seed, key, v.H1)
    st = st.to(dev)
    e = torch.empty(1, T * v.hop, device=dev)
    harm = torch.empty(1, T * v.hop, v.H1, device=dev)
    assert hip.nsf_source(feats[-2:-1].contiguous(), feats[-1:].contiguous(), st[0, 0], st[1, 0], v._src_w, e, S=1, Tc=T,
                          hop=v.hop, H1=v.H1, sr=v.sr, alpha=v.alpha, sigma=v.sigma, bias=v._src_b, harm=harm)
    orig = SourceModule.excitation
    SourceModule.excitation = lambda self, pitch, uv: harm.transpose(1, 2)
    try:
        with torch.no_grad():
            return G(feats[None])[0]
    finally:
        SourceModule.excitation = orig


_LENS = (21, 9, 14)


def _check_model(device, mode, graphs, params=_GNSF, T=21, chunks=(1, 4, 8), many=True):
    import kantts._hip as hip
    from kantts.models.hifigan.chunked_nsf import ChunkedNSFVocoder

    bound = 1e-5 if mode == "fp32" else 2e-3
    hip.set_precision(mode)
    try:
        G = _gnsf(params).to(device)
        utts = [_feats(n, 20 + i).to(device) for i, n in enumerate((T,) + _LENS[1:])]
        vs = [ChunkedNSFVocoder(G, slots=2, graph=gr, seed=5) for gr in graphs]
        refs = [_yardstick(G, vs[0], x, key=i).cpu() for i, x in enumerate(utts if many else utts[:1])]
        plays = []
        for v in vs:
            for n in chunks:
                wav = torch.cat([c.cpu() for c in v.synthesize(utts[0], chunk_frames=n, slot=n % 2, key=0)], dim=1)
                assert wav.shape == refs[0].shape == (1, T * v.hop)
                err = float((wav - refs[0]).abs().mean())
                print("chunked NSF", mode, "graph" if v.graph else "eager", "chunk", n, "mean-abs", err)
                assert err <= bound, (mode, n, err)
                plays.append(wav)
            if many:
                parts = {}
                for i, wav in v.play_many(utts, chunk_frames=8):
                    parts.setdefault(i, []).append(wav.cpu())
                for i, ref in enumerate(refs):
                    wav = torch.cat(parts[i], dim=1)
                    assert wav.shape == ref.shape
                    err = float((wav - ref).abs().mean())
                    print("chunked NSF", mode, "graph" if v.graph else "eager", "play_many utterance", i, "mean-abs", err)
                    assert err <= bound, (mode, i, err)
                    want = torch.cat([c.cpu() for c in v.synthesize(utts[i], chunk_frames=8, slot=1, key=i)], dim=1)
                    assert torch.equal(wav, want), "play_many utterance %d differs from synthesize(key=%d)" % (i, i)
                plays.append(torch.cat(parts[0], dim=1))
        for p in plays[1:]:
            assert torch.equal(p, plays[0]), "chunkings / graph and eager runs must give identical bits"
        other = torch.cat([c.cpu() for c in vs[0].synthesize(utts[0], chunk_frames=8, key=1)], dim=1)
        assert not torch.equal(other, plays[0]), "another key must give another excitation"
    finally:
        hip.set_precision("fp32")


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_chunked_nsf_vocoder_matches_the_generator(mode):
    with kernel_source_on_cpu():
        _check_model("cpu", mode, [False])


def _check_noise_argument(device, graph):
    from kantts.models.hifigan.chunked_nsf import ChunkedNSFVocoder

    G = _gnsf().to(device)
    x = torch.stack([_feats(4, 1), _feats(4, 2)]).to(device)
    v = ChunkedNSFVocoder(G, slots=2, graph=graph)
    with pytest.raises(ValueError):
        v.step(x, noise=torch.zeros(2, 32, 8))
    g = ChunkedNSFVocoder(G, slots=2, graph=graph, given_noise=True)
    with pytest.raises(ValueError):
        g.step(x)
    with pytest.raises(ValueError):
        g.step(x, noise=torch.zeros(2, 32, 7))
    assert g._parity == 0
    zero = g.step(x, noise=torch.zeros(2, 32, 8).to(device))
    g.reset()
    nz = g.step(x, noise=(SIGMA * torch.randn(2, 32, 8)).to(device))
    assert zero.shape == nz.shape == (2, 1, 32) and not torch.equal(zero, nz)
    # the same given noise and phases: the same bits from a fresh object
    h = ChunkedNSFVocoder(G, slots=2, graph=graph, given_noise=True)
    assert torch.equal(h.step(x, noise=torch.zeros(2, 32, 8).to(device)), zero)
    h.reset(phase0=torch.zeros(8))
    assert not torch.equal(h.step(x, noise=torch.zeros(2, 32, 8).to(device)), zero)
    with pytest.raises(ValueError):
        h.reset(phase0=torch.zeros(5))


def test_chunked_nsf_noise_argument():
    with kernel_source_on_cpu():
        _check_noise_argument("cpu", False)


def test_chunked_nsf_refusals():
    import kantts._hip as hip
    from kantts.models.hifigan.chunked import ChunkedVocoder
    from kantts.models.hifigan.chunked_nsf import ChunkedNSFVocoder
    from kantts.models.hifigan.hifigan import Generator

    class _NoLaunch:
        def __getattr__(self, name):
            raise AssertionError("a refusal must not reach the library (%s)" % name)

    saved = hip.lib
    hip.lib = lambda: _NoLaunch()
    try:
        G = _gnsf()
        with pytest.raises(NotImplementedError):
            ChunkedVocoder(G, graph=False)  # the base class keeps refusing NSF generators
        with pytest.raises(ValueError):
            ChunkedNSFVocoder(Generator(channels=64, upsample_scales=[4, 2], upsample_kernal_sizes=[8, 4]).eval(), graph=False)
        with pytest.raises(ValueError):
            ChunkedNSFVocoder(Generator(causal=False, **_GNSF).eval(), graph=False)
        with pytest.raises(ValueError):
            ChunkedNSFVocoder(Generator(**_GNSF), graph=False)  # training mode
        many = dict(_GNSF, nsf_params={"nb_harmonics": 16, "sampling_rate": 16000})
        with pytest.raises(NotImplementedError):
            ChunkedNSFVocoder(Generator(**many).eval(), graph=False)
        odd = _gnsf()
        odd.source_downs[0] = type(odd.source_downs[0])(1, 32, 6, 2)
        with pytest.raises(NotImplementedError):
            ChunkedNSFVocoder(odd, graph=False)
    finally:
        hip.lib = saved


def _write_voice(tmp_path):
    voc_dir = tmp_path / "voc" / "ckpt"
    voc_dir.mkdir(parents=True)
    (tmp_path / "voc" / "config.yaml").write_text(yaml.dump(
        {"Model": {"Generator": {"params": _GNSF}}, "audio_config": {"sampling_rate": 16000}}))
    from kantts.models.hifigan.hifigan import Generator

    torch.manual_seed(0)
    torch.save({"model": {"generator": Generator(**_GNSF).state_dict()}}, voc_dir / "checkpoint_1.pth")
    mel_dir = tmp_path / "feats"
    mel_dir.mkdir()
    lengths = {"utt_a": 21, "utt_b": 5, "utt_c": 14}
    for i, (name, n) in enumerate(lengths.items()):
        x = _feats(n, 40 + i).t().numpy().copy()
        x[:, -1] = 0.2 + 0.7 * x[:, -1]  # a predicted voicing flag: binarised by the command line
        np.save(mel_dir / (name + ".npy"), x.astype(np.float32))
    return str(voc_dir / "checkpoint_1.pth"), str(mel_dir), lengths


def _check_cli(tmp_path):
    from kantts.bin.infer_hifigan import hifigan_infer, main
    from scipy.io import wavfile

    ck, mel_dir, lengths = _write_voice(tmp_path)
    main(["--ckpt", ck, "--input_mel", mel_dir, "--output_dir", str(tmp_path / "one"), "--chunk_frames", "8"])
    main(["--ckpt", ck, "--input_mel", mel_dir, "--output_dir", str(tmp_path / "two"), "--chunk_frames", "8", "--slots", "2"])
    main(["--ckpt", ck, "--input_mel", mel_dir, "--output_dir", str(tmp_path / "again"), "--chunk_frames", "8", "--seed", "0"])
    hifigan_infer(mel_dir, ck, str(tmp_path / "seed1"), chunk_frames=8, seed=1)
    for name, n in lengths.items():
        a, b, c, d = (wavfile.read(tmp_path / k / (name + "_gen.wav"))[1] for k in ("one", "two", "again", "seed1"))
        assert a.dtype == b.dtype == np.int16 and a.shape == b.shape == d.shape == (n * 8,)
        assert np.array_equal(a, b), "one slot and two slots differ: " + name
        assert np.array_equal(a, c), "a second run with the same seed differs: " + name
        assert not np.array_equal(a, d), "another seed must give another excitation: " + name


def test_infer_hifigan_chunked_nsf_cli(tmp_path, monkeypatch):
    import kantts._hip as hip
    from kantts.bin import infer_hifigan

    hip.set_precision("fp32")
    monkeypatch.setattr(infer_hifigan, "_device", lambda: torch.device("cpu"))
    with kernel_source_on_cpu():
        _check_cli(tmp_path)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
@pytest.mark.gpu
def test_nsf_source_and_downs_gpu():
    for hop in (8, 6):
        _check_source_formula("cuda", hop)
    for name in sorted(_DOWN_CASES):
        _check_downs("cuda", name)
    _check_codes("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("given", [True, False], ids=["given", "generated"])
def test_nsf_kernels_do_not_depend_on_the_cuts_gpu(given):
    _check_cut_invariance("cuda", given)


@pytest.mark.gpu
def test_nsf_generated_noise_gpu():
    _check_generated_noise("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_chunked_nsf_vocoder_matches_the_generator_gpu(mode):
    _check_model("cuda", mode, [True, False])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_chunked_nsf_vocoder_shipped_geometry_gpu(mode):
    _check_model("cuda", mode, [True, False], params=_SHIPPED_NSF, T=20, chunks=(8,), many=False)


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [True, False])
def test_chunked_nsf_noise_argument_gpu(graph):
    _check_noise_argument("cuda", graph)


def _check_short_utterances(device, graph):
    """More utterances than slots, one shorter than a chunk: play_many equals synthesize(key=i) bit for bit."""
    from kantts.models.hifigan.chunked_nsf import ChunkedNSFVocoder

    G = _gnsf().to(device)
    v = ChunkedNSFVocoder(G, slots=2, graph=graph, seed=5)
    utts = [_feats(n, 40 + i).to(device) for i, n in enumerate((1, 5, 9))]
    parts = {}
    for i, wav in v.play_many(utts, chunk_frames=4):
        parts.setdefault(i, []).append(wav.cpu())
    for i, x in enumerate(utts):
        want = torch.cat([c.cpu() for c in v.synthesize(x, chunk_frames=4, slot=i % 2, key=i)], dim=1)
        assert want.shape == (1, x.shape[1] * v.hop)
        assert torch.equal(torch.cat(parts[i], dim=1), want), "play_many utterance %d differs from synthesize" % i


def test_chunked_nsf_play_many_short_utterances():
    with kernel_source_on_cpu():
        _check_short_utterances("cpu", False)


@pytest.mark.gpu
def test_chunked_nsf_play_many_short_utterances_gpu():
    _check_short_utterances("cuda", True)


@pytest.mark.gpu
def test_chunked_nsf_graph_is_captured_once_gpu():
    """One capture per chunk size serves every count vector, key and reset: cursor, key and phases live on the device."""
    from kantts.models.hifigan.chunked_nsf import ChunkedNSFVocoder

    G = _gnsf().cuda()
    v = ChunkedNSFVocoder(G, slots=2, graph=True)
    utts = [_feats(n, 30 + i).cuda() for i, n in enumerate(_LENS)]
    list(v.play_many(utts, chunk_frames=8))
    assert v.captures == 1
    list(v.synthesize(utts[0], chunk_frames=8, key=3))
    assert v.captures == 2  # the plain (lockstep) form of a step keeps graphs of its own


@pytest.mark.gpu
def test_infer_hifigan_chunked_nsf_cli_gpu(tmp_path):
    import kantts._hip as hip

    hip.set_precision("fp32")
    _check_cli(tmp_path)
