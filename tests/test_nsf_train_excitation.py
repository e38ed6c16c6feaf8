"""The NSF excitation in training: csrc/nsf_train.hip (kantts_nsf_draw_states, kantts_nsf_source_wgrad), ops.nsf_excite,
SourceModule.enable_device_draws / Generator.enable_device_excitation, and the captured GAN step of an NSF generator
(kantts/train/gan_graph_step.py).

CPU leg: the kernel SOURCE on the host build (util.kernel_source_on_cpu).  GPU leg: the same checks on the device, plus the
captured step.  Inputs a call must not read hold NaN, outputs hold a sentinel, guard words sit around and between outputs.

Bounds.
* Draw: torch.equal with chunked_nsf.initial_state (the kernel forms the phases in fp64 and rounds once, as Python does).
* Weight gradient: against fp64 sums over the fp32 ``harm`` the forward produced,
  |dw_h - ref_h| <= (N + 8) * 2^-24 * sum |dpre * harm_h|, N = S * Tc * hop: the classical worst case of an fp32 sum of N
  terms in any order (N - 1 roundings) plus the roundings of a term (1 + e, the product with 1 - e, the product with de,
  the product with x_h, and one ulp in case x_h were re-associated: at most 8).  Two runs are torch.equal.
* Forward: max-abs <= 2e-5 against the module's formula in fp64, the project's fp32 single-layer bound.
* Module gradients: rel-L2 <= 2e-3 per tensor against conv_cl + tanh fed the same excitation, the bound of
  util.assert_grads_close for generator gradients.
* Captured step: the bounds of test_hifigan.test_graphed_gan_step_matches_eager_gpu."""
import ctypes
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import test_bench_config_parity as _bench_parity
from util import ROOT, kernel_source_on_cpu, rel_l2

SR, ALPHA, SIGMA = 16000, 0.1, 0.003
SENT, NAN, GUARD = -1234.5, float("nan"), 7
SEED = 0xC0FFEE1234567891  # >= 2^63: the device word holds it as a negative int64
_M64 = (1 << 64) - 1
_REPORT = os.path.join(os.path.dirname(_bench_parity._REPORT), "nsf_train_parity.json")  # beside chunked_nc_nsf_parity.json


def _record(key, val):
    try:
        os.makedirs(os.path.dirname(_REPORT), exist_ok=True)
        d = json.load(open(_REPORT)) if os.path.exists(_REPORT) else {}
        d[key] = val
        json.dump(d, open(_REPORT, "w"), indent=1)
    except OSError:
        pass


def _i64(v):
    v &= _M64
    return v - (1 << 64) if v >= (1 << 63) else v


def _words(device, seed, counter):
    return torch.tensor([_i64(seed), counter], dtype=torch.int64).to(device)


def _want_states(seed, counter, S, H1):
    from kantts.models.hifigan.chunked_nsf import initial_state

    return torch.stack([initial_state(seed, (counter << 20) | s, H1) for s in range(S)])


# ---------------------------------------------------------------------------------------------------------------------
# 1. the draw kernel
def _draw_call(device, words, S, H1):
    """One launch into a sentinel-filled buffer with guard words around it and two between items -> (S, 36) int32."""
    import kantts._hip as hip

    W = hip.NSF_STATE_WORDS
    ss = W + 2
    flat = torch.full((16 + S * ss + 16,), GUARD, dtype=torch.int32)
    arena = flat[16:16 + S * ss].view(S, ss)
    arena[:, :W] = -99
    flat = flat.to(device)
    arena = flat[16:16 + S * ss].view(S, ss)
    assert hip.nsf_draw_states(words, arena, S=S, H1=H1, state_ss=ss)
    assert bool((arena[:, W:] == GUARD).all()), "guard words between the items were written"
    assert bool((flat[:16] == GUARD).all()) and bool((flat[-16:] == GUARD).all()), "guard words around the states were written"
    return arena[:, :W].cpu().clone()


def _check_draw(device, H1):
    S = 3
    words = _words(device, SEED, 5)
    for c in (5, 6):
        got = _draw_call(device, words, S, H1)
        assert torch.equal(got, _want_states(SEED, c, S, H1)), (H1, c)
    assert words.cpu().tolist() == [_i64(SEED), 7]


def _check_draw_codes(device):
    import kantts._hip as hip

    L = hip.lib()
    W = hip.NSF_STATE_WORDS
    words = _words(device, SEED, 5)
    out = torch.full((4, W), -99, dtype=torch.int32).to(device)
    BAD, UNS = -1, hip.E_UNSUPPORTED

    def call(w=hip.ptr(words), S=3, H1=8, o=hip.ptr(out), ss=W):
        return L.kantts_nsf_draw_states(w, S, H1, o, ss, hip.stream())

    assert call(S=0) == UNS and call(S=-1) == UNS and call(S=1 << 20) == UNS and call(H1=17) == UNS
    assert call(w=None) == BAD and call(o=None) == BAD and call(H1=0) == BAD
    assert call(w=hip.ptr(words) + 4) == BAD and call(o=hip.ptr(out) + 4) == BAD
    assert call(ss=W + 1) == BAD and call(ss=W - 2) == BAD
    assert bool((out == -99).all()), "a refused call wrote states"
    assert words.cpu().tolist() == [_i64(SEED), 5], "a refused call moved the counter"
    assert call() == 0 and call(S=1, ss=0) == 0
    assert words.cpu().tolist() == [_i64(SEED), 7] and bool((out[3] == -99).all())
    assert hip.nsf_draw_states(words, out, S=3, H1=17) is False
    with pytest.raises(TypeError):
        hip.nsf_draw_states(words.int(), out, S=3, H1=8)


def test_nsf_train_layouts_match_the_header(tmp_path):
    """NsfWgradArgs against gcc's view of include/kantts_hip.h, and the argument kinds of both prototypes."""
    import kantts._hip as hip

    cls, cname = hip.NsfWgradArgs, "kantts_nsf_wgrad_args"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "kantts_hip.h"', 'int main(void) {',
             '  printf("sizeof %%zu\\n", sizeof(%s));' % cname]
    for fname, _ in cls._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(%s, %s));' % (fname, cname, fname))
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    c_layout = dict((ln.split()[0], int(ln.split()[1]))
                    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert ctypes.sizeof(cls) == c_layout["sizeof"]
    for fname, _ in cls._fields_:
        assert getattr(cls, fname).offset == c_layout[fname], fname
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kantts_hip.h")).read(), flags=re.S)
    draw = re.search(r"\bint\s+kantts_nsf_draw_states\s*\(([^;]*?)\)\s*;", header, flags=re.S).group(1)
    kinds = ["p" if "*" in p else "q" if "long long" in p else "i" for p in draw.split(",")]
    assert kinds == ["p", "i", "i", "p", "q", "p"]
    with kernel_source_on_cpu() as L:
        got = L.kantts_nsf_draw_states.argtypes
        assert [t is ctypes.c_void_p for t in got] == [k == "p" for k in kinds]
        assert got[1] is ctypes.c_int and got[2] is ctypes.c_int and got[4] is ctypes.c_longlong
        assert len(L.kantts_nsf_source_wgrad.argtypes) == 2 and hip.has_nsf_train()


@pytest.mark.parametrize("H1", [8, 7])
def test_nsf_draw_states_are_the_host_definition(H1):
    with kernel_source_on_cpu():
        _check_draw("cpu", H1)


def test_nsf_draw_states_return_codes():
    with kernel_source_on_cpu():
        _check_draw_codes("cpu")


# ---------------------------------------------------------------------------------------------------------------------
# 2. / 3. the forward on drawn states and the weight gradient
class _Inputs:
    """Seeded inputs of S utterances of T frames: f0 in 60..400 Hz, voiced frames, runs of uv = 0, one frame with uv = 0.5."""

    def __init__(self, S, T, hop, H1, seed=1):
        g = torch.Generator().manual_seed(seed)
        self.S, self.T, self.hop, self.H1 = S, T, hop, H1
        self.f0 = 60.0 + 340.0 * torch.rand(S, T, generator=g)
        self.uv = torch.ones(S, T)
        self.uv[0, 5:9] = 0.0
        self.uv[1, :3] = 0.0
        self.uv[S - 1, T - 4:] = 0.0
        self.uv[1, min(11, T - 2)] = 0.5
        self.noise = SIGMA * torch.randn(S, T * hop, H1, generator=g)
        self.w = torch.randn(H1, generator=g) * 0.6
        self.b = torch.randn(1, generator=g) * 0.1
        self.de = torch.randn(S, T * hop, generator=g)


def _drawn(device, S, H1, counter=9):
    """(S, 36) int32 states from the draw kernel, on the host."""
    import kantts._hip as hip

    out = torch.zeros(S, hip.NSF_STATE_WORDS, dtype=torch.int32).to(device)
    assert hip.nsf_draw_states(_words(device, SEED, counter), out, S=S, H1=H1)
    return out.cpu()


def _state_arena(device, state):
    import kantts._hip as hip

    S, W = state.shape[0], hip.NSF_STATE_WORDS
    arena = torch.full((2, S, W + 2), GUARD, dtype=torch.int32)
    arena[0, :, :W] = state
    arena[1, :, :W] = -99
    return arena.to(device)


def _forward(device, inp, state, given):
    """kantts_nsf_source_rows over the whole batch -> e (S, T * hop), harm (S, T * hop, H1), on the host."""
    import kantts._hip as hip

    S, T, hop, H1, W = inp.S, inp.T, inp.hop, inp.H1, hip.NSF_STATE_WORDS
    arena = _state_arena(device, state)
    n = S * T * hop
    flat = torch.full((n + 32,), float(GUARD)).to(device)
    e = flat[16:16 + n].view(S, T * hop)
    e.fill_(SENT)
    hm = torch.full((S, T * hop, H1), SENT).to(device)
    assert hip.nsf_source(inp.f0.to(device), inp.uv.to(device), arena[0, 0], arena[1, 0], inp.w.to(device), e, S=S, Tc=T,
                          hop=hop, H1=H1, sr=SR, alpha=ALPHA, sigma=SIGMA, state_ss=W + 2, bias=inp.b.to(device),
                          noise=inp.noise.to(device) if given else None, harm=hm)
    assert bool((arena[:, :, W:] == GUARD).all()) and torch.equal(arena[0, :, :W].cpu(), state)
    assert bool((flat[:16] == GUARD).all()) and bool((flat[-16:] == GUARD).all())
    return e.cpu().clone(), hm.cpu()


def _wgrad(device, inp, state, e, given):
    """One kantts_nsf_source_wgrad on fresh buffers -> dw (H1), dbias (1), on the host.  ws holds NaN (it must be written
    before it is read), dw / dbias a sentinel (they must be overwritten), guard cells sit around all three."""
    import kantts._hip as hip

    S, T, hop, H1, W = inp.S, inp.T, inp.hop, inp.H1, hip.NSF_STATE_WORDS
    arena = _state_arena(device, state)
    nws = S * T * (H1 + 1)
    out = torch.full((16 + H1 + 4 + 1 + 16,), float(GUARD))
    out[16:16 + H1] = SENT
    out[16 + H1 + 4] = SENT
    out = out.to(device)
    dw, db = out[16:16 + H1], out[16 + H1 + 4:16 + H1 + 5]
    wsf = torch.full((16 + nws + 16,), float(GUARD))
    wsf[16:16 + nws] = NAN
    wsf = wsf.to(device)
    assert hip.nsf_source_wgrad(inp.f0.to(device), inp.uv.to(device), arena[0, 0], e.to(device), inp.de.to(device), dw, db,
                                wsf[16:16 + nws], S=S, Tc=T, hop=hop, H1=H1, sr=SR, alpha=ALPHA, sigma=SIGMA, state_ss=W + 2,
                                noise=inp.noise.to(device) if given else None)
    assert bool((arena[:, :, W:] == GUARD).all()) and torch.equal(arena[0, :, :W].cpu(), state)
    assert bool((arena[1, :, :W] == -99).all()), "the weight gradient wrote a state"
    o = out.cpu()
    assert bool((o[:16] == GUARD).all()) and bool((o[16 + H1:16 + H1 + 4] == GUARD).all()) and bool((o[-16:] == GUARD).all())
    w = wsf.cpu()
    assert bool((w[:16] == GUARD).all()) and bool((w[-16:] == GUARD).all()) and not bool(torch.isnan(w).any())
    return o[16:16 + H1].clone(), o[16 + H1 + 4:16 + H1 + 5].clone()


_WGRAD_CASES = {"hop8_h8": (3, 24, 8, 8), "hop6_h8": (3, 24, 6, 8), "hop8_h7": (3, 24, 8, 7), "hop6_h7": (3, 24, 6, 7),
                "hop64_many_partials": (2, 40, 64, 8),
                # hop > 256 threads: a thread adds more than one sample into its LDS column (and 44 threads add one more)
                "hop300_strided": (2, 5, 300, 8)}


def _check_wgrad(device, name, given):
    S, T, hop, H1 = _WGRAD_CASES[name]
    inp = _Inputs(S, T, hop, H1)
    state = _drawn(device, S, H1)
    e, harm = _forward(device, inp, state, given)
    dw, db = _wgrad(device, inp, state, e, given)
    dpre = inp.de.double() * (1.0 - e.double() ** 2)
    terms = dpre[:, :, None] * harm.double()
    N = S * T * hop
    ref = torch.cat([terms.sum((0, 1)), dpre.sum().reshape(1)])
    scale = torch.cat([terms.abs().sum((0, 1)), dpre.abs().sum().reshape(1)])
    got = torch.cat([dw, db]).double()
    ratio = ((got - ref).abs() / ((N + 8) * 2.0 ** -24 * scale)).tolist()
    print("nsf wgrad", name, "given" if given else "generated", device, "err / bound per sum:", ["%.4f" % r for r in ratio])
    _record("wgrad/%s/%s/%s" % (name, "given" if given else "generated", device),
            {"max_err_over_bound": max(ratio), "max_abs_err": float((got - ref).abs().max()), "N": N})
    assert max(ratio) <= 1.0, (name, given, ratio)
    dw2, db2 = _wgrad(device, inp, state, e, given)
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "two runs on the same inputs differ"


def _formula64(inp, phase0):
    """e of the module's formula in fp64 with exact frame indexing: (S, T * hop)."""
    hop, H1 = inp.hop, inp.H1
    ps, us = inp.f0.double()[:, None, :].repeat_interleave(hop, -1), inp.uv.double()[:, None, :].repeat_interleave(hop, -1)
    harm = torch.arange(1, H1 + 1, dtype=torch.float64).view(1, -1, 1)
    theta = 2 * np.pi * (torch.cumsum(ps * harm / SR, dim=-1) % 1)
    noise = inp.noise.double().transpose(1, 2)
    x = (ALPHA * torch.sin(theta + phase0.double()[:, :, None]) + noise) * us + (ALPHA / 3 / SIGMA * noise) * (1 - us)
    return torch.tanh(inp.b.double() + (x * inp.w.double().view(1, -1, 1)).sum(1))


def _check_forward(device, hop):
    S, T, H1 = 3, 24, 8
    inp = _Inputs(S, T, hop, H1)
    state = _drawn(device, S, H1)
    phase0 = state[:, 16:16 + H1].contiguous().view(torch.float32)
    assert bool((phase0[:, 0] == 0).all()) and bool((phase0[:, 1:].abs() <= math.pi).all()) and phase0[:, 1:].unique().numel() > S
    e, _ = _forward(device, inp, state, given=True)
    err = float((e.double() - _formula64(inp, phase0)).abs().max())
    print("nsf forward on drawn states vs fp64 formula: hop", hop, device, "max-abs", err)
    _record("forward/hop%d/%s" % (hop, device), err)
    assert err <= 2e-5, err


def _check_wgrad_codes(device):
    import kantts._hip as hip

    L = hip.lib()
    W = hip.NSF_STATE_WORDS
    t = dict(f0=torch.full((2, 4), 100.0), uv=torch.ones(2, 4), st=torch.zeros(2, W, dtype=torch.int32), e=torch.zeros(2, 32),
             de=torch.ones(2, 32), dw=torch.full((16,), SENT), db=torch.full((1,), SENT), ws=torch.full((2 * 4 * 17,), SENT))
    t = {k: v.to(device) for k, v in t.items()}

    def call(**over):
        g = hip.NsfWgradArgs()
        g.f0, g.uv, g.state_in, g.e, g.de = (hip.ptr(t[k]) for k in ("f0", "uv", "st", "e", "de"))
        g.dw, g.dbias, g.ws, g.ws_floats, g.state_ss = hip.ptr(t["dw"]), hip.ptr(t["db"]), hip.ptr(t["ws"]), 2 * 4 * 9, W
        g.S, g.Tc, g.hop, g.H1, g.sr, g.alpha, g.sigma = 2, 4, 8, 8, SR, ALPHA, SIGMA
        for k, v in over.items():
            setattr(g, k, v)
        return L.kantts_nsf_source_wgrad(ctypes.byref(g), hip.stream())

    BAD, UNS = -1, hip.E_UNSUPPORTED
    assert L.kantts_nsf_source_wgrad(None, hip.stream()) == BAD
    for name in ("f0", "uv", "state_in", "e", "de", "dw", "ws"):
        assert call(**{name: None}) == BAD, name
    assert call(S=0) == BAD and call(Tc=0) == BAD and call(hop=0) == BAD and call(H1=0) == BAD and call(sr=0.0) == BAD
    assert call(sigma=0.0) == BAD and call(state_ss=W - 2) == BAD and call(ws_floats=2 * 4 * 9 - 1) == BAD
    assert call(H1=17) == UNS and call(state_ss=W + 1) == UNS and call(state_in=hip.ptr(t["st"]) + 4) == UNS
    for k in ("dw", "db", "ws"):
        assert bool((t[k] == SENT).all()), "a refused call wrote " + k
    assert call(dbias=None) == 0
    assert bool((t["db"] == SENT).all()) and not bool((t["dw"][:8] == SENT).any()) and bool((t["dw"][8:] == SENT).all())
    assert call() == 0 and not bool((t["db"] == SENT).any())
    assert bool((t["ws"][2 * 4 * 9:] == SENT).all()), "the workspace was written past S * Tc * (H1 + 1)"


_WGRAD_SMALL = sorted(n for n in _WGRAD_CASES if not n.startswith(("hop64", "hop300")))


@pytest.mark.parametrize("given", [True, False], ids=["given", "generated"])
@pytest.mark.parametrize("name", _WGRAD_SMALL)
def test_nsf_source_wgrad_matches_fp64_sums(name, given):
    with kernel_source_on_cpu():
        _check_wgrad("cpu", name, given)


def test_nsf_source_wgrad_many_partials():
    """80 partial sums per column: the second launch's strided walk."""
    with kernel_source_on_cpu():
        _check_wgrad("cpu", "hop64_many_partials", False)


@pytest.mark.parametrize("given", [True, False], ids=["given", "generated"])
def test_nsf_source_wgrad_hop_beyond_the_workgroup(given):
    with kernel_source_on_cpu():
        _check_wgrad("cpu", "hop300_strided", given)


def test_nsf_source_wgrad_return_codes():
    with kernel_source_on_cpu():
        _check_wgrad_codes("cpu")


@pytest.mark.parametrize("hop", [8, 6])
def test_nsf_forward_on_drawn_states_matches_the_fp64_formula(hop):
    with kernel_source_on_cpu():
        _check_forward("cpu", hop)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the module
def _device_harm(sm, pitch, uv, counter):
    """What the module's next forward with its counter at ``counter`` feeds its projection: (B, H + 1, T) through the two
    launches issued by hand with ``harm``; the counter is put back to ``counter``."""
    import kantts._hip as hip
    from kantts.models.hifigan.layers import conv_weight

    B, Tc, H1, hop = pitch.size(0), pitch.size(-1), sm.nb_harmonics + 1, int(sm.upsample_ratio)
    dev = pitch.device
    sm.set_draw_counter(counter)
    st = torch.zeros(2, B, hip.NSF_STATE_WORDS, dtype=torch.int32, device=dev)
    assert hip.nsf_draw_states(sm._draw_words, st[0], S=B, H1=H1)
    sm.set_draw_counter(counter)
    e = torch.empty(B, Tc * hop, device=dev)
    harm = torch.empty(B, Tc * hop, H1, device=dev)
    with torch.no_grad():
        w = conv_weight(sm.ffn[0])[0].reshape(-1).contiguous()  # the weight the module's own forward hands the kernel
    assert hip.nsf_source(pitch.reshape(B, Tc).contiguous(), uv.reshape(B, Tc).contiguous(), st[0], st[1], w, e, S=B, Tc=Tc,
                          hop=hop, H1=H1, sr=float(sm.sampling_rate), alpha=sm.alpha, sigma=sm.sigma,
                          bias=sm.ffn[0].bias.detach(), harm=harm)
    return harm.transpose(1, 2).contiguous(), e.unsqueeze(-1)


def _check_module(device, hop):
    from kantts.models.hifigan.layers import SourceModule

    torch.manual_seed(11)
    sm = SourceModule(7, hop, 16000).to(device)
    keys = list(sm.state_dict().keys())
    sm.enable_device_draws(SEED)
    assert list(sm.state_dict().keys()) == keys and sm.device_draws and sm.draw_counter() == 0
    g = torch.Generator().manual_seed(3)
    B, Tc = 2, 12
    pitch = (60.0 + 340.0 * torch.rand(B, 1, Tc, generator=g)).to(device)
    uv = (torch.rand(B, 1, Tc, generator=g) > 0.3).float().to(device)
    cot = torch.randn(B, Tc * hop, 1, generator=g).to(device)
    names = ["ffn.0.weight_g", "ffn.0.weight_v", "ffn.0.bias"]
    params = dict(sm.named_parameters())

    def grads(e):
        for n in names:
            params[n].grad = None
        (e * cot).sum().backward()
        return [params[n].grad.detach().cpu().clone() for n in names]

    harm, e_kernel = _device_harm(sm, pitch, uv, 3)
    e1 = sm.forward_cl(pitch, uv)
    assert tuple(e1.shape) == (B, Tc * hop, 1) and torch.equal(e1.detach(), e_kernel)
    got = grads(e1)
    e2 = sm.forward_cl(pitch, uv)
    assert sm.draw_counter() == 5 and not torch.equal(e1.detach(), e2.detach()), "two consecutive forwards must differ"
    sm.set_draw_counter(3)
    assert torch.equal(sm.forward_cl(pitch, uv).detach(), e1.detach()), "the same counter must give the same bits"
    # the stock composition fed the same excitation
    sm.disable_device_draws()
    assert not sm.device_draws and list(sm.state_dict().keys()) == keys
    orig = SourceModule.excitation
    SourceModule.excitation = lambda self, p, u: harm
    try:
        e_ref = sm.forward_cl(pitch, uv)
        want = grads(e_ref)
    finally:
        SourceModule.excitation = orig
    assert float((e1.detach() - e_ref.detach()).abs().max()) <= 2e-5
    for n, a, b in zip(names, got, want):
        r = rel_l2(a, b)
        print("nsf module gradient", n, "hop", hop, device, "rel-L2", r)
        _record("module_grad/hop%d/%s/%s" % (hop, n, device), r)
        assert r <= 2e-3, (n, r)


def _check_batch_sizes(device):
    """Batches of 2, 4, then 2 items through ONE module: every forward is the two launches on buffers of its own (nothing a
    larger batch regrows can be written by an earlier forward's launches or read by its backward), so each output is what
    the launches give by hand at that counter, and the FIRST batch's backward, run last, gives the gradients it gives when
    nothing runs in between."""
    from kantts.models.hifigan.layers import SourceModule

    torch.manual_seed(12)
    hop = 8
    sm = SourceModule(7, hop, 16000).to(device)
    sm.enable_device_draws(SEED)
    assert not hasattr(sm, "_draw_scratch"), "no state buffer may live on the module: a captured graph would keep its address"
    g = torch.Generator().manual_seed(4)
    names = ["ffn.0.weight_g", "ffn.0.weight_v", "ffn.0.bias"]
    params = dict(sm.named_parameters())

    def batch(B):
        pitch = (60.0 + 340.0 * torch.rand(B, 1, 10, generator=g)).to(device)
        uv = (torch.rand(B, 1, 10, generator=g) > 0.3).float().to(device)
        return pitch, uv, torch.randn(B, 10 * hop, 1, generator=g).to(device)

    def grads(e, cot):
        for n in names:
            params[n].grad = None
        (e * cot).sum().backward()
        return [params[n].grad.detach().cpu().clone() for n in names]

    batches = [batch(2), batch(4), batch(2)]
    want_e = []
    for c, (pitch, uv, _) in enumerate(batches):
        want_e.append(_device_harm(sm, pitch, uv, c)[1])
    sm.set_draw_counter(0)
    alone = grads(sm.forward_cl(*batches[0][:2]), batches[0][2])
    sm.set_draw_counter(0)
    outs = [sm.forward_cl(pitch, uv) for pitch, uv, _ in batches]
    assert sm.draw_counter() == 3
    for c, (e, w) in enumerate(zip(outs, want_e)):
        assert torch.equal(e.detach(), w), "batch %d of sizes 2, 4, 2" % c
    for n, a, b in zip(names, grads(outs[0], batches[0][2]), alone):
        assert torch.equal(a, b), n


def _check_statistics(device):
    """test_hifigan_nsf.test_source_module_excitation_statistics on the device-drawn harmonics."""
    from kantts.models.hifigan.layers import SourceModule

    sm = SourceModule(nb_harmonics=7, upsample_ratio=64, sampling_rate=16000).to(device)
    sm.enable_device_draws(0)
    pitch = torch.full((2, 1, 50), 200.0)
    uv = torch.zeros(2, 1, 50)
    uv[0] = 1.0
    pitch = pitch * uv
    e, _ = _device_harm(sm, pitch.to(device), uv.to(device), 0)
    e = e.cpu()
    assert tuple(e.shape) == (2, 8, 3200)
    assert abs(float(e[1].std()) - 0.1 / 3) < 2e-3
    assert abs(float(e[0, 0].pow(2).mean().sqrt()) - 0.1 / 2 ** 0.5) < 3e-3
    z = e[0, 0, :1600] - e[0, 0, 80:1680]
    assert float(z.abs().mean()) < 0.01


@pytest.mark.parametrize("hop", [8, 6])
def test_source_module_device_draws(hop):
    with kernel_source_on_cpu():
        _check_module("cpu", hop)


def test_source_module_device_draws_batch_sizes():
    with kernel_source_on_cpu():
        _check_batch_sizes("cpu")


def test_source_module_device_drawn_statistics():
    with kernel_source_on_cpu():
        _check_statistics("cpu")


def test_device_excitation_refusals_and_seeds():
    """Geometry outside the kernel is refused when device draws are ENABLED; replicas get different keys."""
    from kantts.models.hifigan.chunked_nsf import slot_key
    from kantts.models.hifigan.hifigan import Generator
    from kantts.models.hifigan.layers import SourceModule
    from kantts.train.gan_graph_step import excitation_seed

    with kernel_source_on_cpu():
        with pytest.raises(NotImplementedError):
            SourceModule(16, 8, 16000).enable_device_draws(0)
        G = Generator(channels=32, upsample_scales=[4, 2], upsample_kernal_sizes=[8, 4],
                      nsf_params={"nb_harmonics": 7, "sampling_rate": 16000})
        G.enable_device_excitation(1)
        assert G.source_module.device_draws
        G.disable_device_excitation()
        G.source_module.upsample_ratio = 16
        with pytest.raises(NotImplementedError):
            G.enable_device_excitation(1)
        assert not G.source_module.device_draws
        with pytest.raises(NotImplementedError):
            Generator(channels=32).enable_device_excitation(1)
    torch.manual_seed(77)
    s0, s1 = excitation_seed(0), excitation_seed(1)
    assert s0 != s1 and slot_key(s0, 0) != slot_key(s1, 0)
    assert not torch.equal(_want_states(s0, 0, 2, 8), _want_states(s1, 0, 2, 8))
    torch.manual_seed(77)
    assert excitation_seed(0) == s0


def test_emulated_abi_has_no_training_entry_points(emulated_cabi):
    """The numpy model of the C ABI does not have the entries: the probe says so and enabling refuses."""
    import kantts._hip as hip
    from kantts.models.hifigan.layers import SourceModule

    assert not hip.has_nsf_train()
    with pytest.raises(NotImplementedError):
        SourceModule(7, 8, 16000).enable_device_draws(0)


# ---------------------------------------------------------------------------------------------------------------------
# GPU leg
@pytest.mark.gpu
@pytest.mark.parametrize("H1", [8, 7])
def test_nsf_draw_states_are_the_host_definition_gpu(H1):
    _check_draw("cuda", H1)


@pytest.mark.gpu
def test_nsf_train_return_codes_gpu():
    _check_draw_codes("cuda")
    _check_wgrad_codes("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("given", [True, False], ids=["given", "generated"])
@pytest.mark.parametrize("name", _WGRAD_SMALL)
def test_nsf_source_wgrad_matches_fp64_sums_gpu(name, given):
    _check_wgrad("cuda", name, given)


@pytest.mark.gpu
def test_nsf_source_wgrad_many_partials_gpu():
    _check_wgrad("cuda", "hop64_many_partials", False)


@pytest.mark.gpu
@pytest.mark.parametrize("given", [True, False], ids=["given", "generated"])
def test_nsf_source_wgrad_hop_beyond_the_workgroup_gpu(given):
    _check_wgrad("cuda", "hop300_strided", given)


@pytest.mark.gpu
@pytest.mark.parametrize("hop", [8, 6])
def test_nsf_forward_on_drawn_states_matches_the_fp64_formula_gpu(hop):
    _check_forward("cuda", hop)


@pytest.mark.gpu
@pytest.mark.parametrize("hop", [8, 6])
def test_source_module_device_draws_gpu(hop):
    import kantts._hip as hip

    hip.set_precision("fp32")
    _check_module("cuda", hop)


@pytest.mark.gpu
def test_source_module_device_drawn_statistics_gpu():
    _check_statistics("cuda")


@pytest.mark.gpu
def test_source_module_device_draws_batch_sizes_gpu():
    """_check_batch_sizes, and a forward captured at batch 2 that is replayed after a larger batch ran on the module."""
    import kantts._hip as hip
    from kantts.models.hifigan.layers import SourceModule

    hip.set_precision("fp32")
    _check_batch_sizes("cuda")
    torch.manual_seed(13)
    sm = SourceModule(7, 8, 16000).cuda()
    sm.enable_device_draws(SEED)
    g = torch.Generator().manual_seed(6)
    p2, u2 = (60.0 + 340.0 * torch.rand(2, 1, 10, generator=g)).cuda(), torch.ones(2, 1, 10).cuda()
    p4, u4 = (60.0 + 340.0 * torch.rand(4, 1, 10, generator=g)).cuda(), torch.ones(4, 1, 10).cuda()
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            sm.forward_cl(p2, u2)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            out = sm.forward_cl(p2, u2)
        sm.set_draw_counter(7)
        want = sm.forward_cl(p2, u2).clone()
        big = sm.forward_cl(p4, u4)
        held = [torch.full((4, hip.NSF_STATE_WORDS), -99, dtype=torch.int32, device="cuda") for _ in range(64)]
        sm.set_draw_counter(7)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want) and sm.draw_counter() == 8
        assert all(bool((t == -99).all()) for t in held), "the replay wrote into memory allocated after a larger batch"
        assert bool(torch.isfinite(big).all())


@pytest.mark.gpu
def test_graphed_nsf_gan_step_failure_restores_host_draws_gpu(monkeypatch):
    """A construction that ends without a graph leaves a source module IT switched on host-seeded draws again (the eager
    fallback of the trainer is then the step it ran before); a caller's own enable_device_excitation stays."""
    import kantts._hip as hip
    from kantts.train.gan_graph_step import CaptureRefused, GraphedGanStep

    hip.set_precision("fp32")
    config, model, optimizer, scheduler, crit = _small_nsf_gan_setup()
    x = torch.randn(2, 82, 16).cuda()
    x[:, -1] = 1.0
    x[:, -2] = 200.0
    y = torch.randn(2, 1, 4096).clamp(-1, 1).cuda()

    def refuse(self, warmup):
        raise CaptureRefused("refused for the test")

    monkeypatch.setattr(GraphedGanStep, "_build", refuse)
    sm = model["generator"].source_module
    with pytest.raises(NotImplementedError):
        GraphedGanStep(model, optimizer, scheduler, crit, config, y, x, steps=1)
    assert not sm.device_draws
    model["generator"].enable_device_excitation(3)
    with pytest.raises(NotImplementedError):
        GraphedGanStep(model, optimizer, scheduler, crit, config, y, x, steps=1)
    assert sm.device_draws and sm.draw_counter() == 0


def _small_nsf_gan_setup(seed=0):
    """_small_gan_setup of test_hifigan.py with an NSF generator."""
    from kantts.models import model_builder
    from kantts.train.loss import criterion_builder

    opt = {"type": "Adam", "params": {"lr": 2e-4, "betas": [0.5, 0.9], "weight_decay": 0.0}}
    sch = {"type": "MultiStepLR", "params": {"gamma": 0.5, "milestones": [2]}}  # the lr halves after the second step
    config = {"model_type": "hifigan", "Model": {
        "Generator": {"params": {"channels": 64, "nsf_params": {"nb_harmonics": 7, "sampling_rate": 16000}},
                      "optimizer": opt, "scheduler": sch},
        "MultiScaleDiscriminator": {"params": {}, "optimizer": opt, "scheduler": sch},
        "MultiPeriodDiscriminator": {"params": {}, "optimizer": opt, "scheduler": sch}},
        "Loss": {"generator_adv_loss": {"enable": True, "params": {}, "weights": 1.0},
                 "discriminator_adv_loss": {"enable": True, "params": {}, "weights": 1.0},
                 "stft_loss": {"enable": False},
                 "mel_loss": {"enable": True, "params": {}, "weights": 45.0},
                 "feat_match_loss": {"enable": True, "params": {}, "weights": 2.0}},
        "generator_grad_norm": -1, "discriminator_grad_norm": -1, "discriminator_train_start_steps": 0,
        "generator_train_start_steps": 0}
    torch.manual_seed(seed)
    model, optimizer, scheduler = model_builder(config, device="cuda")
    crit = criterion_builder(config, device="cuda")
    return config, model, optimizer, scheduler, crit


@pytest.mark.gpu
@pytest.mark.parametrize("prec,tol", [("fp32", 2e-4), ("bf16", 2e-3)])
def test_graphed_nsf_gan_step_matches_eager_gpu(prec, tol, monkeypatch):
    """The captured GAN step of an NSF generator against the eager step with the same device-drawn excitation (seed K, counter
    0) over four steps: same losses, same weights; the warm-up consumes no draws, a step draws twice."""
    import kantts._hip as hip
    from kantts._hip import ops
    from kantts.train.gan_graph_step import GraphedGanStep
    from kantts.train.gan_step import gan_train_step

    K = 4242
    hip.set_precision(prec)
    old_thr = ops.CCONV_MIN_FLOPS
    ops.CCONV_MIN_FLOPS = 0.0
    try:
        g = torch.Generator().manual_seed(5)
        xs = []
        for _ in range(4):
            x = torch.randn(2, 82, 16, generator=g)
            x[:, -1] = (torch.rand(2, 16, generator=g) > 0.25).float()
            x[:, -1, 3:6] = 0.0
            x[:, -2] = (60.0 + 340.0 * torch.rand(2, 16, generator=g)) * x[:, -1]
            xs.append(x.cuda())
        ys = [torch.randn(2, 1, 4096, generator=g).clamp(-1, 1).cuda() for _ in range(4)]
        config, model, optimizer, scheduler, crit = _small_nsf_gan_setup()
        model["generator"].enable_device_excitation(K)
        eager_losses = []
        for x, y in zip(xs, ys):
            out = gan_train_step(model, optimizer, scheduler, crit, config, y, x, steps=1)
            eager_losses.append({k: float(v.detach()) for k, v in out.items()})
        assert model["generator"].source_module.draw_counter() == 8
        eager_w = [optimizer["generator"].arena.flat.clone()] + [o.arena.flat.clone() for o in optimizer["discriminator"].values()]
        eager_lr = optimizer["generator"].param_groups[0]["lr"]

        config, model, optimizer, scheduler, crit = _small_nsf_gan_setup()
        model["generator"].enable_device_excitation(K)
        step = GraphedGanStep(model, optimizer, scheduler, crit, config, ys[0], xs[0], steps=1)
        assert model["generator"].source_module.draw_counter() == 0, "warm-up and capture must not consume draws"
        for i, (x, y) in enumerate(zip(xs, ys)):
            step.load_batch(y, x)
            out = step()
            got = {k: float(v.detach()) for k, v in out.items()}
            for k, v in eager_losses[i].items():
                print("nsf captured step", prec, i, k, got[k], v)
                assert abs(got[k] - v) <= tol * max(1.0, abs(v)), (prec, i, k, got[k], v)
        graph_w = [optimizer["generator"].arena.flat] + [o.arena.flat for o in optimizer["discriminator"].values()]
        assert optimizer["generator"].param_groups[0]["lr"] == eager_lr
        assert optimizer["generator"]._step == 4
        for a, b in zip(graph_w, eager_w):
            print("nsf captured step", prec, "arena rel-L2", rel_l2(a, b))
            assert rel_l2(a, b) <= tol, prec
        assert model["generator"].source_module.draw_counter() == 8
        monkeypatch.setattr(hip, "has_nsf_train", lambda: False)
        with pytest.raises(NotImplementedError):
            GraphedGanStep(model, optimizer, scheduler, crit, config, ys[0], xs[0], steps=1)
    finally:
        ops.CCONV_MIN_FLOPS = old_thr
        hip.set_precision("fp32")
