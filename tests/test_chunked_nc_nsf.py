"""Chunked inference of NON-CAUSAL NSF generators: csrc/nsf_source_sym.hip (kantts_nsf_source_end_rows,
kantts_nsf_downs_sym_rows), kantts.models.hifigan.chunked_nc_nsf.ChunkedNCNSFVocoder, and its callers (infer_hifigan
--chunk_frames, StreamingTTS(lookahead=True, nsf=...)).

CPU leg: the kernel SOURCE on the host build (util.kernel_source_on_cpu), graph=False.  GPU leg: the same checks on the
device, graph both on and off.  Inputs a call must not read hold NaN; outputs and the state half to be written hold a sentinel
and have guard cells around them.

Bounds.  The down-convolutions against torch.nn.functional.conv1d in fp64: max-abs <= 2e-5, the project's fp32 single-layer
bound.  Whole generator, fp32: mean-abs <= 1e-5 against Generator.forward of the whole utterance, the bound of the other
chunked-vocoder tests for this comparison; bf16: the chunked output errs against the fp32 one-shot output at most twice what
the bf16 one-shot output does, both measured in the same run (the rule of test_chunked_noncausal_generator_bf16_gpu).
Wherever two plays run the same arithmetic the assertion is torch.equal."""
import ctypes
import itertools
import json
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

import test_chunked_acoustic as _ca
import test_chunked_noncausal as NC
import test_chunked_nsf as N
from util import ROOT, assert_close, kernel_source_on_cpu

S, H1, SR, ALPHA, SIGMA = N.S, N.H1, N.SR, N.ALPHA, N.SIGMA
SENT, NAN, GUARD = N.SENT, N.NAN, N.GUARD
LENS = [24, 17, 3]  # frames per slot
FLUSH = 4           # frames every slot of the source test keeps stepping behind its last one
_REPORT = os.path.join(os.path.dirname(NC._REPORT), "chunked_nc_nsf_parity.json")


def _record(key, val):
    try:
        os.makedirs(os.path.dirname(_REPORT), exist_ok=True)
        d = json.load(open(_REPORT)) if os.path.exists(_REPORT) else {}
        d[key] = val
        json.dump(d, open(_REPORT, "w"), indent=1)
    except OSError:
        pass


def _pos_buffer(device, pos):
    """Per-slot positions the way the vocoder's arena holds them: one word per slot, 3 words apart, guard words between."""
    buf = torch.full((len(pos), 3), 77, dtype=torch.int32)
    buf[:, 0] = torch.tensor(pos, dtype=torch.int32)
    return buf.to(device)


def _i32(device, vals):
    return None if vals is None else torch.tensor(vals, dtype=torch.int32).to(device)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the source with an end
def _source_end_call(device, inp, state, f0, uv, noise, rows, end, pos):
    """One launch of kantts_nsf_source_end_rows on fresh buffers -> e (S, Tc * hop), state_out, harm."""
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
    hm = torch.full((nS, Tc * hop, H1), SENT).to(device)
    pb = _pos_buffer(device, pos)
    ok = hip.nsf_source_end(f0.contiguous().to(device), uv.contiguous().to(device), arena[0, 0], arena[1, 0], inp.w.to(device), e,
                            S=nS, Tc=Tc, hop=hop, H1=H1, sr=SR, alpha=ALPHA, sigma=SIGMA, state_ss=ss, bias=inp.b.to(device),
                            noise=None if noise is None else noise.contiguous().to(device), harm=hm, rows=_i32(device, rows),
                            end=_i32(device, end), pos_in=pb, pos_ss=3)
    assert ok
    assert bool((arena[:, :, W:] == GUARD).all()), "guard words behind a slot's state were written"
    assert torch.equal(arena[0, :, :W].cpu(), state), "state_in was written"
    assert bool((flat[:16] == GUARD).all()) and bool((flat[-16:] == GUARD).all()), "guard cells around e were written"
    assert torch.equal(pb.cpu(), _pos_buffer("cpu", pos)), "pos_in was written"
    return e.cpu().clone(), arena[1, :, :W].cpu().clone(), hm.cpu()


def _check_source_end(device, hop, sched, given, late_end):
    inp = N._Inputs(hop)
    st0 = inp.states(given)
    # the yardstick: ONE whole-utterance call of the existing entry point on the live frames
    want_e, want_st, want_h = N._source_call(device, inp, st0, inp.f0, inp.uv, noise=inp.noise if given else None, rows=LENS,
                                             harm=True)
    total = [T + FLUSH for T in LENS]
    pos, state = [0] * S, st0
    es, hs = [[] for _ in range(S)], [[] for _ in range(S)]
    sizes = itertools.cycle(NC._SCHEDULES[sched])
    while any(p < n for p, n in zip(pos, total)):
        Tc = next(sizes)
        counts = [min(Tc, n - p) for p, n in zip(pos, total)]
        f0, uv, nz = torch.full((S, Tc), NAN), torch.full((S, Tc), NAN), torch.full((S, Tc * hop, H1), NAN)
        live, end = [], []
        for s in range(S):
            l = max(0, min(counts[s], LENS[s] - pos[s]))
            f0[s, :l], uv[s, :l] = inp.f0[s, pos[s]:pos[s] + l], inp.uv[s, pos[s]:pos[s] + l]
            nz[s, :l * hop] = inp.noise[s, pos[s] * hop:(pos[s] + l) * hop]
            live.append(l)
            end.append(-1 if late_end and pos[s] + counts[s] <= LENS[s] else LENS[s])
        e, state2, hm = _source_end_call(device, inp, state, f0, uv, nz if given else None, counts, end, pos)
        for s, l in enumerate(live):
            what = (hop, sched, given, late_end, "slot", s, "pos", pos[s])
            assert bool((e[s, l * hop:] == SENT).all()) and bool((hm[s, l * hop:] == SENT).all()), ("written behind l * hop", what)
            if l == 0:
                assert torch.equal(state2[s], state[s]), ("a slot without live frames must keep its state", what)
            es[s].append(e[s, :l * hop])
            hs[s].append(hm[s, :l * hop])
            pos[s] += counts[s]
        state = state2
    for s, T in enumerate(LENS):
        e, h = torch.cat(es[s]), torch.cat(hs[s])
        assert not bool(torch.isnan(e).any()) and not bool(torch.isnan(h).any())
        assert torch.equal(e, want_e[s, :T * hop]), ("e", hop, sched, given, late_end, s)
        assert torch.equal(h, want_h[s, :T * hop]), ("harm", hop, sched, given, late_end, s)
    assert torch.equal(state, want_st), ("final state", hop, sched, given, late_end)
    cur = state[:, 32:34].contiguous().view(torch.int64).reshape(-1)
    assert cur.tolist() == [T * hop for T in LENS], "the cursor must stop at the utterance's end"


def _check_source_end_all(device):
    for hop in (8, 6):
        for sched in NC._SCHEDULES:
            _check_source_end(device, hop, sched, given=sched != "ones", late_end=sched == "mixed")
        _check_source_end(device, hop, "ones", given=True, late_end=True)


# ---------------------------------------------------------------------------------------------------------------------
# 2.-4. the symmetric down-convolutions
# (hop, strides, channels, made-up up-layer delays D_i).  Every case has D_i = 1 for a stage with u > 1 (lag = u + u / 2, the
# smallest a delayed up-layer can give; D = 0 would read the future), lags longer than a one-frame chunk, and lags longer
# than the 3-frame utterance of slot 2.
_SYM_CASES = {
    "hop8": (8, (2, 1), (16, 8), (1, 31)),               # lags 3, 31
    "hop10": (10, (2, 1), (12, 16), (1, 37)),            # lags 3, 37
    "hop200": (200, (20, 4, 2, 1), (16, 8, 8, 4), (1, 60, 450, 1000)),  # lags 30, 242, 901, 1000
}


class _DownsSym(N._Downs):
    """The weights of test_chunked_nsf._Downs read symmetrically: Conv1d(1, C, 2 u, u, padding=u // 2), D_i rows late."""

    def __init__(self, hop, us, Cs, Ds, seed=2):
        super().__init__(hop, us, Cs, seed=seed)
        self.Ds = Ds
        self.ps = [u // 2 if u > 1 else 0 for u in us]
        self.lags = [D * u + p for D, u, p in zip(Ds, us, self.ps)]
        self.Hh = max(self.lags)

    def torch64(self, e):
        """e (n,) of a whole utterance -> [d_i (n / u_i, C_i)] by conv1d in fp64, zero-padded at both ends."""
        x = e.double()[None, None, :]
        return [F.conv1d(x, W.double(), B.double(), stride=u, padding=p)[0].t()
                for u, p, W, B in zip(self.us, self.ps, self.W, self.B)]

    def call(self, device, e, hist, rows=None, end=None, pos=None, lags=None, Hh=None):
        """e (S, Tc * hop), hist (S, Hh) -> [d_i], hist_out."""
        import kantts._hip as hip

        lags = self.lags if lags is None else lags
        Hh = self.Hh if Hh is None else Hh
        nS, n = e.shape
        Tc = n // self.hop
        ss = Hh + 3
        arena = torch.full((2, nS, ss), float(GUARD))
        arena[0, :, :Hh] = hist
        arena[1, :, :Hh] = SENT
        arena = arena.to(device)
        flats, outs = [], []
        for u, C in zip(self.us, self.Cs):
            m = nS * (n // u) * C
            fl = torch.full((m + 32,), float(GUARD)).to(device)
            o = fl[16:16 + m].view(nS, n // u, C)
            o.fill_(SENT)
            flats.append(fl)
            outs.append(o)
        pb = None if pos is None else _pos_buffer(device, pos)
        e_dev = e.contiguous().to(device)
        ok = hip.nsf_downs_sym(e_dev, arena[0, 0], arena[1, 0], self.stages(device), lags, outs, S=nS, Tc=Tc, hop=self.hop,
                               hist_rows=Hh, hist_ss=ss, rows=_i32(device, rows), end=_i32(device, end), pos_in=pb, pos_ss=3)
        assert ok
        assert bool((arena[:, :, Hh:] == GUARD).all()), "guard floats behind a slot's history were written"
        assert torch.equal(arena[0, :, :Hh].cpu(), hist), "hist_in was written"
        assert torch.equal(e_dev.cpu().view(torch.int32), e.contiguous().view(torch.int32)), "e was written"
        for fl in flats:
            assert bool((fl[:16] == GUARD).all()) and bool((fl[-16:] == GUARD).all()), "guard cells around an output were written"
        return [o.cpu().clone() for o in outs], arena[1, :, :Hh].cpu().clone()


def _utterance_e(hop, seed=4):
    return torch.rand(S, max(LENS) * hop, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _play_downs(device, D, e_true, sizes, late_end=False, hold=False):
    """S utterances of LENS frames through the launch, each slot for LENS[s] + flush frames: the stream of every stage
    (S lists of rows) and the final history.  ``hold``: every third step one slot in turn gets rows = 0."""
    hop = D.hop
    flush = max(-(-lag // hop) for lag in D.lags) + 1
    total = [T + flush for T in LENS]
    pos, hist = [0] * S, torch.zeros(S, D.Hh)
    ds = [[[] for _ in D.us] for _ in range(S)]
    sizes = itertools.cycle(sizes)
    step = 0
    while any(p < n for p, n in zip(pos, total)):
        step += 1
        assert step < 2000
        Tc = next(sizes)
        counts = [min(Tc, n - p) for p, n in zip(pos, total)]
        if hold and step % 3 == 0:
            counts[(step // 3) % S] = 0
        e = torch.full((S, Tc * hop), NAN)  # dead frames and flush frames must not be loaded
        end = []
        for s in range(S):
            live = max(0, min(counts[s], LENS[s] - pos[s]))
            e[s, :live * hop] = e_true[s, pos[s] * hop:(pos[s] + live) * hop]
            end.append(-1 if late_end and pos[s] + counts[s] <= LENS[s] else LENS[s])
        outs, hist2 = D.call(device, e, hist, rows=counts, end=end, pos=pos)
        for s, c in enumerate(counts):
            if c == 0:
                assert torch.equal(hist2[s], hist[s]), "a held slot's history changed"
            for i, u in enumerate(D.us):
                assert bool((outs[i][s, c * hop // u:] == SENT).all()), ("dead rows were written", i, s)
                ds[s][i].append(outs[i][s, :c * hop // u])
            pos[s] += c
        hist = hist2
    streams = [[torch.cat(ds[s][i]) for i in range(len(D.us))] for s in range(S)]
    for s in range(S):
        for x in streams[s]:
            assert not bool(torch.isnan(x).any()), "a flush or a dead sample was read"
    return streams, hist


def _check_downs_sym(device, name):
    hop, us, Cs, Ds = _SYM_CASES[name]
    D = _DownsSym(hop, us, Cs, Ds)
    assert any(d == 1 and u > 1 for d, u in zip(Ds, us))
    assert max(D.lags) > hop and max(D.lags) > LENS[2] * hop
    e_true = _utterance_e(hop)
    want = None
    for sched, kw in (("eights", {}), ("ones", dict(late_end=True)), ("mixed", {}), ("mixed", dict(hold=True, late_end=True))):
        streams, hist = _play_downs(device, D, e_true, NC._SCHEDULES[sched], **kw)
        if want is None:
            want = (streams, hist)
            for s, T in enumerate(LENS):  # against torch on the whole utterance, shifted by D_i
                for i, (ref, u, d) in enumerate(zip(D.torch64(e_true[s, :T * hop]), us, Ds)):
                    assert ref.shape[0] == T * hop // u
                    got = streams[s][i][d:d + ref.shape[0]]
                    err = float((got.double() - ref).abs().max())
                    print("nsf downs sym", name, "slot", s, "stage", i, "max-abs", err)
                    assert_close(got.double(), ref, 2e-5, what="%s stage %d slot %d" % (name, i, s))
            continue
        for s in range(S):  # cut invariance: every row of the stream, inside the utterance or not, and the history
            for i in range(len(us)):
                assert torch.equal(streams[s][i], want[0][s][i]), ("rows", name, sched, kw, s, i)
        assert torch.equal(hist, want[1]), ("history", name, sched, kw)


def _check_downs_causal_bits(device):
    """lag = k - 1, end == NULL, Hh = max(k - 1): the bits of kantts_nsf_downs_rows."""
    for name, (hop, us, Cs) in N._DOWN_CASES.items():
        C, T = N._Downs(hop, us, Cs), 10
        Y = _DownsSym(hop, us, Cs, [0] * len(us))
        e = torch.rand(S, T * hop, generator=torch.Generator().manual_seed(4)) * 2 - 1
        h0 = torch.randn(S, C.Hh, generator=torch.Generator().manual_seed(6))
        for rows in (None, [3, 0, T]):
            a, ha = C.call(device, e, h0, rows=rows)
            b, hb = Y.call(device, e, h0, rows=rows, lags=[k - 1 for k in C.ks], Hh=C.Hh)
            assert torch.equal(ha, hb), (name, rows)
            for x, y in zip(a, b):
                assert torch.equal(x, y), (name, rows)


# ---------------------------------------------------------------------------------------------------------------------
# 5. return codes and struct layouts
def _check_codes(device):
    import kantts._hip as hip

    L = hip.lib()
    W = hip.NSF_STATE_WORDS
    assert hip.nsf_sym_entry_points()
    bufs = dict(f0=torch.full((2, 4), 100.0), uv=torch.ones(2, 4), w=torch.ones(16), st=torch.zeros(2, 2, W, dtype=torch.int32),
                e=torch.full((2, 32), SENT), hist=torch.zeros(2, 2, 8), w0=torch.ones(4, 3), w1=torch.ones(1, 3),
                o0=torch.full((2, 16, 3), SENT), o1=torch.full((2, 32, 3), SENT),
                end=torch.full((2,), -1, dtype=torch.int32), pos=torch.zeros(2, dtype=torch.int32))
    bufs = {k: v.to(device) for k, v in bufs.items()}
    st = bufs["st"]
    st[1] = -99
    bufs["hist"][1] = SENT

    def source(**over):
        g = hip.NsfSourceEndArgs()
        g.src.f0, g.src.uv, g.src.w, g.src.e = (hip.ptr(bufs[k]) for k in ("f0", "uv", "w", "e"))
        g.src.state_in, g.src.state_out, g.src.state_ss = hip.ptr(st[0]), hip.ptr(st[1]), W
        g.src.S, g.src.Tc, g.src.hop, g.src.H1, g.src.sr, g.src.alpha, g.src.sigma = 2, 4, 8, 8, SR, ALPHA, SIGMA
        g.end, g.pos_in, g.pos_ss = hip.ptr(bufs["end"]), hip.ptr(bufs["pos"]), 1
        for k, v in over.items():
            setattr(g if k in ("end", "pos_in", "pos_ss") else g.src, k, v)
        return L.kantts_nsf_source_end_rows(ctypes.byref(g), hip.stream())

    def downs(**over):
        g = hip.NsfDownsSymArgs()
        d = g.d
        d.e, d.hist_in, d.hist_out, d.hist_ss = hip.ptr(bufs["e"]), hip.ptr(bufs["hist"][0]), hip.ptr(bufs["hist"][1]), 8
        d.S, d.Tc, d.hop, d.nstages = 2, 4, 8, 2
        d.u[0], d.k[0], d.C[0], d.w[0], d.out[0] = 2, 4, 3, hip.ptr(bufs["w0"]), hip.ptr(bufs["o0"])
        d.u[1], d.k[1], d.C[1], d.w[1], d.out[1] = 1, 1, 3, hip.ptr(bufs["w1"]), hip.ptr(bufs["o1"])
        g.end, g.pos_in, g.pos_ss, g.Hh = hip.ptr(bufs["end"]), hip.ptr(bufs["pos"]), 1, 7
        g.lag[0], g.lag[1] = 7, 5
        for k, v in over.items():
            tgt = g if k in ("end", "pos_in", "pos_ss", "Hh", "lag") else d
            if isinstance(v, tuple):
                getattr(tgt, k)[v[0]] = v[1]
            else:
                setattr(tgt, k, v)
        return L.kantts_nsf_downs_sym_rows(ctypes.byref(g), hip.stream())

    BAD, UNS = -1, hip.E_UNSUPPORTED
    assert L.kantts_nsf_source_end_rows(None, hip.stream()) == BAD and L.kantts_nsf_downs_sym_rows(None, hip.stream()) == BAD
    # the source: what the new arguments add, then everything kantts_nsf_source_rows answers for `src`
    assert source(pos_in=None) == BAD and source(pos_ss=-1) == BAD
    for name in ("f0", "uv", "w", "state_in", "state_out", "e"):
        assert source(**{name: None}) == BAD, name
    assert source(Tc=0) == BAD and source(hop=0) == BAD and source(H1=0) == BAD and source(sr=0.0) == BAD
    assert source(sigma=0.0) == BAD and source(state_out=hip.ptr(st[0])) == BAD and source(state_ss=W - 2) == BAD
    assert source(H1=17) == UNS and source(state_ss=W + 1) == UNS
    # the down-convolutions
    assert downs(pos_in=None) == BAD and downs(pos_ss=-1) == BAD and downs(Hh=-1) == BAD
    assert downs(lag=(0, 1)) == BAD, "lag < k - u reads the future"
    assert downs(lag=(1, -1)) == BAD and downs(lag=(0, 8)) == BAD, "a lag beyond the history"
    assert downs(e=None) == BAD and downs(Tc=0) == BAD and downs(nstages=0) == BAD and downs(hop=0) == BAD
    assert downs(w=(1, None)) == BAD and downs(out=(0, None)) == BAD and downs(C=(0, 0)) == BAD and downs(u=(1, 0)) == BAD
    assert downs(hist_in=None) == BAD and downs(hist_out=hip.ptr(bufs["hist"][0])) == BAD and downs(hist_ss=6) == BAD
    assert downs(nstages=9) == UNS and downs(u=(0, 3)) == UNS and downs(k=(0, 8193)) == UNS
    assert bool((bufs["e"] == SENT).all()) and bool((bufs["o0"] == SENT).all()) and bool((bufs["o1"] == SENT).all())
    assert bool((st[1] == -99).all()) and bool((bufs["hist"][1] == SENT).all()), "a refused call wrote its state"
    # the case as it stands, the smallest legal lags (k - u), and the forms without an end / without a position
    assert source() == 0 and downs() == 0 and downs(lag=(0, 2)) == 0 and downs(lag=(1, 0)) == 0
    assert source(end=None, pos_in=None) == 0 and downs(end=None, pos_in=None) == 0
    assert not bool((bufs["o0"] == SENT).any()) and not bool((bufs["o1"] == SENT).any())
    assert not bool(bufs["hist"][0].any()) and bool((bufs["end"] == -1).all()) and not bool(bufs["pos"].any())
    # the wrappers: declined shapes are False, bad arguments raise
    kw = dict(S=2, Tc=4, hop=8, sr=SR, alpha=ALPHA, sigma=SIGMA)
    assert hip.nsf_source_end(bufs["f0"], bufs["uv"], st[0], st[1], torch.ones(17).to(device), bufs["e"], H1=17, **kw) is False
    with pytest.raises(RuntimeError):
        hip.nsf_source_end(bufs["f0"], bufs["uv"], st[0], st[1], bufs["w"], bufs["e"], H1=8, end=bufs["end"], **kw)  # no pos_in
    with pytest.raises(ValueError):
        hip.nsf_source_end(bufs["f0"], bufs["uv"], st[0], st[1], bufs["w"], bufs["e"], H1=8, pos_in=bufs["pos"],
                           end=torch.zeros(3, dtype=torch.int32).to(device), **kw)
    one = [(1, 1, 3, bufs["w1"], None)]
    dkw = dict(S=2, Tc=4, hop=8, hist_rows=7, hist_ss=8)
    assert hip.nsf_downs_sym(bufs["e"], bufs["hist"][0], bufs["hist"][1], one * 9, [0] * 9, [bufs["o1"]] * 9, **dkw) is False
    with pytest.raises(RuntimeError):
        hip.nsf_downs_sym(bufs["e"], bufs["hist"][0], bufs["hist"][1], one, [-1], [bufs["o1"]], **dkw)
    with pytest.raises(ValueError):
        hip.nsf_downs_sym(bufs["e"], bufs["hist"][0], bufs["hist"][1], one, [0, 0], [bufs["o1"]], **dkw)


def test_nc_nsf_struct_layouts_match_the_header(tmp_path):
    """NsfSourceEndArgs / NsfDownsSymArgs against gcc's view of include/kantts_hip.h."""
    import kantts._hip as hip

    pairs = [(hip.NsfSourceEndArgs, "kantts_nsf_source_end_args"), (hip.NsfDownsSymArgs, "kantts_nsf_downs_sym_args")]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "kantts_hip.h"', 'int main(void) {']
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
    for cls, cname in pairs:
        assert ctypes.sizeof(cls) == c_layout[(cname, "sizeof")], cname
        for fname, _ in cls._fields_:
            assert getattr(cls, fname).offset == c_layout[(cname, fname)], (cname, fname)
    assert hip.NsfSourceEndArgs.src.size == ctypes.sizeof(hip.NsfSourceArgs)
    assert hip.NsfDownsSymArgs.d.size == ctypes.sizeof(hip.NsfDownsArgs)


def test_nsf_source_with_an_end():
    with kernel_source_on_cpu():
        _check_source_end_all("cpu")


@pytest.mark.parametrize("name", sorted(_SYM_CASES))
def test_nsf_downs_sym_match_torch_whatever_the_cuts(name):
    with kernel_source_on_cpu():
        _check_downs_sym("cpu", name)


def test_nsf_downs_sym_with_the_causal_lag_is_the_causal_entry():
    with kernel_source_on_cpu():
        _check_downs_causal_bits("cpu")


def test_nc_nsf_return_codes():
    with kernel_source_on_cpu():
        _check_codes("cpu")


# ---------------------------------------------------------------------------------------------------------------------
# model level
_NSF16 = {"nb_harmonics": 7, "sampling_rate": 16000}
_GEN = {name: dict(in_channels=80, nsf_params=_NSF16, **p) for name, p in NC._GNC.items()}  # s4x2, s5x2: 64 channels
_SHIPPED = dict(in_channels=80, channels=256, upsample_scales=[10, 5, 2, 2], upsample_kernal_sizes=[20, 11, 4, 4],
                resblock_kernel_sizes=[3, 7, 11], resblock_dilations=[[1, 3, 5, 7]] * 3, nsf_params=_NSF16)
_FRAMES = NC._FRAMES  # 23, 9, 2: 2 is fewer than flush_frames
_SEED = 5


def _gen(params, device="cpu"):
    from kantts.models.hifigan.hifigan import Generator

    torch.manual_seed(0)
    G = Generator(causal=False, **params).eval()
    G.remove_weight_norm()
    return G.to(device)


def _utts(device, frames=_FRAMES):
    return [N._feats(T, 20 + i).to(device) for i, T in enumerate(frames)]


def _cat(chunks):
    return torch.cat([c.cpu() for c in chunks], dim=1)


def _chunked(v, utts, n):
    """Every utterance through synthesize(key=i) and all of them through play_many; both give T * hop samples."""
    syn = [_cat(v.synthesize(x, chunk_frames=n, slot=i % v.slots, key=i)) for i, x in enumerate(utts)]
    many = [[] for _ in utts]
    for i, w in v.play_many(utts, chunk_frames=n):
        many[i].append(w)
    many = [_cat(ws) for ws in many]
    for x, a, b in zip(utts, syn, many):
        assert a.shape == b.shape == (1, x.shape[1] * v.hop), (a.shape, b.shape, x.shape)
    return syn, many


def _check_generator_fp32(name, n, device, graph=False):
    import kantts._hip as hip
    from kantts.models.hifigan.chunked_nc_nsf import ChunkedNCNSFVocoder

    hip.set_precision("fp32")
    G, utts = _gen(_GEN[name], device), _utts(device)
    v = ChunkedNCNSFVocoder(G, slots=2, graph=graph, seed=_SEED)
    assert v.delay_samples == ChunkedNCNSFVocoder.delay_of(G) == NC._DELAYS[name][0], "the source module adds no delay"
    assert v.flush_frames == NC._DELAYS[name][1]
    refs = [N._yardstick(G, v, x, key=i).cpu() for i, x in enumerate(utts)]
    syn, many = _chunked(v, utts, n)
    for i, (T, a, b, r) in enumerate(zip(_FRAMES, syn, many, refs)):
        for kind, y in (("synthesize", a), ("play_many", b)):
            err = float((y - r).abs().mean())
            print("chunked non-causal NSF", name, kind, "chunk", n, "frames", T, "mean-abs", err)
            assert err <= 1e-5, (name, kind, n, T, err)
        assert torch.equal(a, b), "play_many utterance %d differs from synthesize(key=%d)" % (i, i)


@pytest.mark.parametrize("n", [1, 4, 8])
@pytest.mark.parametrize("name", list(_GEN))
def test_chunked_nc_nsf_vocoder_matches_the_generator(name, n):
    with kernel_source_on_cpu():
        _check_generator_fp32(name, n, "cpu")


def _manual(v, feats, n, slot, key=0, late_end=False, pause=(), others=None, noise=None):
    """One utterance on ``slot`` by hand-made steps of room ``n`` (test_chunked_noncausal._manual for features and keys):
    ``pause`` lists steps in which the slot gets rows = 0, ``others`` maps other slots to (utterance, key) pairs that play
    beside it, ``noise`` (T * hop, H1) is the slot's given noise.  Returns the slot's waveform."""
    import kantts._hip as hip

    v.reset()
    T, nS, C = int(feats.shape[1]), v.slots, int(feats.shape[0])
    plays = {s: m for s, (m, _) in (others or {}).items()}
    plays[slot] = feats
    for s, (_, k) in (others or {}).items():
        v._assign(s, k)
    v._assign(slot, key)
    pos, out, i = {s: 0 for s in plays}, [], 0
    while pos[slot] < T + v.flush_frames:
        buf = torch.full((nS, C, n), NAN, device=feats.device)  # what is not fed must not be read
        nz = None if noise is None else torch.full((nS, n * v.hop, v.H1), NAN, device=feats.device)
        counts, end = [0] * nS, [-1] * nS
        for s, m in plays.items():
            Ts = int(m.shape[1])
            if s == slot and i in pause:
                end[s] = -1 if late_end and pos[s] <= Ts else Ts
                continue
            counts[s] = max(0, min(n, Ts + v.flush_frames - pos[s]))
            live = max(0, min(counts[s], Ts - pos[s]))
            buf[s, :, :live] = m[:, pos[s]:pos[s] + live]
            if nz is not None:
                nz[s, :live * v.hop] = noise[pos[s] * v.hop:(pos[s] + live) * v.hop] if s == slot else 0.0
            end[s] = -1 if late_end and pos[s] + counts[s] <= Ts else Ts
        before = (v.arena[v._parity, slot].clone(), v._nsf_state[v._parity, slot].clone(), v._nsf_hist[v._parity, slot].clone())
        wav = v.step(buf, rows=counts, end=end, noise=nz)
        if counts[slot] == 0:
            after = (v.arena[v._parity, slot], v._nsf_state[v._parity, slot], v._nsf_hist[v._parity, slot])
            for a, b in zip(after, before):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "a held slot's state moved"
            assert bool((wav[slot] == 0.0).all())
        off, cnt = hip.nc_emit(pos[slot], counts[slot], T, v.delay_samples, v.hop)
        keep = torch.zeros(wav.shape[2], dtype=torch.bool, device=wav.device)
        keep[off:off + cnt] = True
        assert bool((wav[slot, 0][~keep] == 0.0).all()), "samples outside the emitted run must be 0.0"
        out.append(wav[slot, :, off:off + cnt].cpu())
        for s in plays:
            pos[s] += counts[s]
        i += 1
        assert i < 500
    return torch.cat(out, dim=1)


def _check_bits(device, graphs=(False,)):
    """torch.equal at equal chunk size: alone in slot 0 / in slot 2 among other utterances / with held steps / with the end
    learnt late / (GPU) graph replay against eager launches; another key gives another waveform."""
    import kantts._hip as hip
    from kantts.models.hifigan.chunked_nc_nsf import ChunkedNCNSFVocoder

    hip.set_precision("fp32")
    G = _gen(_GEN["s4x2"], device)
    utts = _utts(device, [11, 23, 2])
    base = {}
    for graph in graphs:
        v = ChunkedNCNSFVocoder(G, slots=3, graph=graph, seed=_SEED)
        for n in (4, 5):
            a = _manual(v, utts[0], n, 0, key=7)
            assert a.shape == (1, 11 * v.hop)
            assert torch.equal(a, _cat(v.synthesize(utts[0], chunk_frames=n, key=7))), ("synthesize", n)
            assert torch.equal(a, _manual(v, utts[0], n, 2, key=7, others={0: (utts[1], 1), 1: (utts[2], 2)})), ("among others", n)
            assert torch.equal(a, _manual(v, utts[0], n, 0, key=7, pause=(0, 2, 3, 7), others={1: (utts[1], 3)})), ("held", n)
            assert torch.equal(a, _manual(v, utts[0], n, 0, key=7, late_end=True)), ("late end", n)
            assert torch.equal(a, _manual(v, utts[0], n, 1, key=7, late_end=True, pause=(1, 4), others={2: (utts[1], 7)})), ("all", n)
            assert torch.equal(base.setdefault(n, a), a), ("graph against eager", n)
            assert not torch.equal(a, _manual(v, utts[0], n, 0, key=8)), "another key must give another waveform"


def test_chunked_nc_nsf_bits_kernel_source():
    with kernel_source_on_cpu():
        _check_bits("cpu")


def _check_noise_argument(device, graph):
    import kantts._hip as hip
    from kantts.models.hifigan.chunked_nc_nsf import ChunkedNCNSFVocoder

    hip.set_precision("fp32")
    G = _gen(_GEN["s4x2"], device)
    x = N._feats(5, 3).to(device)
    feats = torch.zeros(2, 82, 4, device=device)
    v = ChunkedNCNSFVocoder(G, slots=2, graph=graph, seed=_SEED)
    with pytest.raises(ValueError):
        v.step(feats, noise=torch.zeros(2, 32, 8))
    g = ChunkedNCNSFVocoder(G, slots=2, graph=graph, seed=_SEED, given_noise=True)
    with pytest.raises(ValueError):
        g.step(feats)
    with pytest.raises(ValueError):
        g.step(feats, noise=torch.zeros(2, 32, 7))
    assert g._parity == 0
    gen = torch.Generator().manual_seed(8)
    nz = (SIGMA * torch.randn(5 * g.hop, 8, generator=gen)).to(device)
    # _manual holds NaN in the noise of every frame at or beyond a slot's live count, flush frames included
    a = _manual(g, x, 4, 1, noise=nz)
    assert a.shape == (1, 5 * g.hop) and not bool(torch.isnan(a).any())
    assert torch.equal(a, _manual(g, x, 4, 1, noise=nz, late_end=True, others={0: (x, 1)}))
    assert not torch.equal(a, _manual(g, x, 4, 1, noise=torch.zeros_like(nz))), "the caller's noise must be used"
    assert not torch.equal(a, _cat(v.synthesize(x, chunk_frames=4, slot=1))), "generated noise is another draw"
    # the given noise is ALL of the randomness but the initial phases, which the key draws
    assert not torch.equal(a, _manual(g, x, 4, 1, key=1, noise=nz))


def test_chunked_nc_nsf_noise_argument():
    with kernel_source_on_cpu():
        _check_noise_argument("cpu", False)


def test_geometry_of_the_shipped_noncausal_nsf_voice():
    """hifigan_noncausal_nsf_v1_16k: the up-layer delays 35 / 678 / 1559 / 3321 of test_delay_of_the_shipped_noncausal_geometry
    at strides u = 20 / 4 / 2 / 1 with paddings 10 / 2 / 1 / 0: lag_i = D_i u_i + p_i."""
    from kantts.models.hifigan.chunked_nc import plan_delays
    from kantts.models.hifigan.chunked_nc_nsf import ChunkedNCNSFVocoder, plan_lags

    G = _gen(_SHIPPED)
    assert ChunkedNCNSFVocoder.delay_of(G) == 3424
    assert [d for name, _, d in plan_delays(G) if name.endswith(".up")] == [35, 678, 1559, 3321]
    assert plan_lags(G) == [35 * 20 + 10, 678 * 4 + 2, 1559 * 2 + 1, 3321] == [710, 2714, 3119, 3321]
    with kernel_source_on_cpu():
        v = ChunkedNCNSFVocoder(G, slots=1, graph=False)
    assert v.delay_samples == 3424 and v.flush_frames == 18 and v.hop == 200
    assert v.lags == [710, 2714, 3119, 3321] and v.excitation_history == 3321
    assert tuple(v._nsf_hist.shape) == (2, 1, 3321) and tuple(v._nsf_state.shape) == (2, 1, 36)


def _refusal_cases():
    from kantts.models.hifigan.hifigan import Generator
    from kantts.models.hifigan.layers import CausalConv1d, Conv1d

    g64 = _GEN["s4x2"]

    def edited(fn, params=g64):
        G = _gen(params)
        fn(G)
        return G

    def drop_last_down(G):
        G.source_downs = torch.nn.ModuleList(list(G.source_downs)[:-1])

    return [
        (Generator(causal=True, **g64).eval(), ValueError, "ChunkedVocoder"),                        # a causal generator
        (Generator(causal=False, **NC._GNC["s4x2"]).eval(), ValueError, "source module"),            # no source module
        (Generator(causal=False, **g64).train(), ValueError, "eval"),
        (Generator(causal=False, out_channels=4, **g64).eval(), NotImplementedError, "out_channels"),
        (Generator(causal=False, **dict(g64, channels=32)).eval(), NotImplementedError, "outside what"),
        (Generator(causal=False, **dict(g64, upsample_scales=[2, 2], upsample_kernal_sizes=[5, 4])).eval(),
         NotImplementedError, "even"),
        (Generator(causal=False, **dict(g64, nsf_params={"nb_harmonics": 16, "sampling_rate": 16000})).eval(),
         NotImplementedError, "harmonics"),
        (edited(lambda G: setattr(G.source_module, "upsample_ratio", 9)), NotImplementedError, "upsample_ratio"),
        (edited(lambda G: G.source_module.ffn.__setitem__(0, torch.nn.Conv1d(8, 1, 3))), NotImplementedError, "1x1"),
        (edited(drop_last_down), NotImplementedError, "source_downs"),
        (edited(lambda G: G.source_downs.__setitem__(0, CausalConv1d(1, 32, 4, 2))), ValueError, "symmetric"),
        (edited(lambda G: G.source_downs.__setitem__(0, Conv1d(1, 32, 6, 2, padding=1))), NotImplementedError, "kernel 4"),
        (edited(lambda G: G.source_downs.__setitem__(0, Conv1d(1, 32, 4, 2, padding=0))), NotImplementedError, "padding 1"),
        (edited(lambda G: G.source_downs.__setitem__(1, Conv1d(1, 16, 3, 1, padding=1))), NotImplementedError, "kernel 1"),
        (Generator(causal=False, **dict(g64, upsample_scales=[2, 3], upsample_kernal_sizes=[4, 5])).eval(),
         NotImplementedError, "odd stride 3"),
    ]


def test_chunked_nc_nsf_refusals():
    """Every refusal comes before the library is touched; the three existing classes keep refusing non-causal NSF."""
    import kantts._hip as hip
    from kantts.models.hifigan.chunked import ChunkedVocoder
    from kantts.models.hifigan.chunked_nc import ChunkedNCVocoder
    from kantts.models.hifigan.chunked_nc_nsf import ChunkedNCNSFVocoder
    from kantts.models.hifigan.chunked_nsf import ChunkedNSFVocoder

    class _NoLaunch:
        def __getattr__(self, name):
            raise AssertionError("a refusal must not reach the library (%s)" % name)

    cases = _refusal_cases()
    G = _gen(_GEN["s4x2"])
    saved = hip.lib
    hip.lib = lambda: _NoLaunch()
    try:
        for bad, exc, pat in cases:
            with pytest.raises(exc, match=pat):
                ChunkedNCNSFVocoder(bad, slots=1, graph=False)
        with pytest.raises(ValueError, match="causal"):
            ChunkedVocoder(G, graph=False)
        with pytest.raises(ValueError, match="causal"):
            ChunkedNSFVocoder(G, graph=False)
        with pytest.raises(NotImplementedError, match="NSF"):
            ChunkedNCVocoder(G, graph=False)
    finally:
        hip.lib = saved
    with kernel_source_on_cpu():
        v = ChunkedNCNSFVocoder(G, slots=2, graph=False)
        with pytest.raises(ValueError):
            v.step(torch.zeros(2, 80, 4))  # the mel alone: f0 and voicing are missing
        with pytest.raises(ValueError):
            v.step(torch.zeros(2, 82, 4), end=[1])
        with pytest.raises(ValueError):
            v.reset(phase0=torch.zeros(5))


# ---------------------------------------------------------------------------------------------------------------------
# 11. infer_hifigan --chunk_frames on a non-causal NSF voice
def _write_voice(tmp_path):
    from kantts.models.hifigan.hifigan import Generator

    voc_dir = tmp_path / "voc" / "ckpt"
    voc_dir.mkdir(parents=True)
    params = dict(_GEN["s4x2"], causal=False)
    (tmp_path / "voc" / "config.yaml").write_text(yaml.dump(
        {"Model": {"Generator": {"params": params}}, "audio_config": {"sampling_rate": 16000}}))
    torch.manual_seed(0)
    torch.save({"model": {"generator": Generator(**params).state_dict()}}, voc_dir / "checkpoint_1.pth")
    mel_dir = tmp_path / "feats"
    mel_dir.mkdir()
    lengths = {"utt_a": 21, "utt_b": 2, "utt_c": 14}
    for i, (name, n) in enumerate(lengths.items()):
        x = N._feats(n, 40 + i).t().numpy().copy()
        x[:, -1] = 0.2 + 0.7 * x[:, -1]  # a predicted voicing flag: binarised by the command line
        np.save(mel_dir / (name + ".npy"), x.astype(np.float32))
    return str(voc_dir / "checkpoint_1.pth"), str(mel_dir), lengths


def _check_cli(tmp_path, monkeypatch):
    from kantts.bin import infer_hifigan
    from kantts.models.hifigan import chunked_nc_nsf
    from scipy.io import wavfile

    built = []
    cls = chunked_nc_nsf.ChunkedNCNSFVocoder

    class _Seen(cls):
        def __init__(self, *a, **k):
            built.append(k.get("slots"))
            super().__init__(*a, **k)

    monkeypatch.setattr(chunked_nc_nsf, "ChunkedNCNSFVocoder", _Seen)
    ck, mel_dir, lengths = _write_voice(tmp_path)
    infer_hifigan.main(["--ckpt", ck, "--input_mel", mel_dir, "--output_dir", str(tmp_path / "one"), "--chunk_frames", "8"])
    infer_hifigan.main(["--ckpt", ck, "--input_mel", mel_dir, "--output_dir", str(tmp_path / "two"), "--chunk_frames", "8",
                        "--slots", "2"])
    infer_hifigan.hifigan_infer(mel_dir, ck, str(tmp_path / "seed1"), chunk_frames=8, seed=1)
    assert built == [1, 2, 1], "the command line must play a non-causal NSF voice through ChunkedNCNSFVocoder"
    for name, n in lengths.items():
        a, b, d = (wavfile.read(tmp_path / k / (name + "_gen.wav"))[1] for k in ("one", "two", "seed1"))
        assert a.dtype == b.dtype == np.int16 and a.shape == b.shape == d.shape == (n * 8,)
        assert np.array_equal(a, b), "one slot and two slots differ: " + name
        assert not np.array_equal(a, d), "another seed must give another excitation: " + name


def test_infer_hifigan_chunked_nc_nsf_cli(tmp_path, monkeypatch):
    import kantts._hip as hip
    from kantts.bin import infer_hifigan

    hip.set_precision("fp32")
    monkeypatch.setattr(infer_hifigan, "_device", lambda: torch.device("cpu"))
    with kernel_source_on_cpu():
        _check_cli(tmp_path, monkeypatch)


# ---------------------------------------------------------------------------------------------------------------------
# 12. StreamingTTS(lookahead=True, nsf=...): the fixtures of tests/test_streaming_tts.py (imported, not edited)
def _check_streaming(leg, dev, Tc):
    """Four utterances (96, 45, 6 frames and a free-running one) through two slots.  Every vocoder step of the pipeline is
    repeated on a twin ChunkedNCNSFVocoder fed the same frames, de-normalised on the HOST (infer_sambert.denorm_f0) from the
    pool's results, with NaN wherever the pipeline handed nothing over: the same bits, sample for sample."""
    import kantts._hip as hip
    import test_streaming_tts as _st
    from kantts.models.hifigan.chunked_nc_nsf import ChunkedNCNSFVocoder
    from kantts.models.streaming import StreamingTTS

    m, _, utts, refs = _st._utterances82(leg, dev)
    G = _gen(_GEN["s4x2"], dev)
    scale_offset, floor, uvt = _st._nsf_settings(refs)
    kw = dict(nsf=scale_offset, f0_threshold=floor, uv_threshold=uvt, seed=_SEED, graph=dev == "cuda")
    with pytest.raises(ValueError, match="causal"):  # without lookahead the refusal stays what it is
        StreamingTTS(m, G, slots=2, max_steps=32, chunk_frames=Tc, **kw)
    tts = StreamingTTS(m, G, slots=2, max_steps=32, chunk_frames=Tc, lookahead=True, **kw)
    assert type(tts.vocoder) is ChunkedNCNSFVocoder and tts.nc
    assert tts.flush_frames == tts.vocoder.flush_frames == 27 and tts.hop == 8 and tts.vocoder.seed == _SEED
    calls, uploads = [], []
    voc_step, step = tts.vocoder.step, tts.step

    def rec_voc(buf, rows=None, end=None):
        wav = voc_step(buf, rows=rows, end=end)
        calls.append((rows.cpu().tolist(), end.cpu().tolist(), wav.clone()))
        return wav

    def rec_step():
        before, vocoded = len(calls), list(tts.vocoded)
        outs = step()
        uploads.append(len(calls) - before)
        if len(calls) > before:
            calls[-1] += ([None if o is None else (o[0], vocoded[s], o[2]) for s, o in enumerate(outs)],)
        return outs

    tts.vocoder.step, tts.step = rec_voc, rec_step
    results, chunks = {}, {}
    for index, first, wav in tts.play_many(utts, results=results):
        assert first == sum(w.shape[-1] for w in chunks.get(index, [])), (index, first)
        chunks.setdefault(index, []).append(wav.clone())
    assert sorted(results) == [0, 1, 2, 3] and tts.index == [None, None]
    assert set(uploads) <= {0, 1}, "at most one vocoder step per step"
    frames = {i: int(r["LR_length_rounded"][0]) for i, r in enumerate(refs)}
    for i, n in frames.items():
        assert sum(w.shape[-1] for w in chunks[i]) == n * tts.hop, i
    # the twin
    twin = ChunkedNCNSFVocoder(G, slots=2, graph=False, seed=_SEED)
    occupant, seen_flush = [None, None], False
    for rows, end, wav, outs in calls:
        buf = torch.full((2, 82, Tc), NAN)
        for s, o in enumerate(outs):
            if o is None:
                assert rows[s] == 0
                continue
            index, lo, n = o
            if occupant[s] != index:
                twin.reset(s)
                twin._assign(s, index)
                occupant[s] = index
            assert end[s] == frames[index] and rows[s] >= n
            seen_flush |= rows[s] > n
            if n:
                buf[s, :, :n] = _st._feats(kw, results[index]["postnet_outputs"][0, lo:lo + n]).t()
        want = twin.step(buf.to(dev), rows=rows, end=end)
        assert torch.equal(wav, want), "a step of the pipeline differs from the vocoder fed the same frames"
    assert seen_flush


@pytest.mark.parametrize("leg", _ca.LEGS)
def test_streaming_tts_lookahead_plays_a_noncausal_nsf_generator(leg):
    import kantts._hip as hip

    ctx, dev = _ca._leg(leg)
    hip.set_precision("bf16")
    try:
        with ctx:
            _check_streaming(leg, dev, 15)
    finally:
        hip.set_precision("fp32")


# ---------------------------------------------------------------------------------------------------------------------
# GPU legs
@pytest.mark.gpu
def test_nsf_source_with_an_end_gpu():
    _check_source_end_all("cuda")


@pytest.mark.gpu
def test_nsf_downs_sym_gpu():
    for name in sorted(_SYM_CASES):
        _check_downs_sym("cuda", name)
    _check_downs_causal_bits("cuda")
    _check_codes("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(_GEN))
def test_chunked_nc_nsf_vocoder_matches_the_generator_gpu(name):
    for n in (1, 4, 8):
        _check_generator_fp32(name, n, "cuda", graph=n != 4)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(_GEN))
def test_chunked_nc_nsf_vocoder_bf16_gpu(name):
    """bf16: the chunked path against the fp32 one-shot output (the yardstick: Generator.forward on the excitation of one
    whole-utterance source call) errs at most twice as much, max-abs over the three utterances, as the bf16 one-shot path
    does against it, measured in the same run.  Both figures go to the parity report."""
    import kantts._hip as hip
    from kantts.models.hifigan.chunked_nc_nsf import ChunkedNCNSFVocoder

    G, utts = _gen(_GEN[name], "cuda"), _utts("cuda")
    try:
        hip.set_precision("bf16")
        v = ChunkedNCNSFVocoder(G, slots=2, graph=False, seed=_SEED)
        hip.set_precision("fp32")
        ref = torch.cat([N._yardstick(G, v, x, key=i).cpu() for i, x in enumerate(utts)], dim=1)
        hip.set_precision("bf16")
        one = float((torch.cat([N._yardstick(G, v, x, key=i).cpu() for i, x in enumerate(utts)], dim=1) - ref).abs().max())
        for n in (1, 4, 8):
            for kind, got in zip(("synthesize", "play_many"), _chunked(v, utts, n)):
                err = float((torch.cat(got, dim=1) - ref).abs().max())
                print("chunked non-causal NSF bf16", name, kind, "chunk", n, "max-abs", err, "one-shot bf16", one)
                _record("bf16_%s_%s_chunk%d" % (name, kind, n), {"chunked_max_abs": err, "one_shot_bf16_max_abs": one})
                assert err <= 2 * one, (name, kind, n, err, one)
    finally:
        hip.set_precision("fp32")


@pytest.mark.gpu
def test_chunked_nc_nsf_bits_gpu():
    _check_bits("cuda", graphs=(False, True))


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [True, False])
def test_chunked_nc_nsf_noise_argument_gpu(graph):
    _check_noise_argument("cuda", graph)


@pytest.mark.gpu
def test_chunked_nc_nsf_shipped_geometry_gpu():
    """hifigan_noncausal_nsf_v1_16k's shapes: one 21-frame utterance, chunk 8, fp32, graph replay, against the yardstick."""
    import kantts._hip as hip
    from kantts.models.hifigan.chunked_nc_nsf import ChunkedNCNSFVocoder

    hip.set_precision("fp32")
    G = _gen(_SHIPPED, "cuda")
    x = N._feats(21, 31).cuda()
    v = ChunkedNCNSFVocoder(G, slots=1, graph=True, seed=_SEED)
    assert v.delay_samples == 3424 and v.flush_frames == 18 and v.lags == [710, 2714, 3119, 3321]
    ref = N._yardstick(G, v, x, key=0).cpu()
    wav = _cat(v.synthesize(x, chunk_frames=8, key=0))
    assert wav.shape == ref.shape == (1, 21 * 200)
    err = float((wav - ref).abs().mean())
    print("chunked non-causal NSF, shipped geometry, chunk 8: mean-abs", err)
    assert err <= 1e-5, err


@pytest.mark.gpu
def test_chunked_nc_nsf_refusals_gpu():
    from kantts.models.hifigan.chunked_nc_nsf import ChunkedNCNSFVocoder

    for G, exc, pat in _refusal_cases():
        with pytest.raises(exc, match=pat):
            ChunkedNCNSFVocoder(G.cuda(), slots=1, graph=True)


@pytest.mark.gpu
def test_infer_hifigan_chunked_nc_nsf_cli_gpu(tmp_path, monkeypatch):
    import kantts._hip as hip

    hip.set_precision("fp32")
    _check_cli(tmp_path, monkeypatch)


@pytest.mark.gpu
def test_symbols_to_wav_streams_a_noncausal_nsf_voice_gpu(tmp_path, monkeypatch):
    """text_to_wav --chunk_frames (symbols_to_wav) on the voices of test_streaming_tts._write_voices with the vocoder replaced by
    a non-causal NSF one: it reaches ChunkedNCNSFVocoder and writes frames * hop samples per sub-sentence."""
    import kantts._hip as hip
    import test_streaming_tts as _st
    from kantts.bin.text_to_wav import symbols_to_wav
    from kantts.models.hifigan import chunked_nc_nsf
    from kantts.models.hifigan.hifigan import Generator
    from scipy.io import wavfile

    cfg, am_ck, voc_ck, sym = _st._write_voices(tmp_path, 1)
    params = dict(_GEN["s4x2"], causal=False)
    (tmp_path / "voc" / "config.yaml").write_text(yaml.dump(
        {"Model": {"Generator": {"params": params}}, "audio_config": {"sampling_rate": 16000}}))
    torch.manual_seed(0)
    torch.save({"model": {"generator": Generator(**params).state_dict()}}, voc_ck)
    built = []

    class _Seen(chunked_nc_nsf.ChunkedNCNSFVocoder):
        def __init__(self, *a, **k):
            built.append(k.get("slots"))
            super().__init__(*a, **k)

    monkeypatch.setattr(chunked_nc_nsf, "ChunkedNCNSFVocoder", _Seen)
    hip.set_precision("bf16")
    try:
        symbols_to_wav(sym, str(tmp_path / "stream"), am_ck, voc_ck, chunk_frames=15, slots=2, slot_steps=64,
                       ling_unit=_ca._FakeLingUnit(cfg))
    finally:
        hip.set_precision("fp32")
    assert built == [2]
    for i in ("0_0", "0_1", "1_0"):
        frames = np.load(tmp_path / "stream" / "feat" / (i + "_mel.npy")).shape[0]
        sr, w = wavfile.read(tmp_path / "stream" / (i + "_mel_gen.wav"))
        assert sr == 16000 and w.dtype == np.int16 and w.shape == (frames * 8,) and w.any(), (i, w.shape, frames)
