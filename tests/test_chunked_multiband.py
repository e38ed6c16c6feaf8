"""Chunked inference of multi-band generators: the tail kernel (csrc/mb_tail.hip, kantts_mb_tail_rows: conv_post, tanh and a
PQMF synthesis that can be cut at a chunk boundary) and kantts.models.hifigan.chunked_mb.ChunkedMBVocoder.

CPU leg: the kernel SOURCE on the host build (util.kernel_source_on_cpu), graph=False.  GPU leg: the same checks on the
device.  Inputs a call must not read hold NaN; outputs hold a sentinel and have guard cells around them; the state and the
history have guard floats between the slots.

References.  The synthesis is the module's own two-convolution form (zero-stuffing by ``updown_filter``, then
``synthesis_filter`` over the padded signal) in fp64, built from the PQMF buffers that carry the reference's values.
Bounds.
  * tail kernel against fp64 torch: max-abs <= 2e-5 * G_max.  2e-5 is the project's single-layer fp32 bound
    (test_chunked_vocoder._check_layer) for conv_post; tanh does not amplify; the synthesis multiplies an error of its input
    by at most G_max = max_r sum_{k, d} |W[r, k, d]|, computed here (7.83 for the default bank).
  * pass-through against the reference-recorded synthesis of tests/golden/multiband.pt: 2e-6, the bound of the one-shot path
    in tests/test_multiband.py.
  * generator, fp32: mean-abs <= 1e-5 * G_mean against hifigan_oracle.generator followed by the fp64 synthesis: 1e-5 is the
    bound of test_chunked_generator_kernel_source_matches_oracle, G_mean = max_k sum_{r, d} |W[r, k, d]| / B (1.69) what the
    synthesis does to a mean-abs error of one sub-band.  bf16: mean-abs <= 2e-3 * G_mean, and over the D * B + 256 samples
    after every chunk boundary a max-abs error of at most twice the one-shot device path's (generator(x) then
    pqmf.synthesis), measured in the same run.
Wherever two plays run the same arithmetic the assertion is torch.equal."""
import ctypes
import json
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

import hifigan_oracle as H
import test_bench_config_parity as _bench_parity
from util import GOLDEN, ROOT, kernel_source_on_cpu

_REPORT = os.path.join(os.path.dirname(_bench_parity._REPORT), "chunked_multiband_parity.json")
SENT, GUARD, NAN = -1234.5, 7.0, float("nan")


def _record(key, val):
    try:
        os.makedirs(os.path.dirname(_REPORT), exist_ok=True)
        d = json.load(open(_REPORT)) if os.path.exists(_REPORT) else {}
        d[key] = val
        json.dump(d, open(_REPORT, "w"), indent=1)
    except OSError:
        pass


_BANKS = {}


def _bank(B=4, taps=62):
    """(PQMF on the host, polyphase weights W (B, B, 2 D + 1), D)"""
    if (B, taps) not in _BANKS:
        from kantts.models.pqmf import PQMF

        pq = PQMF(subbands=B, taps=taps)
        _BANKS[(B, taps)] = (pq, pq._poly_synthesis.contiguous(), -pq.d_min)
    return _BANKS[(B, taps)]


def _synthesis64(pq, z):
    """z (S, T, B) -> (S, T * B) in fp64: zero-stuffing times B, then the synthesis filters over the padded signal."""
    x = F.conv_transpose1d(z.double().transpose(1, 2), pq.updown_filter.double() * pq.subbands, stride=pq.subbands)
    return F.conv1d(F.pad(x, (pq.taps // 2, pq.taps // 2)), pq.synthesis_filter.double())[:, 0]


def _gains(W):
    B = W.shape[0]
    return float(W.abs().sum(dim=(1, 2)).max()), float(W.abs().sum(dim=(0, 2)).max()) / B


class _Tail:
    """The buffers of S slots of the tail kernel between calls: state and history halves with guard floats behind every
    slot.  ``w`` (K, B, Cin) / ``bias`` (B), or the pass-through form without them."""

    def __init__(self, device, B, taps, S, w=None, bias=None):
        import kantts._hip as hip

        self.pq, W, self.D = _bank(B, taps)
        self.device, self.B, self.S = device, B, S
        self.poly = W.to(device)
        self.w = None if w is None else w.contiguous().to(device)
        self.bias = None if bias is None else bias.to(device)
        self.K, self.Cin = (1, B) if w is None else (w.shape[0], w.shape[2])
        self.words = hip.mb_state_words(self.D, B)
        self.ss = -(-self.words // 4) * 4 + 4
        st = torch.full((2, S, self.ss), GUARD)
        st[:, :, :self.words] = 0.0
        self.state = st.to(device)
        self.H = (self.K - 1) * self.Cin
        self.hs = self.H + 8
        hist = torch.full((2, S, self.hs), GUARD)
        hist[:, :, :self.H] = 0.0
        self.hist = hist.to(device)
        self.par = 0

    def words_of(self, half):
        """(S, words) int32: the z rows as bits and the pending count."""
        return self.state[half, :, :self.words].cpu().view(torch.int32).clone()

    def pending(self):
        return self.words_of(self.par)[:, -1].tolist()

    def call(self, x, rows=None, last=None, row_mul=1):
        """One launch: x (S, Tq, Cin) on the host -> (out (S, (Tq + D) * B), emitted list)."""
        import kantts._hip as hip

        S, Tq, _ = x.shape
        dev, p = self.device, self.par
        n = S * (Tq + self.D) * self.B
        flat = torch.full((n + 32,), GUARD).to(dev)
        out = flat[16:16 + n].view(S, -1)
        out.fill_(SENT)
        em = torch.full((S,), -5, dtype=torch.int32).to(dev)
        before = (self.state[p].clone(), self.hist[p].clone())
        i32 = lambda v: None if v is None else torch.tensor(v, dtype=torch.int32).to(dev)  # noqa: E731
        ok = hip.mb_tail(x.contiguous().to(dev), self.hist[p, 0] if self.H else None, self.hist[1 - p, 0] if self.H else None,
                         self.w, self.poly, self.state[p, 0], self.state[1 - p, 0], out, S=S, Tq=Tq, Cin=self.Cin, B=self.B,
                         K=self.K, D=self.D, hist_ss=self.hs, state_ss=self.ss, bias=self.bias, emitted=em, rows=i32(rows),
                         row_mul=row_mul, last=i32(last), in_leaky=None if self.w is None else 0.01)
        assert ok
        assert torch.equal(self.state[p], before[0]) and torch.equal(self.hist[p], before[1]), "an input half was written"
        assert bool((self.state[:, :, self.words:] == GUARD).all()), "guard floats behind a slot's state were written"
        assert bool((self.hist[:, :, self.H:] == GUARD).all()), "guard floats behind a slot's history were written"
        assert bool((flat[:16] == GUARD).all()) and bool((flat[-16:] == GUARD).all()), "guard cells around out were written"
        self.par ^= 1
        return out.cpu().clone(), em.cpu().tolist()


def _play(tail, x, sched, use_rows=False):
    """x (S, T, Cin) through ``sched`` in lockstep from the tail's current state, `last` on the final chunk.
    -> (live samples (S, T * B), emitted samples per chunk)."""
    import kantts._hip as hip

    S, B, D = tail.S, tail.B, tail.D
    parts, counts, t0, pend = [], [], 0, tail.pending()
    for i, n in enumerate(sched):
        final = i == len(sched) - 1
        xc = x[:, t0:t0 + n]
        out, em = tail.call(xc, rows=[n] * S if use_rows else None, last=[1] * S if final else None)
        want = [hip.mb_emit(pend[s], n, final, D) for s in range(S)]
        assert em == [w[0] * B for w in want], (sched, i, em, want)
        pend = [w[1] for w in want]
        assert tail.pending() == pend
        assert bool((out[:, em[0]:] == 0.0).all()), "samples behind the emitted count must be 0.0"
        parts.append(out[:, :em[0]])
        counts.append(em[0])
        t0 += n
    assert t0 == x.shape[1]
    return torch.cat(parts, dim=1), counts


# ---------------------------------------------------------------------------------------------------------------------
# (a) the whole tail against fp64 torch, cut six ways
_SCHEDULES = [[53], [1] * 53, [5, 11, 3, 13, 8, 13], [2, 2, 2, 47], [52, 1], [1, 52]]
_CASES = {"b4_taps62": (16, 7, 4, 62), "b2_taps62": (16, 7, 2, 62), "b4_taps14": (16, 7, 4, 14)}


def _conv_inputs(S, T, Cin, K, B, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(S, T, Cin, generator=g)
    Wc = torch.randn(B, Cin, K, generator=g) / (Cin * K) ** 0.5 * 2.0
    b = torch.randn(B, generator=g) * 0.2
    return x, Wc, b, Wc.permute(2, 0, 1).flip(0).contiguous()  # tap j reads j rows back


def _tail64(pq, x, Wc, b):
    """leaky -> causal conv -> tanh -> synthesis, fp64: (S, T * B)"""
    K = Wc.shape[2]
    h = F.leaky_relu(x.double(), 0.01).transpose(1, 2)
    z = torch.tanh(F.conv1d(F.pad(h, (K - 1, 0)), Wc.double(), b.double()))
    return _synthesis64(pq, z.transpose(1, 2))


def _check_tail(device, name, S):
    Cin, K, B, taps = _CASES[name]
    pq, W, D = _bank(B, taps)
    assert D == {"b4_taps62": 8, "b2_taps62": 16, "b4_taps14": 2}[name]
    x, Wc, b, w_kbc = _conv_inputs(S, 53, Cin, K, B)
    ref = _tail64(pq, x, Wc, b)
    g_max = _gains(W)[0]
    first = None
    for sched in _SCHEDULES:
        got, counts = _play(_Tail(device, B, taps, S, w_kbc, b), x, sched, use_rows=sched[0] == 2)
        assert got.shape == ref.shape == (S, 53 * B)
        if name == "b4_taps62" and sched == [5, 11, 3, 13, 8, 13]:
            assert counts == [0, 32, 12, 52, 32, 84]
        if first is None:
            first = got
            err = float((got.double() - ref).abs().max())
            print("mb tail vs fp64 torch:", name, "S", S, "max-abs", err, "bound", 2e-5 * g_max)
            _record("tail_%s_S%d_%s" % (name, S, device), dict(max_abs=err, g_max=g_max))
            assert err <= 2e-5 * g_max, (name, S, err)
        else:
            assert torch.equal(got, first), ("the samples depend on the cuts", name, S, sched[:4])
    if name == "b4_taps62":
        assert abs(g_max - 7.83) < 0.01


# ---------------------------------------------------------------------------------------------------------------------
# (b) the pass-through form on the reference-recorded fixture
def _check_pass_through(device):
    f = torch.load(os.path.join(GOLDEN, "multiband.pt"), weights_only=False)["pqmf"]
    z = f["analysis"].transpose(1, 2).contiguous()  # (S, L, 4)
    S, L, B = z.shape
    want = f["synthesis"].reshape(S, L * B)
    one, _ = _play(_Tail(device, 4, 62, S), z, [L])
    cut, _ = _play(_Tail(device, 4, 62, S), z, [7] * (L // 7) + ([L % 7] if L % 7 else []))
    e1, e7 = float((one - want).abs().max()), float((cut - want).abs().max())
    print("mb pass-through vs the reference-recorded synthesis: one call", e1, "chunks of 7 rows", e7)
    _record("pass_through_" + device, dict(one_call=e1, chunks_of_7=e7))
    assert e1 <= 2e-6 and e7 <= 2e-6, (e1, e7)
    assert torch.equal(one, cut)


# ---------------------------------------------------------------------------------------------------------------------
# (c) the slots of a call are independent
def _check_slots(device):
    import kantts._hip as hip

    Cin, K, B, taps = _CASES["b4_taps62"]
    pq, W, D = _bank(B, taps)
    x, Wc, b, w_kbc = _conv_inputs(3, 16, Cin, K, B, seed=5)
    counts = [12, 0, 16]
    xn = x.clone()
    for s, n in enumerate(counts):
        xn[s, n:] = NAN  # rows behind a slot's count are never loaded
    # every slot's own utterance in one call on a fresh tail
    alone = []
    for s, n in enumerate(counts):
        if n:
            out, em = _Tail(device, B, taps, 1, w_kbc, b).call(x[s:s + 1, :n], last=[1])
            assert em == [n * B]
            alone.append(out[0, :n * B])
        else:
            alone.append(None)
    t = _Tail(device, B, taps, 3, w_kbc, b)
    # make slot 1's state something to keep: three rows of another signal, nothing emitted yet
    y, _, _, _ = _conv_inputs(3, 16, Cin, K, B, seed=6)
    yn = y.clone()
    yn[0], yn[2], yn[1, 3:] = NAN, NAN, NAN
    _, em = t.call(yn, rows=[0, 3, 0])
    assert em == [0, 0, 0] and t.pending() == [0, 3, 0]
    kept = (t.words_of(t.par)[1], t.hist[t.par, 1].cpu().clone())
    assert bool(kept[0][:-1].any()) and bool(kept[1][:t.H].any())
    # rows in units of row_mul = 2; 99 is clamped to Tq / row_mul; `last` on slot 2 only
    out, em = t.call(xn, rows=[6, 0, 99], last=[0, 0, 1], row_mul=2)
    assert em == [(12 - D) * B, 0, 16 * B] and t.pending() == [D, 3, 0]
    assert not bool(torch.isnan(out).any())
    for s in range(3):
        assert bool((out[s, em[s]:] == 0.0).all()), s
    assert torch.equal(out[0, :em[0]], alone[0][:em[0]]) and torch.equal(out[2, :em[2]], alone[2])
    assert torch.equal(t.words_of(t.par)[1], kept[0]) and torch.equal(t.hist[t.par, 1].cpu(), kept[1]), \
        "a slot with count 0 must keep its state bit for bit"
    assert not bool(t.words_of(t.par)[2].any()) and not bool(t.hist[t.par, 2, :t.H].any()), "after `last` the slot is as after a reset"
    # a flush-only call yields exactly the tail of the one-call output; a second flush emits nothing
    nan = torch.full((3, 4, Cin), NAN)
    out, em = t.call(nan, rows=[0, 0, 0], last=[1, 0, 0])
    assert em == [D * B, 0, 0] and t.pending() == [0, 3, 0]
    assert torch.equal(out[0, :em[0]], alone[0][(12 - D) * B:]) and bool((out[:, em[0]:] == 0.0).all()) and not bool(out[1:].any())
    out, em = t.call(nan, rows=[0, 0, 0], last=[1, 0, 0])
    assert em == [0, 0, 0] and not bool(out.any()) and t.pending() == [0, 3, 0]
    out, em = t.call(nan, rows=[0, 0, 0])  # n = 0 without `last`: nothing emitted, everything kept
    assert em == [0, 0, 0] and torch.equal(t.words_of(t.par)[1], kept[0])
    # after `last`, a second utterance through slots 0 and 2 without a reset equals a fresh slot bit for bit
    zn = y.clone()
    zn[1] = NAN
    fresh = _Tail(device, B, taps, 3, w_kbc, b)
    for rows, last in (([5, 0, 16], None), ([11, 0, 0], [1, 0, 1])):
        a, ea = t.call(zn if last is None else torch.cat([zn[:, 5:], zn[:, :5]], dim=1), rows=rows, last=last)
        c, ec = fresh.call(zn if last is None else torch.cat([zn[:, 5:], zn[:, :5]], dim=1), rows=rows, last=last)
        assert ea == ec and torch.equal(a[0], c[0]) and torch.equal(a[2], c[2])
        assert torch.equal(t.words_of(t.par)[[0, 2]], fresh.words_of(fresh.par)[[0, 2]])
    assert ea == [hip.mb_emit(5, 11, 1, D)[0] * B, 0, D * B] == [16 * B, 0, D * B]


# ---------------------------------------------------------------------------------------------------------------------
# (d) argument errors and refusals: the return codes of include/kantts_hip.h, and nothing launched
def _check_codes(device):
    import kantts._hip as hip

    L = hip.lib()
    _, W, D = _bank(4, 62)
    words = hip.mb_state_words(D, 4)
    ss = 68
    bufs = dict(x=torch.ones(2, 9, 16), w=torch.ones(7, 4, 16), poly=W.clone(), st=torch.zeros(2, 2, ss), hist=torch.zeros(2, 2, 96),
                out=torch.full((2, (8 + D) * 4), SENT), em=torch.full((2,), -5, dtype=torch.int32))
    bufs = {k: v.to(device) for k, v in bufs.items()}
    st, hist = bufs["st"], bufs["hist"]
    st[1], hist[1] = -99.0, -99.0

    def tail(**over):
        g = hip.MbTailArgs()
        g.in_, g.w, g.poly, g.out, g.emitted = (hip.ptr(bufs[k]) for k in ("x", "w", "poly", "out", "em"))
        g.hist_in, g.hist_out, g.hist_ss = hip.ptr(hist[0]), hip.ptr(hist[1]), 96
        g.state_in, g.state_out, g.state_ss = hip.ptr(st[0]), hip.ptr(st[1]), ss
        g.S, g.Tq, g.Cin, g.B, g.K, g.D, g.row_mul, g.in_slope, g.in_act = 2, 8, 16, 4, 7, D, 1, 0.01, 1
        for k, v in over.items():
            setattr(g, k, v)
        return L.kantts_mb_tail_rows(ctypes.byref(g), hip.stream())

    BAD, UNS = -1, hip.E_UNSUPPORTED
    assert words == 65 and L.kantts_mb_tail_rows(None, hip.stream()) == BAD
    for name in ("in_", "poly", "out", "state_in", "state_out"):
        assert tail(**{name: None}) == BAD, name
    assert tail(state_out=hip.ptr(st[0])) == BAD and tail(hist_out=hip.ptr(hist[0])) == BAD and tail(hist_in=None) == BAD
    assert tail(row_mul=0) == BAD and tail(row_mul=3) == BAD and tail(state_ss=words - 1) == BAD and tail(hist_ss=92) == BAD
    for over in (dict(B=1), dict(B=9), dict(D=0), dict(D=17), dict(K=0), dict(K=12), dict(Cin=18), dict(Cin=0), dict(Cin=516),
                 dict(w=None), dict(hist_ss=97), dict(in_=hip.ptr(bufs["x"]) + 4), dict(w=hip.ptr(bufs["w"]) + 8),
                 dict(out=hip.ptr(bufs["out"]) + 4), dict(state_in=hip.ptr(st[0]) + 4), dict(state_out=hip.ptr(st[1]) + 4),
                 dict(poly=hip.ptr(bufs["poly"]) + 4), dict(hist_in=hip.ptr(hist[0]) + 4)):
        assert tail(**over) == UNS, over
    assert tail(S=0) == 0 and tail(Tq=0) == 0 and tail(S=-1) == 0  # nothing to do is not an error, and nothing is launched
    assert bool((bufs["out"] == SENT).all()) and bool((bufs["em"] == -5).all()), "a refused call wrote its output"
    assert bool((st[1] == -99.0).all()) and bool((hist[1] == -99.0).all()), "a refused call wrote its state"
    assert tail() == 0
    assert not bool((bufs["out"] == SENT).any()) and bufs["em"].tolist() == [0, 0] and not bool((hist[1] == -99.0).any())
    assert st[1].cpu().view(torch.int32)[:, words - 1].tolist() == [D, D]
    assert tail(w=None, Cin=4, in_=hip.ptr(bufs["x"])) == 0  # the pass-through form takes Cin == B
    # the wrapper: declined shapes are False, bad arguments raise
    kw = dict(S=2, Tq=8, Cin=16, K=7, hist_ss=96, state_ss=ss)
    assert hip.mb_tail(bufs["x"], hist[0], hist[1], bufs["w"], bufs["poly"], st[0], st[1], bufs["out"], B=9, D=D, **kw) is False
    with pytest.raises(RuntimeError):
        hip.mb_tail(bufs["x"], hist[0], hist[1], bufs["w"], bufs["poly"], st[0], st[0], bufs["out"], B=4, D=D, **kw)
    with pytest.raises(ValueError):
        hip.mb_tail(bufs["x"], hist[0], hist[1], bufs["w"], bufs["poly"], st[0], st[1], bufs["out"], B=4, D=D,
                    last=torch.zeros(3, dtype=torch.int32).to(device), **kw)


def test_mb_emit_is_the_table():
    import kantts._hip as hip

    D = 8
    assert hip.mb_emit(0, 5, 0, D) == (0, 5) and hip.mb_emit(5, 11, 0, D) == (8, 8) and hip.mb_emit(8, 3, 0, D) == (3, 8)
    assert hip.mb_emit(8, 13, 1, D) == (21, 0) and hip.mb_emit(3, 0, 1, D) == (3, 0) and hip.mb_emit(0, 0, 1, D) == (0, 0)
    assert hip.mb_emit(3, 0, 0, D) == (0, 3) and hip.mb_emit(8, 10 ** 9, 0, D) == (10 ** 9, 8)
    assert hip.mb_state_words(8, 4) == 65


def test_mb_struct_layout_matches_the_header(tmp_path):
    """MbTailArgs and the state size against gcc's view of include/kantts_hip.h."""
    import kantts._hip as hip

    cname = "kantts_mb_tail_args"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "kantts_hip.h"', 'int main(void) {',
             '  printf("words %d\\n", KANTTS_MB_STATE_WORDS(8, 4));', '  printf("sizeof %%zu\\n", sizeof(%s));' % cname]
    for fname, _ in hip.MbTailArgs._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(%s, %s));' % (fname, cname, "in" if fname == "in_" else fname))
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    c_layout = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(c_layout["words"]) == hip.mb_state_words(8, 4)
    assert ctypes.sizeof(hip.MbTailArgs) == int(c_layout["sizeof"])
    for fname, _ in hip.MbTailArgs._fields_:
        assert getattr(hip.MbTailArgs, fname).offset == int(c_layout[fname]), fname


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("name", sorted(_CASES))
def test_mb_tail_kernel_source_matches_fp64_torch(name, S):
    with kernel_source_on_cpu():
        _check_tail("cpu", name, S)


def test_mb_tail_pass_through_matches_the_reference_fixture():
    with kernel_source_on_cpu():
        _check_pass_through("cpu")


def test_mb_tail_slots_are_independent():
    with kernel_source_on_cpu():
        _check_slots("cpu")


def test_mb_tail_many_tiles():
    with kernel_source_on_cpu():
        _check_many_tiles("cpu")


def test_mb_tail_return_codes():
    with kernel_source_on_cpu():
        _check_codes("cpu")


# ---------------------------------------------------------------------------------------------------------------------
# (e) model level
_GMB = dict(out_channels=4, channels=64, upsample_scales=[4, 2], upsample_kernal_sizes=[8, 4])
_HOP = 32  # 4 * 2 * 4 sub-bands


def _gmb():
    from kantts.models.hifigan.hifigan import Generator

    torch.manual_seed(0)
    return Generator(**_GMB).eval()


def _play_model(v, x, sched):
    """x (slots, 80, T) in lockstep, `last` on the final chunk -> (slots, T * hop); checks counts and the silent tail."""
    import kantts._hip as hip

    parts, t0, pend = [], 0, [0] * v.slots
    for i, Tc in enumerate(sched):
        final = i == len(sched) - 1
        wav = v.step(x[:, :, t0:t0 + Tc].contiguous(), last=[1] * v.slots if final else None)
        assert wav.shape == (v.slots, 1, Tc * v.hop + v.D * v.B)
        e, p = hip.mb_emit(pend[0], Tc * v.low_hop, final, v.D)
        pend = [p] * v.slots
        assert v.counts == [e * v.B] * v.slots and v.pending == pend
        assert not bool(wav[:, :, e * v.B:].any())
        parts.append(wav[:, 0, :e * v.B].cpu())
        t0 += Tc
    return torch.cat(parts, dim=1)


def _model_reference(G, x):
    """hifigan_oracle.generator, then the fp64 synthesis: (2, T * hop)"""
    P = {k: v.detach().clone().cpu() for k, v in G.state_dict().items()}
    with torch.no_grad():
        sub = H.generator(P, x.cpu(), scales=(4, 2))
    assert sub.shape[1] == 4
    return _synthesis64(_bank()[0], sub.transpose(1, 2))


_LENS = [8, 3, 13, 1, 6]


def _check_model(device, mode, graphs, many_lens=_LENS):
    import kantts._hip as hip
    from kantts.models.hifigan.chunked_mb import ChunkedMBVocoder
    from kantts.models.pqmf import PQMF

    _, W, D = _bank()
    g_mean = _gains(W)[1]
    assert abs(g_mean - 1.69) < 0.01
    rep = {}
    hip.set_precision(mode)
    try:
        G, pq = _gmb().to(device), PQMF().to(device)
        x = torch.randn(2, 80, 8, generator=torch.Generator().manual_seed(1)).to(device)
        ref = _model_reference(G, x)
        vs = [ChunkedMBVocoder(G, pqmf=pq, slots=2, graph=gr) for gr in graphs]
        assert vs[0].hop == _HOP and vs[0].low_hop == 8 and vs[0].D == 8 and vs[0].B == 4
        plays = {}
        for v in vs:
            for sched in ([3, 1, 4], [8]):
                v.reset()
                wav = _play_model(v, x, sched)
                assert wav.shape == ref.shape == (2, 8 * _HOP)
                plays[(v.graph, tuple(sched))] = wav
        first = plays[(vs[0].graph, (3, 1, 4))]
        for key, wav in plays.items():
            assert torch.equal(wav, first), ("chunkings / graph and eager runs must give identical bits", key)
        err = (first.double() - ref).abs()
        rep["mean_abs"], rep["g_mean"] = float(err.mean()), g_mean
        mask = torch.zeros(err.shape[-1], dtype=torch.bool)
        for b in (3 * _HOP, 4 * _HOP):  # the boundaries of [3, 1, 4]
            mask[b:b + D * 4 + 256] = True
        rep["boundary_max"] = float(err[:, mask].max())
        if device != "cpu":  # the one-shot device path against the same oracle, in the same run
            with torch.no_grad():
                one = pq.synthesis(G(x)).reshape(2, -1).cpu()
            rep["one_shot_max"] = float((one.double() - ref).abs().max())
        print("chunked multi-band generator", mode, device, rep)
        # continuous batching: utterances of other lengths through 2 slots equal synthesize of each
        utts = [torch.randn(80, n, generator=torch.Generator().manual_seed(10 + i)).to(device) for i, n in enumerate(many_lens)]
        for v in vs:
            parts = {}
            for i, wav in v.play_many(utts, chunk_frames=4):
                assert wav.shape[-1] > 0
                parts.setdefault(i, []).append(wav.cpu())
            for i, u in enumerate(utts):
                got = torch.cat(parts[i], dim=1)
                assert got.shape == (1, u.shape[1] * _HOP), (i, got.shape)
                want = torch.cat([c.cpu() for c in v.synthesize(u, chunk_frames=4, slot=1)], dim=1)
                assert torch.equal(got, want), "play_many utterance %d differs from synthesize" % i
            assert v.pending == [0] * v.slots
        if len(vs) > 1:
            a = torch.cat([c.cpu() for c in vs[0].synthesize(utts[0], chunk_frames=3)], dim=1)
            b = torch.cat([c.cpu() for c in vs[1].synthesize(utts[0], chunk_frames=5)], dim=1)
            assert torch.equal(a, b)
        # flush(): what the slots hold back after three frames
        v = vs[0]
        v.reset()
        head = v.step(x[:, :, :3].contiguous())
        tail = v.flush()
        assert v.counts == [D * 4] * 2 and tail.shape == (2, 1, _HOP + D * 4)
        assert v.flush() is not None and v.counts == [0, 0]
        assert torch.cat([head[:, 0, :3 * _HOP - D * 4], tail[:, 0, :D * 4]], dim=1).shape == (2, 3 * _HOP)
    finally:
        hip.set_precision("fp32")
        _record("model_%s_%s" % (mode, device), rep)
    if mode == "fp32":
        assert rep["mean_abs"] <= 1e-5 * g_mean, rep
    else:
        assert rep["mean_abs"] <= 2e-3 * g_mean, rep
        if "one_shot_max" in rep:
            assert rep["boundary_max"] <= 2 * rep["one_shot_max"], rep


def test_chunked_mb_generator_kernel_source_matches_oracle():
    with kernel_source_on_cpu():
        _check_model("cpu", "fp32", [False], many_lens=[3, 1, 5])


def test_chunked_mb_refusals():
    import kantts._hip as hip
    import kantts._hip.ops as ops
    import kantts._hip.ops_bf16 as ops_bf16
    from kantts.models.hifigan.chunked import ChunkedVocoder
    from kantts.models.hifigan.chunked_mb import ChunkedMBVocoder
    from kantts.models.hifigan.hifigan import Generator
    from kantts.models.pqmf import PQMF

    class _NoLaunch:
        def __getattr__(self, name):
            raise AssertionError("a refusal must not reach the library (%s)" % name)

    saved = [(m, m.lib) for m in (hip, ops, ops_bf16)]
    for m, _ in saved:
        m.lib = lambda: _NoLaunch()
    try:
        G, pq = _gmb(), PQMF()
        with pytest.raises(NotImplementedError):
            ChunkedVocoder(G, graph=False)  # the base class keeps refusing multi-band generators
        with pytest.raises(ValueError):
            ChunkedMBVocoder(G, graph=False)  # no pqmf given, none attached
        single = dict(_GMB, out_channels=1)
        with pytest.raises(ValueError):
            ChunkedMBVocoder(Generator(**single).eval(), pqmf=pq, graph=False)
        nsf = dict(_GMB, in_channels=80, nsf_params={"nb_harmonics": 7, "sampling_rate": 16000})
        with pytest.raises(NotImplementedError):
            ChunkedMBVocoder(Generator(**nsf).eval(), pqmf=pq, graph=False)
        with pytest.raises(ValueError):
            ChunkedMBVocoder(G, pqmf=PQMF(subbands=2), graph=False)
        with pytest.raises(ValueError):
            ChunkedMBVocoder(Generator(causal=False, **_GMB).eval(), pqmf=pq, graph=False)
        with pytest.raises(ValueError):
            ChunkedMBVocoder(Generator(**_GMB), pqmf=pq, graph=False)  # training mode
        with pytest.raises(NotImplementedError):  # conv_post with 2 input channels
            ChunkedMBVocoder(Generator(out_channels=4, channels=32).eval(), pqmf=pq, graph=False)
        with pytest.raises(NotImplementedError):  # a look-ahead of 31 rows
            ChunkedMBVocoder(Generator(**dict(_GMB, out_channels=2)).eval(), pqmf=PQMF(subbands=2, taps=124), graph=False)
    finally:
        for m, f in saved:
            m.lib = f


def test_chunked_mb_says_so_under_the_emulated_abi():
    from kantts.models.hifigan.chunked_mb import ChunkedMBVocoder
    from kantts.models.pqmf import PQMF
    from util import emulation

    with emulation():
        with pytest.raises(RuntimeError, match="kantts_mb_tail_rows"):
            ChunkedMBVocoder(_gmb(), pqmf=PQMF(), graph=False)


def _check_step_arguments(device, graph):
    from kantts.models.hifigan.chunked_mb import ChunkedMBVocoder
    from kantts.models.pqmf import PQMF

    G = _gmb().to(device)
    G.pqmf = PQMF().to(device)  # as infer_hifigan.load_model attaches it
    v = ChunkedMBVocoder(G, slots=2, graph=graph)
    x = torch.randn(2, 80, 4, generator=torch.Generator().manual_seed(2)).to(device)
    for bad in ([1], [0, 1, 0], torch.zeros(2), torch.zeros(3, dtype=torch.int32)):
        with pytest.raises(ValueError):
            v.step(x, last=bad)
    assert v._parity == 0
    a = v.step(x, rows=[4, 2], last=[0, 1])
    assert v.counts == [(32 - 8) * 4, 16 * 4] and v.pending == [8, 0]
    w = ChunkedMBVocoder(G, slots=2, graph=graph)
    b = w.step(x, rows=torch.tensor([4, 2], dtype=torch.int32).to(device), last=torch.tensor([False, True]).to(device))
    assert torch.equal(a, b)
    if device != "cpu":
        assert w.counts is None and w.pending is None
        with pytest.raises(RuntimeError):
            next(w.synthesize(x[0], chunk_frames=4))
        w.reset()
        assert w.pending == [0, 0]
    with pytest.raises(IndexError):
        v.flush(2)
    tail = v.flush(0)
    assert v.counts == [8 * 4, 0] and not bool(tail[1].any())


def _check_bool_rows(device):
    """A HOST bool tensor is taken as ``rows`` (0 / 1 frames per slot), as it always was; a bool tensor on the device reaches
    the base class and is refused, like every bool tensor given to ``ChunkedVocoder.step``."""
    from kantts.models.hifigan.chunked_mb import ChunkedMBVocoder
    from kantts.models.pqmf import PQMF

    G = _gmb().to(device)
    x = torch.randn(2, 80, 4, generator=torch.Generator().manual_seed(2)).to(device)
    v, w = (ChunkedMBVocoder(G, pqmf=PQMF().to(device), slots=2, graph=False) for _ in range(2))
    a = v.step(x, rows=[1, 0], last=[1, 0])
    b = w.step(x, rows=torch.tensor([True, False]), last=[1, 0])
    assert torch.equal(a, b) and v.counts == w.counts
    if device != "cpu":
        with pytest.raises(ValueError):
            w.step(x, rows=torch.tensor([True, False]).to(device))


def test_chunked_mb_bool_rows():
    with kernel_source_on_cpu():
        _check_bool_rows("cpu")


@pytest.mark.gpu
def test_chunked_mb_bool_rows_gpu():
    _check_bool_rows("cuda")


def test_chunked_mb_step_arguments():
    with kernel_source_on_cpu():
        _check_step_arguments("cpu", False)


def _write_voice(tmp_path):
    import numpy as np
    import yaml

    from kantts.models.hifigan.hifigan import Generator

    voc_dir = tmp_path / "voc" / "ckpt"
    voc_dir.mkdir(parents=True)
    (tmp_path / "voc" / "config.yaml").write_text(yaml.dump(
        {"Model": {"Generator": {"params": _GMB}}, "audio_config": {"sampling_rate": 16000}}))
    torch.manual_seed(0)
    torch.save({"model": {"generator": Generator(**_GMB).state_dict()}}, voc_dir / "checkpoint_1.pth")
    mel_dir = tmp_path / "feats"
    mel_dir.mkdir()
    lengths = {"utt_a": 9, "utt_b": 1, "utt_c": 6}
    for i, (name, n) in enumerate(lengths.items()):
        np.save(mel_dir / (name + ".npy"), torch.randn(n, 80, generator=torch.Generator().manual_seed(40 + i)).numpy())
    return str(voc_dir / "checkpoint_1.pth"), str(mel_dir), lengths


def _check_cli(tmp_path, one_shot):
    import numpy as np
    from scipy.io import wavfile

    from kantts.bin.infer_hifigan import main

    ck, mel_dir, lengths = _write_voice(tmp_path)
    main(["--ckpt", ck, "--input_mel", mel_dir, "--output_dir", str(tmp_path / "one"), "--chunk_frames", "4"])
    main(["--ckpt", ck, "--input_mel", mel_dir, "--output_dir", str(tmp_path / "two"), "--chunk_frames", "4", "--slots", "2"])
    if one_shot:
        main(["--ckpt", ck, "--input_mel", mel_dir, "--output_dir", str(tmp_path / "whole")])
    for name, n in lengths.items():
        a, b = (wavfile.read(tmp_path / k / (name + "_gen.wav"))[1] for k in ("one", "two"))
        assert a.dtype == b.dtype == np.int16 and a.shape == b.shape == (n * _HOP,)
        assert np.array_equal(a, b), "one slot and two slots differ: " + name
        if one_shot:  # the same number of samples as the whole-utterance path, and the same audio up to fp32 rounding
            c = wavfile.read(tmp_path / "whole" / (name + "_gen.wav"))[1]
            assert c.shape == a.shape and int(np.abs(a.astype(np.int32) - c.astype(np.int32)).max()) <= 2, name


def test_infer_hifigan_chunked_multiband_cli(tmp_path, monkeypatch):
    import kantts._hip as hip
    from kantts.bin import infer_hifigan

    hip.set_precision("fp32")
    monkeypatch.setattr(infer_hifigan, "_device", lambda: torch.device("cpu"))
    with kernel_source_on_cpu():
        _check_cli(tmp_path, one_shot=False)


# ---------------------------------------------------------------------------------------------------------------------
# (f) GPU
@pytest.mark.gpu
def test_mb_tail_gpu():
    for name in sorted(_CASES):
        for S in (1, 3):
            _check_tail("cuda", name, S)
    _check_pass_through("cuda")
    _check_slots("cuda")
    _check_codes("cuda")


@pytest.mark.gpu
def test_mb_tail_many_tiles_gpu():
    """Tiles of 256 - 2 D = 240 output rows: nine per slot in one call, and cuts in the middle of a tile -- the tile halos
    and the state must agree bit for bit."""
    _check_many_tiles("cuda")


def _check_many_tiles(device):
    Cin, K, B, taps, S, T = 32, 7, 4, 62, 4, 2048
    x, Wc, b, w_kbc = _conv_inputs(S, T, Cin, K, B, seed=9)
    pq, W, D = _bank(B, taps)
    one = _Tail(device, B, taps, S, w_kbc, b)
    cut = _Tail(device, B, taps, S, w_kbc, b)
    a, _ = _play(one, x, [T])
    c, counts = _play(cut, x, [700, 5, 1343], use_rows=True)
    assert counts == [(700 - D) * B, 5 * B, (1343 + D) * B]  # samples
    assert torch.equal(a, c)
    assert torch.equal(one.words_of(one.par), cut.words_of(cut.par))
    err = float((a.double() - _tail64(pq, x, Wc, b)).abs().max())
    print("mb tail, 2048 rows: max-abs", err)
    assert err <= 2e-5 * _gains(W)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_chunked_mb_generator_gpu_matches_oracle(mode):
    _check_model("cuda", mode, [True, False])


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [True, False])
def test_chunked_mb_step_arguments_gpu(graph):
    _check_step_arguments("cuda", graph)


@pytest.mark.gpu
def test_infer_hifigan_chunked_multiband_cli_gpu(tmp_path):
    import kantts._hip as hip

    hip.set_precision("fp32")
    _check_cli(tmp_path, one_shot=True)
