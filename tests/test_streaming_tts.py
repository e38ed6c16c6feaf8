"""Symbols to waveform on the device: the hand-over kernel (csrc/handover.hip, kantts_mel_handover_rows), the pipeline built
on it (kantts/models/streaming.py, StreamingTTS over AcousticSlots and the chunked vocoders) and its entry point
(kantts/bin/text_to_wav.py).

Every kernel-level and model-level case runs twice, as tests/test_acoustic_slots.py does: on the host build of the kernel
SOURCES (util.kernel_source_on_cpu, graph=False -- the emulated C ABI of oracle/ has no hand-over entry point) and, marked
``gpu``, on the device.

Kernel level: against torch indexing and the project's own ``infer_sambert.denorm_f0`` bit for bit.  ``src`` is NaN outside
every slot's clamped window and ``out`` is NaN before the launch, so a read outside a window or an element left unwritten
shows.  The f0 de-normalisation must round product and sum separately: the test first shows on the CPU that a fused
multiply-add would give other bits for at least one element of its draw.

Pipeline level: every audio chunk against a twin driven by the test -- a fresh vocoder of the same class, slots and seed,
fed with torch indexing (and host ``denorm_f0``) from the acoustic results at the pipeline's own cuts -- bit for bit; the
schedule read off the recorded steps; the acoustic half against ``forward`` at batch 1 within the bounds of
tests/test_acoustic_slots.py.  Equality across DIFFERENT cuts is not claimed (the convolutions do not promise it)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import test_acoustic_slots as _as
import test_chunked_acoustic as _ca
import torch_oracle as O
from test_chunked_acoustic import LEGS, _leg
from test_chunked_nsf import _GNSF, _gnsf
from test_chunked_vocoder import _G64, _g64
from util import ROOT, emulation

_NAN = float("nan")
_E_BADARG, _E_UNSUPPORTED = -1, -2  # include/kantts_hip.h
_SCALE, _OFFSET, _FLOOR, _UVT = 137.5, 211.25, 30.0, 0.6
_HOP = 8  # both 64-channel generators: upsample_scales [4, 2]


def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def _denorm(rows, scale=_SCALE, offset=_OFFSET, floor=_FLOOR, uvt=_UVT):
    """infer_sambert.denorm_f0 on a copy of (n, C) fp32 rows, as a tensor."""
    from kantts.bin.infer_sambert import denorm_f0

    a = np.array(rows.detach().cpu().numpy(), dtype=np.float32, copy=True)
    out = torch.from_numpy(denorm_f0(a, scale, offset, f0_threshold=floor, uv_threshold=uvt))
    assert out.dtype == torch.float32
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1. kernel level
_S, _T = 3, 40


def _launches(Tc):
    """(start, rows) per launch, one value per slot: non-zero starts; counts of 0, partial, Tc, Tc + 7 and -2; a window that
    runs past T; starts below 0 and above T."""
    return [([3, 0, 17], [0, max(Tc // 2, 1), Tc]),
            ([5, _T - 2, 11], [Tc + 7, Tc + 7, -2]),
            ([-4, _T + 3, _T - 1], [Tc, 3, 5])]


def _window(a, n, Tc):
    a = min(max(a, 0), _T)
    return a, min(min(max(n, 0), Tc), _T - a)


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("nsf", [0, 1], ids=["plain", "nsf"])
@pytest.mark.parametrize("Tc", [1, 5, 24, 37])  # 37: more than one tile of 32 frames
@pytest.mark.parametrize("C", [80, 82])         # 80: the 16-byte loads; 82: 4-byte loads and a second tile of 64 channels
def test_handover_equals_torch_and_denorm_f0(C, Tc, nsf, leg):
    import kantts._hip as hip

    ctx, dev = _leg(leg)
    g = torch.Generator().manual_seed(1000 + 10 * C + Tc)
    fused_differs = hit_floor = above_floor = voiced = unvoiced = False
    with ctx:
        for k, (start, rows) in enumerate(_launches(Tc)):
            src = torch.full((_S, _T, C), _NAN)
            for s in range(_S):
                a, n = _window(start[s], rows[s], Tc)
                src[s, a:a + n] = torch.randn(n, C, generator=g)
            if k == 0 and Tc > 1:
                src[2, 17 + 1, C - 1] = _UVT  # a voicing score exactly at the threshold (fp32(0.6) on both sides): voiced
            want = torch.zeros(_S, C, Tc)
            for s in range(_S):
                a, n = _window(start[s], rows[s], Tc)
                live = src[s, a:a + n]
                if nsf and n:
                    v = live[:, C - 2]
                    sep = v * _SCALE + _OFFSET  # two fp32 roundings, as numpy's
                    fma = (v.double() * _SCALE + _OFFSET).float()  # one rounding: what a fused multiply-add returns
                    assert torch.equal(sep, torch.from_numpy(v.numpy() * _SCALE + _OFFSET))
                    fused_differs |= bool(((sep != fma) & (sep > _FLOOR) & (fma > _FLOOR)).any())
                    live = _denorm(live)
                    hit_floor |= bool((live[:, C - 2] == _FLOOR).any())
                    above_floor |= bool((live[:, C - 2] > _FLOOR).any())
                    voiced |= bool((live[:, C - 1] == 1).any())
                    unvoiced |= bool((live[:, C - 1] == 0).any())
                    if k == 0 and Tc > 1 and s == 2:
                        assert float(live[1, C - 1]) == 1.0, "a score at the threshold is voiced"
                want[s, :, :n] = live.t()
            out = torch.full((_S, C, Tc), _NAN, device=dev)
            rc = hip.mel_handover(src.to(dev), _i32(start, dev), _i32(rows, dev), out,
                                  nsf=(_SCALE, _OFFSET) if nsf else None, f0_floor=_FLOOR, uv_threshold=_UVT)
            assert rc == 0
            out = out.cpu()
            assert not bool(torch.isnan(out).any()), (k, "an element of out was not written, or NaN was read")
            assert torch.equal(out, want), (k, start, rows)
    if nsf and Tc >= 5:  # the draw exercises what it is meant to: a fused multiply-add cannot pass, every branch is taken
        assert fused_differs, "no element of the draw tells the fused product-sum from the separately rounded one"
        assert hit_floor and above_floor and voiced and unvoiced


@pytest.mark.parametrize("leg", LEGS)
def test_handover_return_codes(leg):
    import kantts._hip as hip

    ctx, dev = _leg(leg)
    S, T, C, Tc = 2, 9, 8, 4
    with ctx:
        src = torch.randn(S, T, C).to(dev)
        start, rows = _i32([0, 1], dev), _i32([4, 2], dev)
        out = torch.full((S, C, Tc), _NAN, device=dev)
        L = hip.lib()

        def call(src_=src, start_=start, rows_=rows, out_=out, S_=S, T_=T, C_=C, Tc_=Tc, nsf=0):
            return L.kantts_mel_handover_rows(hip.ptr(src_), hip.ptr(start_), hip.ptr(rows_), hip.ptr(out_), S_, T_, C_, Tc_,
                                              nsf, 1.0, 0.0, 30.0, 0.6, hip.stream())

        for bad in (dict(src_=None), dict(start_=None), dict(rows_=None), dict(out_=None), dict(S_=-1), dict(Tc_=-1),
                    dict(T_=0), dict(C_=0), dict(C_=2, nsf=1)):
            assert call(**bad) == _E_BADARG, bad
        assert call(S_=65536) == _E_UNSUPPORTED
        assert call(S_=0) == 0 and call(Tc_=0) == 0
        assert _ca._all_nan(out.cpu()), "a refused or empty call must not write"
        assert call(C_=3, T_=T * C // 3, nsf=1) == 0 and call() == 0  # the smallest NSF width; then the case as it stands
        want = torch.zeros(S, C, Tc)
        want[0] = src[0, 0:4].t().cpu()
        want[1, :, :2] = src[1, 1:3].t().cpu()
        assert torch.equal(out.cpu(), want)


# ---------------------------------------------------------------------------------------------------------------------
# 2. pipeline level
_UTT82 = {}


def _utterances82(leg, dev):
    """tests/test_acoustic_slots.py::_utterances for an NSF acoustic model: the tiny SAM-BERT of
    tests/test_chunked_acoustic.py::_tiny_model(dur_bias=1.5) built with num_mels = 82 (80 mel bins, f0, voicing)."""
    if leg not in _UTT82:
        from kantts.models.sambert.kantts_sambert import KanTtsSAMBERT

        torch.manual_seed(0)
        m = KanTtsSAMBERT(dict(O.sambert_config(tiny=True), num_mels=82))
        with torch.no_grad():
            for n, p in m.named_parameters():
                if n.endswith("bias") or "layer_norm" in n or n.endswith("ln.weight"):
                    p.add_(0.1 * torch.randn_like(p))
            m.variance_adaptor.duration_predictor.fc.bias.fill_(1.5)
        m = m.to(dev).eval()
        m.mel_decoder.decode_mode = "kernel"
        batch = _ca._inputs(dev, "durations")
        utts = [{k: v[i:i + 1].contiguous() for k, v in batch.items()} for i in range(3)]
        utts.append({k: v[0:1].contiguous() for k, v in _ca._inputs(dev, "free").items()})
        with torch.no_grad():
            refs = [m(**u) for u in utts]
        assert m.mel_decoder._decode_kernel is not None, "the one-shot side did not take the one-launch decoder"
        assert [int(r["LR_length_rounded"][0]) for r in refs[:3]] == [96, 45, 6]
        _UTT82[leg] = (m, batch, utts, refs)
    return _UTT82[leg]


def _nsf_settings(refs):
    """(nsf, f0_threshold, uv_threshold) that make the handed-over frames take every branch of the kernel: the voicing
    threshold is the median of the one-shot forward's voicing channel, the f0 floor the median of its de-normalised f0."""
    live = torch.cat([r["postnet_outputs"][0, :int(r["LR_length_rounded"][0])].cpu() for r in refs])
    return (_SCALE, _OFFSET), float((live[:, -2] * _SCALE + _OFFSET).median()), float(live[:, -1].median())


def _setup(leg, dev, nsf):
    """(model, utterances, one-shot references, generator, StreamingTTS keywords) of a kind, inside the leg's context."""
    if nsf:
        m, _, utts, refs = _utterances82(leg, dev)
        G = _gnsf().to(dev)
        scale_offset, floor, uvt = _nsf_settings(refs)
        kw = dict(nsf=scale_offset, f0_threshold=floor, uv_threshold=uvt, seed=5)
    else:
        m, _, utts, refs = _as._utterances(leg, dev)
        G = _g64().to(dev)
        kw = {}
    kw["graph"] = dev == "cuda"
    return m, utts, refs, G, kw


def _feats(kw, rows):
    return _denorm(rows, kw["nsf"][0], kw["nsf"][1], kw["f0_threshold"], kw["uv_threshold"]) if "nsf" in kw else rows.cpu()


class _Recorder:
    """Wraps a pipeline's own step, its pool's step and its vocoder's step to record what they did."""

    def __init__(self, tts):
        self.tts, self.steps, self.voc_calls = tts, [], 0
        self._hi = None
        pool_step, voc_step, step = tts.pool.step, tts.vocoder.step, tts.step

        def rec_pool(counts, capacity=None):
            outs = pool_step(counts, capacity=capacity)
            self._hi = [None if o is None else o[1] for o in outs]
            return outs

        def rec_voc(*a, **k):
            self.voc_calls += 1
            return voc_step(*a, **k)

        def rec_step():
            before = self.voc_calls
            outs = step()
            self.steps.append(dict(outs=[None if o is None else (o[0], o[1], o[2], o[3].clone()) for o in outs],
                                   hi=list(self._hi), voc=self.voc_calls - before))
            return outs

        tts.pool.step, tts.vocoder.step, tts.step = rec_pool, rec_voc, rec_step


def _check_schedule_and_twin(rec, results, frames, twin, kw, Tc, C):
    """The recorded steps against the documented schedule, and every chunk against the twin vocoder."""
    S = len(rec.steps[0]["outs"])
    pos, occupant, total = {}, [None] * S, {}
    seen_floor = seen_above = seen_v = seen_u = False
    for k, st in enumerate(rec.steps):
        buf = torch.zeros(S, C, Tc)
        ns = [0] * S
        for s, o in enumerate(st["outs"]):
            if o is None:
                continue
            index, lo, n, wav = o
            if occupant[s] != index:  # an utterance starts in slot s
                assert index not in pos and lo == 0, (k, s, index)
                if occupant[s] is not None:
                    twin.reset(s)
                twin._assign(s, index)
                occupant[s], pos[index] = index, 0
            assert lo == pos[index], (k, s, lo, pos[index])
            final = min(st["hi"][s], frames[index])
            assert n == min(Tc, final - lo), (k, s, "a slot with final frames pending must hand over what fits", n, final, lo)
            assert tuple(wav.shape) == (1, n * _HOP), (k, s, tuple(wav.shape))
            pos[index] = lo + n
            ns[s] = n
            if n:
                rows = _feats(kw, results[index]["postnet_outputs"][0, lo:lo + n])
                buf[s, :, :n] = rows.t()
                if "nsf" in kw:
                    seen_floor |= bool((rows[:, -2] == kw["f0_threshold"]).any())
                    seen_above |= bool((rows[:, -2] > kw["f0_threshold"]).any())
                    seen_v |= bool((rows[:, -1] == 1).any())
                    seen_u |= bool((rows[:, -1] == 0).any())
        assert st["voc"] == (1 if any(ns) else 0), (k, ns, st["voc"])  # all rows zero: no vocoder step was launched
        if any(ns):
            want = twin.step(buf.to(twin.device), rows=ns)
            for s, o in enumerate(st["outs"]):
                if o is not None and ns[s]:
                    assert torch.equal(o[3], want[s, :, :ns[s] * _HOP]), (k, s, "differs from the hand-chained twin")
                    total[o[0]] = total.get(o[0], 0) + o[3].shape[-1]
    assert sorted(pos) == sorted(frames) and all(pos[i] == frames[i] for i in pos), (pos, frames)
    assert total == {i: n * _HOP for i, n in frames.items()}, total
    if "nsf" in kw:
        assert seen_floor and seen_above and seen_v and seen_u, "the handed-over frames must take every branch"


_PLAYED = {}


def _played(leg, dev, nsf, Tc):
    """All four utterances through a two-slot pipeline, once per (leg, kind, chunk): the recorder, the acoustic results,
    the chunks play_many yielded and what the test needs to build the twin."""
    key = (leg, nsf, Tc)
    if key not in _PLAYED:
        from kantts.models.streaming import StreamingTTS

        m, utts, refs, G, kw = _setup(leg, dev, nsf)
        tts = StreamingTTS(m, G, slots=2, max_steps=32, chunk_frames=Tc, **kw)
        rec = _Recorder(tts)
        results, chunks = {}, {}
        for index, first, wav in tts.play_many(utts, results=results):
            chunks.setdefault(index, []).append((first, wav.clone()))
        assert sorted(results) == [0, 1, 2, 3] and tts.pool.free_slots() == [0, 1] and tts.index == [None, None]
        _PLAYED[key] = (rec, results, chunks, refs, G, kw)
    return _PLAYED[key]


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("nsf,Tc", [(0, 3), (0, 15), (0, 96), (1, 3), (1, 15)],
                         ids=["plain-3", "plain-15", "plain-96", "nsf-3", "nsf-15"])
def test_streaming_tts_equals_the_hand_chained_twin(nsf, Tc, leg):
    import kantts._hip as hip
    from kantts.models.hifigan.chunked import ChunkedVocoder
    from kantts.models.hifigan.chunked_nsf import ChunkedNSFVocoder

    ctx, dev = _leg(leg)
    hip.set_precision("bf16")
    try:
        with ctx:
            rec, results, chunks, refs, G, kw = _played(leg, dev, nsf, Tc)
            frames = {i: int(r["LR_length_rounded"][0]) for i, r in enumerate(refs)}
            if nsf:
                twin = ChunkedNSFVocoder(G, slots=2, graph=kw["graph"], seed=kw["seed"])
            else:
                twin = ChunkedVocoder(G, slots=2, graph=kw["graph"])
            _check_schedule_and_twin(rec, results, frames, twin, kw, Tc, 82 if nsf else 80)
            # what play_many yields: the non-empty entries of the steps, in step and slot order
            flat = [(o[0], o[1] * _HOP, o[3]) for st in rec.steps for o in st["outs"] if o is not None and o[2] > 0]
            got = sorted(((i, f, w) for i, cs in chunks.items() for f, w in cs), key=lambda c: (c[0], c[1]))
            flat.sort(key=lambda c: (c[0], c[1]))
            assert len(flat) == len(got)
            for a, b in zip(flat, got):
                assert a[:2] == b[:2] and torch.equal(a[2], b[2])
            for i, n in frames.items():
                assert sum(w.shape[-1] for _, w in chunks[i]) == n * _HOP, i
                assert [f for f, _ in chunks[i]] == list(np.cumsum([0] + [w.shape[-1] for _, w in chunks[i]][:-1])), i
    finally:
        hip.set_precision("fp32")


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("nsf", [0, 1], ids=["plain", "nsf"])
def test_streaming_tts_leaves_the_acoustic_half_unchanged(nsf, leg):
    import kantts._hip as hip

    ctx, dev = _leg(leg)
    hip.set_precision("bf16")
    try:
        with ctx:
            _, results, _, refs, _, _ = _played(leg, dev, nsf, 15)
            for i, ref in enumerate(refs):
                got = results[i]
                assert set(got) == set(ref), i
                for k in _as._KEYS_EXACT:
                    assert torch.equal(got[k], ref[k]), (i, k)
                _as._twin_bounds(got["postnet_outputs"], ref["postnet_outputs"], "streaming utterance %d %s nsf=%d" % (i, leg, nsf))
    finally:
        hip.set_precision("fp32")


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("nsf", [0, 1], ids=["plain", "nsf"])
def test_streaming_tts_stale_occupant(nsf, leg):
    """Utterance B played in the slot pair utterance A has just left equals B played in a fresh pipeline (as utterance 1
    either way: an NSF voice keys its excitation by the index) bit for bit."""
    import kantts._hip as hip
    from kantts.models.streaming import StreamingTTS

    ctx, dev = _leg(leg)
    hip.set_precision("bf16")
    try:
        with ctx:
            m, utts, _, G, kw = _setup(leg, dev, nsf)
            for a, b in ((0, 1), (2, 3)):  # a longer occupant before a shorter one, and a shorter before a longer
                used = StreamingTTS(m, G, slots=1, max_steps=32, chunk_frames=15, **kw)
                first = [(f, w.clone()) for i, f, w in used.play_many([utts[a], utts[b]]) if i == 1]
                fresh = StreamingTTS(m, G, slots=1, max_steps=32, chunk_frames=15, **kw)
                fresh.admit(0, 1, utts[b])
                second, n_steps = [], 0
                while not fresh.done(0):
                    index, lo, n, wav = fresh.step()[0]
                    n_steps += 1
                    assert index == 1 and n_steps <= 40
                    if n:
                        second.append((lo * _HOP, wav.clone()))
                fresh.release(0)
                assert len(first) == len(second) and len(first) >= 1, (a, b, len(first), len(second))
                for (f0, w0), (f1, w1) in zip(first, second):
                    assert f0 == f1 and torch.equal(w0, w1), (a, b, f0, f1)
    finally:
        hip.set_precision("fp32")


@pytest.mark.parametrize("leg", LEGS)
def test_streaming_tts_refuses_what_it_cannot_play(leg):
    import kantts._hip as hip
    from kantts.models.hifigan.hifigan import Generator
    from kantts.models.streaming import StreamingTTS

    ctx, dev = _leg(leg)
    try:
        with ctx:
            hip.set_precision("bf16")
            m80, utts, _, G, kw = _setup(leg, dev, 0)
            m82, _, _, GN, kwn = _setup(leg, dev, 1)
            for bad in (None, 0, -3, 4, 16):  # outputs_per_step is 3
                with pytest.raises(ValueError, match="chunk_frames"):
                    StreamingTTS(m80, G, slots=2, max_steps=32, chunk_frames=bad, **kw)
            with pytest.raises(ValueError, match="num_mels"):
                StreamingTTS(m80, GN, slots=2, max_steps=32, chunk_frames=15, **kwn)
            with pytest.raises(ValueError, match="num_mels"):
                StreamingTTS(m82, G, slots=2, max_steps=32, chunk_frames=15, **kw)
            with pytest.raises(ValueError, match="nsf="):
                StreamingTTS(m82, GN, slots=2, max_steps=32, chunk_frames=15, graph=kw["graph"])
            with pytest.raises(ValueError, match="source module"):
                StreamingTTS(m80, G, slots=2, max_steps=32, chunk_frames=15, nsf=(_SCALE, _OFFSET), graph=kw["graph"])
            # what the underlying classes refuse comes through unchanged
            with pytest.raises(ValueError, match="causal"):
                StreamingTTS(m80, Generator(causal=False, **_G64).eval().to(dev), slots=2, max_steps=32, chunk_frames=15, **kw)
            with pytest.raises(ValueError, match="eval"):
                StreamingTTS(m80, Generator(**_G64).to(dev), slots=2, max_steps=32, chunk_frames=15, **kw)
            with pytest.raises(ValueError, match="slots and max_steps"):
                StreamingTTS(m80, G, slots=0, max_steps=32, chunk_frames=15, **kw)
            m80.train()
            try:
                with pytest.raises(ValueError, match="eval"):
                    StreamingTTS(m80, G, slots=2, max_steps=32, chunk_frames=15, **kw)
            finally:
                m80.eval()
            hip.set_precision("fp32")
            with pytest.raises(ValueError, match="bf16"):
                StreamingTTS(m80, G, slots=2, max_steps=32, chunk_frames=15, **kw)
            hip.set_precision("bf16")
            tts = StreamingTTS(m80, G, slots=2, max_steps=32, chunk_frames=15, **kw)
            assert tts.admit(1, 7, utts[2]) == 6
            with pytest.raises(ValueError, match="occupied"):
                tts.admit(1, 8, utts[1])
            with pytest.raises(ValueError, match="free"):
                tts.done(0)
            with pytest.raises(ValueError, match="every slot free"):
                next(tts.play_many([utts[1]]))
    finally:
        hip.set_precision("fp32")


def test_streaming_tts_says_so_under_the_emulated_abi():
    import kantts._hip as hip
    from kantts.models.streaming import StreamingTTS

    hip.set_precision("bf16")
    try:
        with emulation():
            assert not hip.handover_entry_points()
            with pytest.raises(RuntimeError, match="kantts_mel_handover_rows"):
                StreamingTTS(_ca._tiny_model("cpu"), _g64(), slots=2, max_steps=32, chunk_frames=15, graph=False)
    finally:
        hip.set_precision("fp32")


# ---------------------------------------------------------------------------------------------------------------------
# 3. entry point
_SR = 16000


def _write_voices(tmp_path, nsf):
    """A tiny AM voice and a tiny vocoder voice, the way the ``*_cli_gpu`` tests of the two halves write theirs."""
    from kantts.models.hifigan.hifigan import Generator
    from kantts.models.sambert.kantts_sambert import KanTtsSAMBERT

    cfg = dict(O.sambert_config(tiny=True), num_mels=82 if nsf else 80)
    am_dir = tmp_path / "am" / "ckpt"
    am_dir.mkdir(parents=True)
    params = {k: v for k, v in cfg.items() if k not in O.SAMBERT_VOCAB}
    if nsf:
        params.update(NSF=True, nsf_norm_type="mean_std")
        np.save(tmp_path / "am" / "mvn.npy", np.array([[_OFFSET], [_SCALE]], dtype=np.float32))  # rows: mean, std of f0
    config = {"model_type": "sambert", "Model": {"KanTtsSAMBERT": {
        "params": params,
        "optimizer": {"type": "Adam", "params": {"lr": 0.001, "betas": [0.9, 0.98], "eps": 1e-9, "weight_decay": 0.0}},
        "scheduler": {"type": "NoamLR", "params": {"warmup_steps": 4000}}}}, "grad_norm": 1.0, "batch_size": 2}
    (tmp_path / "am" / "config.yaml").write_text(yaml.dump(config))
    torch.manual_seed(0)
    m = KanTtsSAMBERT(dict(cfg))
    with torch.no_grad():
        m.variance_adaptor.duration_predictor.fc.bias.fill_(1.5)
    am_ck = str(am_dir / "checkpoint_1.pth")
    torch.save({"model": m.state_dict()}, am_ck)
    voc_dir = tmp_path / "voc" / "ckpt"
    voc_dir.mkdir(parents=True)
    gp = _GNSF if nsf else _G64
    (tmp_path / "voc" / "config.yaml").write_text(yaml.dump(
        {"Model": {"Generator": {"params": gp}}, "audio_config": {"sampling_rate": _SR}}))
    torch.manual_seed(0)
    voc_ck = str(voc_dir / "checkpoint_1.pth")
    torch.save({"model": {"generator": Generator(**gp).state_dict()}}, voc_ck)
    sym = tmp_path / "symbols.lst"
    sym.write_text("0_0\ta b c d e f g h i j k\n0_1\tg h i j\n1_0\ta b c d e f g\n")
    return cfg, am_ck, voc_ck, str(sym)


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


@pytest.mark.gpu
@pytest.mark.parametrize("nsf", [0, 1], ids=["plain", "nsf"])
def test_symbols_to_wav_cli_gpu(nsf, tmp_path):
    import kantts._hip as hip
    from kantts.bin import infer_hifigan, infer_sambert
    from kantts.bin.text_to_wav import symbols_to_wav
    from kantts.models.streaming import StreamingTTS
    from scipy.io import wavfile

    cfg, am_ck, voc_ck, sym = _write_voices(tmp_path, nsf)
    ids = ["0_0", "0_1", "1_0"]
    hip.set_precision("bf16")
    try:
        lu = _ca._FakeLingUnit(cfg)
        stats = symbols_to_wav(sym, str(tmp_path / "stream"), am_ck, voc_ck, chunk_frames=15, slots=2, slot_steps=64,
                               ling_unit=lu)
        print("symbols_to_wav nsf=%d chunk_frames=15 slots=2:" % nsf, stats)
        assert symbols_to_wav(sym, str(tmp_path / "whole"), am_ck, voc_ck, ling_unit=lu) is None
        # the same inputs and seed through the pipeline in this process
        device, _, se, scale_offset, fsnet = infer_sambert.load_am(am_ck, ling_unit=lu)
        G = infer_hifigan.load_model(voc_ck)
        G.remove_weight_norm()
        G = G.eval().to(device)
        tts = StreamingTTS(fsnet, G, slots=2, max_steps=64, chunk_frames=15, nsf=scale_offset, seed=0,
                           graph=device.type == "cuda")
        lines = [ln.split("\t") for ln in open(sym).read().splitlines()]
        with torch.no_grad():
            reqs = [infer_sambert.am_inputs(ln[1], lu, device, se=se) for ln in lines]
            parts = {}
            for index, _, wav in tts.play_many(reqs):
                parts.setdefault(index, []).append(wav.reshape(-1).cpu())
    finally:
        hip.set_precision("fp32")
    assert (scale_offset == (_SCALE, _OFFSET)) if nsf else scale_offset is None
    assert _files(tmp_path / "stream") == _files(tmp_path / "whole")
    assert [f for f in _files(tmp_path / "stream") if not f.startswith("feat")] == \
        sorted(["%s_mel_gen.wav" % i for i in ids] + ["res_wavs/0.wav", "res_wavs/1.wav"])
    n = {}
    for k, i in enumerate(ids):
        frames = np.load(tmp_path / "stream" / "feat" / (i + "_mel.npy")).shape[0]
        assert np.load(tmp_path / "whole" / "feat" / (i + "_mel.npy")).shape == (frames, 82 if nsf else 80)
        for run in ("stream", "whole"):
            sr, w = wavfile.read(tmp_path / run / (i + "_mel_gen.wav"))
            assert sr == _SR and w.dtype == np.int16 and w.shape == (frames * _HOP,), (run, i, w.shape, frames)
        n[i] = frames * _HOP
        y = torch.cat(parts[k]).numpy()
        want = (np.clip(y, -1.0, 1.0) * 32767.0).astype(np.int16)
        assert np.array_equal(wavfile.read(tmp_path / "stream" / (i + "_mel_gen.wav"))[1], want), i
    assert n["0_0"] > 15 * _HOP  # the first sentence spans several chunks
    for run in ("stream", "whole"):
        _, w0 = wavfile.read(tmp_path / run / "res_wavs" / "0.wav")
        _, w1 = wavfile.read(tmp_path / run / "res_wavs" / "1.wav")
        assert w0.shape == (n["0_0"] + n["0_1"] + int(0.28 * _SR) + int(0.05 * _SR),), (run, w0.shape)
        assert w1.shape == (n["1_0"] + int(0.05 * _SR),), (run, w1.shape)
        _, a = wavfile.read(tmp_path / run / "0_0_mel_gen.wav")
        _, b = wavfile.read(tmp_path / run / "0_1_mel_gen.wav")
        gap = int(0.28 * _SR)
        assert np.array_equal(w0[:len(a)], a) and not w0[len(a):len(a) + gap].any()
        assert np.array_equal(w0[len(a) + gap:len(a) + gap + len(b)], b) and not w0[len(a) + gap + len(b):].any()


def test_concat_process_joins_sub_sentences(tmp_path):
    from kantts.bin.text_to_wav import concat_process
    from scipy.io import wavfile

    rng = np.random.default_rng(0)
    waves = {"0_0": 400, "0_1": 30, "0_2": 77, "2_0": 120, "10_0": 5}
    for name, n in waves.items():
        wavfile.write(tmp_path / (name + "_mel_gen.wav"), _SR, rng.integers(-3000, 3000, n).astype(np.int16))
    wavfile.write(tmp_path / "stray.wav", _SR, np.zeros(9, dtype=np.int16))  # not a sub-sentence: left alone
    concat_process(str(tmp_path), str(tmp_path / "res_wavs"))
    assert sorted(os.listdir(tmp_path / "res_wavs")) == ["0.wav", "10.wav", "2.wav"]
    gap, end = int(0.28 * _SR), int(0.05 * _SR)
    sr, w = wavfile.read(tmp_path / "res_wavs" / "0.wav")
    assert sr == _SR and w.dtype == np.int16 and w.shape == (400 + 30 + 77 + 2 * gap + end,)
    parts = [wavfile.read(tmp_path / ("0_%d_mel_gen.wav" % k))[1] for k in range(3)]
    want = np.concatenate([parts[0], np.zeros(gap, np.int16), parts[1], np.zeros(gap, np.int16), parts[2],
                           np.zeros(end, np.int16)])
    assert np.array_equal(w, want)
    assert wavfile.read(tmp_path / "res_wavs" / "2.wav")[1].shape == (120 + end,)
    assert wavfile.read(tmp_path / "res_wavs" / "10.wav")[1].shape == (5 + end,)


def test_text_to_wav_without_the_front_end_and_help(tmp_path):
    from kantts.bin.text_to_wav import symbols_to_wav, text_to_wav

    with pytest.raises(NotImplementedError, match="symbols_to_wav"):
        text_to_wav(str(tmp_path / "t.txt"), str(tmp_path / "out"), str(tmp_path / "res.zip"), "am.pth", "voc.pth")
    assert not (tmp_path / "out").exists()
    with pytest.raises(ValueError, match="--slots"):
        symbols_to_wav(str(tmp_path / "s.lst"), str(tmp_path / "out"), "am.pth", "voc.pth", slots=2)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "kan-tts_amd"), os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-m", "kantts.bin.text_to_wav", "--help"], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "--symbols" in r.stdout and "--chunk_frames" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
