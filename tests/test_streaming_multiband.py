"""StreamingTTS with a multi-band voice: the acoustic slot pool feeding kantts.models.hifigan.chunked_mb.ChunkedMBVocoder.

Three utterances (96, 45 and 6 frames) of the tiny acoustic model of tests/test_streaming_tts.py through two slots, and a
hand-chained twin: a fresh ChunkedMBVocoder fed from the pool's results at the pipeline's own cuts, with `last` where the
pipeline must have set it (the step that hands over an utterance's last frame).  Every chunk is torch.equal with the
twin's: both run the same launches on the same frames.  GPU legs, and one leg on the host build of the kernel sources."""
import pytest
import torch

import test_acoustic_slots as _as
from test_chunked_multiband import _GMB
from test_streaming_tts import _Recorder


def _check(dev, Tc):
    import kantts._hip as hip
    from kantts.models.hifigan.chunked_mb import ChunkedMBVocoder
    from kantts.models.hifigan.hifigan import Generator
    from kantts.models.pqmf import PQMF
    from kantts.models.streaming import StreamingTTS

    m, _, utts, refs = _as._utterances("cuda" if dev == "cuda" else "hostsim", dev)
    utts, refs = utts[:3], refs[:3]
    frames = {i: int(r["LR_length_rounded"][0]) for i, r in enumerate(refs)}
    assert frames == {0: 96, 1: 45, 2: 6}
    torch.manual_seed(0)
    G = Generator(**_GMB).eval()  # in_channels 80: the acoustic model's num_mels
    G.pqmf = PQMF()  # as infer_hifigan.load_model attaches it
    G = G.to(dev)
    graph = dev == "cuda"
    tts = StreamingTTS(m, G, slots=2, max_steps=32, chunk_frames=Tc, graph=graph)
    assert isinstance(tts.vocoder, ChunkedMBVocoder)
    hop, B, D, low = tts.hop, tts.vocoder.B, tts.vocoder.D, tts.vocoder.low_hop
    assert hop == 32 and (B, D, low) == (4, 8, 8)
    rec = _Recorder(tts)
    results, chunks = {}, {}
    for index, first, wav in tts.play_many(utts, results=results):
        chunks.setdefault(index, []).append((first, wav.clone()))
    assert sorted(results) == [0, 1, 2]
    assert tts.pool.free_slots() == [0, 1] and tts.index == [None, None], "every slot must have been released"

    twin = ChunkedMBVocoder(G, slots=2, graph=graph)
    pos, occupant, total, pend, flat = {}, [None, None], {}, [0, 0], []
    for k, st in enumerate(rec.steps):
        buf = torch.zeros(2, 80, Tc)
        ns, last = [0, 0], [0, 0]
        for s, o in enumerate(st["outs"]):
            if o is None:
                continue
            index, lo, n, wav = o
            if occupant[s] != index:  # an utterance starts in slot s
                assert index not in pos and lo == 0, (k, s, index)
                if occupant[s] is not None:
                    twin.reset(s)
                occupant[s], pos[index], pend[s] = index, 0, 0
            assert lo == pos[index], (k, s, lo, pos[index])
            assert n == min(Tc, min(st["hi"][s], frames[index]) - lo), (k, s, n)
            pos[index] = lo + n
            ns[s], last[s] = n, int(n > 0 and lo + n == frames[index])
            if n:
                buf[s, :, :n] = results[index]["postnet_outputs"][0, lo:lo + n].cpu().t()
        assert st["voc"] == (1 if any(ns) else 0), (k, ns, st["voc"])
        if not any(ns):
            assert all(o is None or o[3].shape[-1] == 0 for o in st["outs"])
            continue
        want = twin.step(buf.to(twin.device), rows=ns, last=last)
        for s, o in enumerate(st["outs"]):
            if o is None:
                continue
            e, pend[s] = hip.mb_emit(pend[s], ns[s] * low, last[s], D) if ns[s] else (0, pend[s])
            assert twin.counts[s] == e * B and tuple(o[3].shape) == (1, e * B), (k, s, tuple(o[3].shape), e)
            assert torch.equal(o[3], want[s, :, :e * B]), (k, s, "differs from the hand-chained twin")
            if e:
                flat.append((o[0], total.get(o[0], 0), o[3]))
            total[o[0]] = total.get(o[0], 0) + e * B
            if last[s]:
                assert pend[s] == 0
    assert all(pos[i] == frames[i] for i in frames), (pos, frames)
    assert total == {i: n * hop for i, n in frames.items()}, total
    # what play_many yields: the non-empty chunks in step and slot order, first_sample the utterance's running sample count
    got = sorted(((i, f, w) for i, cs in chunks.items() for f, w in cs), key=lambda c: (c[0], c[1]))
    flat.sort(key=lambda c: (c[0], c[1]))
    assert len(flat) == len(got)
    for a, b in zip(flat, got):
        assert a[:2] == b[:2] and torch.equal(a[2], b[2])
    for i, n in frames.items():
        assert sum(w.shape[-1] for _, w in chunks[i]) == n * hop, i
        firsts, run = [f for f, _ in chunks[i]], 0
        for f, w in chunks[i]:
            assert f == run, (i, firsts)
            run += w.shape[-1]


def test_streaming_tts_multiband_equals_the_hand_chained_twin_kernel_source():
    import kantts._hip as hip
    from util import kernel_source_on_cpu

    hip.set_precision("bf16")
    try:
        with kernel_source_on_cpu():
            _check("cpu", 15)
    finally:
        hip.set_precision("fp32")


@pytest.mark.gpu
@pytest.mark.parametrize("Tc", [3, 15])
def test_streaming_tts_multiband_equals_the_hand_chained_twin_gpu(Tc):
    import kantts._hip as hip

    hip.set_precision("bf16")
    try:
        _check("cuda", Tc)
    finally:
        hip.set_precision("fp32")
