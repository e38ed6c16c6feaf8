"""The host side of the five chunked vocoders (kantts/models/hifigan/chunked*.py), without a kernel: the stateless
multi-band emission rule against the running ``hip.mb_emit`` chain, the one schedule of ``play_many`` against the table the
three former loops produced, and the one place that picks the class for a generator."""
import random

import pytest
import torch

# ---------------------------------------------------------------------------------------------------------------------
# the multi-band rule


@pytest.mark.parametrize("D", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("low_hop", [1, 2, 3, 8])
def test_stateless_multiband_rule_is_the_running_chain(D, low_hop):
    """``mb_emitted(pos, n, T, ...)`` needs no running count: along every cut sequence it gives what ``hip.mb_emit`` gives
    when it is fed its own ``pending``, the pending count before a step is min(pos * low_hop, D), and the counts of an
    utterance add up to T * low_hop * B.  Cuts are drawn from {0, 1, 2, 3, 5} (0: a step that takes nothing)."""
    import kantts._hip as hip
    from kantts.models.hifigan.chunked_mb import mb_emitted

    B = 4
    rng = random.Random(1000 * D + low_hop)
    steps = 0
    for T in range(1, 14):
        for _ in range(6):
            pos = pending = total = 0
            while pos < T:
                n = min(rng.choice([0, 1, 2, 3, 5]), T - pos)
                last = int(n > 0 and pos + n >= T)
                assert pending == min(pos * low_hop, D), (T, pos, n)
                e, pending = hip.mb_emit(pending, n * low_hop, last, D)
                assert mb_emitted(pos, n, T, low_hop, D, B) == (0, e * B), (T, pos, n)
                pos, total, steps = pos + n, total + e * B, steps + 1
            assert pending == 0 and total == T * low_hop * B, (T, total)
    assert steps > 200


# ---------------------------------------------------------------------------------------------------------------------
# the schedule

_LENGTHS, _SLOTS, _CHUNK = [5, 1, 9], 2, 4
# per step, per slot: None (idle) or (index, pos, take, live); ``schedule`` adds ``done`` behind them
_TABLE = {
    0: [[(0, 0, 4, 4), (1, 0, 1, 1)],
        [(0, 4, 1, 1), (2, 0, 4, 4)],
        [None, (2, 4, 4, 4)],
        [None, (2, 8, 1, 1)]],
    3: [[(0, 0, 4, 4), (1, 0, 4, 1)],
        [(0, 4, 4, 1), (2, 0, 4, 4)],
        [None, (2, 4, 4, 4)],
        [None, (2, 8, 4, 1)]],
}


@pytest.mark.parametrize("flush", [0, 3])
def test_the_one_schedule(flush):
    """``schedule`` on lengths [5, 1, 9], 2 slots, chunk 4.  The literal table was recorded from the three ``play_many``
    loops this schedule replaced (``ChunkedVocoder`` and ``ChunkedMBVocoder`` for flush 0 -- they agreed --,
    ``ChunkedNCVocoder`` for flush 3), run with a stubbed ``step`` before they were deleted."""
    from kantts.models.hifigan.chunked import schedule

    table = list(schedule(_LENGTHS, _SLOTS, _CHUNK, flush))
    assert [[p and p[:4] for p in row] for row in table] == _TABLE[flush]
    takes, seen = [0] * len(_LENGTHS), []
    for row in table:
        for p in row:
            if p is not None:
                index, pos, take, live, done = p
                assert pos == takes[index] and 1 <= take <= _CHUNK
                assert done == (pos + take >= _LENGTHS[index] + flush)
                assert live == max(0, min(take, _LENGTHS[index] - pos))
                takes[index] += take
                if index not in seen:
                    seen.append(index)
        # no slot idles while an utterance is unassigned
        assert None not in row or len(seen) == len(_LENGTHS)
    assert takes == [T + flush for T in _LENGTHS]
    assert seen == [0, 1, 2], "input order"


# what the former loops did around the steps, recorded in the same run: the resets, the utterance each slot was named, the
# arguments of every step, and the (index, samples) of every chunk yielded
_RUNS = {
    "causal": dict(
        events=[("reset", None), ("assign", 0, 0), ("assign", 1, 1), ("step", [4, 1], None), ("reset", 1), ("assign", 1, 2),
                ("step", [1, 4], None), ("reset", 0), ("step", [0, 4], None), ("step", [0, 1], None), ("reset", 1)],
        yields=[(0, 32), (1, 8), (0, 8), (2, 32), (2, 32), (2, 8)]),
    "mb": dict(
        events=[("reset", None), ("assign", 0, 0), ("assign", 1, 1), ("step", [4, 1], [0, 1]), ("reset", 1), ("assign", 1, 2),
                ("step", [1, 4], [1, 0]), ("reset", 0), ("step", [0, 4], [0, 0]), ("step", [0, 1], [0, 1]), ("reset", 1)],
        yields=[(0, 20), (1, 8), (0, 20), (2, 20), (2, 32), (2, 20)]),
    "nc": dict(
        events=[("reset", None), ("assign", 0, 0), ("assign", 1, 1), ("step", [4, 4], [5, 1]), ("reset", 1), ("assign", 1, 2),
                ("step", [4, 4], [5, 9]), ("reset", 0), ("step", [0, 4], [-1, 9]), ("step", [0, 4], [-1, 9]), ("reset", 1)],
        yields=[(0, 11), (1, 8), (0, 29), (2, 11), (2, 32), (2, 29)]),
}


@pytest.mark.parametrize("kind", list(_RUNS))
def test_play_many_around_a_stubbed_step(kind):
    """``play_many`` of a causal, a multi-band and a non-causal class with ``step``, ``reset`` and ``_assign`` stubbed: the
    order of resets and assignments, the ``rows`` and ``last`` / ``end`` of every step and the chunk lengths are what the
    class's own former loop gave (hop 8; multi-band: 2 rows per frame, D = 3, B = 4; non-causal: 3 flush frames, a delay of
    21 samples)."""
    from kantts.models.hifigan.chunked import ChunkedVocoder
    from kantts.models.hifigan.chunked_mb import ChunkedMBVocoder
    from kantts.models.hifigan.chunked_nc import ChunkedNCVocoder

    v = object.__new__({"causal": ChunkedVocoder, "mb": ChunkedMBVocoder, "nc": ChunkedNCVocoder}[kind])
    v.slots, v._step_channels, v.device, v.hop = _SLOTS, 2, torch.device("cpu"), 8
    v.low_hop, v.D, v.B = 2, 3, 4
    if kind == "nc":
        v.flush_frames, v.delay_samples = 3, 21
    events = []
    v.reset = lambda slot=None: events.append(("reset", slot))
    v._assign = lambda slot, index: events.append(("assign", slot, index))

    def step(buf, rows=None, last=None, end=None):
        events.append(("step", list(rows), last if end is None else end))
        return torch.zeros(_SLOTS, 1, _CHUNK * v.hop + 64)

    v.step = step
    mels = [torch.zeros(2, T) for T in _LENGTHS]
    yields = [(i, int(w.shape[1])) for i, w in v.play_many(mels, chunk_frames=_CHUNK)]
    assert events == _RUNS[kind]["events"]
    assert yields == _RUNS[kind]["yields"]
    for i, T in enumerate(_LENGTHS):
        assert sum(n for j, n in yields if j == i) == T * v.hop


# ---------------------------------------------------------------------------------------------------------------------
# the class for a generator


def test_the_class_for_a_generator():
    from kantts.models.hifigan import chunked_vocoder_class
    from kantts.models.hifigan.chunked import ChunkedVocoder
    from kantts.models.hifigan.chunked_mb import ChunkedMBVocoder
    from kantts.models.hifigan.chunked_nc import ChunkedNCVocoder
    from kantts.models.hifigan.chunked_nc_nsf import ChunkedNCNSFVocoder
    from kantts.models.hifigan.chunked_nsf import ChunkedNSFVocoder
    from kantts.models.hifigan.hifigan import Generator

    g64 = dict(channels=64, upsample_scales=[4, 2], upsample_kernal_sizes=[8, 4])
    nsf = dict(in_channels=80, nsf_params={"nb_harmonics": 7, "sampling_rate": 16000})
    kinds = [  # generator, the class without lookahead, the class with it
        (Generator(**g64), ChunkedVocoder, ChunkedVocoder),
        (Generator(**g64, **nsf), ChunkedNSFVocoder, ChunkedNSFVocoder),
        (Generator(out_channels=4, **g64), ChunkedMBVocoder, ChunkedMBVocoder),
        (Generator(causal=False, **g64), ChunkedVocoder, ChunkedNCVocoder),
        (Generator(causal=False, **g64, **nsf), ChunkedNSFVocoder, ChunkedNCNSFVocoder),
    ]
    for G, without, with_ in kinds:
        assert chunked_vocoder_class(G) is without
        assert chunked_vocoder_class(G, lookahead=True) is with_
    # without lookahead a non-causal generator reaches a causal class, which refuses it
    with pytest.raises(ValueError, match="causal"):
        chunked_vocoder_class(kinds[3][0])(kinds[3][0].eval(), graph=False)
    # what nothing plays goes to the class whose refusal names it: multi-band first, as StreamingTTS always did
    assert chunked_vocoder_class(Generator(out_channels=4, **g64, **nsf), lookahead=True) is ChunkedMBVocoder
    assert chunked_vocoder_class(Generator(causal=False, out_channels=4, **g64), lookahead=True) is ChunkedMBVocoder
