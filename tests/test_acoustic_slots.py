"""Independently advancing SAM-BERT streaming slots: the four per-slot entry points (csrc/ar_infer.hip, csrc/lstm.hip,
csrc/seq.hip, csrc/batching.hip) and the pool built on them (kantts/models/sambert/slots.py).

Every kernel-level and model-level case runs twice, as tests/test_chunked_acoustic.py does: on the host build of the kernel
SOURCES (util.kernel_source_on_cpu -- the emulated C ABI of oracle/ has none of the four) and, marked ``gpu``, on the device.

Kernel level: a launch with per-sequence ranges over full-length buffers must reproduce, for every sequence, the rows of
ONE whole-sequence launch bit for bit, must leave every row outside the sequence's own (clamped) range untouched and must
not depend on input rows that do not exist yet -- unfilled buffers hold NaN, so a read ahead or a stray write shows.

Model level: every utterance played through the pool against the model's own forward of that utterance at batch 1:
dec_outputs and the index / prediction tensors bit for bit, postnet_outputs within the bounds the existing tests use for
a bf16 path against its twin (rel_l2 < 3e-3, max-abs < 3e-2 * scale)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

if __name__ == "__main__":  # the child of the bf16 quad kernel case: the paths pytest's conftest sets
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (os.path.join(_root, "kan-tts_amd"), os.path.join(_root, "oracle"), _root, os.path.join(_root, "tests")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import test_chunked_acoustic as _ca
import torch_oracle as O
from test_chunked_acoustic import LEGS, _all_nan, _leg, _same_bits
from util import emulation, rel_l2

_NAN = float("nan")
_E_BADARG = -1  # include/kantts_hip.h


def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


# ---------------------------------------------------------------------------------------------------------------------
# 1. kernel level: decoder
_DEC_COUNTS = [[5, 0, 1], [11, 24, 0], [0, 0, 0], [8, 0, 23]]


def _dec_slots(p, xkv, out, t0, t1, bws=None):
    import kantts._hip as hip

    c = _ca._DEC
    return hip.pnca_decode_run(p.w, p.f, p.memory, p.hkv, xkv, out, p.lens, p.bws if bws is None else bws, 0, c["d_mel"],
                               c["layers"], 128 ** 0.5, 1e-6, slots=(t0, t1))


def _dec_check(p, out, cur, what):
    for b, t in enumerate(cur):
        assert torch.equal(out[b, :t], p.ref[b, :t]), (what, b, t)
        assert _all_nan(out[b, t:]), (what, b, t)


@pytest.mark.parametrize("leg", LEGS)
def test_decoder_slots_equal_one_launch(leg):
    ctx, dev = _leg(leg)
    with ctx:
        p = _ca._decoder_problem(leg, dev)
        L = _ca._DEC["L"]
        xkv, out = p.buffers()
        cur = [0, 0, 0]
        for counts in _DEC_COUNTS:
            before = xkv.clone()
            nxt = [min(t + n, L) for t, n in zip(cur, counts)]
            assert _dec_slots(p, xkv, out, _i32(cur, dev), _i32(nxt, dev)) == 0
            _dec_check(p, out, nxt, counts)
            for b, n in enumerate(counts):
                if n == 0:  # a sequence that did not advance: its K | V cache is untouched, bit for bit
                    assert _same_bits(xkv[:, b], before[:, b]), (counts, b)
                else:       # an advancing one: only the rows of its own range were written
                    assert _same_bits(xkv[:, b, :cur[b]], before[:, b, :cur[b]]) and _all_nan(xkv[:, b, nxt[b]:]), (counts, b)
            cur = nxt
        assert cur == [L, L, L]


@pytest.mark.parametrize("leg", LEGS)
def test_decoder_slots_clamps_poison_and_arguments(leg):
    ctx, dev = _leg(leg)
    with ctx:
        p = _ca._decoder_problem(leg, dev)
        L = _ca._DEC["L"]
        # out-of-range device values behave as their clamps: t0 = -3 -> 0, t1 < t0 -> empty, t1 = L + 9 -> L
        xkv, out = p.buffers()
        assert _dec_slots(p, xkv, out, _i32([-3, -3, 9], dev), _i32([4, 5, 2], dev)) == 0
        _dec_check(p, out, [4, 5, 0], "clamp low")
        assert _all_nan(xkv[:, 2])
        assert _dec_slots(p, xkv, out, _i32([4, 5, 0], dev), _i32([L + 9, L + 9, L + 9], dev)) == 0
        _dec_check(p, out, [L, L, L], "clamp high")
        # a NULL array is an argument error and launches nothing
        xkv, out = p.buffers()
        t = _i32([0, 0, 0], dev)
        assert _dec_slots(p, xkv, out, None, t) == _E_BADARG and _dec_slots(p, xkv, out, t, None) == _E_BADARG
        assert _all_nan(out) and _all_nan(xkv)
        # a device-side band width above 127 poisons the rows of the range of that sequence only
        assert _dec_slots(p, xkv, out, _i32([0, 0, 0], dev), _i32([2, 3, 1], dev)) == 0
        bad = _i32([2, 200, 0], dev)
        assert _dec_slots(p, xkv, out, _i32([2, 3, 1], dev), _i32([5, 7, 1], dev), bws=bad) == 0
        assert torch.equal(out[0, :5], p.ref[0, :5]) and _all_nan(out[0, 5:])
        assert torch.equal(out[1, :3], p.ref[1, :3]) and _all_nan(out[1, 3:])  # poison is NaN as well: rows 3..7
        assert torch.equal(out[2, :1], p.ref[2, :1]) and _all_nan(out[2, 1:])


# ---------------------------------------------------------------------------------------------------------------------
# 1. kernel level: LSTM
_LSTM_COUNTS = [[8, 0, 37], [0, 20, 0], [29, 3, 0], [0, 14, 0]]  # per launch, per sequence; every sequence ends at T = 37


def _lstm_slots_case(dev, lens, prec):
    import kantts._hip as hip

    B, T = 3, 37
    g = torch.Generator().manual_seed(7)
    gx = torch.randn(B, T, 512, generator=g).to(dev)
    whh = (torch.randn(1, 512, 128, generator=g) / 128 ** 0.5).to(dev)
    bhh = (0.1 * torch.randn(1, 512, generator=g)).to(dev)
    lens_t = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
    ref = _ca._lstm_full(gx, whh, bhh, lens_t, prec)
    gxs = torch.full_like(gx, _NAN)
    out, gates, cst = (torch.full_like(r, _NAN) for r in ref)
    cur = [0] * B
    for counts in _LSTM_COUNTS:
        nxt = [t + n for t, n in zip(cur, counts)]
        for b in range(B):
            gxs[b, cur[b]:nxt[b]] = gx[b, cur[b]:nxt[b]]  # rows of gx at or after a sequence's t1 do not exist yet
        assert hip.lstm_fwd_slots(gxs, whh, bhh, lens_t, out, gates, cst, _i32(cur, dev), _i32(nxt, dev), prec) == 0
        cur = nxt
        for b, t in enumerate(cur):
            assert _same_bits(out[b, :t], ref[0][b, :t]), (counts, b)
            assert _same_bits(gates[0, b, :t], ref[1][0, b, :t]) and _same_bits(cst[0, b, :t], ref[2][0, b, :t]), (counts, b)
            assert _all_nan(out[b, t:]) and _all_nan(gates[0, b, t:]) and _all_nan(cst[0, b, t:]), (counts, b)
            if lens is not None:  # the tail inside what has been run is exactly zero
                assert bool((out[b, lens[b]:t] == 0).all()), (counts, b)
    assert cur == [T] * B
    # clamps (t0 < 0, t1 > T, t1 < t0) in one launch over fresh buffers, then the argument checks
    out, gates, cst = (torch.full_like(r, _NAN) for r in ref)
    assert hip.lstm_fwd_slots(gx, whh, bhh, lens_t, out, gates, cst, _i32([-3, 0, 9], dev), _i32([T + 9, 11, 2], dev), prec) == 0
    assert _same_bits(out[0], ref[0][0]) and _same_bits(out[1, :11], ref[0][1, :11])
    assert _all_nan(out[1, 11:]) and _all_nan(out[2]) and _all_nan(cst[0, 2]) and _all_nan(gates[0, 2])
    out, gates, cst = (torch.full_like(r, _NAN) for r in ref)
    t = _i32([0, 0, 0], dev)
    assert hip.lstm_fwd_slots(gx, whh, bhh, lens_t, out, gates, cst, None, t, prec) == _E_BADARG
    assert hip.lstm_fwd_slots(gx, whh, bhh, lens_t, out, gates, cst, t, None, prec) == _E_BADARG
    assert hip.lstm_fwd_slots(gx, whh, bhh, lens_t, out, gates, cst, t, t, prec) == 0
    assert _all_nan(out) and _all_nan(gates) and _all_nan(cst)


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("prec", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("lens", [[37, 20, 0], None], ids=["ragged", "nolens"])
def test_lstm_slots_equal_one_launch(lens, prec, leg):
    ctx, dev = _leg(leg)
    with ctx:
        _lstm_slots_case(dev, lens, prec)


@pytest.mark.parametrize("leg", LEGS)
def test_lstm_slots_bf16_quad_kernel_in_a_fresh_process(leg):
    """KANTTS_LSTM_PAIR=0 selects the quad kernel at precision 1; the launchers read it once per process, so one child
    process runs the bf16 cases above and exits non-zero on a mismatch (as tests/test_lstm_recurrence.py does)."""
    env = dict(os.environ, KANTTS_LSTM_PAIR="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), leg], env=env, capture_output=True, text=True, timeout=600,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and "bf16 quad slots ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ---------------------------------------------------------------------------------------------------------------------
# 1. kernel level: FIR
# (t0 per sequence, t1 per sequence, max_rows): sequence 1 starts before sequence 0's window ends and sequence 2's window is
# empty; then a max_rows (17) smaller than the windows sequences 0 and 2 ask for, with a negative t0; then values past T.
_FIR_LAUNCHES = [([0, 13, 7], [20, 40, 7], 50), ([20, -4, 0], [50, 13, 50], 17), ([37, 40, 17], [99, 60, 50], 50)]


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("K,lp", [(41, 37), (41, 20), (5, 3)])
@pytest.mark.parametrize("C", [256, 80])
def test_fir_slots_equal_one_launch(C, K, lp, with_res, leg):
    import kantts._hip as hip

    ctx, dev = _leg(leg)
    B, T, rp = 3, 50, K - 1 - lp
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, T, C, generator=g).to(dev)
    w = (torch.randn(C, K, generator=g) / K ** 0.5).to(dev)
    res = torch.randn(B, T, C, generator=g).to(dev) if with_res else None
    lens = torch.tensor([50, 29, 50], dtype=torch.int64, device=dev)
    with ctx:
        ref = torch.full_like(x, _NAN)
        rc = hip.lib().kantts_fsmn_dwconv_fwd(hip.ptr(x), hip.ptr(w), hip.ptr(res), hip.ptr(lens), hip.ptr(ref), B, T, C, K, lp,
                                              hip.stream())
        assert rc == 0 and torch.isfinite(ref).all()
        y = torch.full_like(x, _NAN)
        done = torch.zeros(B, T, dtype=torch.bool)
        for t0, t1, max_rows in _FIR_LAUNCHES:
            xs = x.clone()
            for b in range(B):
                c0 = min(max(t0[b], 0), T)
                c1 = min(min(max(t1[b], c0), T), c0 + max_rows)  # the clamp is part of the contract
                xs[b, min(c1 + rp, T):] = _NAN                  # these rows of x do not exist yet
                done[b, c0:c1] = True
            assert hip.fsmn_dwconv_fwd_slots(xs, w, res, lens, y, lp, _i32(t0, dev), _i32(t1, dev), max_rows) == 0
            assert torch.equal(y[done], ref[done]), (t0, t1, max_rows)
            assert _all_nan(y[~done]), (t0, t1, max_rows)
        assert bool(done.all())
        y = torch.full_like(x, _NAN)
        t = _i32([0, 0, 0], dev)
        assert hip.fsmn_dwconv_fwd_slots(x, w, res, lens, y, lp, None, t, 8) == _E_BADARG
        assert hip.fsmn_dwconv_fwd_slots(x, w, res, lens, y, lp, t, None, 8) == _E_BADARG
        assert hip.fsmn_dwconv_fwd_slots(x, w, res, lens, y, lp, t, _i32([9, 9, 9], dev), -1) == _E_BADARG
        assert hip.fsmn_dwconv_fwd_slots(x, w, res, lens, y, lp, t, _i32([9, 9, 9], dev), 0) == 0
        assert hip.fsmn_dwconv_fwd_slots(x, w, res, lens, y, lp, _i32([9, 50, 3], dev), _i32([9, 50, 1], dev), 8) == 0
        assert _all_nan(y)


# ---------------------------------------------------------------------------------------------------------------------
# 1. kernel level: scatter
@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("C", [80, 256, 6])
def test_scatter_rows_inverts_ragged_rows(C, leg):
    import kantts._hip as hip

    ctx, dev = _leg(leg)
    rows, Tmax = 120, 10
    g = torch.Generator().manual_seed(3)
    src = torch.randn(rows, C, generator=g).to(dev)
    row_off = torch.tensor([0, 40, 90, 100], dtype=torch.int64, device=dev)
    start, lens = _i32([3, 0, 5, 2], dev), _i32([7, 12, 0, 1], dev)  # 12 > Tmax: clamped to 10; one empty window
    with ctx:
        packed = hip.ragged_rows(src, row_off, lens, Tmax, start=start)
        canvas = torch.full_like(src, _NAN)
        assert hip.scatter_rows(packed, row_off, lens, canvas, start=start) == 0
        hit = torch.zeros(rows, dtype=torch.bool)
        for o, s, n in zip([0, 40, 90, 100], [3, 0, 5, 2], [7, 10, 0, 1]):
            hit[o + s:o + s + n] = True
        assert torch.equal(canvas[hit], src[hit]) and _all_nan(canvas[~hit])
        # start == NULL is an offset of zero; NULL row offsets / lengths are argument errors
        canvas = torch.full_like(src, _NAN)
        assert hip.scatter_rows(packed[:1].contiguous(), row_off[1:2], lens[:1], canvas) == 0
        assert torch.equal(canvas[40:47], src[3:10]) and _all_nan(canvas[:40]) and _all_nan(canvas[47:])
        L = hip.lib()
        assert L.kantts_scatter_rows_f32(hip.ptr(packed), None, None, hip.ptr(lens), hip.ptr(canvas), 4, Tmax, C,
                                         hip.stream()) == _E_BADARG
        assert L.kantts_scatter_rows_f32(hip.ptr(packed), hip.ptr(row_off), None, None, hip.ptr(canvas), 4, Tmax, C,
                                         hip.stream()) == _E_BADARG


# ---------------------------------------------------------------------------------------------------------------------
# 2. model level
_KEYS_EXACT = ("dec_outputs", "LR_length_rounded", "log_duration_predictions", "pitch_predictions", "energy_predictions")
_UTT_CACHE = {}


def _utterances(leg, dev):
    """One model (free-running durations of a few frames per token), four batch-1 utterances -- the three of the
    ``durations`` case of tests/test_chunked_acoustic.py (96, 45 and 6 frames; 32, 15 and 2 decoder steps) and one
    free-running -- and the model's own forward of each, computed once per leg (inside its context, bf16 mode)."""
    if leg not in _UTT_CACHE:
        m = _ca._tiny_model(dev, dur_bias=1.5)
        batch = _ca._inputs(dev, "durations")
        utts = [{k: v[i:i + 1].contiguous() for k, v in batch.items()} for i in range(3)]
        utts.append({k: v[0:1].contiguous() for k, v in _ca._inputs(dev, "free").items()})
        with torch.no_grad():
            refs = [m(**u) for u in utts]
        assert m.mel_decoder._decode_kernel is not None, "the one-shot side did not take the one-launch decoder"
        assert [int(r["LR_length_rounded"][0]) for r in refs[:3]] == [96, 45, 6]
        assert [r["dec_outputs"].size(1) for r in refs[:3]] == [96, 45, 6] and refs[3]["dec_outputs"].size(1) <= 96
        _UTT_CACHE[leg] = (m, batch, utts, refs)
    return _UTT_CACHE[leg]


def _play_pool(pool, utts, chunk_steps):
    """play_many over ``utts``; checks the windows; returns the per-utterance results and the streamed mels."""
    results, seen, mels = {}, {}, {}
    for index, lo, hi, mel in pool.play_many(utts, chunk_steps, results=results):
        assert lo == seen.get(index, 0) and hi > lo and tuple(mel.shape) == (hi - lo, 80), (index, lo, hi)
        seen[index] = hi
        mels.setdefault(index, []).append(mel.clone())
    assert sorted(results) == list(range(len(utts))) and pool.free_slots() == list(range(pool.S))
    for i, res in results.items():  # contiguous from 0 to the utterance's own padded frame count
        assert seen[i] == res["postnet_outputs"].size(1), (i, seen[i])
        assert torch.equal(torch.cat(mels[i]), res["postnet_outputs"][0]), i
    return results


def _twin_bounds(a, b, what):
    a, b = a.cpu(), b.cpu()
    scale = float(b.abs().max())
    err = (rel_l2(a, b), float((a - b).abs().max()))
    print("acoustic slots", what, "rel_l2 %.3e max-abs %.3e scale %.3e" % (err + (scale,)))
    assert err[0] < 3e-3 and err[1] < 3e-2 * scale, (what, err)


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("chunk_steps", [1, 5, 32])
def test_acoustic_slots_match_forward(chunk_steps, leg):
    import kantts._hip as hip
    from kantts.models.sambert.slots import AcousticSlots

    ctx, dev = _leg(leg)
    hip.set_precision("bf16")
    try:
        with ctx:
            m, _, utts, refs = _utterances(leg, dev)
            pool = AcousticSlots(m, slots=2, max_steps=32)
            assert pool.lookahead == 12
            results = _play_pool(pool, utts, chunk_steps)
            for i, (got, ref) in enumerate(zip((results[i] for i in range(4)), refs)):
                assert set(got) == set(ref), i
                for k in _KEYS_EXACT:
                    assert torch.equal(got[k], ref[k]), (i, k)
                _twin_bounds(got["postnet_outputs"], ref["postnet_outputs"], "utterance %d chunk %d %s" % (i, chunk_steps, leg))
                n = int(ref["LR_length_rounded"][0])
                assert bool((got["postnet_outputs"][0, n:] == 0).all()) and bool((got["dec_outputs"][0, n:] == 0).all()), i
    finally:
        hip.set_precision("fp32")


@pytest.mark.parametrize("leg", LEGS)
def test_acoustic_slots_stale_occupant(leg):
    """Utterance B played in the slot utterance A has just left equals B played in a fresh pool bit for bit: admit clears
    nothing, so every row B reads must be a row B wrote."""
    import kantts._hip as hip
    from kantts.models.sambert.slots import AcousticSlots

    ctx, dev = _leg(leg)
    hip.set_precision("bf16")
    try:
        with ctx:
            m, _, utts, _ = _utterances(leg, dev)
            for a, b in ((0, 1), (2, 3)):  # a longer occupant before a shorter one, and a shorter before a longer
                used = _play_pool(AcousticSlots(m, slots=1, max_steps=32), [utts[a], utts[b]], 5)[1]
                fresh = _play_pool(AcousticSlots(m, slots=1, max_steps=32), [utts[b]], 5)[0]
                assert set(used) == set(fresh)
                for k, v in fresh.items():
                    if torch.is_tensor(v):
                        assert _same_bits(used[k].float(), v.float()) and used[k].dtype == v.dtype, (a, b, k)
    finally:
        hip.set_precision("fp32")


@pytest.mark.parametrize("leg", LEGS)
def test_acoustic_slots_lockstep_equals_chunked_session(leg):
    """A pool stepped with equal counts against a ChunkedAcoustic session over the same batch."""
    import kantts._hip as hip
    from kantts.models.sambert.chunked import ChunkedAcoustic
    from kantts.models.sambert.slots import AcousticSlots

    ctx, dev = _leg(leg)
    hip.set_precision("bf16")
    try:
        with ctx:
            m, batch, utts, _ = _utterances(leg, dev)
            sess = ChunkedAcoustic(m).open(**batch)
            for _ in sess.stream(5):
                pass
            ref = sess.result()
            pool = AcousticSlots(m, slots=3, max_steps=32)
            assert [pool.admit(s, **utts[s]) for s in range(3)] == [96, 45, 6] and pool.free_slots() == []
            n_steps = 0
            while not all(pool.finished(s) for s in range(3)):
                outs = pool.step([5, 5, 5])
                n_steps += 1
                assert all(o is not None for o in outs) and n_steps <= 7
            assert n_steps == 7  # ceil(32 / 5): the post-net of a slot flushes in the step that ends its decoder
            for s in range(3):
                got = pool.result(s)
                Tp = got["dec_outputs"].size(1)
                assert Tp == [96, 45, 6][s]
                assert torch.equal(got["dec_outputs"][0], ref["dec_outputs"][s, :Tp]), s
                assert bool((ref["dec_outputs"][s, Tp:] == 0).all())
                _twin_bounds(got["postnet_outputs"][0], ref["postnet_outputs"][s, :Tp], "lockstep slot %d %s" % (s, leg))
                assert pool.live_rows(s, 40, 50) == [10, 5, 0][s]
    finally:
        hip.set_precision("fp32")


@pytest.mark.parametrize("leg", LEGS)
def test_acoustic_slots_zero_count_step_launches_nothing(leg, monkeypatch):
    import kantts._hip as hip
    from kantts._hip import ops
    from kantts.models.sambert.slots import AcousticSlots

    ctx, dev = _leg(leg)
    hip.set_precision("bf16")
    try:
        with ctx:
            m, _, utts, _ = _utterances(leg, dev)
            pool = AcousticSlots(m, slots=2, max_steps=32)
            pool.admit(1, **utts[1])
            outs = pool.step([0, 4])
            assert outs[0] is None and outs[1][:2] == (0, 0)
            calls = []
            for mod, name in ((hip, "pnca_decode_run"), (hip, "ragged_rows"), (hip, "scatter_rows"), (hip, "lstm_fwd_slots"),
                              (hip, "fsmn_dwconv_fwd_slots"), (ops, "linear")):
                monkeypatch.setattr(mod, name, lambda *a, _n=name, **k: calls.append(_n))
            outs = pool.step([0, 0])
            assert calls == [] and outs[0] is None and outs[1][:2] == (0, 0) and outs[1][2].shape == (0, 80)
            outs = pool.step([3, 0])  # a count for a free slot is ignored
            assert calls == [] and outs[0] is None
    finally:
        hip.set_precision("fp32")


@pytest.mark.parametrize("leg", LEGS)
def test_acoustic_slots_refuse_what_they_cannot_play(leg):
    import kantts._hip as hip
    from kantts.models.sambert.slots import AcousticSlots

    ctx, dev = _leg(leg)
    try:
        with ctx:
            hip.set_precision("bf16")
            m, batch, utts, _ = _utterances(leg, dev)
            hip.set_precision("fp32")
            with pytest.raises(ValueError):
                AcousticSlots(m, slots=2, max_steps=32)
            hip.set_precision("bf16")
            m.train()
            try:
                with pytest.raises(ValueError):
                    AcousticSlots(m, slots=2, max_steps=32)
            finally:
                m.eval()
            pool = AcousticSlots(m, slots=2, max_steps=16)
            assert pool.admit(0, **utts[1]) == 45
            with pytest.raises(ValueError, match="occupied"):
                pool.admit(0, **utts[2])
            with pytest.raises(ValueError, match="max_steps"):
                pool.admit(1, **utts[0])  # 32 decoder steps
            wide = {k: v.clone() for k, v in utts[2].items()}
            wide["duration_targets"][0, 0] = 384  # band width int(384 / 3 + 0.5) = 128
            with pytest.raises(ValueError, match="band width"):
                AcousticSlots(m, slots=1, max_steps=200).admit(0, **wide)
            assert pool.free_slots() == [1]
            pool.step([3, 0])
            with pytest.raises(RuntimeError):
                pool.result(0)  # before the end
            with pytest.raises(ValueError):
                pool.result(1)  # a free slot
            with pytest.raises(ValueError):
                pool.step([1, -1])
    finally:
        hip.set_precision("fp32")


def test_acoustic_slots_say_so_under_the_emulated_abi():
    import kantts._hip as hip
    from kantts.models.sambert.slots import AcousticSlots

    hip.set_precision("bf16")
    try:
        with emulation():
            assert not hip.slot_entry_points()
            with pytest.raises(RuntimeError, match="per-slot entry points"):
                AcousticSlots(_ca._tiny_model("cpu"), slots=2, max_steps=32)
    finally:
        hip.set_precision("fp32")


# ---------------------------------------------------------------------------------------------------------------------
# 3. CLI
@pytest.mark.gpu
def test_infer_sambert_slots_cli_gpu(tmp_path):
    import kantts._hip as hip
    from kantts.bin.infer_sambert import am_infer
    from kantts.models.sambert.kantts_sambert import KanTtsSAMBERT

    cfg = O.sambert_config(tiny=True)
    am_dir = tmp_path / "am" / "ckpt"
    am_dir.mkdir(parents=True)
    config = {"model_type": "sambert", "Model": {"KanTtsSAMBERT": {
        "params": {k: v for k, v in cfg.items() if k not in O.SAMBERT_VOCAB},
        "optimizer": {"type": "Adam", "params": {"lr": 0.001, "betas": [0.9, 0.98], "eps": 1e-9, "weight_decay": 0.0}},
        "scheduler": {"type": "NoamLR", "params": {"warmup_steps": 4000}}}}, "grad_norm": 1.0, "batch_size": 2}
    (tmp_path / "am" / "config.yaml").write_text(yaml.dump(config))
    torch.manual_seed(0)
    m = KanTtsSAMBERT(dict(cfg))
    with torch.no_grad():
        m.variance_adaptor.duration_predictor.fc.bias.fill_(1.5)
    ck = str(am_dir / "checkpoint_1.pth")
    torch.save({"model": m.state_dict()}, ck)
    sent = tmp_path / "sentences.txt"
    sent.write_text("utt_a\ta b c d e f g h i j k\nutt_b\tg h i j\nutt_c\ta b c d e f g\n")
    hip.set_precision("bf16")
    try:
        am_infer(str(sent), ck, str(tmp_path / "chunked"), ling_unit=_ca._FakeLingUnit(cfg), chunk_frames=6)
        am_infer(str(sent), ck, str(tmp_path / "slots"), ling_unit=_ca._FakeLingUnit(cfg), chunk_frames=6, slots=2,
                 slot_steps=64)
        with pytest.raises(ValueError, match="--slots"):
            am_infer(str(sent), ck, str(tmp_path / "refused"), ling_unit=_ca._FakeLingUnit(cfg), slots=2)
    finally:
        hip.set_precision("fp32")
    assert sorted(os.listdir(tmp_path / "chunked" / "feat")) == sorted(os.listdir(tmp_path / "slots" / "feat"))
    for utt in ("utt_a", "utt_b", "utt_c"):
        a = np.load(tmp_path / "chunked" / "feat" / (utt + "_mel.npy"))
        b = np.load(tmp_path / "slots" / "feat" / (utt + "_mel.npy"))
        assert a.shape == b.shape and (utt != "utt_a" or a.shape[0] > 6)  # utt_a spans several chunks
        scale = float(np.abs(a).max())
        assert rel_l2(torch.from_numpy(b), torch.from_numpy(a)) < 3e-3 and float(np.abs(a - b).max()) < 3e-2 * scale
        for ext in ("_dur.txt", "_f0.txt", "_energy.txt"):
            assert (tmp_path / "chunked" / "feat" / (utt + ext)).read_bytes() == (tmp_path / "slots" / "feat" / (utt + ext)).read_bytes()


# ------------------------------------------------------------------------------- the child of the bf16 quad kernel case
if __name__ == "__main__":
    assert os.environ.get("KANTTS_LSTM_PAIR") == "0"
    _ctx, _dev = _leg(sys.argv[1])
    with _ctx:
        for _lens in ([37, 20, 0], None):
            _lstm_slots_case(_dev, _lens, 1)
    print("bf16 quad slots ok")
