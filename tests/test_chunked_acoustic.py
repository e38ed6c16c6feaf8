"""Streaming SAM-BERT inference: the three range entry points (csrc/ar_infer.hip, csrc/lstm.hip, csrc/seq.hip) and the
sessions built on them (kantts/models/sambert/chunked.py).

Every kernel-level and model-level case runs twice: on the host build of the kernel SOURCES (util.kernel_source_on_cpu --
the emulated C ABI of oracle/ has no range entry points) and, marked ``gpu``, on the device.

Kernel level: a range over full-length buffers must reproduce the rows of ONE whole-sequence launch bit for bit
(torch.equal; rows the whole launch leaves unspecified are compared as bit patterns), must leave every row outside the
range untouched and must not depend on input rows that do not exist yet -- unfilled buffers hold NaN, so a read ahead or a
stray write shows.

Post-net level: against a float64 plain-torch restatement written here; the chunked path's max-abs error is at most
max(2 x the one-shot path's error in the same run, 2e-5 * max(1, |ref|max)) -- 2e-5 is the project's fp32 floor
(tests/test_lstm_recurrence.py).

Model level: dec_outputs and the index tensors bit for bit, postnet_outputs within the bounds tests/test_ar_kernels.py uses
for a bf16 path against its twin (rel_l2 < 3e-3, max-abs < 3e-2 * scale)."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

import test_bench_config_parity as _bench_parity
import torch_oracle as O
from util import emulation, kernel_source_on_cpu, rel_l2

_REPORT = os.path.join(os.path.dirname(_bench_parity._REPORT), "chunked_acoustic_parity.json")
_NAN = float("nan")
_E_BADARG, _E_UNSUPPORTED = -1, -2  # include/kantts_hip.h

LEGS = [pytest.param("hostsim", id="kernel_source"), pytest.param("cuda", id="gpu", marks=pytest.mark.gpu)]


def _leg(leg):
    """(context, torch device) of a leg."""
    return (kernel_source_on_cpu(), "cpu") if leg == "hostsim" else (contextlib.nullcontext(), "cuda")


def _record(key, val):
    try:
        os.makedirs(os.path.dirname(_REPORT), exist_ok=True)
        d = json.load(open(_REPORT)) if os.path.exists(_REPORT) else {}
        d[key] = val
        json.dump(d, open(_REPORT, "w"), indent=1)
    except OSError:
        pass


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _all_nan(t):
    return bool(torch.isnan(t).all())


# ---------------------------------------------------------------------------------------------------------------------
# 1. kernel level: decoder
_DEC = dict(d_mel=80, d_mem=160, d_out=240, layers=2, B=3, L=24, lens=[24, 13, 1], bws=[2, 20, 0])
_DEC_SCHEDULES = [[24], [1] * 24, [5, 11, 8], [7, 7, 7, 3]]


class _DecoderProblem:
    """Random blobs and inputs of the raw ABI; ``ref`` is the one-launch kantts_pnca_decode_run result."""

    def __init__(self, dev):
        import kantts._hip as hip

        c = _DEC
        g = torch.Generator().manual_seed(11)
        nw, nf = hip.decode_blob_sizes(c["d_mel"], c["d_mem"], c["d_out"], c["layers"])
        self.w = (0.08 * torch.randn(nw, generator=g)).to(torch.bfloat16).to(dev)
        self.f = (0.1 * torch.randn(nf, generator=g) + 0.3).to(dev)  # biases and LayerNorm gains: every term matters
        self.memory = (0.7 * torch.randn(c["B"], c["L"], c["d_mem"], generator=g)).to(dev)
        self.hkv = (0.5 * torch.randn(c["B"], c["L"], c["layers"] * 256, generator=g)).to(dev)
        self.lens = torch.tensor(c["lens"], dtype=torch.int32, device=dev)
        self.bws = torch.tensor(c["bws"], dtype=torch.int32, device=dev)
        self.dev = dev
        xkv, out = self.buffers()
        self.call(xkv, out)
        self.ref = out
        assert torch.isfinite(out).all()

    def buffers(self):
        c = _DEC
        return (torch.full((c["layers"], c["B"], c["L"], 256), _NAN, device=self.dev),
                torch.full((c["B"], c["L"], c["d_out"]), _NAN, device=self.dev))

    def call(self, xkv, out, steps=None, bws=None):
        import kantts._hip as hip

        return hip.pnca_decode_run(self.w, self.f, self.memory, self.hkv, xkv, out, self.lens, self.bws if bws is None else bws,
                                   0, _DEC["d_mel"], _DEC["layers"], 128 ** 0.5, 1e-6, steps=steps)


_DEC_PROBLEM = {}


def _decoder_problem(leg, dev):
    """The problem and its one-launch reference, computed once per leg."""
    if leg not in _DEC_PROBLEM:
        _DEC_PROBLEM[leg] = _DecoderProblem(dev)
    return _DEC_PROBLEM[leg]


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("sched", _DEC_SCHEDULES, ids=lambda s: "x".join(map(str, s[:4])))
def test_decoder_range_equals_one_launch(sched, leg):
    ctx, dev = _leg(leg)
    with ctx:
        p = _decoder_problem(leg, dev)
        xkv, out = p.buffers()
        t = 0
        for n in sched:
            assert p.call(xkv, out, steps=(t, t + n)) == 0
            t += n
            assert torch.equal(out[:, :t], p.ref[:, :t]), (sched, t)
            assert _all_nan(out[:, t:]), (sched, t)
        assert t == _DEC["L"]


@pytest.mark.parametrize("leg", LEGS)
def test_decoder_range_poison_and_arguments(leg):
    ctx, dev = _leg(leg)
    with ctx:
        p = _decoder_problem(leg, dev)
        # a device-side band width above 127 poisons the rows of the range of that sequence only
        xkv, out = p.buffers()
        assert p.call(xkv, out, steps=(0, 2)) == 0
        bad = torch.tensor([2, 200, 0], dtype=torch.int32, device=dev)
        assert p.call(xkv, out, steps=(2, 5), bws=bad) == 0
        assert torch.equal(out[0, :5], p.ref[0, :5]) and torch.equal(out[2, :5], p.ref[2, :5])
        assert torch.equal(out[1, :2], p.ref[1, :2]) and _all_nan(out[1, 2:5])
        assert _all_nan(out[:, 5:])
        # argument checks; an empty range is a no-op
        xkv, out = p.buffers()
        for steps in ((-1, 3), (3, 25), (5, 4)):
            assert p.call(xkv, out, steps=steps) == _E_BADARG, steps
        for steps in ((0, 0), (7, 7), (24, 24)):
            assert p.call(xkv, out, steps=steps) == 0, steps
        assert _all_nan(out) and _all_nan(xkv)


# ---------------------------------------------------------------------------------------------------------------------
# 1. kernel level: LSTM
_LSTM_SCHEDULES = [[37], [1] * 37, [8, 8, 8, 8, 5], [3, 9, 16, 9]]


def _lstm_full(gx, whh, bhh, lens, prec):
    import kantts._hip as hip

    B, T = gx.shape[0], gx.shape[1]
    out, gates, cst = (torch.full(s, _NAN, device=gx.device) for s in ((B, T, 128), (1, B, T, 512), (1, B, T, 128)))
    rc = hip.lib().kantts_lstm_fwd(hip.ptr(gx), hip.ptr(whh), hip.ptr(bhh), hip.ptr(lens), hip.ptr(out), hip.ptr(gates),
                                   hip.ptr(cst), B, T, 128, 1, 0, prec, hip.stream())
    assert rc == 0
    return out, gates, cst


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("prec", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("lens", [[37, 20, 0], None], ids=["ragged", "nolens"])
def test_lstm_range_equals_one_launch(lens, prec, leg):
    import kantts._hip as hip

    ctx, dev = _leg(leg)
    B, T = 3, 37
    g = torch.Generator().manual_seed(7)
    gx = torch.randn(B, T, 512, generator=g).to(dev)
    whh = (torch.randn(1, 512, 128, generator=g) / 128 ** 0.5).to(dev)
    bhh = (0.1 * torch.randn(1, 512, generator=g)).to(dev)
    lens_t = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
    with ctx:
        ref = _lstm_full(gx, whh, bhh, lens_t, prec)
        for sched in _LSTM_SCHEDULES:
            gxs = torch.full_like(gx, _NAN)
            bufs = [torch.full_like(r, _NAN) for r in ref]
            out, gates, cst = bufs
            t = 0
            for n in sched:
                gxs[:, t:t + n] = gx[:, t:t + n]  # rows of gx at or after t1 do not exist yet
                assert hip.lstm_fwd_range(gxs, whh, bhh, lens_t, out, gates, cst, t, t + n, prec) == 0
                t += n
                assert _same_bits(out[:, :t], ref[0][:, :t]), (sched, t)
                assert _same_bits(gates[:, :, :t], ref[1][:, :, :t]), (sched, t)
                assert _same_bits(cst[:, :, :t], ref[2][:, :, :t]), (sched, t)
                assert _all_nan(out[:, t:]) and _all_nan(gates[:, :, t:]) and _all_nan(cst[:, :, t:]), (sched, t)
                for b, ln in enumerate(lens or []):  # the tail inside what has been run is exactly zero
                    assert bool((out[b, ln:t] == 0).all()), (sched, t, b)
            assert t == T
        # one forward direction only; argument checks; an empty range is a no-op
        out, gates, cst = (torch.full_like(r, _NAN) for r in ref)
        assert hip.lstm_fwd_range(gx, whh, bhh, lens_t, out, gates, cst, 0, 8, prec, ndir=2) == _E_UNSUPPORTED
        assert hip.lstm_fwd_range(gx, whh, bhh, lens_t, out, gates, cst, 0, 8, prec, reverse_first=1) == _E_UNSUPPORTED
        for t0, t1 in ((-1, 3), (3, 38), (5, 4)):
            assert hip.lstm_fwd_range(gx, whh, bhh, lens_t, out, gates, cst, t0, t1, prec) == _E_BADARG, (t0, t1)
        assert hip.lstm_fwd_range(gx, whh, bhh, lens_t, out, gates, cst, 9, 9, prec) == 0
        assert _all_nan(out) and _all_nan(gates) and _all_nan(cst)


# ---------------------------------------------------------------------------------------------------------------------
# 1. kernel level: FIR
_FIR_RANGES = [[(0, 50)], [(0, 1)], [(13, 14)], [(16, 32)], [(45, 50)], [(0, 5), (5, 16), (16, 17), (17, 50)]]


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("K,lp", [(41, 37), (41, 20), (5, 3)])
@pytest.mark.parametrize("C", [256, 80])
def test_fir_rows_equal_one_launch(C, K, lp, with_res, leg):
    import kantts._hip as hip

    ctx, dev = _leg(leg)
    B, T, rp = 2, 50, K - 1 - lp
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, T, C, generator=g).to(dev)
    w = (torch.randn(C, K, generator=g) / K ** 0.5).to(dev)
    res = torch.randn(B, T, C, generator=g).to(dev) if with_res else None
    lens = torch.tensor([50, 29], dtype=torch.int64, device=dev)
    with ctx:
        ref = torch.full_like(x, _NAN)
        rc = hip.lib().kantts_fsmn_dwconv_fwd(hip.ptr(x), hip.ptr(w), hip.ptr(res), hip.ptr(lens), hip.ptr(ref), B, T, C, K, lp,
                                              hip.stream())
        assert rc == 0 and torch.isfinite(ref).all()
        for walk in _FIR_RANGES:
            y = torch.full_like(x, _NAN)
            done = torch.zeros(T, dtype=torch.bool)
            for t0, t1 in walk:
                xs = x.clone()
                xs[:, min(t1 + rp, T):] = _NAN  # these rows of x do not exist yet
                assert hip.fsmn_dwconv_fwd_rows(xs, w, res, lens, y, lp, t0, t1) == 0
                done[t0:t1] = True
                assert torch.equal(y[:, done], ref[:, done]), (walk, t0, t1)
                assert _all_nan(y[:, ~done]), (walk, t0, t1)
        y = torch.full_like(x, _NAN)
        for t0, t1 in ((-1, 3), (3, 51), (5, 4)):
            assert hip.fsmn_dwconv_fwd_rows(x, w, res, lens, y, lp, t0, t1) == _E_BADARG, (t0, t1)
        assert hip.fsmn_dwconv_fwd_rows(x, w, res, lens, y, lp, 9, 9) == 0
        assert _all_nan(y)


# ---------------------------------------------------------------------------------------------------------------------
# 2. post-net level
def _postnet_fp64(pn, x, lens):
    """Plain-torch float64 restatement of PostNet.forward(x, mask, res=x, zero_rows=mask)."""
    x = x.double()
    T = x.size(1)
    keep = (torch.arange(T)[None, :] < lens[:, None]).unsqueeze(-1).double()
    h = x
    for ffn, mb in zip(pn.fsmn.ffn_lst, pn.fsmn.memory_block_lst):
        c = F.relu(F.linear(h, ffn.w_1.weight.double().squeeze(-1), ffn.w_1.bias.double()))
        c = F.linear(c, ffn.w_2.weight.double().squeeze(-1)) * keep
        m = F.conv1d(F.pad(c.transpose(1, 2), (mb.lp, mb.rp)), mb.conv_dw.weight.double(), groups=c.size(-1)).transpose(1, 2)
        m = (m + c) * keep
        h = m + h if h.size(-1) == m.size(-1) else m
    lstm = torch.nn.LSTM(pn.num_memory_units, pn.lstm_units, batch_first=True).double()
    lstm.load_state_dict({k: v.double() for k, v in pn.lstm.state_dict().items()})
    h, _ = lstm(h)
    return (F.linear(h, pn.fc.weight.double(), pn.fc.bias.double()) + x) * keep


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_chunked_postnet_matches_fp64(mode, leg):
    import kantts._hip as hip
    from kantts.models.sambert.chunked import ChunkedPostNet
    from kantts.models.sambert.kantts_sambert import PostNet
    from kantts.models.utils import SeqInfo

    ctx, dev = _leg(leg)
    torch.manual_seed(0)
    pn = PostNet(O.sambert_config(tiny=True)).eval()
    lens = torch.tensor([96, 45])
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 96, 80, generator=g) * (torch.arange(96)[None, :] < lens[:, None]).unsqueeze(-1)
    with torch.no_grad():
        ref = _postnet_fp64(pn, x, lens)
    floor = 2e-5 * max(1.0, float(ref.abs().max()))
    pn, xd, ld = pn.to(dev), x.to(dev), lens.to(dev)
    rep = {}
    hip.set_precision(mode)
    try:
        with ctx, torch.no_grad():
            info = SeqInfo(ld, 96)
            one = pn(xd, info, res=xd, zero_rows=info.mask).cpu()
            rep["one_shot"] = float((one.double() - ref).abs().max())
            cp = ChunkedPostNet(pn)
            assert cp.lookahead == 12
            for chunk in (3, 15, 300):
                buf = torch.full_like(xd, _NAN)  # the caller's input buffer: rows arrive chunk by chunk
                run = cp.open(buf, ld)
                D, seen = 0, 0
                while D < 96:
                    n = min(chunk, 96 - D)
                    buf[:, D:D + n] = xd[:, D:D + n]
                    D += n
                    lo, hi = run.advance(D)
                    assert lo == seen and hi == (96 if D == 96 else max(D - 12, 0)), (chunk, D, lo, hi)
                    seen = hi
                got = run.y.cpu()
                assert bool((got[1, 45:] == 0).all())
                rep["chunk_%d" % chunk] = float((got.double() - ref).abs().max())
    finally:
        hip.set_precision("fp32")
        _record("postnet_%s_%s" % (leg, mode), rep)
    print("chunked post-net vs fp64", leg, mode, rep, "floor", floor)
    for chunk in (3, 15, 300):
        assert rep["chunk_%d" % chunk] <= max(2 * rep["one_shot"], floor), (chunk, rep, floor)


# ---------------------------------------------------------------------------------------------------------------------
# 3. model level
def _tiny_model(dev, dur_bias=None):
    from kantts.models.sambert.kantts_sambert import KanTtsSAMBERT

    torch.manual_seed(0)
    m = KanTtsSAMBERT(dict(O.sambert_config(tiny=True)))
    with torch.no_grad():  # as tests/test_ar_kernels.py::_model: make every term of the decoder's blobs matter
        for n, p in m.named_parameters():
            if n.endswith("bias") or "layer_norm" in n or n.endswith("ln.weight"):
                p.add_(0.1 * torch.randn_like(p))
        if dur_bias is not None:  # free-running durations of a few frames per token (tests/test_decode_graph.py)
            m.variance_adaptor.duration_predictor.fc.bias.fill_(dur_bias)
    m = m.to(dev).eval()
    m.mel_decoder.decode_mode = "kernel"
    return m


def _inputs(dev, case):
    batch = O.synthetic_sambert_batch(B=3, T_in=12, seed=4, min_len=6, dur_hi=6)
    args = {k: batch[k].to(dev) for k in ("inputs_ling", "inputs_emotion", "inputs_speaker", "input_lengths")}
    if case == "durations":  # 96, 45 and 6 frames: one ends in the middle of a chunk, one is shorter than the look-ahead
        args["input_lengths"] = torch.tensor([12, 9, 6], device=dev)
        dur = torch.zeros(3, 12, dtype=torch.int64)
        dur[0, :12], dur[1, :9], dur[2, :6] = 8, 5, 1
        args["duration_targets"] = dur.to(dev)
    return args


_MODEL_CACHE = {}


def _model_case(leg, dev, case):
    """Model, inputs and the one-shot forward of a (leg, case), computed once (inside the leg's context, bf16 mode)."""
    if (leg, case) not in _MODEL_CACHE:
        m = _tiny_model(dev, dur_bias=1.5 if case == "free" else None)
        args = _inputs(dev, case)
        with torch.no_grad():
            res = m(**args)
        assert m.mel_decoder._decode_kernel is not None, "the one-shot side did not take the one-launch decoder"
        _MODEL_CACHE[(leg, case)] = (m, args, res)
    return _MODEL_CACHE[(leg, case)]


def _play(ca, args, chunk_steps):
    sess = ca.open(**args)
    Tp = sess.steps * sess.r
    seen, D, n_calls = 0, 0, 0
    while not sess.finished:
        lo, hi, mel = sess.step(chunk_steps)
        n_calls += 1
        D = min(D + chunk_steps * sess.r, Tp)
        assert lo == seen, (lo, seen)
        assert hi == (Tp if D == Tp else min(max(D - ca.lookahead, 0), Tp)), (D, hi)
        assert tuple(mel.shape) == (sess.B, hi - lo, 80)
        seen = hi
        assert n_calls <= sess.steps + 1
    assert seen == Tp
    return sess, sess.result()


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("chunk_steps", [1, 5, 32, 100])
@pytest.mark.parametrize("case", ["durations", "free"])
def test_chunked_acoustic_matches_forward(case, chunk_steps, leg):
    import kantts._hip as hip
    from kantts.models.sambert.chunked import ChunkedAcoustic

    ctx, dev = _leg(leg)
    hip.set_precision("bf16")
    try:
        with ctx:
            m, args, ref = _model_case(leg, dev, case)
            ca = ChunkedAcoustic(m)
            assert ca.lookahead == 12
            sess, got = _play(ca, args, chunk_steps)
            assert set(got) == set(ref)
            frames = [int(v) for v in ref["LR_length_rounded"]]
            if case == "durations":
                assert frames == [96, 45, 6] and sess.steps == 32
            assert torch.equal(sess.frames, ref["LR_length_rounded"])
            for k in ("dec_outputs", "LR_length_rounded", "log_duration_predictions", "pitch_predictions", "energy_predictions"):
                assert torch.equal(got[k], ref[k]), k
            a, b = got["postnet_outputs"].cpu(), ref["postnet_outputs"].cpu()
            scale = float(b.abs().max())
            err = (rel_l2(a, b), float((a - b).abs().max()))
            print("chunked acoustic vs forward", leg, case, chunk_steps, "rel_l2 %.3e max-abs %.3e scale %.3e" % (err + (scale,)))
            assert err[0] < 3e-3 and err[1] < 3e-2 * scale, err
            for bi, n in enumerate(frames):
                assert bool((a[bi, n:] == 0).all()) and bool((got["dec_outputs"][bi, n:] == 0).all()), bi
            if chunk_steps == 5:  # a second session on the same object reproduces the first bit for bit
                _, again = _play(ca, args, chunk_steps)
                assert torch.equal(again["postnet_outputs"], got["postnet_outputs"])
                assert torch.equal(again["dec_outputs"], got["dec_outputs"])
    finally:
        hip.set_precision("fp32")


@pytest.mark.parametrize("leg", LEGS)
def test_chunked_acoustic_refuses_what_it_cannot_stream(leg):
    import kantts._hip as hip
    from kantts.models.sambert.chunked import ChunkedAcoustic

    ctx, dev = _leg(leg)
    try:
        with ctx:
            m = _tiny_model(dev)
            hip.set_precision("fp32")
            with pytest.raises(ValueError):
                ChunkedAcoustic(m)
            hip.set_precision("bf16")
            m.train()
            with pytest.raises(ValueError):
                ChunkedAcoustic(m)
            m.eval()
            ca = ChunkedAcoustic(m)
            args = _inputs(dev, "durations")
            args["duration_targets"][0, 0] = 384  # band width int(384 / 3 + 0.5) = 128
            with pytest.raises(ValueError, match="band width"):
                ca.open(**args)
            sess = ca.open(**_inputs(dev, "durations"))
            sess.step(3)
            with pytest.raises(RuntimeError):
                sess.result()  # before the end
    finally:
        hip.set_precision("fp32")


def test_chunked_acoustic_says_so_under_the_emulated_abi():
    import kantts._hip as hip
    from kantts.models.sambert.chunked import ChunkedAcoustic

    hip.set_precision("bf16")
    try:
        with emulation():
            with pytest.raises(RuntimeError, match="range entry points"):
                ChunkedAcoustic(_tiny_model("cpu"))
    finally:
        hip.set_precision("fp32")


# ---------------------------------------------------------------------------------------------------------------------
# 4. CLI
class _FakeLingUnit:
    """Stands in for the text front-end: symbols are already integer streams (as tests/test_entrypoints.py)."""

    def __init__(self, cfg):
        self.cfg = cfg

    def using_byte(self):
        return False

    def get_unit_size(self):
        return {k: self.cfg[k] for k in O.SAMBERT_VOCAB}

    def encode_symbol_sequence(self, seq):
        n = len(seq.split()) + 1
        g = np.random.default_rng(n)
        return [g.integers(0, 5, n), g.integers(0, 5, n), g.integers(0, 5, n), g.integers(0, 5, n),
                g.integers(0, 5, n), np.zeros(n, dtype=np.int64)]


@pytest.mark.gpu
def test_infer_sambert_chunk_frames_cli_gpu(tmp_path):
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
    sent.write_text("utt_a\ta b c d e f g h i j k\nutt_b\tg h i j\n")
    hip.set_precision("bf16")
    try:
        am_infer(str(sent), ck, str(tmp_path / "whole"), ling_unit=_FakeLingUnit(cfg))
        am_infer(str(sent), ck, str(tmp_path / "chunked"), ling_unit=_FakeLingUnit(cfg), chunk_frames=15)
        with pytest.raises(ValueError, match="chunk_frames"):
            am_infer(str(sent), ck, str(tmp_path / "refused"), ling_unit=_FakeLingUnit(cfg), chunk_frames=16)
    finally:
        hip.set_precision("fp32")
    for utt in ("utt_a", "utt_b"):
        a = np.load(tmp_path / "whole" / "feat" / (utt + "_mel.npy"))
        b = np.load(tmp_path / "chunked" / "feat" / (utt + "_mel.npy"))
        assert a.shape == b.shape and (utt != "utt_a" or a.shape[0] > 15)  # utt_a spans several chunks
        scale = float(np.abs(a).max())
        assert rel_l2(torch.from_numpy(b), torch.from_numpy(a)) < 3e-3 and float(np.abs(a - b).max()) < 3e-2 * scale
        for ext in ("_dur.txt", "_f0.txt", "_energy.txt"):
            assert (tmp_path / "whole" / "feat" / (utt + ext)).read_bytes() == (tmp_path / "chunked" / "feat" / (utt + ext)).read_bytes()
