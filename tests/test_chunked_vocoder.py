"""Chunked HiFi-GAN inference with carried convolution state (csrc/sconv.hip, kantts/models/hifigan/chunked.py).

CPU leg: the kernel SOURCE on the host build (util.kernel_source_on_cpu) -- the emulated C ABI of oracle/ does not know
the entry point.  Bounds are the project's own for the same arithmetic: single layer fp32 2e-5
(test_conv_win_emulated_matches_torch), bf16 max-abs <= 4e-2 * max(1, |ref|max) (test_conv_win_gpu_matches_torch[bf16]);
generator fp32 wav mean-abs <= 1e-5 (the ``wtol`` of test_hifigan._check_models for the device arithmetic); V1 against the
reference fixture: fp32 mean-abs <= 1e-5 / max-abs <= 2e-4, bf16 mean-abs <= 2e-3 (_HIFI_B32_BOUNDS of
test_bench_config_parity.py) and, over the 256 samples after every chunk boundary, a max-abs error of at most twice the
one-shot path's max-abs error against the same fixture (measured in the same run)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

import hifigan_oracle as H
import test_bench_config_parity as _bench_parity
from util import GOLDEN, assert_close, kernel_source_on_cpu

# beside the parity report of the bench configurations (same scratch directory, same _record)
_REPORT = os.path.join(os.path.dirname(_bench_parity._REPORT), "chunked_vocoder_parity.json")


def _record(key, val):
    try:
        os.makedirs(os.path.dirname(_REPORT), exist_ok=True)
        d = json.load(open(_REPORT)) if os.path.exists(_REPORT) else {}
        d[key] = val
        json.dump(d, open(_REPORT, "w"), indent=1)
    except OSError:
        pass


# ---------------------------------------------------------------------------------------------------------------------
# 1. single layer against plain torch (fp64)
_CONV_CASES = [(80, 32, 7, 1), (32, 32, 3, 7), (16, 16, 11, 3), (32, 1, 7, 1)]
_POLY_CASES = [(64, 2, 32, 2), (32, 2, 16, 4)]  # (Cin, scale, Cout, J): N = scale * Cout, K = J taps, step 1
_SCHEDULES = [[8, 8, 8, 8, 8], [1] * 40, [5, 11, 3, 13, 8]]


def _play_layer(x, w_knc, bias, step, prec, schedule, device):
    """x (S, T, Cin) in chunks from zero state -> (S, T, N); asserts the state copy after every chunk."""
    import kantts._hip as hip

    S, T, Cin = x.shape
    K, N, _ = w_knc.shape
    Hh = (K - 1) * step
    ss = Hh * Cin + 8  # slot stride with a gap: a write past a slot's state would show up in the guard floats
    arena = torch.zeros(2, S, ss, device=device)
    arena[:, :, Hh * Cin:] = 7.0
    bf = prec == "bf16" and N > 1
    w = w_knc.to(torch.bfloat16 if bf else torch.float32).contiguous().to(device)
    outs, t0, par = [], 0, 0
    for Tc in schedule:
        xc = x[:, t0:t0 + Tc].contiguous().to(device)
        out = torch.empty(S, Tc, N, device=device)
        ok = hip.sconv(xc, arena[par, 0], arena[1 - par, 0], w, out, S=S, Tc=Tc, Cin=Cin, N=N, K=K, step=step, hist_ss=ss,
                       precision=hip.PREC_BF16 if prec == "bf16" else hip.PREC_FP32,
                       bias=None if bias is None else bias.to(device))
        assert ok
        # the state is a copy: the last H rows of [hist_in ; in], exactly -- also when Tc < H
        want = torch.cat([arena[par, :, :Hh * Cin].view(S, Hh, Cin), xc], dim=1)[:, Tc:]
        assert torch.equal(arena[1 - par, :, :Hh * Cin].view(S, Hh, Cin), want), "state after a chunk of %d" % Tc
        assert bool((arena[:, :, Hh * Cin:] == 7.0).all()), "guard floats between the slots were written"
        outs.append(out.cpu())
        t0 += Tc
        par ^= 1
    assert t0 == T
    return torch.cat(outs, dim=1)


def _check_layer(kind, case, prec, S, device):
    g = torch.Generator().manual_seed(3)
    T = 40
    if kind == "conv":
        Cin, N, K, step = case
        x = torch.randn(S, T, Cin, generator=g)
        W = torch.randn(N, Cin, K, generator=g) / (Cin * K) ** 0.5
        b = torch.randn(N, generator=g)
        ref = F.conv1d(F.pad(x.double().transpose(1, 2), ((K - 1) * step, 0)), W.double(), b.double(), dilation=step)
        ref = ref.transpose(1, 2)
        w_knc = W.permute(2, 0, 1).flip(0)
    else:
        Cin, s, Cout, J = case
        step, K, N = 1, J, s * Cout
        x = torch.randn(S, T, Cin, generator=g)
        W = torch.randn(Cin, Cout, J * s, generator=g) / (Cin * J) ** 0.5
        b = torch.randn(Cout, generator=g)
        ref = F.conv_transpose1d(x.double().transpose(1, 2), W.double(), b.double(), stride=s)[..., :T * s]
        ref = ref.transpose(1, 2).reshape(S, T, N)  # row q = the s output samples of input token q
        w_knc = W.view(Cin, Cout, J, s).permute(2, 3, 1, 0).reshape(J, N, Cin)
        b = b.repeat(s)
    for sched in _SCHEDULES:
        got = _play_layer(x, w_knc, b, step, prec, sched, device)
        if prec == "fp32" or N == 1:
            assert_close(got, ref.float(), 2e-5, what="%s %s S=%d %s" % (kind, case, S, sched[:3]))
        else:
            err = float((got.double() - ref).abs().max())
            assert err <= 4e-2 * max(1.0, float(ref.abs().max())), (kind, case, S, sched[:3], err)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", _CONV_CASES, ids=lambda c: "c%d_n%d_k%d_d%d" % c)
def test_sconv_layer_kernel_source_matches_torch(case, prec, S):
    with kernel_source_on_cpu():
        _check_layer("conv", case, prec, S, "cpu")


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("case", _POLY_CASES, ids=lambda c: "c%d_s%d_o%d_j%d" % c)
def test_sconv_polyphase_kernel_source_matches_torch(case, prec, S):
    with kernel_source_on_cpu():
        _check_layer("poly", case, prec, S, "cpu")


def test_sconv_declines_shapes_outside_its_contract():
    import kantts._hip as hip

    with kernel_source_on_cpu():
        x, out, st = torch.zeros(1, 4, 12), torch.zeros(1, 4, 16), torch.zeros(2, 1, 64)
        for Cin, N, K, step in [(12, 16, 3, 1), (8, 16, 3, 1), (520, 16, 3, 1), (16, 8, 3, 1), (16, 16, 13, 1), (16, 16, 3, 8)]:
            w = torch.zeros(K, N, Cin)
            assert hip.sconv(x, st[0], st[1], w, out, S=1, Tc=4, Cin=Cin, N=N, K=K, step=step, hist_ss=64,
                             precision=hip.PREC_FP32) is False
        # clamped lengths: nothing to do is not an error
        w = torch.zeros(3, 16, 16)
        assert hip.sconv(x, st[0], st[1], w, out, S=1, Tc=0, Cin=16, N=16, K=3, step=1, hist_ss=64, precision=hip.PREC_FP32)
        assert hip.sconv(x, st[0], st[1], w, out, S=-2, Tc=4, Cin=16, N=16, K=3, step=1, hist_ss=64, precision=hip.PREC_FP32)


# ---------------------------------------------------------------------------------------------------------------------
# 2. generator level, 3. refusals
_G64 = dict(channels=64, upsample_scales=[4, 2], upsample_kernal_sizes=[8, 4])


def _g64():
    from kantts.models.hifigan.hifigan import Generator

    torch.manual_seed(0)
    return Generator(**_G64).eval()


def _play(v, x, schedule):
    outs, t0 = [], 0
    for Tc in schedule:
        outs.append(v.step(x[:, :, t0:t0 + Tc].contiguous()))
        t0 += Tc
    assert t0 == x.shape[2]
    return torch.cat(outs, dim=2)


def test_chunked_generator_kernel_source_matches_oracle():
    import kantts._hip as hip
    from kantts.models.hifigan.chunked import ChunkedVocoder

    G = _g64()
    P = {k: v.detach().clone() for k, v in G.state_dict().items()}
    x = torch.randn(2, 80, 8)
    with torch.no_grad():
        ref = H.generator(P, x, scales=(4, 2))
    hip.set_precision("fp32")
    with kernel_source_on_cpu():
        v = ChunkedVocoder(G, slots=2, graph=False)
        assert v.state_floats == sum(L.H * L.Cin for L in v.layers) and len(v.layers) == 1 + 2 * 19 + 1
        for sched in ([3, 1, 4], [8]):
            v.reset()
            wav = _play(v, x, sched)
            assert wav.shape == ref.shape == (2, 1, 64)
            err = float((wav - ref).abs().mean())
            print("chunked generator (kernel source)", sched, "mean-abs", err)
            assert err <= 1e-5, (sched, err)


def test_chunked_vocoder_refuses_what_it_cannot_play():
    from kantts.models.hifigan.chunked import ChunkedVocoder
    from kantts.models.hifigan.hifigan import Generator

    class _NoLaunch:
        def __getattr__(self, name):
            raise AssertionError("a refusal must not reach the library (%s)" % name)

    import kantts._hip as hip

    torch.manual_seed(0)
    cases = [
        (Generator(causal=False, **_G64), ValueError),
        (Generator(nsf_params={"nb_harmonics": 7, "sampling_rate": 16000}, in_channels=80, **_G64), NotImplementedError),
        (Generator(out_channels=4, **_G64), NotImplementedError),
        (Generator(channels=32), NotImplementedError),  # 2-channel last stage
    ]
    import kantts._hip.ops as ops
    import kantts._hip.ops_bf16 as ops_bf16

    saved = [(m, m.lib) for m in (hip, ops, ops_bf16)]
    for m, _ in saved:
        m.lib = lambda: _NoLaunch()
    try:
        for G, exc in cases:
            with pytest.raises(exc):
                ChunkedVocoder(G.eval(), slots=1, graph=False)
    finally:
        for m, f in saved:
            m.lib = f


# ---------------------------------------------------------------------------------------------------------------------
# GPU
@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_sconv_layer_gpu_matches_torch(prec):
    """The single-layer cases of the CPU leg on the device (same bounds), plus wide / long shapes of the shipped models."""
    for case in _CONV_CASES + [(512, 512, 11, 5), (256, 256, 7, 7), (128, 16, 3, 1)]:
        for S in (1, 3):
            _check_layer("conv", case, prec, S, "cuda")
    for case in _POLY_CASES + [(512, 8, 256, 2), (256, 10, 128, 2), (64, 3, 32, 3)]:
        for S in (1, 3):
            _check_layer("poly", case, prec, S, "cuda")


def _boundaries(schedule, hop):
    t, out = 0, []
    for Tc in schedule[:-1]:
        t += Tc
        out.append(t * hop)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_chunked_v1_gpu_matches_reference_fixture(mode):
    """The 32 utterances of tests/golden/hifigan_v1_b32.pt through 4 slots, eight rounds of four; reset() between rounds,
    in every second round slot by slot; graph replay and eager launches give identical bits."""
    import kantts._hip as hip
    from kantts.models.hifigan.chunked import ChunkedVocoder
    from kantts.models.hifigan.hifigan import Generator

    fix = torch.load(os.path.join(GOLDEN, "hifigan_v1_b32.pt"), weights_only=False)
    g = torch.Generator().manual_seed(fix["seed"])
    x = torch.randn(32, 80, 32, generator=g).cuda()
    ref = fix["wav"]
    torch.manual_seed(0)
    G = Generator().eval().cuda()
    rep = {}
    hip.set_precision(mode)
    try:
        with torch.no_grad():
            one = G(x).cpu()
        e1 = (one - ref).abs()
        rep["one_shot"] = (float(e1.mean()), float(e1.max()))
        vs = {gr: ChunkedVocoder(G, slots=4, graph=gr) for gr in (True, False)}
        # 1 + 4 fused dual-path stages + 72 residual convolutions + 1; the stages carry J - 1 = 1, 1, 3, 3 input tokens
        # (1344 floats) where the unfused pair of the reference would carry 1 token + 6 repeated rows (6720)
        assert vs[True].state_floats == 111072 - 6720 + 1344 and len(vs[True].layers) == 78
        for name, sched, rounds in (("8x4", [8, 8, 8, 8], 8), ("5_11_3_13", [5, 11, 3, 13], 8), ("1x32", [1] * 32, 1)):
            wavs = {}
            for gr, v in vs.items():
                got = []
                for r in range(rounds):
                    if r % 2:
                        for s in range(4):
                            v.reset(s)
                    else:
                        v.reset()
                    got.append(_play(v, x[4 * r:4 * r + 4], sched).cpu())
                wavs[gr] = torch.cat(got, dim=0)
            assert torch.equal(wavs[True], wavs[False]), "graph replay and eager launches differ (%s)" % name
            err = (wavs[True] - ref[:4 * rounds]).abs()
            per_utt_mean = err.mean(dim=(1, 2))
            mask = torch.zeros(err.shape[-1], dtype=torch.bool)
            for b in _boundaries(sched, 256):
                mask[b:b + 256] = True
            rep[name] = dict(mean_worst_utt=float(per_utt_mean.max()), max=float(err.max()),
                             boundary_max=float(err[..., mask].max()))
            print("chunked V1 vs reference", mode, name, rep[name], "one-shot (mean, max)", rep["one_shot"])
    finally:
        hip.set_precision("fp32")
        _record("v1_b32_" + mode, rep)
    for name in ("8x4", "5_11_3_13", "1x32"):
        if mode == "fp32":
            assert rep[name]["mean_worst_utt"] <= 1e-5 and rep[name]["max"] <= 2e-4, (name, rep)
        else:
            assert rep[name]["mean_worst_utt"] <= 2e-3, (name, rep)
            assert rep[name]["boundary_max"] <= 2 * rep["one_shot"][1], (name, rep)


_SHIPPED = {
    # reference kantts/configs/hifigan_v1_16k.yaml / hifigan_v1_24k.yaml, Model.Generator.params
    "16k": dict(channels=256, upsample_scales=[10, 5, 2, 2], upsample_kernal_sizes=[20, 10, 4, 4],
                resblock_kernel_sizes=[3, 7, 11], resblock_dilations=[[1, 3, 5, 7]] * 3),
    "24k": dict(channels=512, upsample_scales=[8, 5, 3, 2], upsample_kernal_sizes=[16, 10, 6, 4],
                resblock_kernel_sizes=[3, 7, 11], resblock_dilations=[[1, 3, 5]] * 3),
}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("cfg", ["16k", "24k"])
def test_chunked_shipped_shapes_gpu_match_oracle(cfg, mode):
    import kantts._hip as hip
    from kantts.models.hifigan.chunked import ChunkedVocoder
    from kantts.models.hifigan.hifigan import Generator

    p = _SHIPPED[cfg]
    torch.manual_seed(0)
    G = Generator(**p).eval()
    P = {k: v.detach().clone() for k, v in G.state_dict().items()}
    x = torch.randn(2, 80, 24)
    with torch.no_grad():
        ref = H.generator(P, x, scales=tuple(p["upsample_scales"]), dilations=tuple(tuple(d) for d in p["resblock_dilations"]))
    G = G.cuda()
    rep = {}
    hip.set_precision(mode)
    try:
        v = ChunkedVocoder(G, slots=2, graph=True)
        for sched in ([8, 8, 8], [7, 1, 16]):
            v.reset()
            wav = _play(v, x.cuda(), sched).cpu()
            assert wav.shape == ref.shape
            rep[str(sched)] = float((wav - ref).abs().mean())
    finally:
        hip.set_precision("fp32")
        _record("shipped_%s_%s" % (cfg, mode), rep)
    print("chunked", cfg, mode, rep)
    for k, e in rep.items():
        assert e <= (1e-5 if mode == "fp32" else 2e-3), (k, rep)


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [True, False])
def test_chunked_slots_are_independent_gpu(graph):
    import kantts._hip as hip
    from kantts.models.hifigan.chunked import ChunkedVocoder

    hip.set_precision("fp32")
    G = _g64().cuda()
    g = torch.Generator().manual_seed(5)
    A, B, C = (torch.randn(80, 32, generator=g).cuda() for _ in range(3))
    v = ChunkedVocoder(G, slots=2, graph=graph)
    got = []
    for i in range(4):
        if i == 2:
            v.reset(1)
        other = B[:, 8 * i:8 * i + 8] if i < 2 else C[:, 8 * (i - 2):8 * (i - 2) + 8]
        got.append(v.step(torch.stack([A[:, 8 * i:8 * i + 8], other]))[0])
    w = ChunkedVocoder(G, slots=2, graph=graph)
    alone = [w.step(torch.stack([A[:, 8 * i:8 * i + 8], torch.zeros(80, 8, device="cuda")]))[0] for i in range(4)]
    assert torch.equal(torch.cat(got, dim=1), torch.cat(alone, dim=1))
    # and the slot that was reset plays C as a fresh vocoder would
    v.reset()
    c_fresh = torch.cat([v.step(torch.stack([torch.zeros(80, 8, device="cuda"), C[:, 8 * i:8 * i + 8]]))[1] for i in range(2)], dim=1)
    w.reset()
    for i in range(2):
        w.step(torch.stack([A[:, 8 * i:8 * i + 8], B[:, 8 * i:8 * i + 8]]))
    w.reset(1)
    c_after = torch.cat([w.step(torch.stack([A[:, 16 + 8 * i:24 + 8 * i], C[:, 8 * i:8 * i + 8]]))[1] for i in range(2)], dim=1)
    assert torch.equal(c_fresh, c_after)


@pytest.mark.gpu
def test_infer_hifigan_chunk_frames_cli_gpu(tmp_path):
    import kantts._hip as hip
    from kantts.bin.infer_hifigan import hifigan_infer
    from scipy.io import wavfile

    hip.set_precision("fp32")
    voc_dir = tmp_path / "voc" / "ckpt"
    voc_dir.mkdir(parents=True)
    (tmp_path / "voc" / "config.yaml").write_text(yaml.dump(
        {"Model": {"Generator": {"params": _G64}}, "audio_config": {"sampling_rate": 16000}}))
    torch.save({"model": {"generator": _g64().state_dict()}}, voc_dir / "checkpoint_1.pth")
    np.save(tmp_path / "utt_a.npy", np.random.default_rng(0).standard_normal((21, 80)).astype(np.float32))
    ck = str(voc_dir / "checkpoint_1.pth")
    hifigan_infer(str(tmp_path / "utt_a.npy"), ck, str(tmp_path / "whole"))
    hifigan_infer(str(tmp_path / "utt_a.npy"), ck, str(tmp_path / "chunked"), chunk_frames=8)
    _, a = wavfile.read(tmp_path / "whole" / "utt_a_gen.wav")
    _, b = wavfile.read(tmp_path / "chunked" / "utt_a_gen.wav")
    assert a.dtype == b.dtype == np.int16 and a.shape == b.shape == (21 * 8,)
    assert int(np.abs(a.astype(np.int32) - b.astype(np.int32)).max()) <= 1
