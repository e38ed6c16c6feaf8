"""Pins oracle/torch_oracle.py (and the product's parameter construction) against fixtures dumped
from the UNTOUCHED reference by oracle/make_golden.py.  CPU only; travels to the GPU box."""
import os

import pytest
import torch

import torch_oracle as O
from util import GOLDEN, assert_close


def _load(name):
    return torch.load(os.path.join(GOLDEN, name + ".pt"), weights_only=False)


def _product_weights(fix):
    from kantts.models.sambert.kantts_sambert import KanTtsSAMBERT

    torch.manual_seed(fix["seed_w"])
    m = KanTtsSAMBERT(dict(fix["cfg"]))
    return m.state_dict()


@pytest.mark.parametrize("name", ["sambert_tiny", "sambert_tiny16"])
def test_state_dict_matches_reference(name):
    """Same keys, shapes and (seeded) values as the reference's KanTtsSAMBERT.state_dict()."""
    fix = _load(name)
    sd = _product_weights(fix)
    ref = fix["weight_checksums"]
    assert list(sd.keys()) == list(ref.keys())
    for k, v in sd.items():
        shape, s, a = ref[k]
        assert tuple(v.shape) == tuple(shape), k
        assert abs(float(v.double().sum()) - s) <= 1e-9 * max(1.0, abs(a)), k
        assert abs(float(v.double().abs().sum()) - a) <= 1e-9 * max(1.0, abs(a)), k


@pytest.mark.parametrize("name", ["sambert_tiny", "sambert_tiny16"])
def test_oracle_reproduces_reference_outputs(name):
    fix = _load(name)
    sd = _product_weights(fix)
    P = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
    batch = O.synthetic_sambert_batch(**fix["batch_args"])
    out = O.sambert_forward(P, fix["cfg"], **batch)
    assert out["x_band_width"] == fix["x_band_width"] and out["h_band_width"] == fix["h_band_width"]
    assert torch.equal(out["LR_length_rounded"], fix["outputs"]["LR_length_rounded"])  # bit-exact
    for k, ref in fix["outputs"].items():
        if ref.is_floating_point():
            assert_close(out[k].detach(), ref, atol=2e-5, what=k)
    nb = 2
    assert_close(out["enc_slf_attn_lst"][0][:nb].detach(), fix["attn_checks"]["enc0"], 1e-6, what="enc attn")
    assert_close(out["pnca_x_attn_lst"][-1][:nb].detach(), fix["attn_checks"]["pnca_x_last"], 1e-6, what="x attn")
    assert_close(out["pnca_h_attn_lst"][-1][:nb].detach(), fix["attn_checks"]["pnca_h_last"], 1e-6, what="h attn")
    L = O.sambert_losses(out, batch["input_lengths"], batch["output_lengths"], batch["mel_targets"])
    for k, v in fix["losses"].items():
        assert abs(float(L[k]) - v) <= 2e-5 * max(1.0, abs(v)), k
    L["total"].backward()
    for k, g in fix["grads"].items():
        assert_close(P[k].grad, g, atol=1e-6 + 1e-4 * float(g.abs().max()), what="grad " + k)
    for k, (s, nrm) in fix["grad_summaries"].items():
        assert abs(float(P[k].grad.double().norm()) - nrm) <= 1e-3 * nrm + 1e-7, k


def test_audio_oracle_reproduces_reference():
    import audio_oracle as A

    fix = _load("melspec")
    x = fix["wav"]
    assert_close(A.mel_spectrogram(x), fix["mel_v1"], 2e-5, what="mel V1")
    assert_close(A.mel_spectrogram(x, 16000, 2048, 200, 1000, 80, 0, 8000), fix["mel_16k"], 2e-5, what="mel 16k")
    assert_close(A.stft_magnitude(x, 1024, 120, 600), fix["stft_1024_120_600"], 2e-5, what="stft")


def _infer_inputs(fix, B=None, seed=None):
    args = dict(fix["batch_args"])
    if B is not None:
        args["B"] = B
    if seed is not None:
        args["seed"] = seed
    batch = O.synthetic_sambert_batch(**args)
    return {k: batch[k] for k in ("inputs_ling", "inputs_emotion", "inputs_speaker", "input_lengths")}


def test_oracle_reproduces_reference_free_running_inference():
    """Free-running path (AR duration predictor, predicted-duration length regulation, AR decoder loop) of the
    oracle against the reference's own inference run (batch 1 -- the only size the reference can infer at)."""
    fix = _load("sambert_tiny_infer")
    sd = _product_weights(fix)
    sd["variance_adaptor.duration_predictor.fc.bias"] = torch.full_like(
        sd["variance_adaptor.duration_predictor.fc.bias"], fix["dur_bias"])
    with torch.no_grad():
        out = O.sambert_forward(dict(sd), fix["cfg"], **_infer_inputs(fix))
    assert out["x_band_width"] == fix["x_band_width"]
    assert torch.equal(out["LR_length_rounded"], fix["outputs"]["LR_length_rounded"])  # bit-exact frame counts
    for k, ref in fix["outputs"].items():
        if ref.is_floating_point():
            assert_close(out[k], ref, atol=2e-5, what=k)


def test_get_mask_from_lengths_bit_exact():
    """kantts.models.utils.get_mask_from_lengths and the oracle's pad_mask against masks recorded from the reference's
    own function (kantts/models/utils.py:13-23), with and without max_len; SeqInfo round-trips the lengths."""
    from kantts.models.utils import SeqInfo, get_mask_from_lengths

    for c in _load("masks"):
        m = get_mask_from_lengths(c["lengths"])
        assert m.dtype == torch.bool and torch.equal(m, c["mask"])
        assert torch.equal(get_mask_from_lengths(c["lengths"], max_len=c["max_len"]), c["mask_maxlen"])
        assert torch.equal(O.pad_mask(c["lengths"], c["max_len"]), c["mask_maxlen"])
        info = SeqInfo.of(c["mask_maxlen"])
        assert torch.equal(info.lens64, c["lengths"]) and torch.equal(info.mask, c["mask_maxlen"])


def test_mse_and_hinge_criteria_match_the_reference_classes():
    """The criteria variants no shipped yaml selects (loss_type="mse" of the reconstruction losses, loss_type="hinge" of the
    adversarial losses) against values and input gradients recorded from the reference classes
    (tests/golden/loss_variants.pt, oracle/make_golden.py::loss_variants_case).  They are plain elementwise arithmetic on
    whatever device the tensors live on, so the host tensors of the fixture exercise the shipped code."""
    from kantts.train.loss import (DiscriminatorAdversarialLoss, GeneratorAdversarialLoss, MelReconLoss,
                                   ProsodyReconLoss)

    fix = torch.load(os.path.join(GOLDEN, "loss_variants.pt"), weights_only=False)

    def close(a, b, tol=1e-6):
        assert torch.allclose(torch.as_tensor(a), torch.as_tensor(b), rtol=1e-5, atol=tol), (a, b)

    dec, post = fix["dec"].clone().requires_grad_(True), fix["post"].clone().requires_grad_(True)
    a, b = MelReconLoss("mse")(fix["output_lengths"], fix["mel_targets"], dec, post)
    (a + 2 * b).backward()
    for got, want in zip((a, b, dec.grad, post.grad), fix["mel_mse"]):
        close(got.detach(), want)
    only, zero = MelReconLoss("mse")(fix["output_lengths"], fix["mel_targets"], fix["dec"])
    close(only, fix["mel_mse_no_postnet"])
    assert zero == 0.0
    lp, pp, ep = (fix[k].clone().requires_grad_(True) for k in ("logdur_p", "pitch_p", "energy_p"))
    d, p, e = ProsodyReconLoss("mse")(fix["input_lengths"], fix["dur"], fix["pitch"], fix["energy"], lp, pp, ep)
    (d + 2 * p + 3 * e).backward()
    for got, want in zip((d, p, e, lp.grad, pp.grad, ep.grad), fix["prosody_mse"]):
        close(got.detach(), want)
    with pytest.raises(ValueError):
        MelReconLoss("huber")
    with pytest.raises(ValueError):
        ProsodyReconLoss("huber")

    fake, real, hinge = fix["d_fake"], fix["d_real"], fix["hinge"]
    for avg in (True, False):
        scores = [f[-1].clone().requires_grad_(True) for f in fake]
        v = GeneratorAdversarialLoss(average_by_discriminators=avg, loss_type="hinge")(scores)
        v.backward()
        want_v, want_g = hinge[("g_list", avg)]
        close(v.detach(), want_v)
        for s_, w in zip(scores, want_g):
            close(s_.grad, w)
        fk = [[t.clone().requires_grad_(True) for t in f] for f in fake]
        rl = [[t.clone().requires_grad_(True) for t in f] for f in real]
        r_, f_ = DiscriminatorAdversarialLoss(average_by_discriminators=avg, loss_type="hinge")(fk, rl)
        (r_ + 2 * f_).backward()
        want_r, want_f, gf, gr = hinge[("d_nested", avg)]
        close(r_.detach(), want_r)
        close(f_.detach(), want_f)
        for t, w in zip(fk, gf):
            close(t[-1].grad, w)
        for t, w in zip(rl, gr):
            close(t[-1].grad, w)
    one = fake[0][-1].clone().requires_grad_(True)
    v = GeneratorAdversarialLoss(loss_type="hinge")(one)
    v.backward()
    close(v.detach(), hinge["g_tensor"][0])
    close(one.grad, hinge["g_tensor"][1])
    r_, f_ = DiscriminatorAdversarialLoss(loss_type="hinge")(fake[1][-1], real[1][-1])
    close(r_, hinge["d_tensor"][0])
    close(f_, hinge["d_tensor"][1])
    with pytest.raises(AssertionError):
        GeneratorAdversarialLoss(loss_type="wasserstein")


def test_lstm_aten_equals_the_time_loop():
    """oracle/torch_oracle.py::lstm_aten (the ATen kernel the reference's nn.LSTM modules call, packed where the reference
    packs) against the readable time loop ``lstm_layer`` it replaced: values and gradients, uni- and bidirectional, one and
    two layers, ragged lengths (padded outputs zero, the reverse direction starting at each row's last valid token)."""
    import torch_oracle as O

    g = torch.Generator().manual_seed(3)
    B, T, C, H = 5, 11, 12, 8

    def weights(pre, layers, bidir):
        P = {}
        for l in range(layers):
            for sfx in ("", "_reverse") if bidir else ("",):
                cin = C if l == 0 else H * (2 if bidir else 1)
                for n, shape in (("weight_ih", (4 * H, cin)), ("weight_hh", (4 * H, H)), ("bias_ih", (4 * H,)), ("bias_hh", (4 * H,))):
                    P["%s.%s_l%d%s" % (pre, n, l, sfx)] = (0.4 * torch.randn(*shape, generator=g)).requires_grad_(True)
        return P

    for layers, bidir, lens in ((1, False, None), (2, False, None), (1, True, [11, 3, 7, 1, 11]), (1, True, None)):
        P = weights("m", layers, bidir)
        x = torch.randn(B, T, C, generator=g).requires_grad_(True)
        lengths = None if lens is None else torch.tensor(lens)
        got = O.lstm_aten(P, "m", x, layers, bidir, lengths)
        h = x
        for l in range(layers):
            outs = [O._lstm_named(P, "m", h, l, lengths, rev) for rev in ((False, True) if bidir else (False,))]
            h = torch.cat(outs, -1)
        assert got.shape == h.shape
        assert float((got - h).abs().max()) < 2e-6
        if lens is not None:
            for b, n in enumerate(lens):
                assert float(got[b, n:].abs().max() if n < T else 0.0) == 0.0
        w = torch.randn(got.shape, generator=g)
        ga = torch.autograd.grad((got * w).sum(), [x] + list(P.values()))
        gb = torch.autograd.grad((h * w).sum(), [x] + list(P.values()))
        for a, b in zip(ga, gb):
            assert float((a - b).abs().max()) < 1e-5 * max(1.0, float(b.abs().max()))


def _checksums_match(sd, ref, what):
    assert list(sd.keys()) == list(ref.keys()), what
    for k, (shape, s, a) in ref.items():
        assert tuple(sd[k].shape) == tuple(shape), (what, k)
        assert abs(float(sd[k].double().sum()) - s) <= 1e-9 * max(1.0, abs(a)), (what, k)


def _like(t, ref, what, max_abs=None, rel_l2=None):
    """``t`` against a make_golden.sketch() of the reference value, to the live check's bound on the whole tensor: the
    largest elementwise difference (``max_abs``) or ||t - ref|| / ||ref|| (``rel_l2``).  For a sketch, what that bound
    implies: on the sampled positions, the norm and the sum."""
    t = t.detach().double()
    assert tuple(t.shape) == tuple(ref["shape"]), (what, tuple(t.shape), ref["shape"])
    if "full" in ref:
        d, ref_norm = t - ref["full"].double(), float(ref["full"].double().norm())
        ok = float(d.abs().max()) <= max_abs if max_abs is not None else float(d.norm()) <= rel_l2 * ref_norm + 1e-30
        assert ok, (what, float(d.abs().max()), ref_norm)
        return
    flat = t.reshape(-1)
    n = flat.numel()
    d = flat[torch.linspace(0, n - 1, ref["sample"].numel()).long()] - ref["sample"].double()
    dsum, dnorm = abs(float(flat.sum()) - ref["sum"]), abs(float(flat.norm()) - ref["norm"])
    if max_abs is not None:
        ok = float(d.abs().max()) <= max_abs and dsum <= max_abs * n and dnorm <= max_abs * n ** 0.5
    else:
        bound = rel_l2 * ref["norm"] + 1e-30
        ok = float(d.norm()) <= bound and dnorm <= bound and dsum <= bound * n ** 0.5
    assert ok, (what, float(d.abs().max()), dsum, dnorm, ref["norm"])


def test_oracle_matches_reference_check_cases():
    """What oracle/check_vs_reference.py compares live, against the reference's values recorded by
    oracle/make_golden.py::check_cases_case: SAM-BERT at the tiny and the FULL configuration (outputs <= 2e-6, attention
    maps <= 1e-6, losses, every parameter gradient rel-L2 <= 1e-5), HiFi-GAN G / MPD / MSD at 512 and 64 generator
    channels (outputs <= 2e-6, feature maps <= 2e-5, every parameter gradient rel-L2 <= 1e-4) and a mel spectrogram
    (<= 1e-6).  Weights are rebuilt from the seed by the product's classes and must be the reference's (checksums)."""
    import audio_oracle as A
    import hifigan_oracle as H
    from kantts.models.hifigan.hifigan import Generator, MultiPeriodDiscriminator, MultiScaleDiscriminator
    from kantts.models.sambert.kantts_sambert import KanTtsSAMBERT

    fix = _load("check_cases_sambert")
    assert set(fix["sambert"]) == {"tiny", "full"}
    for name, rec in fix["sambert"].items():
        cfg = O.sambert_config(tiny=rec["tiny"])
        torch.manual_seed(0)
        sd = KanTtsSAMBERT(dict(cfg)).state_dict()
        _checksums_match(sd, rec["weight_checksums"], name)
        P = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in sd.items()}
        batch = O.synthetic_sambert_batch(**rec["batch_args"])
        out = O.sambert_forward(P, cfg, **batch)
        for k, ref in rec["outputs"].items():
            _like(out[k], ref, "%s %s" % (name, k), max_abs=2e-6)
        assert torch.equal(out["LR_length_rounded"], rec["LR_length_rounded"]), name
        assert out["x_band_width"] == rec["x_band_width"], name
        for k, refs in rec["attn"].items():
            assert len(out[k]) == len(refs), (name, k)
            for i, (a, ref) in enumerate(zip(out[k], refs)):
                _like(a, ref, "%s %s[%d]" % (name, k, i), max_abs=1e-6)
        L = O.sambert_losses(out, batch["input_lengths"], batch["output_lengths"], batch["mel_targets"])
        for k, v in rec["losses"].items():
            assert abs(float(L[k]) - v) <= 2e-5 * max(1.0, abs(v)), (name, k)
        L["total"].backward()
        for k, ref in rec["grads"].items():
            assert P[k].grad is not None, (name, k)
            _like(P[k].grad, ref, "%s grad %s" % (name, k), rel_l2=1e-5)

    fix = _load("check_cases_hifigan")
    assert set(fix["hifigan"]) == {512, 64}
    for channels, rec in fix["hifigan"].items():
        torch.manual_seed(0)
        G, D1, D2 = Generator(channels=channels), MultiPeriodDiscriminator(), MultiScaleDiscriminator()
        _checksums_match(G.state_dict(), rec["G_checksums"], "G %d" % channels)
        g = torch.Generator().manual_seed(1)
        xm = torch.randn(rec["B"], 80, rec["frames"], generator=g)
        yw = torch.randn(rec["B"], 1, rec["frames"] * 256, generator=g).clamp(-1, 1)
        PG = {k: v.detach().clone().requires_grad_(True) for k, v in G.state_dict().items()}
        wav = H.generator(PG, xm)
        _like(wav, rec["G_out"], "G %d out" % channels, max_abs=2e-6)
        wav.sum().backward()
        for k, ref in rec["G_grads"].items():
            _like(PG[k].grad, ref, "G %d grad %s" % (channels, k), rel_l2=1e-4)
        for D, f, nm in ((D1, H.mpd, "mpd"), (D2, H.msd, "msd")):
            r = rec[nm]
            _checksums_match(D.state_dict(), r["checksums"], "%s %d" % (nm, channels))
            P = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in D.state_dict().items()}
            o, fm = f(P, yw)
            assert len(o) == len(r["out"]) and len(fm) == len(r["fmaps"]), nm
            for i, (u, ref) in enumerate(zip(o, r["out"])):
                _like(u, ref, "%s %d out %d" % (nm, channels, i), max_abs=2e-6)
            for i, (fa, fb) in enumerate(zip(fm, r["fmaps"])):
                assert len(fa) == len(fb), (nm, i)
                for j, (u, ref) in enumerate(zip(fa, fb)):
                    _like(u, ref, "%s %d fmap %d.%d" % (nm, channels, i, j), max_abs=2e-5)
            (sum((u * u).mean() for u in o) + sum(u.abs().mean() for fa in fm for u in fa)).backward()
            for k, ref in r["grads"].items():
                _like(P[k].grad, ref, "%s %d grad %s" % (nm, channels, k), rel_l2=1e-4)

    mel = _load("check_cases_sambert")["mel"]
    got = A.mel_spectrogram(mel["x"])
    assert got.numel() == mel["mel"].numel()
    assert_close(got.reshape(mel["mel"].shape), mel["mel"], 1e-6, what="mel")
