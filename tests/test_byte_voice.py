"""Byte-input voices (configs/sambert_16k_MAS_byte.yaml: ``using_byte: True``): one table of byte symbols where the other
voices sum four linguistic ones, carried through the model, the host collate, the device-resident corpus, the trainer
(eager and captured) and inference (one-shot, chunked, slots).

  * tests/golden/sambert_tiny_byte.pt (scripts/record_byte_golden.py): the untouched reference on the CPU with the tiny
    configuration plus ``MAS: True, using_byte: True, byte_index: 259`` at the geometry of sambert_tiny_mas (B = 3,
    T_in = 12) -- forward, the seven losses, backward, state_dict keys -- and the reference's KanTtsLinguisticUnit /
    AM_Dataset.collate_fn on byte items (``frontend``).

Legs: ``emulated`` (the numpy model of the C ABI: host logic), ``kernel_source`` (the kernel sources on the CPU) and, marked
``gpu``, the device.  Bounds of the model check are those of tests/test_mas.py::_check_mas_model; of the captured step those
of tests/test_mas.py::test_captured_mas_step_equals_eager_mas_step_gpu; of the device-side prior those of
tests/test_device_corpus_mas_se.py (one fp32 rounding of the fp64 value, at most 1e-3 of the live cells differing in bits);
of the alignment CTC those of tests/test_ctc.py; of the streamed frames those of tests/test_chunked_acoustic.py."""
import contextlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util import GOLDEN, assert_close, emulation, kernel_source_on_cpu, rel_l2

ALL_LEGS = [pytest.param("emulated", id="emulated"), pytest.param("hostsim", id="kernel_source"),
            pytest.param("cuda", id="gpu", marks=pytest.mark.gpu)]
LEGS = ALL_LEGS[1:]
_FIX = {}


def _leg(leg):
    ctx = {"emulated": emulation, "hostsim": kernel_source_on_cpu, "cuda": contextlib.nullcontext}[leg]()
    return ctx, ("cuda" if leg == "cuda" else "cpu")


def _fix():
    if "fix" not in _FIX:
        _FIX["fix"] = torch.load(os.path.join(GOLDEN, "sambert_tiny_byte.pt"), weights_only=False)
    return _FIX["fix"]


def _losses(m, res, b, epoch):
    from kantts.train.loss import AttentionBinarizationLoss, AttentionCTCLoss, MelReconLoss, ProsodyReconLoss

    mel_, mel = MelReconLoss()(b["output_lengths"], b["mel_targets"], res["dec_outputs"], res["postnet_outputs"])
    d, p, e = ProsodyReconLoss()(b["input_lengths"], res["duration_targets"], res["pitch_targets"], res["energy_targets"],
                                 res["log_duration_predictions"], res["pitch_predictions"], res["energy_predictions"])
    ctc = AttentionCTCLoss()(res["attn_logprob"], b["input_lengths"], b["output_lengths"])
    kl = AttentionBinarizationLoss()(epoch, res["attn_hard"], res["attn_soft"])
    total = mel_ + mel + d + p + e + ctc + kl
    return dict(mel_loss_=mel_, mel_loss=mel, dur_loss=d, pitch_loss=p, energy_loss=e, attn_ctc_loss=ctc, attn_kl_loss=kl,
                total=total)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the model against the reference fixture
@pytest.mark.parametrize("leg", ALL_LEGS)
def test_byte_model_matches_reference_fixture(leg):
    import kantts._hip as hip
    from kantts.models.sambert.kantts_sambert import KanTtsSAMBERT

    fix = _fix()
    ctx, dev = _leg(leg)
    hip.set_precision("fp32")
    with ctx:
        torch.manual_seed(fix["seed_w"])
        m = KanTtsSAMBERT(dict(fix["cfg"]))
        sd = m.state_dict()
        assert sorted(sd.keys()) == fix["state_keys"]  # byte_index_emb and none of the four linguistic tables
        assert tuple(sd["text_encoder.byte_index_emb.weight"].shape) == (259, fix["cfg"]["embedding_dim"])
        for k, (shape, s, a) in fix["weight_checksums"].items():
            assert tuple(sd[k].shape) == shape and abs(float(sd[k].double().sum()) - s) <= 1e-6 * max(1.0, a), k
        # a reference checkpoint (a state dict with exactly those keys) loads strictly
        m.load_state_dict({k: sd[k].clone() for k in fix["state_keys"]}, strict=True)
        m = m.to(dev).eval()
        b = {k: (v.clone().to(dev) if torch.is_tensor(v) else v) for k, v in fix["batch"].items()}
        assert tuple(b["inputs_ling"].shape) == (3, 12, 1)
        res = m(**b)
        loss = _losses(m, res, b, fix["epoch"])
        loss["total"].backward()
        losses = {k: float(v.detach()) for k, v in loss.items()}
    # tests/test_mas.py::_check_mas_model
    tol, out = 1e-5, fix["outputs"]
    assert torch.equal(res["attn_hard"].cpu(), out["attn_hard"])
    assert torch.equal(res["duration_targets"].cpu(), out["duration_targets"])
    assert torch.equal(res["LR_length_rounded"].cpu(), out["LR_length_rounded"])
    assert res["x_band_width"] == fix["x_band_width"]
    assert_close(res["attn_soft"].detach().cpu(), out["attn_soft"], 1e-5, what="attn_soft")
    assert_close(res["attn_logprob"].detach().cpu(), out["attn_logprob"], 1e-4, what="attn_logprob")
    for k in ["pitch_targets", "energy_targets", "dec_outputs", "postnet_outputs", "log_duration_predictions"]:
        dlt = (res[k].detach().cpu() - out[k]).abs()
        assert float(dlt.mean()) <= tol and float(dlt.max()) <= 20 * tol, (k, float(dlt.mean()), float(dlt.max()))
    for k, v in fix["losses"].items():
        assert abs(losses[k] - v) <= 1e-4 * max(1.0, abs(v)), (k, losses[k], v)
    named = dict(m.named_parameters())
    for k, g in fix["grads"].items():
        assert rel_l2(named[k].grad.cpu(), g) <= 1e-3, k
    for k, (s, nrm) in fix["grad_summaries"].items():
        assert named[k].grad is not None, k
        assert abs(float(named[k].grad.double().norm()) - nrm) <= 2e-3 * nrm + 1e-7, k


def test_byte_with_fp_or_se_is_refused_at_construction():
    from kantts.models.sambert.kantts_sambert import KanTtsSAMBERT

    for other in ("FP", "SE"):
        cfg = dict(_fix()["cfg"])
        cfg[other] = True
        with pytest.raises(NotImplementedError, match="using_byte together with %s" % other):
            KanTtsSAMBERT(cfg)


# ---------------------------------------------------------------------------------------------------------------------
# 2. host collate
def _reference_byte_collate(batch, unit_pad, lfeat_types):
    """reference dataset.py:699-707, :748-771, :781-783 line by line (the symbol streams and the lengths)."""
    from kantts.datasets.batching import Padder

    padder, data = Padder(), {}
    max_input_length = max(len(x[0][0]) for x in batch)
    lfeat_type_index = 0
    lfeat_type = lfeat_types[lfeat_type_index]
    inputs_byte_index = padder._prepare_scalar_inputs([x[0][lfeat_type_index] for x in batch], max_input_length,
                                                      unit_pad[lfeat_type]).long()
    data["input_lings"] = torch.stack([inputs_byte_index], dim=2)
    lfeat_type_index = lfeat_type_index + 1
    lfeat_type = lfeat_types[lfeat_type_index]
    data["input_emotions"] = padder._prepare_scalar_inputs([x[0][lfeat_type_index] for x in batch], max_input_length,
                                                           unit_pad[lfeat_type]).long()
    lfeat_type_index = lfeat_type_index + 1
    lfeat_type = lfeat_types[lfeat_type_index]
    data["input_speakers"] = padder._prepare_scalar_inputs([x[0][lfeat_type_index] for x in batch], max_input_length,
                                                           unit_pad[lfeat_type]).long()
    data["valid_input_lengths"] = torch.as_tensor([len(x[0][0]) - 1 for x in batch], dtype=torch.long)
    return data


def _byte_unit():
    from kantts.utils.ling_unit import KanTtsLinguisticUnit

    return KanTtsLinguisticUnit({"linguistic_unit": dict(_fix()["frontend"]["unit"])})


def _frontend_items(unit):
    from kantts.datasets.batching import beta_binomial_prior_distribution

    fe = _fix()["frontend"]
    items = []
    for line, enc, (ling, mel, f0, en) in zip(fe["lines"], fe["encoded"], fe["items"]):
        mine = unit.encode_symbol_sequence(line)
        assert len(mine) == 3 and all(np.array_equal(a, b) for a, b in zip(mine, enc))  # the reference's encoding
        items.append((mine, mel, None, f0, en, beta_binomial_prior_distribution(len(mine[0]), len(mel)), None, None))
    return items


def test_byte_collate_equals_the_reference_collate():
    from kantts.datasets.batching import am_collate

    fe = _fix()["frontend"]
    unit = _byte_unit()
    assert unit.using_byte() and unit.get_unit_size() == fe["unit_size"]
    pad_ids = [unit._sub_unit_pad[t] for t in unit._lfeat_type_list]
    assert pad_ids == fe["pad_ids"]
    items = _frontend_items(unit)
    got = am_collate(items, fe["r"], pad_ids)
    assert tuple(got["input_lings"].shape) == (2, 6, 1) and got["input_lings"].dtype == torch.int64
    assert got["valid_input_lengths"].tolist() == [3, 5]
    assert got["input_lings"][0, 4:, 0].tolist() == [pad_ids[0]] * 2 and got["input_emotions"][0, 4:].tolist() == [pad_ids[1]] * 2
    assert got["input_speakers"][0, 4:].tolist() == [pad_ids[2]] * 2
    restated = _reference_byte_collate(items, unit._sub_unit_pad, unit._lfeat_type_list)
    for k, v in restated.items():
        assert got[k].dtype == v.dtype and torch.equal(got[k], v), k
    ref = fe["collated"]  # what the reference's AM_Dataset.collate_fn returned for these items
    assert set(got) == set(ref)
    for k, v in ref.items():
        if v is None:
            assert got[k] is None, k
        else:
            assert got[k].dtype == v.dtype and torch.equal(got[k], v), k
    with pytest.raises(ValueError, match="pad ids"):
        am_collate(items, fe["r"], pad_ids + [0])


# ---------------------------------------------------------------------------------------------------------------------
# 3. the device-resident corpus
def _byte_items(n=6, seed=1, nsym=(5, 15), dur_hi=6):
    """Duration-free byte items in the manner of tests/test_device_corpus_mas_se.py::_items: three streams."""
    rng = np.random.RandomState(seed)
    items = []
    for _ in range(n):
        ns = int(rng.randint(*nsym))
        frames = int(rng.randint(1, dur_hi, size=ns - 1).sum())
        ling = [rng.randint(0, hi, size=ns).astype(np.int64) for hi in (256, 33, 4)]
        items.append((ling, rng.randn(frames, 80).astype(np.float32), None, rng.randn(frames).astype(np.float32),
                      rng.randn(frames).astype(np.float32), None, None, None))
    return items


def _with_host_prior(items):
    from kantts.datasets.batching import beta_binomial_prior_distribution

    return [it[:5] + (beta_binomial_prior_distribution(len(it[0][0]), len(it[1])),) + it[6:] for it in items]


def _same_batch(got, ref, what=""):
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    for k, v in ref.items():
        if v is None:
            assert got[k] is None, k
            continue
        assert got[k].shape == v.shape and got[k].dtype == v.dtype, (what, k, got[k].shape, got[k].dtype, v.shape, v.dtype)
        g = got[k].cpu()
        if k != "attn_priors":
            assert torch.equal(g, v), (what, k)
            continue
        for b, (P, M) in enumerate(zip((ref["valid_input_lengths"] + 1).tolist(), ref["valid_output_lengths"].tolist())):
            live = torch.zeros(v.shape[1:], dtype=torch.bool)
            live[:M, :P] = True
            assert bool((g[b][~live] == 0).all()), (what, b, "padding")
            err = (g[b].double() - v[b].double()).abs()
            assert bool((err <= 2.0 ** -23 * v[b].double() + 2.0 ** -126).all()), (what, b, float(err.max()))
            assert int((g[b][live] != v[b][live]).sum()) <= 1e-3 * P * M, (what, b)


PAD_IDS = [256, 33, 4]


@pytest.mark.parametrize("leg", LEGS)
def test_device_set_byte_batches_equal_the_host_collate(leg):
    from kantts.datasets.batching import am_collate
    from kantts.datasets.device_batching import DeviceAMSet

    ctx, dev = _leg(leg)
    items = _byte_items()
    host_items = _with_host_prior(items)
    with ctx:
        ds = DeviceAMSet(items, 3, PAD_IDS, dev)
        assert len(ds) == 6 and ds.mas and ds.ling.shape[1] == 3  # flat rows three wide
        for idx in ([0, 1, 2], [5, 3, 3, 4], [2]):
            ref = am_collate([host_items[i] for i in idx], 3, PAD_IDS)
            got = ds.batch(idx)
            assert got.get("band_width") is None
            got.pop("band_width", None)
            assert got["input_lings"].shape[2] == 1 and got["input_lings"].is_contiguous()
            assert all(v is None or v.device.type == dev for v in got.values())
            _same_batch(got, ref, "byte %s" % idx)
        with pytest.raises(ValueError, match="pad ids"):
            DeviceAMSet(items, 3, PAD_IDS + [0, 0, 0], dev)  # six pad ids for three streams


def _byte_voice_dataset(tmp, n=5):
    """A byte voice directory as AudioProcessor lays it out (no duration/, frame-level f0 / energy)."""
    from kantts.datasets.dataset import AM_Dataset

    unit = dict(_fix()["frontend"]["unit"])
    config = {"model_type": "sambert", "linguistic_unit": unit,
              "Model": {"KanTtsSAMBERT": {"params": {"outputs_per_step": 3, "MAS": True, "using_byte": True}}}}
    root = os.path.join(str(tmp), "data_byte")
    for d in ("mel", "f0", "energy", "frame_f0", "frame_uv"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    rs = np.random.RandomState(7)
    with open(os.path.join(root, "am_train.lst"), "w") as f:
        for u in range(n):
            name, text = "u%d" % u, ("byte %d é" % u).encode("utf-8")[: 4 + u]
            f.write("%s\t%s\n" % (name, " ".join("{%d$emotion_neutral$F7}" % c for c in text)))
            frames = int(rs.randint(2, 6, size=len(text)).sum())
            np.save(os.path.join(root, "mel", name + ".npy"), rs.randn(frames, 80).astype(np.float32))
            for d in ("f0", "energy"):
                np.save(os.path.join(root, d, name + ".npy"), rs.randn(frames).astype(np.float32))
    return AM_Dataset(config, os.path.join(root, "am_train.lst"), root)


def test_byte_dataset_items_and_collate(tmp_path):
    ds = _byte_voice_dataset(tmp_path)
    assert ds.ling_unit.using_byte() and ds.mas_enable and not ds.with_duration and len(ds) == 5
    items = [ds[i] for i in range(5)]
    assert all(len(it[0]) == 3 and it[2] is None for it in items)
    assert items[4][0][0].tolist()[:4] == list(b"byte") and items[4][0][0][-1] == ds.ling_unit._streams["byte_index"].eos
    out = ds.collate_fn(items[:3])
    assert tuple(out["input_lings"].shape) == (3, 7, 1) and out["valid_input_lengths"].tolist() == [4, 5, 6]
    assert out["durations"] is None and out["attn_priors"].shape == out["mel_targets"].shape[:2] + (7,)


@pytest.mark.gpu
def test_make_train_loader_serves_the_byte_voice_from_hbm(tmp_path):
    from kantts.datasets.batching import beta_binomial_prior_distribution
    from kantts.datasets.device_batching import DeviceCorpusLoader, make_train_loader

    ds = _byte_voice_dataset(tmp_path)
    host_items = [ds[i] for i in range(len(ds))]
    beta_binomial_prior_distribution.cache_clear()
    loader = make_train_loader("am", ds, None, "cuda", 2, mode="hbm")
    assert isinstance(loader, DeviceCorpusLoader) and loader.set.mas and loader.set.n_streams == 3
    assert beta_binomial_prior_distribution.cache_info().misses == 0 and ds.attach_prior is True
    for k, batch in enumerate(DeviceCorpusLoader(loader.set, 2, shuffle=False)):
        assert batch["input_lings"].is_cuda and batch["input_lings"].shape[2] == 1
        _same_batch(dict(batch), ds.collate_fn(host_items[2 * k: 2 * k + 2]), "byte voice directory")


# ---------------------------------------------------------------------------------------------------------------------
# 4. trainer steps: a long batch (more than 511 tokens: the wide alignment CTC), eager and captured
def _reference_attention_ctc(attn_logprob, in_lens, out_lens, blank_logprob=-1):
    """kantts/train/loss.py:488-508 of the reference (as tests/test_ctc.py restates it)."""
    ctc = torch.nn.CTCLoss(zero_infinity=True)
    padded = F.pad(attn_logprob, pad=(1, 0, 0, 0, 0, 0, 0, 0), value=blank_logprob)
    total = 0.0
    for bid in range(attn_logprob.shape[0]):
        target = torch.arange(1, int(in_lens[bid]) + 1).unsqueeze(0)
        cur = padded[bid].permute(1, 0, 2)[: int(out_lens[bid]), :, : int(in_lens[bid]) + 1]
        cur = torch.log_softmax(cur[None], dim=3)[0]
        total = total + ctc(cur, target, input_lengths=out_lens[bid:bid + 1], target_lengths=in_lens[bid:bid + 1])
    return total / attn_logprob.shape[0]


def _long_batch(in_lens=(530, 40), out_lens=(600, 90), seed=77):
    """Two byte utterances, one of them wider than the narrow CTC takes; the layout of ``sambert_mas_batch``."""
    from kantts.datasets.batching import beta_binomial_prior_distribution

    g = torch.Generator().manual_seed(seed)
    B, T_in, T_mel = len(in_lens), max(in_lens) + 1, (max(out_lens) + 2) // 3 * 3
    lens, olens = torch.tensor(in_lens), torch.tensor(out_lens)
    valid = torch.arange(T_mel)[None, :] < olens[:, None]
    pri = torch.zeros(B, T_mel, T_in)
    for b in range(B):
        p = beta_binomial_prior_distribution(in_lens[b] + 1, out_lens[b])
        pri[b, :p.shape[0], :p.shape[1]] = p
    return dict(inputs_ling=torch.randint(0, 256, (B, T_in, 1), generator=g), inputs_emotion=torch.randint(0, 33, (B, T_in), generator=g),
                inputs_speaker=torch.zeros(B, T_in, dtype=torch.long), input_lengths=lens, output_lengths=olens,
                mel_targets=torch.randn(B, T_mel, 80, generator=g) * valid[:, :, None], duration_targets=None,
                pitch_targets=torch.randn(B, T_mel, generator=g) * (torch.rand(B, T_mel, generator=g) > 0.3) * valid,
                energy_targets=torch.randn(B, T_mel, generator=g) * valid, attn_priors=pri)


def _no_dropout_cfg():
    cfg = dict(_fix()["cfg"])
    for k in list(cfg):
        if "dropout" in k:
            cfg[k] = 0.0
    return cfg


@pytest.mark.gpu
def test_long_byte_batch_forward_losses_backward_gpu():
    import kantts._hip as hip
    from kantts.models.sambert.kantts_sambert import KanTtsSAMBERT

    hip.set_precision("fp32")
    torch.manual_seed(0)
    m = KanTtsSAMBERT(_no_dropout_cfg()).cuda().eval()
    host = _long_batch()
    b = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in host.items()}
    res = m(**b)
    assert tuple(res["attn_logprob"].shape) == (2, 1, 600, 531)  # 1063 CTC states: the wide entry
    loss = _losses(m, res, b, 50)
    assert len(loss) == 8 and all(bool(torch.isfinite(v)) for v in loss.values())
    logprob = res["attn_logprob"]
    logprob.retain_grad()
    loss["total"].backward()
    for n, p in m.named_parameters():
        if p.grad is not None:
            assert bool(torch.isfinite(p.grad).all()), n
            if n.startswith("align_attention."):
                assert float(p.grad.abs().max()) > 0, n
    assert float(m.text_encoder.byte_index_emb.weight.grad.abs().max()) > 0
    # AttentionCTCLoss on the model's own attn_logprob against the restated loop in fp64 (bounds of tests/test_ctc.py)
    from kantts.train.loss import AttentionCTCLoss

    x = logprob.detach().cpu()
    xr = x.double().requires_grad_(True)
    ref = _reference_attention_ctc(xr, host["input_lengths"], host["output_lengths"])
    ref.backward()
    x32 = x.clone().requires_grad_(True)
    _reference_attention_ctc(x32, host["input_lengths"], host["output_lengths"]).backward()
    err_aten = float((x32.grad.double() - xr.grad).abs().max())
    xd = logprob.detach().clone().requires_grad_(True)
    got = AttentionCTCLoss()(xd, b["input_lengths"], b["output_lengths"])
    got.backward()
    assert abs(float(got.detach()) - float(loss["attn_ctc_loss"].detach())) <= 1e-6 * max(1.0, abs(float(ref.detach())))
    assert abs(float(got.detach()) - float(ref.detach())) <= 2e-5 * max(1.0, abs(float(ref.detach())))
    gmax, err = float(xr.grad.abs().max()), float((xd.grad.cpu().double() - xr.grad).abs().max())
    print("long byte batch: ctc %.6f ref %.6f, gradient err %.3e (gmax %.3e, ATen fp32 err %.3e)" % (
        float(got.detach()), float(ref.detach()), err, gmax, err_aten))
    assert err <= max(1e-4 * max(gmax, 1e-6), 4.0 * err_aten), (err, gmax, err_aten)


@pytest.mark.gpu
def test_captured_long_byte_step_equals_eager_step_gpu(tmp_path):
    """Sambert_Trainer(graph=True) on the long byte batch against the eager trainer: bounds of
    tests/test_mas.py::test_captured_mas_step_equals_eager_mas_step_gpu."""
    import kantts._hip as hip
    from kantts.models import model_builder
    from kantts.train.loss import criterion_builder
    from kantts.train.trainer import Sambert_Trainer
    from kantts.utils.synthetic import to_collate_format

    hip.set_precision("fp32")
    config = {"model_type": "sambert", "Model": {"KanTtsSAMBERT": {
        "params": _no_dropout_cfg(),
        "optimizer": {"type": "Adam", "params": {"lr": 0.001, "betas": [0.9, 0.98], "eps": 1e-9, "weight_decay": 0.0}},
        "scheduler": {"type": "NoamLR", "params": {"warmup_steps": 4000}}}},
        "Loss": {"MelReconLoss": {"enable": True, "params": {"loss_type": "mae"}},
                 "ProsodyReconLoss": {"enable": True, "params": {"loss_type": "mae"}},
                 "AttentionCTCLoss": {"enable": True},
                 "AttentionBinarizationLoss": {"enable": True, "params": {"start_epoch": 0, "warmup_epoch": 4}}},
        "grad_norm": 1.0, "batch_size": 2, "log_interval_steps": 1}
    batch = to_collate_format(_long_batch())

    def run(graph):
        torch.manual_seed(0)
        model, opt, sch = model_builder(config, device="cuda")
        model["KanTtsSAMBERT"].eval()
        crit = criterion_builder(config, "cuda")
        tr = Sambert_Trainer(config, model, opt, sch, crit, torch.device("cuda"), None, [batch], None, max_steps=10 ** 6,
                             save_dir=str(tmp_path / ("g" if graph else "e")), save_interval=10 ** 6, valid_interval=10 ** 6,
                             log_interval=1, grad_clip=1.0, graph=graph)
        tr.set_model_state = lambda state="train": None
        tr.epoch = 2
        losses = []
        for _ in range(3):
            losses.append(float(tr.train_step(batch)))
            tr.steps += 1
        return losses, tr.optimizer["KanTtsSAMBERT"].arena.flat.detach().cpu().clone(), tr

    le, fe, _ = run(False)
    lg, fg, trg = run(True)
    assert trg.with_MAS and len(trg._graphs) >= 1
    print("long byte step: eager %s captured %s weights rel-L2 %.2e" % (le, lg, float((fg - fe).norm() / fe.norm())))
    for a, b in zip(lg, le):
        assert abs(a - b) <= 2e-4 * max(1.0, abs(b)), (lg, le)
    assert float((fg - fe).norm() / fe.norm()) < 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# 5. inference
def test_am_inputs_takes_the_byte_branch():
    """reference infer_sambert.py:62-66, :87-122: one (1, T, 1) stream, the "~" dropped from every stream."""
    from kantts.bin.infer_sambert import am_inputs

    fe = _fix()["frontend"]
    unit = _byte_unit()
    for line, enc in zip(fe["lines"], fe["encoded"]):
        ling, emo, spk, n = am_inputs(line, unit, "cpu")
        T = len(enc[0]) - 1
        assert tuple(ling.shape) == (1, T, 1) and ling.dtype == torch.int64 and n.tolist() == [T]
        assert ling[0, :, 0].tolist() == enc[0][:-1].tolist()
        assert emo.tolist() == [enc[1][:-1].tolist()] and spk.tolist() == [enc[2][:-1].tolist()]


_STREAM_CACHE = {}


def _stream_case(leg, dev):
    """A tiny byte model (free-running durations of a few frames per token, as tests/test_chunked_acoustic.py::_tiny_model),
    one short utterance through ``am_inputs`` and the model's one-shot forward: once per leg, in bf16 mode."""
    from kantts.bin.infer_sambert import am_inputs
    from kantts.models.sambert.kantts_sambert import KanTtsSAMBERT

    if leg not in _STREAM_CACHE:
        torch.manual_seed(0)
        m = KanTtsSAMBERT(dict(_fix()["cfg"]))
        with torch.no_grad():
            for n, p in m.named_parameters():
                if n.endswith("bias") or "layer_norm" in n or n.endswith("ln.weight"):
                    p.add_(0.1 * torch.randn_like(p))
            m.variance_adaptor.duration_predictor.fc.bias.fill_(1.5)
        m = m.to(dev).eval()
        m.mel_decoder.decode_mode = "kernel"
        args = am_inputs(_fix()["frontend"]["lines"][1], _byte_unit(), dev)
        with torch.no_grad():
            ref = m(*args)
        assert m.mel_decoder._decode_kernel is not None, "the one-shot side did not take the one-launch decoder"
        _STREAM_CACHE[leg] = (m, args, ref)
    return _STREAM_CACHE[leg]


_KEYS_EXACT = ("dec_outputs", "LR_length_rounded", "log_duration_predictions", "pitch_predictions", "energy_predictions")


def _check_streamed(got, ref, what):
    assert set(got) == set(ref)
    for k in _KEYS_EXACT:
        assert torch.equal(got[k], ref[k]), (what, k)
    a, b = got["postnet_outputs"].cpu(), ref["postnet_outputs"].cpu()
    scale = float(b.abs().max())
    err = (rel_l2(a, b), float((a - b).abs().max()))
    print("byte voice", what, "rel_l2 %.3e max-abs %.3e scale %.3e" % (err + (scale,)))
    assert err[0] < 3e-3 and err[1] < 3e-2 * scale, (what, err)


@pytest.mark.parametrize("leg", LEGS)
def test_byte_model_streams_what_its_forward_gives(leg):
    import kantts._hip as hip
    from kantts.models.sambert.chunked import ChunkedAcoustic
    from kantts.models.sambert.slots import AcousticSlots

    ctx, dev = _leg(leg)
    hip.set_precision("bf16")
    try:
        with ctx:
            m, args, ref = _stream_case(leg, dev)
            frames = int(ref["LR_length_rounded"][0])
            assert frames > 0 and tuple(args[0].shape) == (1, 5, 1)
            sess = ChunkedAcoustic(m).open(*args)
            seen = 0
            for lo, hi, mel in sess.stream(4):
                assert lo == seen and tuple(mel.shape) == (1, hi - lo, 80)
                seen = hi
            assert seen == sess.steps * sess.r
            _check_streamed(sess.result(), ref, "chunked %s" % leg)
            pool = AcousticSlots(m, slots=2, max_steps=max(32, sess.steps))
            results = {}
            mels = [mel.clone() for _, _, _, mel in pool.play_many([args], 4, results=results)]
            _check_streamed(results[0], ref, "slots %s" % leg)
            assert torch.equal(torch.cat(mels), results[0]["postnet_outputs"][0])
    finally:
        hip.set_precision("fp32")
