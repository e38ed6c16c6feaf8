"""TEST INFRASTRUCTURE -- records tests/golden/sambert_tiny_byte.pt by running the UNTOUCHED reference on the CPU with the
tiny SAM-BERT configuration plus ``MAS: True, using_byte: True, byte_index: 259`` (the byte-input voice,
configs/sambert_16k_MAS_byte.yaml): one table of byte symbols instead of the four linguistic ones.

    python scripts/record_byte_golden.py          # needs the reference tree (oracle/ref_harness.py)

The file holds data only: the seeded batch, reference outputs / losses, per-parameter gradient summaries, a checksum per
state_dict entry (the weights are reproduced from the seed, as for the other sambert_tiny_* fixtures) and the sorted
state_dict keys.  Geometry of sambert_tiny_mas: B = 3, T_in = 12; the byte stream is drawn first, then the draws of
``synthetic_sambert_batch`` behind it.

``frontend``: the reference's KanTtsLinguisticUnit on a byte ``lfeat_type_list`` -- the encoded streams of one symbol line,
the pad ids and table sizes -- and AM_Dataset.collate_fn (dataset.py:690-827) called on two such items.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_harness  # noqa: E402

ref_harness.import_reference()
import torch_oracle as O  # noqa: E402
from kantts.datasets.dataset import AM_Dataset, Padder, beta_binomial_prior_distribution  # noqa: E402
from kantts.models.sambert.kantts_sambert import KanTtsSAMBERT  # noqa: E402
from kantts.train.loss import (AttentionBinarizationLoss, AttentionCTCLoss, MelReconLoss,  # noqa: E402
                               ProsodyReconLoss)
from kantts.utils.ling_unit.ling_unit import KanTtsLinguisticUnit  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "sambert_tiny_byte.pt")
UNIT = {"cleaners": "english_cleaners", "lfeat_type_list": "byte_index,emo_category,speaker_category",
        "speaker_list": "F7,F74,M7,FBYN"}
LINES = ["{104$emotion_neutral$F7} {105$emotion_neutral$F7} {33$emotion_happy$F7}",
         "{228$emotion_sad$M7} {189$emotion_sad$M7} {160$emotion_sad$M7} {32$emotion_sad$M7} {0$emotion_sad$M7}"]


def checksums(sd):
    return {k: (tuple(v.shape), float(v.double().sum()), float(v.double().abs().sum())) for k, v in sd.items()}


def byte_config():
    cfg = O.sambert_config(tiny=True)
    cfg.update(MAS=True, using_byte=True, byte_index=259)
    return cfg


def byte_batch(B=3, T_in=12, min_len=6, dur_hi=6, seed_b=4321):
    """The duration-free batch of sambert_tiny_mas (oracle/make_golden.py::mas_batch) with a (B, T_in, 1) byte stream."""
    g = torch.Generator().manual_seed(seed_b + 2)
    ling = torch.randint(0, 256, (B, T_in, 1), generator=g)
    batch = O.synthetic_sambert_batch(B=B, T_in=T_in, seed=seed_b, min_len=min_len, dur_hi=dur_hi)
    g = torch.Generator().manual_seed(seed_b + 1)
    T_mel = batch["mel_targets"].shape[1]
    valid = torch.arange(T_mel)[None, :] < batch["output_lengths"][:, None]
    pitch = torch.randn(B, T_mel, generator=g) * (torch.rand(B, T_mel, generator=g) > 0.3) * valid
    energy = torch.randn(B, T_mel, generator=g) * valid
    pri = torch.zeros(B, T_mel, T_in)
    for b in range(B):
        p = beta_binomial_prior_distribution(int(batch["input_lengths"][b]) + 1, int(batch["output_lengths"][b]))
        pri[b, :p.shape[0], :p.shape[1]] = p
    batch.update(inputs_ling=ling, duration_targets=None, pitch_targets=pitch, energy_targets=energy, attn_priors=pri)
    return batch


def model_case(seed_w=0, epoch=50):
    cfg = byte_config()
    torch.manual_seed(seed_w)
    m = KanTtsSAMBERT(dict(cfg))
    m.eval()
    batch = byte_batch()
    # binarize_attention_parallel ends with .to(attn.get_device()), which is -1 (invalid) for CPU tensors: give it the
    # tensor's device for the duration of the call -- no arithmetic is touched
    orig_get_device = torch.Tensor.get_device
    torch.Tensor.get_device = lambda self: self.device
    try:
        res = m(**{k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()})
    finally:
        torch.Tensor.get_device = orig_get_device
    mel_, mel = MelReconLoss()(batch["output_lengths"], batch["mel_targets"], res["dec_outputs"], res["postnet_outputs"])
    d, p, e = ProsodyReconLoss()(batch["input_lengths"], res["duration_targets"], res["pitch_targets"],
                                 res["energy_targets"], res["log_duration_predictions"], res["pitch_predictions"],
                                 res["energy_predictions"])
    ctc = AttentionCTCLoss()(res["attn_logprob"], batch["input_lengths"], batch["output_lengths"])
    kl = AttentionBinarizationLoss()(epoch, res["attn_hard"], res["attn_soft"])
    total = mel_ + mel + d + p + e + ctc + kl
    total.backward()
    grads = {n: p_.grad.clone() for n, p_ in m.named_parameters()
             if n.startswith("align_attention.") and p_.grad is not None and p_.numel() <= 20000}
    gsum = {n: (float(p_.grad.double().sum()), float(p_.grad.double().norm())) for n, p_ in m.named_parameters()
            if p_.grad is not None}
    keep = ["dec_outputs", "postnet_outputs", "LR_length_rounded", "log_duration_predictions", "attn_soft", "attn_hard",
            "attn_logprob", "duration_targets", "pitch_targets", "energy_targets"]
    return dict(cfg=cfg, seed_w=seed_w, epoch=epoch, batch=batch,
                outputs={k: res[k].detach().clone() for k in keep}, x_band_width=res["x_band_width"],
                losses=dict(mel_loss_=float(mel_), mel_loss=float(mel), dur_loss=float(d), pitch_loss=float(p),
                            energy_loss=float(e), attn_ctc_loss=float(ctc), attn_kl_loss=float(kl), total=float(total)),
                grads=grads, grad_summaries=gsum, weight_checksums=checksums(m.state_dict()),
                state_keys=sorted(m.state_dict().keys()), torch_version=str(torch.__version__))


def frontend_case():
    unit = KanTtsLinguisticUnit({"linguistic_unit": dict(UNIT), "Model": {"KanTtsSAMBERT": {"params": {}}}})
    assert unit.using_byte()
    encoded = [[np.asarray(s).astype(np.int64) for s in unit.encode_symbol_sequence(ln)] for ln in LINES]
    rs = np.random.RandomState(5)
    items = []
    for ling, frames in zip(encoded, (10, 17)):
        items.append((ling, rs.randn(frames, 80).astype(np.float32), None, rs.randn(frames).astype(np.float32),
                      rs.randn(frames).astype(np.float32), beta_binomial_prior_distribution(len(ling[0]), frames), None, None))
    me = types.SimpleNamespace(ling_unit=unit, padder=Padder(), with_duration=False, se_enable=False, fp_enable=False, r=3)
    collated = AM_Dataset.collate_fn(me, items)
    return dict(unit=dict(UNIT), lines=LINES, encoded=encoded,
                pad_ids=[int(unit._sub_unit_pad[t]) for t in unit._lfeat_type_list], unit_size=dict(unit.get_unit_size()),
                items=[(it[0], it[1], it[3], it[4]) for it in items], r=3,
                collated={k: (v.clone() if torch.is_tensor(v) else v) for k, v in collated.items()})


def main():
    fix = model_case()
    fix["frontend"] = frontend_case()
    torch.save(fix, OUT)
    print("sambert_tiny_byte: losses", fix["losses"], "\n keys", [k for k in fix["state_keys"] if "emb" in k][:6],
          "\n pad ids", fix["frontend"]["pad_ids"], "sizes", fix["frontend"]["unit_size"], "bytes", os.path.getsize(OUT))


if __name__ == "__main__":
    main()
