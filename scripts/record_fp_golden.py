"""TEST INFRASTRUCTURE -- records tests/golden/sambert_tiny_fp.pt by running the UNTOUCHED reference on the CPU with the
tiny SAM-BERT configuration plus ``FP: True`` (the filled-pause voice, configs/sambert_fp_8k.yaml).

    python scripts/record_fp_golden.py            # needs the reference tree (oracle/ref_harness.py)

The file holds data only: seeded inputs, reference outputs / losses, per-parameter gradient summaries and a checksum per
state_dict entry (the weights are reproduced from the seed, as for the other sambert_tiny_* fixtures).

(a) ``train``: teacher-forced forward + backward in eval() (dropout off) at B = 3, T = 7, lengths 7 / 5 / 4, with
    ``fp_label`` (five insertions of all three classes, inter lengths 16 / 8 / 7, so T' = 16 and delta = 9 > T: the
    reference's padding wraps twice).  The targets are as wide as the inter lengths.  ``insert_fp`` is also called on its
    own and its four outputs are kept together with the text_hid and the filler rows it saw.
(b) ``infer``: free-running inference at B = 1 (the reference's own batched inference fails, with or without FP) with
    duration_predictor.fc.bias = 1.5 as sambert_tiny_infer; the batch seed is the first one whose predicted insertions
    have at least two different classes.
``FpCELoss`` is used unmodified; its constructor's ``.cuda()`` is redirected to a no-op while it runs.
"""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_harness  # noqa: E402

ref_harness.import_reference()
import torch_oracle as O  # noqa: E402
from kantts.models.sambert.kantts_sambert import KanTtsSAMBERT  # noqa: E402
from kantts.models.utils import get_mask_from_lengths  # noqa: E402
from kantts.train.loss import FpCELoss, MelReconLoss, ProsodyReconLoss  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "sambert_tiny_fp.pt")
# fixed filler ids (sy, tone, syllable_flag, word_segment) x 3 tokens: inside the tiny vocabulary, all different
FP_IDS = {1: [[5, 4, 0, 0], [17, 4, 1, 1], [140, 6, 2, 4]],
          2: [[6, 4, 0, 0], [23, 4, 1, 1], [140, 6, 2, 4]],
          3: [[5, 4, 0, 0], [41, 4, 1, 1], [140, 6, 2, 4]]}
FP_LABEL = [[0, 1, 0, 0, 2, 0, 3], [0, 0, 3, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0]]
LENS = [7, 5, 4]


def checksums(sd):
    return {k: (tuple(v.shape), float(v.double().sum()), float(v.double().abs().sum())) for k, v in sd.items()}


def fp_config():
    cfg = O.sambert_config(tiny=True)
    cfg["FP"] = True
    return cfg


def fp_dict():
    return {k: torch.tensor(v, dtype=torch.long).unsqueeze(0) for k, v in FP_IDS.items()}


def build(seed_w):
    torch.manual_seed(seed_w)
    m = KanTtsSAMBERT(dict(fp_config()))
    m.eval()
    m.fp_dict = fp_dict()
    return m


def train_batch(seed=2024, dur_hi=6):
    """Token side of width T = 7, target side of width T' = 16 (the inter lengths)."""
    g = torch.Generator().manual_seed(seed)
    B, T = len(LENS), len(FP_LABEL[0])
    lens = torch.tensor(LENS)
    label = torch.tensor(FP_LABEL)
    inter = lens + 3 * (label > 0).sum(1)
    Tp = T + int(inter.max()) - int(lens.max())
    V = (147, 10, 8, 8)
    ling = torch.stack([torch.randint(0, V[k] - 3, (B, T), generator=g) for k in range(4)], -1)
    emo = torch.randint(0, 33, (B, T), generator=g)
    spk = torch.zeros(B, T, dtype=torch.long)
    dur = torch.randint(2, dur_hi, (B, Tp), generator=g)
    dur = dur * (torch.arange(Tp)[None, :] < inter[:, None])
    out_lens = dur.sum(1)
    T_mel = int(math.ceil(int(out_lens.max()) / 3) * 3)
    for b in range(B):
        pad = T_mel - int(out_lens[b])
        if int(inter[b]) < Tp:
            dur[b, inter[b]] = pad          # the slot after the last token takes the r-padding (Padder._pad_durations)
        else:                               # no such slot: the frames are real ones of the last token
            dur[b, Tp - 1] += pad
            out_lens[b] += pad
    mel = torch.randn(B, T_mel, 80, generator=g)
    mel = mel * (torch.arange(T_mel)[None, :, None] < out_lens[:, None, None])
    pitch = torch.randn(B, Tp, generator=g)
    energy = torch.randn(B, Tp, generator=g)
    return dict(inputs_ling=ling, inputs_emotion=emo, inputs_speaker=spk, input_lengths=lens, output_lengths=out_lens,
                mel_targets=mel, duration_targets=dur, pitch_targets=pitch, energy_targets=energy, fp_label=label)


def train_case(seed_w=0):
    m = build(seed_w)
    batch = train_batch()
    # insert_fp on its own, on the reference's text_hid (no gradient: its in-place row assignment needs none here)
    with torch.no_grad():
        masks = get_mask_from_lengths(batch["input_lengths"], max_len=batch["inputs_ling"].size(1))
        text_hid, _, _ = m.text_encoder(batch["inputs_ling"], masks, return_attns=True)
        fillers = torch.stack([m.text_encoder(m.fp_dict[c], return_attns=True)[0].squeeze() for c in (1, 2, 3)])
        fp_p = m.FP_predictor(text_hid)
        ins = m.insert_fp(text_hid.clone(), fp_p, batch["fp_label"], m.fp_dict, batch["inputs_emotion"],
                          batch["inputs_speaker"], batch["input_lengths"], masks)
    res = m(**{k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()})
    mel_, mel = MelReconLoss()(batch["output_lengths"], batch["mel_targets"], res["dec_outputs"], res["postnet_outputs"])
    d, p, e = ProsodyReconLoss()(res["valid_inter_lengths"], res["duration_targets"], res["pitch_targets"],
                                 res["energy_targets"], res["log_duration_predictions"], res["pitch_predictions"],
                                 res["energy_predictions"])
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self   # FpCELoss.__init__ moves its weight with .cuda(): stay on the host
    try:
        fp_crit = FpCELoss()
    finally:
        torch.Tensor.cuda = orig_cuda
    fp = fp_crit(batch["input_lengths"], res["fp_predictions"], batch["fp_label"])
    total = mel_ + mel + d + p + e + fp
    total.backward()
    gsum = {n: (float(p_.grad.double().sum()), float(p_.grad.double().norm())) for n, p_ in m.named_parameters()
            if p_.grad is not None}
    keep = ["dec_outputs", "postnet_outputs", "LR_length_rounded", "log_duration_predictions", "LR_spk_outputs",
            "fp_predictions", "valid_inter_lengths"]
    return dict(batch=batch, text_hid=text_hid, fillers=fillers,
                insert_fp=dict(text_hid=ins[0], inputs_emotion=ins[1], inputs_speaker=ins[2], inter_lengths=ins[3]),
                outputs={k: res[k].detach().clone() for k in keep}, x_band_width=res["x_band_width"],
                losses=dict(mel_loss_=float(mel_), mel_loss=float(mel), dur_loss=float(d), pitch_loss=float(p),
                            energy_loss=float(e), fp_loss=float(fp), total=float(total)),
                grad_summaries=gsum, weight_checksums=checksums(m.state_dict()),
                state_keys=sorted(m.state_dict().keys()))


def decisions(fp_p, lens):
    """The reference's decision (kantts_sambert.py:787-791, :830-844) restated on its recorded probabilities."""
    valid = torch.arange(fp_p.size(1))[None, :] < lens[:, None]
    mask = (fp_p == fp_p.max(dim=2, keepdim=True)[0]).to(torch.int32)[:, :, 1:] * valid.unsqueeze(2)
    first = torch.where(mask[:, :, 0] == 1, 1, torch.where(mask[:, :, 1] == 1, 2, torch.where(mask[:, :, 2] == 1, 3, 0)))
    return first.to(torch.int32), mask.sum((1, 2)).to(torch.int32)


def infer_case(seed_w=0, T_in=8, dur_bias=1.5):
    m = build(seed_w)
    with torch.no_grad():
        m.variance_adaptor.duration_predictor.fc.bias.fill_(dur_bias)
    for seed_b in range(77, 400):
        batch = O.synthetic_sambert_batch(B=1, T_in=T_in, seed=seed_b, min_len=T_in - 2, dur_hi=6)
        args = {k: batch[k] for k in ("inputs_ling", "inputs_emotion", "inputs_speaker", "input_lengths")}
        with torch.no_grad():
            res = m(**{k: v.clone() for k, v in args.items()})
        label, number = decisions(res["fp_predictions"], args["input_lengths"])
        if len(set(label[label > 0].tolist())) >= 2:
            break
    else:
        raise RuntimeError("no batch seed gives insertions of two classes")
    keep = ["dec_outputs", "postnet_outputs", "LR_length_rounded", "log_duration_predictions", "pitch_predictions",
            "energy_predictions", "LR_text_outputs", "fp_predictions", "valid_inter_lengths"]
    return dict(seed_b=seed_b, dur_bias=dur_bias, batch=args, label=label, fp_number=number,
                outputs={k: res[k].detach().clone() for k in keep}, x_band_width=res["x_band_width"],
                weight_checksums=checksums(m.state_dict()))


def fpdict_case():
    """get_fpdict of the reference on its own sambert_fp_8k.yaml (PinYin): the ids a real FP voice gets."""
    import yaml
    from kantts.utils.ling_unit.ling_unit import get_fpdict

    with open(os.path.join(ref_harness.REFERENCE_ROOT, "kantts", "configs", "sambert_fp_8k.yaml")) as f:
        config = yaml.safe_load(f)
    ids = {k: torch.from_numpy(v).long() for k, v in get_fpdict(config).items()}
    return dict(unit=dict(config["linguistic_unit"]), ids=ids)


def _tok(sy, emo="emotion_neutral"):
    return "{%s$tone1$s_both$word_both$%s$F7}" % (sy, emo)


def fplabel_case():
    """get_fp_label of the reference (datasets/dataset.py:348-388) on three ``fpadd`` lines: the filler tokens carry
    emotion_disgust; one line per class."""
    from kantts.datasets.dataset import get_fp_label

    d = "emotion_disgust"
    n, h = "emotion_neutral", "emotion_happy"
    lines = [" ".join([_tok("a"), _tok("ga", d), _tok("a_c", d), _tok("b"), _tok("c")]),
             " ".join([_tok("a"), _tok("b"), _tok("ge", d), _tok("en_c", d), _tok("c"), _tok("a")]),
             " ".join([_tok("b"), _tok("ge", d), _tok("e_c", d), _tok("c"), _tok("a")]),
             # the ambiguous ones: a run at index 0 / 1, a tagged second token behind an untagged first, runs longer than
             # two tokens, adjacent runs, a run that ends the line, a line that starts with a filler and a happy token
             " ".join([_tok("ga", d), _tok("a_c", d), _tok("b"), _tok("c")]),
             " ".join([_tok("a"), _tok("ga", d), _tok("b"), _tok("c")]),
             " ".join([_tok("ge", d), _tok("b", n), _tok("c"), _tok("a")]),
             " ".join([_tok("ge", d), _tok("b", h), _tok("c")]),
             " ".join([_tok("a"), _tok("b"), _tok("ge", d), _tok("en_c", d), _tok("#3", d), _tok("c"), _tok("a")]),
             " ".join([_tok("a"), _tok("b"), _tok("ga", d), _tok("a_c", d), _tok("c"), _tok("ge", d), _tok("e_c", d),
                       _tok("a"), _tok("b")]),
             " ".join([_tok("a"), _tok("b"), _tok("ga", d), _tok("a_c", d), _tok("c"), _tok("ge", d), _tok("en_c", d)]),
             " ".join([_tok("a"), _tok("b"), _tok("c", h), _tok("ge", d), _tok("en_c", d)]),
             _tok("a")]
    return dict(lines=lines, labels=[get_fp_label(ln).tolist() for ln in lines])


def main():
    fix = dict(cfg=fp_config(), seed_w=0, fp_ids=FP_IDS, train=train_case(), infer=infer_case(), fpdict=fpdict_case(),
               fplabel=fplabel_case(), torch_version=str(torch.__version__))
    print("fp labels", fix["fplabel"]["labels"])
    torch.save(fix, OUT)
    inf = fix["infer"]
    print("sambert_tiny_fp: losses", fix["train"]["losses"], "\n infer seed", inf["seed_b"], "labels", inf["label"].tolist(),
          "number", inf["fp_number"].tolist(), "inter", inf["outputs"]["valid_inter_lengths"].tolist(), "frames",
          inf["outputs"]["LR_length_rounded"].tolist(), "xbw", inf["x_band_width"], "bytes", os.path.getsize(OUT))


if __name__ == "__main__":
    main()
