"""TEST INFRASTRUCTURE -- records tests/golden/sybert_tiny.pt by running the UNTOUCHED reference on the CPU: the host side
of sy-BERT pre-training (MaskingActor, BERT_Text_Dataset) and KanTtsTextsyBERT + SeqCELoss at the tiny encoder
configuration.

    python scripts/record_sybert_golden.py            # needs the reference tree (oracle/ref_harness.py)

The file holds data only: seeded inputs, the arrays and scalars the reference computes from them, per-parameter gradient
summaries and a checksum per state_dict entry (the weights are reproduced from the seed, as for the sambert_tiny_*
fixtures).

(a) ``masking``: for seeds k = 0, 1, 2 and lengths 1, 2, 5, 12, 40, under ``np.random.seed(k); random.seed(k)``:
    ``_get_random_mask(L, 0.3)`` followed by ``_input_bert_masking`` on it, then -- seeded again --
    ``BERT_Text_Dataset.bert_masking``; and ``collate_fn`` of a three-item batch.  The dataset object is made without its
    constructor (which wants metafiles and language resources) and carries a stand-in for the linguistic unit that answers
    the four questions these methods ask (the [MASK] id, the inventory size, the stream names, the pad ids) with the
    PinYin sizes of SURVEY section 8; every line that runs is the reference's.
(b) ``model``: ``KanTtsTextsyBERT`` in eval(), B = 3, T = 7, ``input_lengths`` 6 / 4 / 3 (the lengths minus the closing
    "~").  The wrapper's own ``forward`` raises -- kantts_sambert.py:1060 unpacks two of the three values
    ``TextFftEncoder.forward`` returns (:337) -- so that ONE line is stepped around: the logits are
    ``model.fc(model.text_encoder(inputs_ling, masks, return_attns=True)[0])`` with ``masks`` exactly as :1058 builds them,
    i.e. the two statements around the broken one, module by module.  Then the reference's SeqCELoss, ``loss / V`` as
    trainer.py:1148,1171 divide it, and the gradients of that quotient.
"""
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_harness  # noqa: E402

ref_harness.import_reference()
import torch_oracle as O  # noqa: E402
from kantts.datasets.dataset import BERT_Text_Dataset, MaskingActor, Padder  # noqa: E402
from kantts.models.sambert.kantts_sambert import KanTtsTextsyBERT  # noqa: E402
from kantts.models.utils import get_mask_from_lengths  # noqa: E402
from kantts.train.loss import SeqCELoss  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "sybert_tiny.pt")
SIZES = dict(sy=147, tone=10, syllable_flag=8, word_segment=8)
RATIO = 0.3
LENGTHS = (1, 2, 5, 12, 40)


class Unit:
    """Stand-in for KanTtsLinguisticUnit (see the module docstring); inventories end with pad, "~", [MASK]."""
    _mask = "@[MASK]"
    _lfeat_type_list = ["sy", "tone", "syllable_flag", "word_segment", "emo_category", "speaker_category"]
    _sub_unit_pad = {k: n - 3 for k, n in SIZES.items()}

    def encode_sy(self, sy):
        assert sy == [self._mask]
        return [SIZES["sy"] - 1]

    def get_unit_size(self):
        return dict(SIZES)


def dataset():
    ds = BERT_Text_Dataset.__new__(BERT_Text_Dataset)
    ds.ling_unit, ds.padder, ds.masking_actor = Unit(), Padder(), MaskingActor(RATIO)
    return ds


def sentence(L):
    rs = np.random.RandomState(100 + L)
    return [np.append(rs.randint(0, SIZES[k] - 3, size=L - 1), SIZES[k] - 2).astype(np.int32)
            for k in ("sy", "tone", "syllable_flag", "word_segment")]


def masking_case():
    ds = dataset()
    actor = ds.masking_actor
    out = {"ratio": RATIO, "mask_id": SIZES["sy"] - 1, "nsym": SIZES["sy"], "lengths": LENGTHS, "records": []}
    for k in range(3):
        for L in LENGTHS:
            ling = sentence(L)
            np.random.seed(k)
            random.seed(k)
            mask = actor._get_random_mask(L, p1=RATIO)
            masked = actor._input_bert_masking(ling[0], SIZES["sy"], SIZES["sy"] - 1, mask)
            np.random.seed(k)
            random.seed(k)
            bm_mask, bm_ids = ds.bert_masking(ling)
            out["records"].append(dict(seed=k, L=L, ling=[a.copy() for a in ling], random_mask=np.array(mask),
                                       input_masked=np.array(masked), bert_mask=np.array(bm_mask), bert_ids=np.array(bm_ids)))
    np.random.seed(7)
    random.seed(7)
    items = []
    for L in (5, 12, 2):
        ling = sentence(L)
        m, ids = ds.bert_masking(ling)
        items.append((ling, ids, m))
    batch = ds.collate_fn(items)
    out["collate"] = dict(seed=7, lengths=(5, 12, 2), batch={k: v.numpy().copy() for k, v in batch.items()},
                          dtypes={k: str(v.dtype) for k, v in batch.items()})
    return out


def checksums(sd):
    return {k: (tuple(v.shape), float(v.double().sum()), float(v.double().abs().sum())) for k, v in sd.items()}


def model_case(seed_w=0):
    cfg = O.sambert_config(tiny=True)
    torch.manual_seed(seed_w)
    m = KanTtsTextsyBERT(dict(cfg))
    m.eval()
    g = torch.Generator().manual_seed(2025)
    B, T = 3, 7
    lens = torch.tensor([6, 4, 3])
    ling = torch.stack([torch.randint(0, SIZES[k] - 3, (B, T), generator=g)
                        for k in ("sy", "tone", "syllable_flag", "word_segment")], -1)
    targets = torch.randint(0, SIZES["sy"] - 3, (B, T), generator=g)
    masks = ((torch.rand(B, T, generator=g) < 0.5) & (torch.arange(T)[None, :] < lens[:, None])).float()
    assert float(masks.sum()) >= 3
    input_masks = get_mask_from_lengths(lens, max_len=ling.size(1))                    # kantts_sambert.py:1058
    text_hid = m.text_encoder(ling, input_masks, return_attns=True)[0]                 # :1060-1062, all three values taken
    logits = m.fc(text_hid)                                                            # :1063
    loss, err = SeqCELoss()(logits, targets, masks)
    V = logits.size(-1)
    (loss / V).backward()
    named = dict(m.named_parameters())
    gsum = {n: (float(p.grad.double().sum()), float(p.grad.double().norm())) for n, p in named.items() if p.grad is not None}
    return dict(cfg=cfg, batch=dict(inputs_ling=ling, input_lengths=lens, targets=targets, bert_masks=masks),
                logits=logits.detach().clone(), loss=float(loss), loss_over_v=float(loss / V), err=float(err), V=V,
                grad_summaries=gsum, head_grads={n: named[n].grad.detach().clone() for n in ("fc.weight", "fc.bias")},
                weight_checksums=checksums(m.state_dict()), state_keys=sorted(m.state_dict().keys()))


if __name__ == "__main__":
    fix = dict(masking=masking_case(), model=model_case())
    torch.save(fix, OUT)
    print("wrote %s (%d bytes); loss %.6f err %.4f" % (OUT, os.path.getsize(OUT), fix["model"]["loss"], fix["model"]["err"]))
