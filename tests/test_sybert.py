"""sy-BERT pre-training: csrc/sybert.hip (kantts_bert_mask_rows, kantts_mlm_head_fwd / _bwd), ops.mlm_head_ce /
ops.bert_mask_rows, kantts.datasets.bert_masking (the numpy twin of the mask kernel), the host dataset (MaskingActor,
BERT_Text_Dataset), KanTtsTextsyBERT's fused training form, SeqCELoss, Textsy_BERT_Trainer, DeviceTextSet and
kantts.bin.train_sybert.

Legs as in tests/test_device_corpus_mas_se.py: ``kernel_source`` (the kernel sources on the CPU, util.kernel_source_on_cpu)
and, marked ``gpu``, the device.

Bounds.  The mask kernel against its numpy twin: torch.equal.  The head against the reference's formula in fp64 on the same
fp32 inputs: a logit is an fp32 fmaf chain of C products plus a bias, so per row
    |dlogit| <= (C + 2) * 2^-24 * max_v (sum_c |h_c w_vc| + |b_v|)                                   (the row bound)
the loss within 2 * max_row bound + 4 * 2^-24 * |loss|; the error rate exactly, after leaving out rows whose two largest
fp64 logits lie within twice the row bound (at most 1 % of the masked rows; the seeds below leave out none); gradients
rel-L2 <= 1e-4 against the fp64 gradients (the project's fp32 gradient bound, tests/test_oracle_golden.py).  Model against
the recorded reference fixture: logits 2e-5, losses 1e-5, gradients rel-L2 1e-4 (the project's fixture bounds)."""
import contextlib
import math
import os
import random

import numpy as np
import pytest
import torch

from util import GOLDEN, kernel_source_on_cpu

LEGS = [pytest.param("hostsim", id="kernel_source"), pytest.param("cuda", id="gpu", marks=pytest.mark.gpu)]
_E_BADARG, _E_UNSUPPORTED, _E_WORKSPACE = -1, -2, -3
_SENT = -777


def _leg(leg):
    return (kernel_source_on_cpu(), "cpu") if leg == "hostsim" else (contextlib.nullcontext(), "cuda")


# ---------------------------------------------------------------------------------------------------------------------
# 2. the mask kernel against bert_masking.draw
_B, _T = 6, 300
_LENS = [1, 2, 3, 11, 64, 300]
_MASK_ID, _NSYM, _SEED, _START = 145, 147, 0xF123456789ABCDEF, 41


def _mask_call(dev, targets, lens, thr, words, T=None, B=None, offset=0, nsym=_NSYM):
    """kantts_bert_mask_rows into flat sentinel buffers with one guard item in front of and behind the (B, T, 4) ids and
    the (B, T) masks.  Returns (code, ids (B, T, 4), masks (B, T)) on the host after checking the guards."""
    import kantts._hip as hip

    Bt, Tt = targets.shape
    n4, n1 = Tt * 4, Tt
    lings = torch.full(((Bt + 2) * n4,), _SENT, dtype=torch.int64, device=dev)
    masks = torch.full(((Bt + 2) * n1 + 4,), float(_SENT), device=dev)
    lv, mv = lings[n4: n4 + Bt * n4], masks[n1 + offset: n1 + offset + Bt * n1]
    rc = hip.bert_mask_rows_raw(words, targets, lens, lv, mv, B=Bt if B is None else B, T=Tt if T is None else T, thr=thr,
                                mask_id=_MASK_ID, nsym=nsym)
    hl, hm = lings.cpu(), masks.cpu()
    assert bool((hl[:n4] == _SENT).all()) and bool((hl[n4 + Bt * n4:] == _SENT).all()), "ids: a guard item was written"
    assert bool((hm[:n1 + offset] == _SENT).all()) and bool((hm[n1 + offset + Bt * n1:] == _SENT).all()), "masks: guard"
    return rc, hl[n4: n4 + Bt * n4].view(Bt, Tt, 4), hm[n1 + offset: n1 + offset + Bt * n1].view(Bt, Tt)


def _mask_inputs(dev):
    rs = np.random.RandomState(3)
    targets = rs.randint(0, _NSYM - 2, size=(_B, _T)).astype(np.int64)
    return targets, torch.from_numpy(targets).to(dev), torch.tensor(_LENS, dtype=torch.int32).to(dev)


def _words(dev, counter=_START):
    return torch.tensor([_SEED - (1 << 64), counter], dtype=torch.int64).to(dev)  # the seed's bits as a signed word


@pytest.mark.parametrize("leg", LEGS)
def test_mask_kernel_equals_the_numpy_twin(leg):
    from kantts.datasets import bert_masking as bm

    ctx, dev = _leg(leg)
    with ctx:
        import kantts._hip as hip

        assert hip.has_sybert()
        tg_np, tg, lens = _mask_inputs(dev)
        words = _words(dev)
        thr = bm.threshold(0.3)
        calls = []
        for k in range(2):
            rc, ids, masks = _mask_call(dev, tg, lens, thr, words, offset=k)  # masks at an even and an odd cell
            assert rc == 0
            ref_ids, ref_masks = bm.draw(_SEED, _START + k, tg_np, _LENS, 0.3, _MASK_ID, _NSYM)
            assert torch.equal(ids[:, :, 0], torch.from_numpy(ref_ids)) and torch.equal(masks, torch.from_numpy(ref_masks))
            assert bool((ids[:, :, 1:] == _SENT).all()), "columns 1-3 of input_lings were written"
            calls.append((ids, masks))
        assert not torch.equal(calls[0][1], calls[1][1]), "the second call drew the same numbers"
        assert words.cpu().tolist() == [_SEED - (1 << 64), _START + 2]
        words[1] = _START  # a counter set back replays the first call
        rc, ids, masks = _mask_call(dev, tg, lens, thr, words)
        assert rc == 0 and torch.equal(ids, calls[0][0]) and torch.equal(masks, calls[0][1])
        assert int(masks[5].sum()) > 30 and int((ids[5, :, 0] == _MASK_ID).sum()) == 4 * int(masks[5].sum()) // 5
        # ratio 0: nothing; ratio 1: everything but the last token of every sequence
        rc, ids, masks = _mask_call(dev, tg, lens, bm.threshold(0.0), words)
        assert rc == 0 and bool((masks == 0).all()) and torch.equal(ids[:, :, 0], torch.from_numpy(tg_np))
        rc, ids, masks = _mask_call(dev, tg, lens, bm.threshold(1.0), words)
        assert rc == 0
        want = (torch.arange(_T)[None, :] < (torch.tensor(_LENS)[:, None] - 1)).float()
        assert torch.equal(masks, want)
        ref_ids, _ = bm.draw(_SEED, _START + 2, tg_np, _LENS, 1.0, _MASK_ID, _NSYM)
        assert torch.equal(ids[:, :, 0], torch.from_numpy(ref_ids))
        # lengths outside [0, T] are clamped: nothing outside the tensors is touched (the guards), the twin agrees
        wild = [-5, 0, _T + 9, 2 ** 31 - 1, 7, 1]
        rc, ids, masks = _mask_call(dev, tg, torch.tensor(wild, dtype=torch.int32).to(dev), thr, words)
        ref_ids, ref_masks = bm.draw(_SEED, _START + 3, tg_np, wild, 0.3, _MASK_ID, _NSYM)
        assert rc == 0 and torch.equal(ids[:, :, 0], torch.from_numpy(ref_ids)) and torch.equal(masks, torch.from_numpy(ref_masks))
        # in place: the unmasked ids ARE column 0 of input_lings; the dense targets come out of the same launch
        import kantts._hip.ops as ops

        lings = torch.full((_B, _T, 4), _SENT, dtype=torch.int64)
        lings[:, :, 0] = torch.from_numpy(tg_np)
        lings = lings.to(dev)
        m, to = torch.empty(_B, _T, device=dev), torch.empty((_B, _T), dtype=torch.int64, device=dev)
        words[1] = _START
        ops.bert_mask_rows(words, None, lens, lings, m, mask_ratio=0.3, mask_id=_MASK_ID, nsym=_NSYM, targets_out=to)
        assert torch.equal(lings.cpu(), calls[0][0]) and torch.equal(m.cpu(), calls[0][1])
        assert torch.equal(to.cpu(), torch.from_numpy(tg_np))


@pytest.mark.parametrize("leg", LEGS)
def test_mask_kernel_refusals_write_nothing(leg):
    from kantts.datasets import bert_masking as bm

    ctx, dev = _leg(leg)
    with ctx:
        import kantts._hip as hip

        _, tg, lens = _mask_inputs(dev)
        words = _words(dev)
        thr = bm.threshold(0.3)
        lings = torch.full((_B, _T, 4), _SENT, dtype=torch.int64, device=dev)
        masks = torch.full((_B, _T), float(_SENT), device=dev)
        ok = dict(B=_B, T=_T, thr=thr, mask_id=_MASK_ID, nsym=_NSYM)
        raw = hip.bert_mask_rows_raw
        assert raw(None, tg, lens, lings, masks, **ok) == _E_BADARG
        assert raw(words, None, lens, lings, masks, **ok) == _E_BADARG
        assert raw(words, tg, None, lings, masks, **ok) == _E_BADARG
        assert raw(words, tg, lens, None, masks, **ok) == _E_BADARG
        assert raw(words, tg, lens, lings, None, **ok) == _E_BADARG
        for bad in (dict(ok, B=0), dict(ok, T=0), dict(ok, thr=(1 << 24) + 1), dict(ok, thr=-1), dict(ok, ling_ts=0), dict(ok, tgt_ts=0)):
            assert raw(words, tg, lens, lings, masks, **bad) == _E_BADARG
        for bad in (dict(ok, T=4097), dict(ok, B=1 << 20), dict(ok, nsym=0)):
            assert raw(words, tg, lens, lings, masks, **bad) == _E_UNSUPPORTED
        # pointers that are not aligned to their element: the entry point itself, with raw addresses
        L, c = hip.lib(), (int(_B), int(_T), int(thr), _MASK_ID, _NSYM, None)
        a = dict(w=words.data_ptr(), t=tg.data_ptr(), n=lens.data_ptr(), l=lings.data_ptr(), m=masks.data_ptr(), o=0)
        for k in "wtnlmo":
            b = dict(a, **{k: a[k] + (2 if k in "nm" else 4)})
            assert L.kantts_bert_mask_rows(b["w"], b["t"], 1, b["n"], b["l"], 4, b["m"], b["o"] or None, *c) == _E_BADARG, k
        assert bool((lings == _SENT).all()) and bool((masks == _SENT).all()), "a refused call wrote"
        assert words.cpu().tolist() == [_SEED - (1 << 64), _START], "a refused call moved the counter"
        assert raw(words, tg, lens, lings, masks, **ok) == 0 and int(words[1]) == _START + 1


# ---------------------------------------------------------------------------------------------------------------------
# 3. the rule itself, on the numpy twin
def test_the_masking_rule_counts_and_shares():
    from kantts.datasets import bert_masking as bm

    mask_id, nsym = 200, 147  # [MASK] outside the targets' range: a random symbol can never read as [MASK]
    rs = np.random.RandomState(11)
    B, T = 4096, 56
    lens = np.full(B, 50)
    lens[:64] = rs.randint(1, T + 1, size=64)
    targets = rs.randint(0, nsym, size=(B, T)).astype(np.int64)
    ids, masks = bm.draw(77, 5, targets, lens, 0.3, mask_id, nsym)
    first, last, share = [], [], []
    for b in range(B):
        L = int(lens[b])
        pos = np.nonzero(masks[b])[0]
        n = len(pos)
        assert masks[b, L - 1] == 0 and not masks[b, L:].any() and np.array_equal(ids[b, L - 1:], targets[b, L - 1:])
        assert np.array_equal(ids[b, masks[b] == 0], targets[b, masks[b] == 0])
        assert int((ids[b] == mask_id).sum()) == 4 * n // 5
        changed = (ids[b] != targets[b]) & (ids[b] != mask_id)
        assert int(changed.sum()) <= n // 10 and len(set(ids[b, changed].tolist())) <= 1  # ONE random symbol per sequence
        if b >= 64 and n >= 5:
            first.append(ids[b, pos[0]] == mask_id), last.append(ids[b, pos[-1]] == mask_id), share.append((4 * n // 5) / n)
    got = masks[64:, :49].mean()
    cells = (B - 64) * 49
    assert abs(got - 0.3) <= 4 * math.sqrt(0.21 / cells), (got, cells)
    # the sequences of length 50 alone are the issue's 4096 x 49 = 200 704 cells when none is replaced
    ids50, masks50 = bm.draw(78, 0, targets, np.full(B, 50), 0.3, mask_id, nsym)
    assert abs(masks50[:, :49].mean() - 0.3) <= 4 * math.sqrt(0.21 / 200704) and not masks50[:, 49:].any()
    p = float(np.mean(share))
    sd = math.sqrt(p * (1 - p) / len(first))
    assert len(first) > 3000 and abs(np.mean(first) - p) <= 4 * sd and abs(np.mean(last) - p) <= 4 * sd, \
        (np.mean(first), np.mean(last), p, sd)
    for n in range(4097):  # the integer divisions are the reference's fp64 floors
        assert 4 * n // 5 == int(math.floor(n * 0.8)) and n // 10 == int(math.floor(n * 0.1)), n
    assert bm.threshold(0.3) == 5033164 and bm.threshold(1.0) == 1 << 24 and bm.threshold(0.0) == 0


# ---------------------------------------------------------------------------------------------------------------------
# 4. the head against an fp64 interval reference
_HEAD_CASES = {  # name: (M, C, V, which rows are masked, seed)
    "shipped_width": (37, 128, 147, "30%", 1),
    "smallest": (5, 16, 5, "30%", 2),
    "ragged_tiles": (130, 128, 257, "30%", 3),
    "widest": (64, 512, 33, "30%", 4),
    "one_row": (37, 128, 147, "one", 5),
    "no_row": (37, 128, 147, "none", 6),
}
_HEAD_REF = {}


def _head_case(name):
    """Inputs (fp32, host) and the fp64 reference of a case, computed once."""
    if name in _HEAD_REF:
        return _HEAD_REF[name]
    M, C, V, rows, seed = _HEAD_CASES[name]
    g = torch.Generator().manual_seed(seed)
    hid = torch.randn(M, C, generator=g)
    W = torch.randn(V, C, generator=g) / math.sqrt(C)
    b = 0.1 * torch.randn(V, generator=g)
    tg = torch.randint(0, V, (M,), generator=g)
    if rows == "30%":
        mask = (torch.rand(M, generator=g) < 0.3).float()
        mask[int(torch.randint(0, M, (1,), generator=g))] = 1.0
    else:
        mask = torch.zeros(M)
        if rows == "one":
            mask[M // 2] = 1.0
    h64, w64, b64, m64 = hid.double(), W.double(), b.double(), mask.double()
    logits = h64 @ w64.t() + b64
    bound = (C + 2) * 2.0 ** -24 * ((h64.abs() @ w64.abs().t()) + b64.abs()).max(dim=1).values  # per row
    lse = torch.logsumexp(logits, dim=1)
    ce = lse - logits[torch.arange(M), tg]
    msum = m64.sum()
    loss = (ce * m64).sum() / msum
    top2 = logits.topk(min(2, V), dim=1).values
    sure = (top2[:, 0] - top2[:, -1] > 2 * bound) if V > 1 else torch.ones(M, dtype=torch.bool)
    wrong = (logits.argmax(dim=1) != tg)
    dlog = (torch.softmax(logits, dim=1) - torch.nn.functional.one_hot(tg, V).double()) * (m64 / msum)[:, None]
    ref = dict(hid=hid, W=W, b=b, tg=tg, mask=mask, bound=bound, loss=loss, sure=sure, wrong=wrong,
               d_hid=dlog @ w64, d_W=dlog.t() @ h64, d_b=dlog.sum(0))
    _HEAD_REF[name] = ref
    return ref


def _rel(a, b):
    return float((a.double() - b).norm() / b.norm())


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("name", list(_HEAD_CASES))
def test_head_against_the_fp64_reference(name, leg):
    ctx, dev = _leg(leg)
    r = _head_case(name)
    M, C, V, rows, _ = _HEAD_CASES[name]
    with ctx:
        import kantts._hip.ops as ops

        outs = []
        for _ in range(2):
            hid, W, b = (r[k].clone().to(dev).requires_grad_(True) for k in ("hid", "W", "b"))
            loss, err = ops.mlm_head_ce(hid, W, b, r["tg"].to(dev), r["mask"].to(dev))
            assert loss.shape == () and err.shape == () and not err.requires_grad
            if rows != "none":
                loss.backward()
                outs.append([t.detach().cpu() for t in (loss, err, hid.grad, W.grad, b.grad)])
            else:
                outs.append([t.detach().cpu() for t in (loss, err)])
    loss, err = outs[0][:2]
    masked = r["mask"] != 0
    if rows == "none":
        assert torch.isnan(r["loss"]) and torch.isnan(loss) and torch.isnan(err)  # NaN both sides
        return
    for a, c in zip(outs[0], outs[1]):
        assert torch.equal(a, c), "two calls on equal inputs differ in bits"
    tol = 2 * float(r["bound"][masked].max()) + 4 * 2.0 ** -24 * abs(float(r["loss"]))
    d = abs(float(loss) - float(r["loss"]))
    print("%s: loss %.7f ref %.7f, |d| %.2e of %.2e" % (name, float(loss), float(r["loss"]), d, tol))
    assert d <= tol
    keep = masked & r["sure"]
    left_out = int(masked.sum()) - int(keep.sum())
    assert left_out == 0, "the seeds are chosen so that the fp64 reference leaves out no row"
    assert left_out <= 0.01 * int(masked.sum())
    want_err = float((r["wrong"] & keep).sum()) / float(r["mask"].sum())
    assert float(err) == np.float32(want_err) or abs(float(err) - want_err) <= 2.0 ** -23 * want_err, (float(err), want_err)
    d_hid, d_W, d_b = outs[0][2:]
    rels = _rel(d_hid, r["d_hid"]), _rel(d_W, r["d_W"]), _rel(d_b, r["d_b"])
    print("%s: rel-L2 d_hid %.2e d_W %.2e d_bias %.2e" % ((name,) + rels))
    assert max(rels) <= 1e-4
    assert bool((d_hid[~masked] == 0).all()), "d_hid is not exactly zero on an unmasked row"


@pytest.mark.parametrize("leg", LEGS)
def test_head_ignores_unmasked_rows_and_flags_bad_targets(leg):
    ctx, dev = _leg(leg)
    r = _head_case("shipped_width")
    unmasked = int((r["mask"] == 0).nonzero()[0])
    masked = int((r["mask"] != 0).nonzero()[0])
    with ctx:
        import kantts._hip.ops as ops

        base = ops.mlm_head_ce(r["hid"].to(dev), r["W"].to(dev), r["b"].to(dev), r["tg"].to(dev), r["mask"].to(dev))
        hid, tg = r["hid"].clone(), r["tg"].clone()
        hid[unmasked] = float("nan")  # a non-finite logit row and a wild target where the mask is 0: no trace
        tg[unmasked] = 10 ** 9
        got = ops.mlm_head_ce(hid.to(dev), r["W"].to(dev), r["b"].to(dev), tg.to(dev), r["mask"].to(dev))
        assert torch.equal(got[0].cpu(), base[0].cpu()) and torch.equal(got[1].cpu(), base[1].cpu())
        for bad in (-1, 147):
            tg = r["tg"].clone()
            tg[masked] = bad
            loss, _ = ops.mlm_head_ce(r["hid"].to(dev), r["W"].to(dev), r["b"].to(dev), tg.to(dev), r["mask"].to(dev))
            assert torch.isnan(loss.cpu())
        # equal maxima: the lowest index, as torch.argmax on the CPU -- two identical weight rows, the target the second
        W = r["W"].clone()
        W[:] = 0.0
        b = torch.zeros(147)
        b[[20, 99]] = 1.0
        ones = torch.ones(37)
        tg = torch.full((37,), 99)
        _, err = ops.mlm_head_ce(r["hid"].to(dev), W.to(dev), b.to(dev), tg.to(dev), ones.to(dev))
        assert float(err) == 1.0
        _, err = ops.mlm_head_ce(r["hid"].to(dev), W.to(dev), b.to(dev), torch.full((37,), 20).to(dev), ones.to(dev))
        assert float(err) == 0.0


@pytest.mark.parametrize("leg", LEGS)
def test_head_refusals(leg):
    ctx, dev = _leg(leg)
    with ctx:
        import kantts._hip as hip

        M, C, V = 20, 32, 9
        f = lambda *s: torch.full(s, float(_SENT), device=dev)  # noqa: E731
        hid, W, b, mask = torch.zeros(M, C, device=dev), torch.zeros(V, C, device=dev), torch.zeros(V, device=dev), torch.ones(M, device=dev)
        tg = torch.zeros(M, dtype=torch.int64, device=dev)
        out, lse, ws = f(3), f(M), f(6)
        ok = dict(M=M, C=C, V=V)
        args = [hid, W, b, tg, mask, out, lse, ws]
        for k in (0, 1, 3, 4, 5, 6, 7):  # every pointer but the bias is required
            a = list(args)
            a[k] = None
            assert hip.mlm_head_fwd_raw(*a, **ok) == _E_BADARG, k
        assert hip.mlm_head_fwd_raw(*args, **dict(ok, M=0)) == _E_BADARG
        assert hip.mlm_head_fwd_raw(hid.view(-1)[1:], *args[1:], **dict(ok, M=M - 1)) == _E_BADARG  # hid not 16-byte aligned
        for bad in (dict(ok, C=24), dict(ok, C=0), dict(ok, C=528), dict(ok, V=0), dict(ok, V=4097), dict(ok, M=(1 << 24) + 1)):
            assert hip.mlm_head_fwd_raw(*args, **bad) == _E_UNSUPPORTED, bad
        assert hip.mlm_head_fwd_raw(*args, ws_floats=5, **ok) == _E_WORKSPACE
        assert all(bool((t == _SENT).all()) for t in (out, lse, ws)), "a refused forward wrote"
        assert hip.mlm_head_fwd_raw(*args, **ok) == 0
        dl = torch.ones(1, device=dev)
        d_hid, d_W, d_b, bws = f(M, C), f(V, C), f(V), f(32 * 16)
        bargs = [hid, W, b, tg, mask, lse, out, dl, 1.0, d_hid, d_W, d_b, bws]
        for k in (0, 1, 3, 4, 5, 6, 7, 9, 10, 12):  # bias and d_bias may be absent
            a = list(bargs)
            a[k] = None
            assert hip.mlm_head_bwd_raw(*a, **ok) == _E_BADARG, k
        for bad in (dict(ok, C=24), dict(ok, V=4097)):
            assert hip.mlm_head_bwd_raw(*bargs, **bad) == _E_UNSUPPORTED
        assert hip.mlm_head_bwd_raw(*bargs, ws_floats=32 * 16 - 1, **ok) == _E_WORKSPACE
        a = list(bargs)
        a[12] = f(32 * 16 + 4)[1:]
        assert hip.mlm_head_bwd_raw(*a, ws_floats=32 * 16, **ok) == _E_BADARG  # workspace not 16-byte aligned
        assert all(bool((t == _SENT).all()) for t in (d_hid, d_W, d_b, bws)), "a refused backward wrote"
        assert hip.mlm_head_bwd_raw(*bargs, **ok) == 0
        assert bool(torch.isfinite(d_hid).all()) and bool(torch.isfinite(d_W).all()) and bool(torch.isfinite(d_b).all())


# ---------------------------------------------------------------------------------------------------------------------
# 1. host masking and collate against the reference's arrays
_FIX = {}


def _fix():
    if not _FIX:
        _FIX.update(torch.load(os.path.join(GOLDEN, "sybert_tiny.pt"), weights_only=False))
    return _FIX


def _tiny_config(cfg=None, dropout=None, batch_size=4, max_steps=4):
    if cfg is None:
        cfg = _fix()["model"]["cfg"]
    keys = ("max_len", "embedding_dim", "encoder_num_layers", "encoder_num_heads", "encoder_num_units",
            "encoder_ffn_inner_dim", "encoder_dropout", "encoder_attention_dropout", "encoder_relu_dropout",
            "encoder_projection_units", "sy", "tone", "syllable_flag", "word_segment")
    params = {k: cfg[k] for k in keys}
    params["mask_ratio"] = 0.3
    if dropout is not None:
        for k in params:
            if "dropout" in k:
                params[k] = dropout
    return {"model_type": "sybert",
            "Model": {"KanTtsTextsyBERT": {
                "params": params,
                "optimizer": {"type": "Adam", "params": {"lr": 0.001, "betas": [0.9, 0.98], "eps": 1e-9, "weight_decay": 0.0}},
                "scheduler": {"type": "NoamLR", "params": {"warmup_steps": 5}}}},
            "linguistic_unit": {"cleaners": "english_cleaners", "speaker_list": "F7",
                                "lfeat_type_list": "sy,tone,syllable_flag,word_segment,emo_category,speaker_category"},
            "Loss": {"SeqCELoss": {"enable": True, "params": {"loss_type": "ce"}}},
            "batch_size": batch_size, "pin_memory": False, "num_workers": 0, "allow_cache": True, "grad_norm": 1.0,
            "train_max_steps": max_steps, "save_interval_steps": 10 ** 6, "eval_interval_steps": 10 ** 6,
            "log_interval_steps": 1, "num_save_intermediate_results": 1}


def test_host_masking_and_collate_equal_the_reference():
    from kantts.datasets.dataset import MaskingActor, SyntheticTextDataset

    fx = _fix()["masking"]
    ds = SyntheticTextDataset(_tiny_config(), 0)
    assert (ds.mask_id, ds.nsym, ds.masking_actor.mask_ratio) == (fx["mask_id"], fx["nsym"], fx["ratio"])
    actor = MaskingActor(fx["ratio"])
    assert len(fx["records"]) == 15
    for rec in fx["records"]:
        np.random.seed(rec["seed"])
        random.seed(rec["seed"])
        mask = actor._get_random_mask(rec["L"], p1=fx["ratio"])
        masked = actor._input_bert_masking(rec["ling"][0], fx["nsym"], fx["mask_id"], mask)
        assert np.array_equal(mask, rec["random_mask"]) and np.array_equal(masked, rec["input_masked"]), rec["seed"]
        np.random.seed(rec["seed"])
        random.seed(rec["seed"])
        bm_mask, bm_ids = ds.bert_masking(rec["ling"])
        assert np.array_equal(bm_mask, rec["bert_mask"]) and np.array_equal(bm_ids, rec["bert_ids"]), (rec["seed"], rec["L"])
        assert bm_mask[-1] == 0
    col = fx["collate"]
    by_len = {rec["L"]: rec["ling"] for rec in fx["records"]}
    np.random.seed(col["seed"])
    random.seed(col["seed"])
    items = []
    for L in col["lengths"]:
        m, ids = ds.bert_masking(by_len[L])
        items.append((by_len[L], ids, m))
    got = ds.collate_fn(items)
    assert set(got) == set(col["batch"])
    for k, ref in col["batch"].items():
        assert str(got[k].dtype) == col["dtypes"][k] and np.array_equal(got[k].numpy(), ref), k


# ---------------------------------------------------------------------------------------------------------------------
# 5. / 6. the model against the recorded reference and against its own unfused form
def _model(dev):
    from kantts.models.sambert.kantts_sambert import KanTtsTextsyBERT

    torch.manual_seed(0)
    m = KanTtsTextsyBERT(dict(_fix()["model"]["cfg"]))
    m.eval()
    return m.to(dev)


@pytest.mark.parametrize("leg", LEGS)
def test_model_against_the_reference_fixture(leg):
    import kantts._hip as hip

    fx = _fix()["model"]
    ctx, dev = _leg(leg)
    with ctx, hip.precision_scope("fp32"):
        m = _model("cpu")
        assert sorted(m.state_dict().keys()) == fx["state_keys"]
        for k, (shape, s, a) in fx["weight_checksums"].items():
            v = m.state_dict()[k]
            assert tuple(v.shape) == shape and abs(float(v.double().sum()) - s) <= 1e-6 * max(1.0, a), k
        m = m.to(dev)
        b = {k: v.to(dev) for k, v in fx["batch"].items()}
        res = m(b["inputs_ling"], b["input_lengths"])
        assert set(res) == {"logits", "enc_slf_attn_lst"}
        err = float((res["logits"].detach().cpu() - fx["logits"]).abs().max())
        print("sybert fixture", dev, "logits %.2e" % err)
        assert err <= 2e-5
        V = fx["V"]
        res = m(b["inputs_ling"], b["input_lengths"], b["targets"], b["bert_masks"], grad_scale=1.0 / V)
        assert "logits" not in res and set(res) == {"loss", "err", "enc_slf_attn_lst"}
        loss = float(res["loss"].detach())
        print("sybert fixture", dev, "loss %.2e, loss / V %.2e" % (abs(loss - fx["loss"]), abs(loss / V - fx["loss_over_v"])))
        assert abs(loss - fx["loss"]) <= 1e-5 and abs(float(res["loss"].detach() / V) - fx["loss_over_v"]) <= 1e-5
        assert float(res["err"]) == np.float32(fx["err"])
        res["loss"].backward()  # the gradient of loss / V: the head scales it
        named = {k: v for k, v in m.named_parameters()}
        assert sorted(k for k, v in named.items() if v.grad is not None) == sorted(fx["grad_summaries"])
        worst = 0.0
        for k, (s, nrm) in fx["grad_summaries"].items():
            gr = named[k].grad.double().cpu()
            e_n = abs(float(gr.norm()) - nrm) / nrm
            e_s = abs(float(gr.sum()) - s) / (gr.numel() ** 0.5 * nrm)
            worst = max(worst, e_n, e_s)
            assert e_n <= 1e-4 and e_s <= 1e-4, (k, e_n, e_s)
        for k, ref in fx["head_grads"].items():
            rel = _rel(named[k].grad.cpu(), ref.double())
            worst = max(worst, rel)
            assert rel <= 1e-4, (k, rel)
        print("sybert fixture", dev, "worst gradient figure %.2e" % worst)


@pytest.mark.parametrize("leg", LEGS)
def test_fused_training_form_equals_the_unfused_one(leg):
    import kantts._hip as hip
    from kantts.train.loss import SeqCELoss

    fx = _fix()["model"]
    ctx, dev = _leg(leg)
    with ctx, hip.precision_scope("fp32"):
        m = _model(dev)
        b = {k: v.to(dev) for k, v in fx["batch"].items()}
        res = m(b["inputs_ling"], b["input_lengths"], b["targets"], b["bert_masks"])
        res["loss"].backward()
        fused = {k: v.grad.detach().cpu().clone() for k, v in m.named_parameters() if v.grad is not None}
        m.zero_grad(set_to_none=True)
        loss, err = SeqCELoss()(m(b["inputs_ling"], b["input_lengths"])["logits"], b["targets"], b["bert_masks"])
        loss.backward()
        print("fused %.7f unfused %.7f" % (float(res["loss"].detach()), float(loss.detach())))
        assert abs(float(res["loss"].detach()) - float(loss.detach())) <= 1e-5 and float(res["err"]) == float(err)
        assert sorted(fused) == sorted(k for k, v in m.named_parameters() if v.grad is not None) and "fc.weight" in fused
        for k, v in m.named_parameters():
            if v.grad is None:
                continue
            rel = _rel(fused[k], v.grad.detach().cpu().double())
            assert rel <= 1e-4, (k, rel)
        # the attention maps only on request
        assert all(a is None for a in res["enc_slf_attn_lst"]) or len(res["enc_slf_attn_lst"]) == 0
        m.return_attns = True
        with torch.no_grad():
            maps = m(b["inputs_ling"], b["input_lengths"])["enc_slf_attn_lst"]
        assert len(maps) == fx["cfg"]["encoder_num_layers"] and all(torch.is_tensor(a) for a in maps)
        with pytest.raises(ValueError, match="bert_masks"):
            m(b["inputs_ling"], b["input_lengths"], b["targets"])


# ---------------------------------------------------------------------------------------------------------------------
# 7. trainer and entry point
def test_criterion_builder_knows_seqceloss():
    from kantts.train.loss import SeqCELoss, criterion_builder

    crit = criterion_builder({"Loss": {"SeqCELoss": {"enable": True, "params": {"loss_type": "ce"}}}}, "cpu")
    assert isinstance(crit["SeqCELoss"], SeqCELoss) and crit["SeqCELoss"].loss_type == "ce"
    logits = torch.randn(2, 5, 7)
    tg, mk = torch.randint(0, 7, (2, 5)), (torch.rand(2, 5) < 0.6).float()
    mk[0, 0] = 1.0
    loss, err = crit["SeqCELoss"](logits, tg, mk)
    ce = torch.nn.functional.cross_entropy(logits.view(-1, 7), tg.view(-1), reduction="none")
    assert torch.allclose(loss, (ce * mk.view(-1)).sum() / mk.sum())
    assert torch.allclose(err, ((logits.argmax(-1) != tg) * mk).sum() / mk.sum())
    with pytest.raises(ValueError):
        SeqCELoss("mse")


def _write_yaml(tmp_path, config):
    import yaml

    path = os.path.join(str(tmp_path), "sybert_tiny.yaml")
    with open(path, "w") as f:
        yaml.dump(config, f)
    return path


def _run_cli(tmp_path, dev, corpus, batch_size=4):
    """Three steps: ``3 * batch_size`` synthetic sentences, one epoch (the trainers count their steps from 1)."""
    from kantts.bin import train_sybert

    stage = os.path.join(str(tmp_path), "stage_" + corpus)
    tr = train_sybert.train(_write_yaml(tmp_path, _tiny_config(dropout=0.0, batch_size=batch_size)), [], stage,
                            synthetic=3 * batch_size, device_corpus=corpus)
    assert tr.steps == 4 and tr.device.type == dev and os.path.exists(os.path.join(stage, "config.yaml"))
    return tr, stage


def _check_checkpoint(tr, stage, dev):
    """The reference's four keys; train_sambert's loader takes text_encoder.* from it and ignores fc.*."""
    from kantts.models import model_builder
    from kantts.train.trainer import Sambert_Trainer

    path = os.path.join(stage, "ckpt", "checkpoint_%d.pth" % tr.steps)
    tr.save_checkpoint(path)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert sorted(ck) == ["model", "optimizer", "scheduler", "steps"] and ck["steps"] == 4
    assert sorted(ck["model"]) == _fix()["model"]["state_keys"]
    import torch_oracle as O

    cfg = dict(O.sambert_config(tiny=True))
    config = {"model_type": "sambert", "Model": {"KanTtsSAMBERT": {
        "params": cfg,
        "optimizer": {"type": "Adam", "params": {"lr": 0.001, "betas": [0.9, 0.98], "eps": 1e-9, "weight_decay": 0.0}},
        "scheduler": {"type": "NoamLR", "params": {"warmup_steps": 4000}}}}, "batch_size": 3}
    model, opt, sch = model_builder(config, device="cpu")
    am = Sambert_Trainer(config, model, opt, sch, {}, torch.device("cpu"), None, [], None, save_dir=None)
    before = {k: v.clone() for k, v in model["KanTtsSAMBERT"].state_dict().items()}
    am.load_checkpoint(path, False, False)
    after = model["KanTtsSAMBERT"].state_dict()
    enc = [k for k in ck["model"] if k.startswith("text_encoder.")]
    assert enc and all(torch.equal(after[k], ck["model"][k]) for k in enc)
    assert not any(k.startswith("fc.") for k in after)
    rest = [k for k in after if k not in ck["model"]]
    assert "text_encoder.ling_proj.weight" in rest and all(torch.equal(after[k], before[k]) for k in rest)
    assert any(not torch.equal(before[k], after[k]) for k in enc)


def test_entry_point_trains_on_the_kernel_sources(tmp_path):
    with kernel_source_on_cpu():
        tr, stage = _run_cli(tmp_path, "cpu", "host", batch_size=1)  # (a step of this leg takes a second per 100 symbols)
        _check_checkpoint(tr, stage, "cpu")
        _check_eval_and_intermediate_results(tr)
        with pytest.raises(ValueError, match="device_corpus"):
            from kantts.bin import train_sybert

            train_sybert.train(_tiny_config(), [], stage, synthetic=4, device_corpus="pinned")


@pytest.mark.gpu
@pytest.mark.parametrize("corpus", ["hbm", "host", "auto"])
def test_entry_point_trains_gpu(corpus, tmp_path):
    from kantts.datasets.device_batching import DeviceCorpusLoader, DeviceTextSet

    tr, stage = _run_cli(tmp_path, "cuda", corpus)
    resident = isinstance(tr.train_loader, DeviceCorpusLoader)
    assert resident == (corpus != "host") and (not resident or isinstance(tr.train_loader.set, DeviceTextSet))
    if corpus == "hbm":
        assert int(tr.train_loader.set.words[1]) == 3  # one draw per step
        _check_checkpoint(tr, stage, "cuda")


def _check_eval_and_intermediate_results(tr):
    from kantts.datasets.dataset import SyntheticTextDataset

    ds = SyntheticTextDataset(tr.config, 3, lo=4, hi=9)
    out = tr.genearete_and_save_intermediate_result(ds.collate_fn([ds[i] for i in range(3)]))
    L = len(ds.encoded(0)[0])
    longest = max(len(ds.encoded(i)[0]) for i in range(3))
    assert out.startswith(tr.log_dir) and np.load(os.path.join(out, "pred.npy")).shape == (longest,)
    assert np.array_equal(np.load(os.path.join(out, "target.npy"))[:L], ds.encoded(0)[0])
    assert np.load(os.path.join(out, "bert_mask.npy")).shape == (longest,)
    tr.eval_step(ds.collate_fn([ds[i] for i in range(3)]))
    tr._flush_losses(tr.total_eval_loss, "eval")
    assert set(tr.total_eval_loss) == {"eval/TotalLoss", "eval/Error", "eval/batch_size"}
    assert tr.total_eval_loss["eval/batch_size"] == 3 and np.isfinite(tr.total_eval_loss["eval/TotalLoss"])


def _twenty_steps(dev, tmp_path, resident):
    """20 steps over ONE batch of 8 sentences at dropout 0 (new masks every step): the per-step TotalLoss on the host."""
    from kantts.datasets.dataset import SyntheticTextDataset
    from kantts.datasets.device_batching import DeviceTextSet
    from kantts.models import model_builder
    from kantts.train.loss import criterion_builder
    from kantts.train.trainer import Textsy_BERT_Trainer

    config = _tiny_config(dropout=0.0, batch_size=8, max_steps=20)
    ds = SyntheticTextDataset(config, 8, lo=6, hi=14)
    torch.manual_seed(0)
    np.random.seed(0)
    random.seed(0)
    model, opt, sch = model_builder(config, device=dev)
    tr = Textsy_BERT_Trainer(config, model, opt, sch, criterion_builder(config, dev), torch.device(dev), None, [], None,
                             max_steps=20, save_dir=str(tmp_path), save_interval=10 ** 6, valid_interval=10 ** 6,
                             log_interval=10 ** 6, grad_clip=1.0)
    tr.set_model_state("train")
    if resident:
        pad_ids = [ds.ling_unit._sub_unit_pad[t] for t in ds.ling_unit._lfeat_type_list]
        dset = DeviceTextSet([ds.encoded(i) for i in range(8)], pad_ids, dev, 0.3, ds.mask_id, ds.nsym, seed=5)
    losses = []
    for _ in range(20):
        batch = dset.batch(list(range(8))) if resident else ds.collate_fn([ds[i] for i in range(8)])
        losses.append(tr.train_step(batch))
        tr.steps += 1
    losses = [float(x) for x in torch.stack(losses).cpu()]
    print("resident" if resident else "host", " ".join("%.4f" % x for x in losses))
    assert all(np.isfinite(x) for x in losses)
    assert np.mean(losses[-5:]) < 0.8 * np.mean(losses[:5]), losses
    _check_eval_and_intermediate_results(tr)


@pytest.mark.gpu
@pytest.mark.parametrize("resident", [True, False], ids=["resident", "host"])
def test_losses_decrease_over_twenty_steps_gpu(resident, tmp_path):
    _twenty_steps("cuda", tmp_path, resident)


# ---------------------------------------------------------------------------------------------------------------------
# 8. DeviceTextSet.batch
@pytest.mark.parametrize("leg", LEGS)
def test_device_text_set_batches(leg):
    from kantts.datasets import bert_masking as bm
    from kantts.datasets.dataset import SyntheticTextDataset
    from kantts.datasets.device_batching import DeviceTextSet

    ctx, dev = _leg(leg)
    ds = SyntheticTextDataset(_tiny_config(), 9, lo=2, hi=70)
    items = [ds.encoded(i) for i in range(len(ds))]
    pad_ids = [ds.ling_unit._sub_unit_pad[t] for t in ds.ling_unit._lfeat_type_list]
    seed = 0xC0FFEE1234567890
    with ctx:
        dset = DeviceTextSet(items, pad_ids, dev, 0.3, ds.mask_id, ds.nsym, seed=seed)
        assert len(dset) == 9
        dset.batch([0])  # (allocator and library warm: the census below sees one batch)
        counter = 1
        for idx in ([0, 1, 2], [8, 3, 3, 4, 7], [5]):
            if dev == "cuda":
                torch.cuda.synchronize()
                torch.cuda.set_sync_debug_mode("error")  # a device-to-host read (or any other synchronising call) raises
            try:
                got = dset.batch(idx)
            finally:
                if dev == "cuda":
                    torch.cuda.set_sync_debug_mode("default")
            assert list(got) == list(DeviceTextSet.KEYS) and all(v.device.type == dev for v in got.values())
            np.random.seed(1)
            random.seed(1)
            ref = ds.collate_fn([ds[i] for i in idx])
            lens = [len(items[i][0]) for i in idx]
            ids, masks = bm.draw(seed, counter, ref["targets"].numpy(), lens, 0.3, ds.mask_id, ds.nsym)
            counter += 1
            assert got["bert_masks"].dtype == torch.float32 and torch.equal(got["bert_masks"].cpu(), torch.from_numpy(masks))
            for k in ("valid_input_lengths", "targets"):
                assert got[k].dtype == ref[k].dtype and torch.equal(got[k].cpu(), ref[k]), k
            assert got["input_lings"].dtype == torch.int64 and got["input_lings"].is_contiguous()
            assert torch.equal(got["input_lings"][:, :, 1:].cpu(), ref["input_lings"][:, :, 1:])
            assert torch.equal(got["input_lings"][:, :, 0].cpu(), torch.from_numpy(ids))
        assert dset.words.cpu().tolist() == [seed - (1 << 64), counter]
        with pytest.raises(ValueError, match="mask_ratio"):
            DeviceTextSet(items, pad_ids, dev, 1.5, ds.mask_id, ds.nsym)
