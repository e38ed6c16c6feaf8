"""Filled-pause voices (FP: True, sambert_fp_8k.yaml): the kernels of csrc/fp.hip, FP_Predictor and the device-side
insertion inside KanTtsSAMBERT, FpCELoss, and everything above the model (get_fpdict, dataset / collate, trainer).

Every kernel-level and model-level case runs twice: on the host build of the kernel SOURCES (util.kernel_source_on_cpu;
the emulated C ABI of oracle/ does not get these entries, test_emulated_abi_has_no_filled_pause_entry_points) and, marked
``gpu``, on the device.  The reference data of the model tests is tests/golden/sambert_tiny_fp.pt
(scripts/record_fp_golden.py: the untouched reference on the CPU).

Bounds.  Integer outputs and the forward insertion (a gather) are compared with torch.equal.  The insertion's backward is
a sum of n rows per element: |got - ref| <= (n - 1) 2^-24 sum|terms| against fp64.  Head / CE: forward 2e-5 absolute,
gradients rel-L2 <= 1e-4, the project's fp32 bounds (tests/test_oracle_golden.py).  Fixture parity: float outputs 2e-5 on
the host leg and 1e-4 on the device (the bounds of the sambert_tiny_infer tests), losses 1e-5 absolute, gradient summaries
1e-4 relative -- a parameter's gradient SUM is measured against sqrt(numel) * norm, the size a sum of that many elements of
that norm can have (a sum near zero has no relative error of its own)."""
import contextlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util import GOLDEN, kernel_source_on_cpu, rel_l2

LEGS = [pytest.param("hostsim", id="kernel_source"), pytest.param("cuda", id="gpu", marks=pytest.mark.gpu)]
_E_BADARG, _E_UNSUPPORTED = -1, -2
_SENTINEL = -777
_FIX = {}


def _leg(leg):
    return (kernel_source_on_cpu(), "cpu") if leg == "hostsim" else (contextlib.nullcontext(), "cuda")


def _fix():
    if not _FIX:
        _FIX.update(torch.load(os.path.join(GOLDEN, "sambert_tiny_fp.pt"), weights_only=False))
    return _FIX


@contextlib.contextmanager
def _precision(mode):
    import kantts._hip as hip

    hip.set_precision(mode)
    try:
        yield
    finally:
        hip.set_precision("fp32")


# ---------------------------------------------------------------------------------------------------------------------
# the closed form of the issue, restated in torch (host)
def _closed_form(text_hid, fill, label, lens, number, emo, spk):
    B, T, C = text_hid.shape
    inter = lens + 3 * number
    Tp = T + int(inter.max()) - int(lens.max())
    out = torch.empty(B, Tp, C)
    src = torch.empty(B, Tp, dtype=torch.int64)
    for b in range(B):
        rows, p = [], 0
        while len(rows) < Tp:
            if p < T and int(label[b, p]) > 0:
                rows += [-(1 + 3 * (int(label[b, p]) - 1) + k) for k in range(3)]
            rows.append(p % T)
            p += 1
        src[b] = torch.tensor(rows[:Tp])
        for q, s in enumerate(rows[:Tp]):
            out[b, q] = text_hid[b, s] if s >= 0 else fill.reshape(9, C)[-s - 1]
    wrap = torch.arange(Tp) % T
    return out, inter, Tp, emo[:, wrap], spk[:, wrap], src


def _case(name):
    """(label (B, T) int32, lens (B) int32, fp_number (B) int32, C)."""
    g = torch.Generator().manual_seed(5)
    C = 32
    number = None
    if name == "none":
        label, lens = torch.zeros(3, 7, dtype=torch.int32), [7, 5, 4]
    elif name == "fixture":
        tr = _fix()["train"]
        label, lens = tr["batch"]["fp_label"].int(), tr["batch"]["input_lengths"].tolist()
    elif name == "edges":  # at j = 0 and at j = len - 1
        label, lens = torch.zeros(3, 7, dtype=torch.int32), [7, 5, 4]
        label[0, 0], label[0, 6], label[1, 0], label[1, 4], label[2, 3] = 1, 2, 3, 3, 1
    elif name == "length1":
        label, lens = torch.zeros(2, 5, dtype=torch.int32), [1, 5]
        label[0, 0] = 2
    elif name == "wave":  # labels on both sides of the 63 | 64 wave boundary
        label, lens = torch.zeros(3, 130, dtype=torch.int32), [130, 65, 1]
        for b, js in enumerate(([5, 62, 63, 64, 65, 127, 129], [63, 64], [0])):
            for i, j in enumerate(js):
                label[b, j] = 1 + i % 3
    elif name == "tiles":  # three tiles of 256 tokens, ~10 % labels
        label = ((torch.rand(2, 515, generator=g) < 0.1) * torch.randint(1, 4, (2, 515), generator=g)).int()
        label[0, 255], label[0, 256], label[1, 511], label[1, 512], label[1, 514] = 1, 2, 3, 1, 2
        lens = [515, 300]
    elif name == "c4":
        label, lens, C = torch.zeros(2, 6, dtype=torch.int32), [6, 3], 4
        label[0, 2], label[1, 1] = 3, 1
    elif name == "ties":  # inference: ties count severally, so fp_number exceeds the insertions and T' with it
        label, lens = torch.zeros(2, 6, dtype=torch.int32), [6, 4]
        label[0, 1], label[1, 0], label[1, 3] = 1, 1, 2
        number = torch.tensor([3, 5], dtype=torch.int32)
    else:
        raise KeyError(name)
    lens = torch.tensor(lens, dtype=torch.int32)
    if number is None:
        number = (label > 0).sum(1).int()
    return label, lens, number, C


_CASES = ["none", "fixture", "edges", "length1", "wave", "tiles", "c4", "ties"]


def _plan_raw(dev, label, lens, number, emo, spk, cap):
    """kantts_fp_plan into buffers with a guard row on either side; returns the host view of everything."""
    import kantts._hip as hip

    B, T = label.shape
    i32 = dict(device=dev, dtype=torch.int32)
    src = torch.full((B + 2, cap), _SENTINEL, **i32)
    e_out = torch.full((B + 2, cap), _SENTINEL, device=dev, dtype=torch.int64)
    s_out = torch.full((B + 2, cap), _SENTINEL, device=dev, dtype=torch.int64)
    inter, meta = torch.full((B + 2,), _SENTINEL, **i32), torch.full((B + 3,), _SENTINEL, **i32)
    pos, nins = torch.full((B + 2, T), _SENTINEL, **i32), torch.full((B + 2,), _SENTINEL, **i32)
    rc = hip.fp_plan(label.to(dev), lens.to(dev), number.to(dev), emo.to(dev), spk.to(dev), inter[1:B + 1], meta[1:B + 2],
                     src[1:B + 1], pos[1:B + 1], nins[1:B + 1], e_out[1:B + 1], s_out[1:B + 1], B=B, T=T, cap=cap)
    for t in (src, e_out, s_out, pos):  # guard rows
        assert bool((t[0] == _SENTINEL).all()) and bool((t[-1] == _SENTINEL).all())
    for t in (inter, nins):
        assert int(t[0]) == _SENTINEL and int(t[-1]) == _SENTINEL
    assert int(meta[0]) == _SENTINEL and int(meta[-1]) == _SENTINEL
    return rc, dict(src=src[1:B + 1], emo=e_out[1:B + 1], spk=s_out[1:B + 1], inter=inter[1:B + 1], meta=meta[1:B + 2],
                    pos=pos[1:B + 1], nins=nins[1:B + 1])


# ---------------------------------------------------------------------------------------------------------------------
# 1. plan + insert forward
@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("name", _CASES)
def test_plan_and_insert_forward_equal_the_closed_form(name, leg):
    import kantts._hip as hip

    ctx, dev = _leg(leg)
    label, lens, number, C = _case(name)
    B, T = label.shape
    g = torch.Generator().manual_seed(11)
    text_hid, fill = torch.randn(B, T, C, generator=g), torch.randn(3, 3, C, generator=g)
    emo, spk = torch.randint(0, 33, (B, T), generator=g), torch.randint(0, 6, (B, T), generator=g)
    want, inter, Tp, emo_w, spk_w, src_w = _closed_form(text_hid, fill, label, lens, number, emo, spk)
    with ctx:
        assert hip.has_fp()
        cap = Tp + 5
        rc, o = _plan_raw(dev, label, lens, number, emo, spk, cap)
        assert rc == 0
        meta = o["meta"].cpu()
        assert int(meta[0]) == Tp and bool((meta[1:] == 0).all())
        if name == "none":
            assert Tp == T
        assert torch.equal(o["inter"].cpu().long(), inter.long())
        assert torch.equal(o["src"][:, :Tp].cpu().long(), src_w)
        assert torch.equal(o["emo"][:, :Tp].cpu(), emo_w) and torch.equal(o["spk"][:, :Tp].cpu(), spk_w)
        for k in ("src", "emo", "spk"):  # nothing at or past column T'
            assert bool((o[k][:, Tp:] == _SENTINEL).all()), k
        assert torch.equal(o["nins"].cpu(), (label > 0).sum(1).int())
        # the gather: output rows between two NaN guard blocks
        guard = 3
        buf = torch.full((B * Tp + 2 * guard, C), float("nan"), device=dev)
        out = buf[guard:guard + B * Tp].view(B, Tp, C)
        assert hip.fp_insert_fwd(text_hid.to(dev), fill.to(dev), o["src"], out, B=B, T=T, Tp=Tp, cap=cap, C=C) == 0
        assert torch.equal(out.cpu(), want)
        assert bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + B * Tp:]).all())


def _check_fixture_insert(dev):
    """The product's insert_fp on the reference's own text_hid and filler rows: the reference's four outputs, bit for bit."""
    from kantts._hip import ops

    tr = _fix()["train"]
    b = tr["batch"]
    lab = b["fp_label"].int().to(dev)
    plan = ops.fp_plan(lab, b["input_lengths"].int().to(dev), (lab > 0).sum(1).int(), b["inputs_emotion"].to(dev),
                       b["inputs_speaker"].to(dev))
    out = ops.fp_insert(tr["text_hid"].to(dev), tr["fillers"].to(dev), plan)
    ref = tr["insert_fp"]
    assert plan.Tp == 16 and plan.Tp - b["inputs_ling"].size(1) > b["inputs_ling"].size(1)  # delta > T: wraps twice
    assert torch.equal(out.cpu(), ref["text_hid"])
    assert torch.equal(plan.emo.cpu(), ref["inputs_emotion"]) and torch.equal(plan.spk.cpu(), ref["inputs_speaker"])
    assert torch.equal(plan.inter_len.cpu().long(), ref["inter_lengths"])


@pytest.mark.parametrize("leg", LEGS)
def test_insert_fp_equals_the_reference_bit_for_bit(leg):
    ctx, dev = _leg(leg)
    with ctx:
        _check_fixture_insert(dev)


@pytest.mark.parametrize("leg", LEGS)
def test_plan_and_insert_return_codes(leg):
    import kantts._hip as hip
    from kantts._hip import ops

    ctx, dev = _leg(leg)
    label, lens, number, _ = _case("edges")
    B, T = label.shape
    emo = spk = torch.zeros(B, T, dtype=torch.int64)
    with ctx:
        # C = 6: no float4 per lane
        x6, f6 = torch.zeros(B, T, 6, device=dev), torch.zeros(9, 6, device=dev)
        rc, o = _plan_raw(dev, label, lens, number, emo, spk, 32)
        assert rc == 0
        out6 = torch.full((B, 13, 6), float("nan"), device=dev)
        assert hip.fp_insert_fwd(x6, f6, o["src"], out6, B=B, T=T, Tp=13, cap=32, C=6) == _E_UNSUPPORTED
        assert bool(torch.isnan(out6).all())
        with pytest.raises(RuntimeError, match="C = 6"):
            ops.fp_head(x6, torch.zeros(4, 6, device=dev), torch.zeros(4, device=dev), lens.to(dev))
        assert hip.fp_insert_fwd(torch.zeros(B, T, 8, device=dev), torch.zeros(9, 8, device=dev), o["src"],
                                 torch.zeros(B, 40, 8, device=dev), B=B, T=T, Tp=40, cap=32, C=8) == _E_BADARG  # Tp > cap
        # cap < T' (13): reported, and nothing is written outside cap
        rc, o = _plan_raw(dev, label, lens, number, emo, spk, 9)
        meta = o["meta"].cpu()
        assert rc == 0 and int(meta[0]) == 13 and bool((meta[1:] & hip.FP_ERR_CAP).all())
        with pytest.raises(ValueError, match="9 columns.*13"):
            ops.fp_plan(label.to(dev), lens.to(dev), number.to(dev), cap=9)
        assert ops.fp_plan(label.to(dev), lens.to(dev), number.to(dev)).Tp == 13
        # a tie-inflated T' beyond the default map width (4 T) is planned again at its own width
        big = ops.fp_plan(label.to(dev), lens.to(dev), torch.tensor([21, 0, 0], dtype=torch.int32, device=dev))
        assert big.Tp == T + 7 + 63 - 7 and big.cap == big.Tp
        # negative length
        bad = lens.clone()
        bad[1] = -2
        rc, o = _plan_raw(dev, label, bad, number, emo, spk, 32)
        assert rc == 0 and o["meta"].cpu()[1:].tolist() == [0, hip.FP_ERR_LENGTH, 0]
        with pytest.raises(ValueError, match="length"):
            ops.fp_plan(label.to(dev), bad.to(dev), number.to(dev))
        # label 4
        lab4 = label.clone()
        lab4[2, 1] = 4
        rc, o = _plan_raw(dev, lab4, lens, number, emo, spk, 32)
        assert rc == 0 and o["meta"].cpu()[1:].tolist() == [0, 0, hip.FP_ERR_LABEL]
        with pytest.raises(ValueError, match="label"):
            ops.fp_plan(lab4.to(dev), lens.to(dev), number.to(dev))
        # host-visible argument errors
        assert hip.fp_plan(label.to(dev), lens.to(dev), number.to(dev), None, None, o["inter"], o["meta"], o["src"], o["pos"],
                           o["nins"], None, None, B=B, T=0, cap=32) == _E_BADARG


# ---------------------------------------------------------------------------------------------------------------------
# 2. decision
def _decide(dev, logits, lens, fp_label=None, weight=None):
    """The head on rows that ARE the logits (C = 4, identity weight) or with a given weight."""
    from kantts._hip import ops

    w = torch.eye(4) if weight is None else weight
    p, label, number = ops.fp_head(logits.to(dev), w.to(dev), torch.zeros(4, device=dev), lens.to(dev),
                                   None if fp_label is None else fp_label.to(dev))
    return p.cpu(), label.cpu(), number.cpu()


@pytest.mark.parametrize("leg", LEGS)
def test_decision_rule(leg):
    ctx, dev = _leg(leg)
    with ctx:
        # unique maximum: the arg-max class inserts unless it is class 0 or the token is padding
        lens = torch.tensor([5, 3], dtype=torch.int32)
        cls = torch.tensor([[0, 1, 2, 3, 0], [3, 0, 2, 1, 3]])
        logits = F.one_hot(cls, 4).float() * 2.0
        p, label, number = _decide(dev, logits, lens)
        want = cls.int() * (torch.arange(5)[None] < lens[:, None])
        assert torch.equal(label, want) and torch.equal(number, (want > 0).sum(1).int())
        assert torch.allclose(p, torch.softmax(logits, -1), atol=2e-5, rtol=0)
        # all tie: zero weight -> 0.25 everywhere; three counts per valid token, class 1 inserted, padding never
        p, label, number = _decide(dev, torch.randn(2, 5, 4), lens, weight=torch.zeros(4, 4))
        assert bool((p == 0.25).all())
        assert torch.equal(number, 3 * lens) and torch.equal(label, (torch.arange(5)[None] < lens[:, None]).int())
        # class 0 ties with class 2: still inserts class 2, counted once
        logits = torch.tensor([1.0, 0.0, 1.0, 0.0]).repeat(2, 5, 1)
        _, label, number = _decide(dev, logits, lens)
        assert torch.equal(number, lens) and torch.equal(label, 2 * (torch.arange(5)[None] < lens[:, None]).int())
        # teacher forcing: the labels as given, padded slots included
        given = torch.tensor([[0, 1, 0, 0, 3], [0, 0, 0, 2, 1]], dtype=torch.int32)
        _, label, number = _decide(dev, logits, lens, fp_label=given)
        assert torch.equal(label, given) and number.tolist() == [2, 2]
        # more tokens than a workgroup has threads
        lens = torch.tensor([300, 257], dtype=torch.int32)
        cls = torch.randint(0, 4, (2, 300), generator=torch.Generator().manual_seed(2))
        _, label, number = _decide(dev, F.one_hot(cls, 4).float(), lens)
        want = cls.int() * (torch.arange(300)[None] < lens[:, None])
        assert torch.equal(label, want) and torch.equal(number, (want > 0).sum(1).int())


# ---------------------------------------------------------------------------------------------------------------------
# 3. insert backward
@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("name", ["fixture", "wave", "ties", "c4"])
def test_insert_backward_against_fp64_sums(name, leg):
    from kantts._hip import ops

    ctx, dev = _leg(leg)
    label, lens, number, C = _case(name)
    B, T = label.shape
    g = torch.Generator().manual_seed(21)
    with ctx:
        plan = ops.fp_plan(label.to(dev), lens.to(dev), number.to(dev))
        Tp = plan.Tp
        d_out = torch.randn(B, Tp, C, generator=g)
        runs = []
        for _ in range(2):
            x = torch.zeros(B, T, C, device=dev, requires_grad=True)
            fill = torch.zeros(3, 3, C, device=dev, requires_grad=True)
            ops.fp_insert(x, fill, plan).backward(d_out.to(dev))
            runs.append((x.grad.cpu(), fill.grad.cpu()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])  # equal bits
        src = plan.src[:, :Tp].cpu().long()
    u = 2.0 ** -24
    d64 = d_out.double()
    for b in range(B):
        for j in range(T):
            terms = d64[b][src[b] == j]
            err = (runs[0][0][b, j].double() - terms.sum(0)).abs()
            assert bool((err <= max(len(terms) - 1, 0) * u * terms.abs().sum(0)).all()), (b, j, len(terms))
    n_max = 0
    for r in range(9):
        terms = d64[src == -(r + 1)]
        n_max = max(n_max, len(terms))
        err = (runs[0][1].reshape(9, C)[r].double() - terms.sum(0)).abs()
        assert bool((err <= max(len(terms) - 1, 0) * u * terms.abs().sum(0)).all()), (r, len(terms))
    assert n_max >= 1


# ---------------------------------------------------------------------------------------------------------------------
# 4. head and CE against plain torch
_CE_WEIGHT = [1.0, 4.0, 4.0, 8.0]


def _torch_ce(p, label, lens, single=False):
    mask = torch.arange(label.size(1))[None] < lens[:, None]
    w = torch.tensor(_CE_WEIGHT)
    if single:  # what a criterion WITHOUT the second softmax would give: weighted NLL of the probabilities themselves
        ce = -w[label] * torch.log(torch.gather(p, 2, label.unsqueeze(-1)).squeeze(-1))
    else:
        ce = torch.nn.CrossEntropyLoss(weight=w, reduction="none")(p.transpose(2, 1), label)
    return (ce * mask).sum() / mask.sum()


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("shape", [(3, 9, 32, [9, 5, 1]), (2, 300, 8, [300, 129])], ids=["small", "two_tiles"])
def test_head_and_ce_against_torch(shape, leg):
    from kantts._hip import ops

    B, T, C, lens = shape
    ctx, dev = _leg(leg)
    g = torch.Generator().manual_seed(31)
    x, w, b = torch.randn(B, T, C, generator=g), 0.5 * torch.randn(4, C, generator=g), torch.randn(4, generator=g)
    label = torch.randint(0, 4, (B, T), generator=g)
    lens = torch.tensor(lens)
    ref_in = [t.clone().requires_grad_(True) for t in (x, w, b)]
    p_ref = F.softmax(F.linear(*ref_in), dim=2)
    loss_ref = _torch_ce(p_ref, label, lens)
    g_ref = torch.autograd.grad(loss_ref, ref_in + [p_ref], retain_graph=True)
    cot = torch.randn(B, T, 4, generator=g)  # the head's backward on its own, with a dense cotangent
    h_ref = torch.autograd.grad((p_ref * cot).sum(), ref_in)
    with ctx:
        got_in = [t.clone().to(dev).requires_grad_(True) for t in (x, w, b)]
        p, _, _ = ops.fp_head(got_in[0], got_in[1], got_in[2], lens.int().to(dev))
        loss = ops.fp_ce(p, label.int().to(dev), lens.int().to(dev), torch.tensor(_CE_WEIGHT, device=dev))
        g_got = torch.autograd.grad(loss, got_in + [p], retain_graph=True)
        h_got = torch.autograd.grad((p * cot.to(dev)).sum(), got_in)
        print("fp head/ce", shape[:3], "probs %.2e loss %.2e" % (float((p.detach().cpu() - p_ref.detach()).abs().max()),
                                                                abs(float(loss.detach()) - float(loss_ref.detach()))),
              "grads", ["%.1e" % rel_l2(a.cpu(), r) for a, r in zip(list(g_got) + list(h_got), list(g_ref) + list(h_ref))])
        assert float((p.detach().cpu() - p_ref.detach()).abs().max()) <= 2e-5
        assert abs(float(loss.detach()) - float(loss_ref.detach())) <= 2e-5
        for a, r in zip(list(g_got) + list(h_got), list(g_ref) + list(h_ref)):
            assert rel_l2(a.cpu(), r) <= 1e-4
        assert bool((g_got[3].cpu()[torch.arange(T)[None] >= lens[:, None]] == 0).all())  # no gradient on padding
    # the second softmax is part of the contract: without it the loss is a different number
    assert abs(float(_torch_ce(p_ref.detach(), label, lens, single=True)) - float(loss_ref)) > 2e-5


@pytest.mark.parametrize("leg", LEGS)
def test_fpce_module_follows_the_input_device(leg):
    from kantts.train.loss import FpCELoss, criterion_builder

    ctx, dev = _leg(leg)
    crit = criterion_builder({"Loss": {"FpCELoss": {"enable": True, "params": {"loss_type": "ce", "weight": [1, 4, 4, 8]}},
                                       "MelReconLoss": {"enable": True, "params": {"loss_type": "mae"}}}})
    assert isinstance(crit["FpCELoss"], FpCELoss) and crit["FpCELoss"].weights == 1.0
    tr = _fix()["train"]
    with ctx:  # the module was built on the host (no .cuda() in the constructor); the weight follows the input
        got = crit["FpCELoss"](tr["batch"]["input_lengths"].to(dev), tr["outputs"]["fp_predictions"].to(dev),
                               tr["batch"]["fp_label"].to(dev))
        assert abs(float(got) - tr["losses"]["fp_loss"]) <= 1e-5
    with pytest.raises(ValueError):
        FpCELoss(loss_type="mse")


def test_emulated_abi_has_no_filled_pause_entry_points(emulated_cabi):
    """The numpy model of the C ABI does not get these entries: the probe says so and an FP model refuses to be built."""
    import kantts._hip as hip
    from kantts.models.sambert.kantts_sambert import KanTtsSAMBERT

    assert not hip.has_fp() and sorted(hip.missing_fp_symbols()) == sorted(hip.FP_SYMBOLS)
    with pytest.raises(RuntimeError, match="kantts_fp_plan"):
        KanTtsSAMBERT(dict(_fix()["cfg"]))


# ---------------------------------------------------------------------------------------------------------------------
# 5. fixture parity of the product model
def _fp_model(dev, dur_bias=None, seed=None):
    from kantts.models.sambert.kantts_sambert import KanTtsSAMBERT

    fix = _fix()
    torch.manual_seed(fix["seed_w"] if seed is None else seed)
    m = KanTtsSAMBERT(dict(fix["cfg"]))
    m.fp_dict = {k: torch.tensor(v, dtype=torch.long).unsqueeze(0) for k, v in fix["fp_ids"].items()}
    if dur_bias is not None:
        with torch.no_grad():
            m.variance_adaptor.duration_predictor.fc.bias.fill_(dur_bias)
    return m.to(dev).eval()


def _check_train_fixture(dev, atol):
    from kantts.train.loss import FpCELoss, MelReconLoss, ProsodyReconLoss

    fix = _fix()
    tr = fix["train"]
    m = _fp_model("cpu")
    assert sorted(m.state_dict().keys()) == tr["state_keys"]
    for k, (shape, s, a) in tr["weight_checksums"].items():
        v = m.state_dict()[k]
        assert tuple(v.shape) == shape and abs(float(v.double().sum()) - s) <= 1e-6 * max(1.0, a), k
    m = m.to(dev)
    b = {k: v.to(dev) for k, v in tr["batch"].items()}
    res = m(**b)
    assert res["x_band_width"] == tr["x_band_width"]
    for k, ref in tr["outputs"].items():
        got = res[k].detach().cpu()
        if ref.is_floating_point():
            err = float((got - ref).abs().max())
            print("fp train fixture", dev, k, "%.2e" % err)
            assert got.shape == ref.shape and err <= atol, (k, err)
        else:
            assert torch.equal(got, ref), k
    mel_, mel = MelReconLoss()(b["output_lengths"], b["mel_targets"], res["dec_outputs"], res["postnet_outputs"])
    d, p, e = ProsodyReconLoss()(res["valid_inter_lengths"], res["duration_targets"], res["pitch_targets"],
                                 res["energy_targets"], res["log_duration_predictions"], res["pitch_predictions"],
                                 res["energy_predictions"])
    fp = FpCELoss()(b["input_lengths"], res["fp_predictions"], b["fp_label"])
    total = mel_ + mel + d + p + e + fp
    got = dict(mel_loss_=mel_, mel_loss=mel, dur_loss=d, pitch_loss=p, energy_loss=e, fp_loss=fp, total=total)
    for k, ref in tr["losses"].items():
        print("fp train fixture", dev, k, "%.2e" % abs(float(got[k].detach()) - ref))
        assert abs(float(got[k]) - ref) <= 1e-5, (k, float(got[k]), ref)
    total.backward()
    named = dict(m.named_parameters())
    assert sorted(k for k, v in named.items() if v.grad is not None) == sorted(tr["grad_summaries"])
    worst = 0.0
    for k, (s, nrm) in tr["grad_summaries"].items():
        gr = named[k].grad.double()
        e_n = abs(float(gr.norm()) - nrm) / nrm
        e_s = abs(float(gr.sum()) - s) / (gr.numel() ** 0.5 * nrm)
        worst = max(worst, e_n, e_s)
        assert e_n <= 1e-4 and e_s <= 1e-4, (k, e_n, e_s)
    print("fp train fixture", dev, "worst gradient summary %.2e" % worst)


def _check_infer_fixture(dev, atol):
    inf = _fix()["infer"]
    m = _fp_model(dev, dur_bias=inf["dur_bias"])
    with torch.no_grad():
        ts = m._token_side(**{k: v.to(dev) for k, v in inf["batch"].items()})
        res = m(**{k: v.to(dev) for k, v in inf["batch"].items()})
    label, number = ts.fp_decisions
    assert torch.equal(label.cpu(), inf["label"]) and torch.equal(number.cpu(), inf["fp_number"])
    assert len(set(inf["label"][inf["label"] > 0].tolist())) >= 2  # insertions of at least two classes
    assert res["x_band_width"] == inf["x_band_width"]
    for k, ref in inf["outputs"].items():
        got = res[k].detach().cpu()
        if ref.is_floating_point():
            err = float((got - ref).abs().max())
            print("fp infer fixture", dev, k, "%.2e" % err)
            assert got.shape == ref.shape and err <= atol, (k, err)
        else:
            assert torch.equal(got, ref), k  # valid_inter_lengths, LR_length_rounded: identical


def test_fixture_parity_teacher_forced_kernel_source():
    with kernel_source_on_cpu():
        _check_train_fixture("cpu", 2e-5)


def test_fixture_parity_inference_kernel_source():
    with kernel_source_on_cpu():
        _check_infer_fixture("cpu", 2e-5)


@pytest.mark.gpu
def test_fixture_parity_teacher_forced_gpu():
    with _precision("fp32"):
        _check_train_fixture("cuda", 1e-4)


@pytest.mark.gpu
def test_fixture_parity_inference_gpu():
    with _precision("fp32"):
        _check_infer_fixture("cuda", 1e-4)


# ---------------------------------------------------------------------------------------------------------------------
# 6. batched inference
def _infer_batch(dev, B=3, T_in=9):
    import torch_oracle as O

    batch = O.synthetic_sambert_batch(B=B, T_in=T_in, seed=91, min_len=4, dur_hi=6)
    args = {k: batch[k].to(dev) for k in ("inputs_ling", "inputs_emotion", "inputs_speaker", "input_lengths")}
    args["input_lengths"] = torch.tensor([T_in - 1, 6, 4][:B], device=dev)
    return args


def _check_batched_inference(dev, atol):
    """A batch gives every utterance the frames of ITS ROW inferred at batch 1, i.e. at the same padded width T.  Not of
    the utterance trimmed to its own length: two reference quirks that are kept depend on T -- the predictor's unmasked
    k = 3 window behind the last token, and the emotion / speaker ids repeated with period T (KanTtsSAMBERT.forward)."""
    import kantts._hip as hip

    m = _fp_model(dev, dur_bias=1.5)
    args = _infer_batch(dev)
    with torch.no_grad():
        with hip.precision_scope("fp32"):
            res = m(**args)
            ts32 = m._token_side(**args)
        with hip.precision_scope("bf16"):
            ts16 = m._token_side(**args)
        for a, b in zip(ts32.fp_decisions, ts16.fp_decisions):  # index decisions: the same in both precision modes
            assert torch.equal(a, b)
        assert torch.equal(ts32.inter_lengths, ts16.inter_lengths) and torch.equal(ts32.fp_predictions, ts16.fp_predictions)
        label, number = ts32.fp_decisions
        assert int((label > 0).sum(1).min()) >= 1
        for i in range(args["inputs_ling"].size(0)):
            n_in = int(args["input_lengths"][i])
            # the same padded row at batch 1: the reference repeats the (unshifted) emotion / speaker ids with period T
            one = m(**{k: v[i:i + 1].contiguous() for k, v in args.items()})
            n = int(one["LR_length_rounded"][0])
            assert int(res["LR_length_rounded"][i]) == n and n > 0
            assert torch.equal(res["valid_inter_lengths"][i:i + 1], one["valid_inter_lengths"])
            assert torch.equal(res["fp_predictions"][i, :n_in].argmax(-1), one["fp_predictions"][0, :n_in].argmax(-1))
            err = float((res["postnet_outputs"][i, :n] - one["postnet_outputs"][0, :n]).abs().max())
            print("fp batched inference", dev, i, n, "%.2e" % err)
            assert err <= atol, (i, err)


def test_batched_inference_equals_batch_1_of_the_same_padded_row_kernel_source():
    with kernel_source_on_cpu():
        _check_batched_inference("cpu", 2e-5)


@pytest.mark.gpu
def test_batched_inference_equals_batch_1_of_the_same_padded_row_gpu():
    with _precision("fp32"):
        _check_batched_inference("cuda", 1e-4)


# ---------------------------------------------------------------------------------------------------------------------
# 7. streaming
_EXACT = ("dec_outputs", "LR_length_rounded", "log_duration_predictions", "pitch_predictions", "energy_predictions",
          "fp_predictions", "valid_inter_lengths")


def _twin(a, b, what):
    """The bounds the existing streaming tests use for a bf16 path against its twin (tests/test_acoustic_slots.py)."""
    a, b = a.cpu(), b.cpu()
    scale = float(b.abs().max())
    err = (rel_l2(a, b), float((a - b).abs().max()))
    print("fp streaming", what, "rel_l2 %.3e max-abs %.3e scale %.3e" % (err + (scale,)))
    assert err[0] < 3e-3 and err[1] < 3e-2 * scale, (what, err)


def _check_streaming(dev):
    from kantts.models.sambert.chunked import ChunkedAcoustic
    from kantts.models.sambert.slots import AcousticSlots

    m = _fp_model(dev, dur_bias=1.5)
    m.mel_decoder.decode_mode = "kernel"
    args = _infer_batch(dev)
    utts = [{k: (v[i:i + 1, :int(args["input_lengths"][i])].contiguous() if k != "input_lengths" else v[i:i + 1])
             for k, v in args.items()} for i in range(3)]
    with torch.no_grad():
        refs = [m(**u) for u in utts]
    for r in refs:  # at least one insertion per utterance
        assert int(r["valid_inter_lengths"][0]) > int(r["fp_predictions"].size(1))
    # one session per utterance
    ca = ChunkedAcoustic(m)
    for i, (u, ref) in enumerate(zip(utts, refs)):
        sess = ca.open(**u)
        while not sess.finished:
            sess.step(4)
        got = sess.result()
        assert set(got) == set(ref)
        for k in _EXACT:
            assert torch.equal(got[k], ref[k]), (i, k)
        _twin(got["postnet_outputs"], ref["postnet_outputs"], "session %d" % i)
    # two slots, three utterances: the third is admitted when a slot frees, steps after the first two
    steps = max(r["dec_outputs"].size(1) for r in refs) // m.mel_decoder.r
    pool = AcousticSlots(m, slots=2, max_steps=steps)
    results = {}
    for _ in pool.play_many(utts, 3, results=results):
        pass
    assert sorted(results) == [0, 1, 2]
    for i, ref in enumerate(refs):
        for k in _EXACT:
            assert torch.equal(results[i][k], ref[k]), (i, k)
        _twin(results[i]["postnet_outputs"], ref["postnet_outputs"], "slot utterance %d" % i)
    # over capacity: the pool is sized in decoder steps, and the inserted rows count; both numbers are in the message
    own = int(refs[0]["dec_outputs"].size(1)) // m.mel_decoder.r
    inter = int(refs[0]["valid_inter_lengths"][0])
    small = AcousticSlots(m, slots=1, max_steps=own - 1)
    with pytest.raises(ValueError, match=r"%d decoder steps \(%d token rows.*max_steps = %d" % (own, inter, own - 1)):
        small.admit(0, **utts[0])
    assert small.free_slots() == [0]
    assert AcousticSlots(m, slots=1, max_steps=own).admit(0, **utts[0]) == int(refs[0]["LR_length_rounded"][0])


@pytest.mark.parametrize("leg", LEGS)
def test_streaming_sessions_and_slots_give_the_frames_of_forward(leg):
    ctx, dev = _leg(leg)
    with _precision("bf16"), ctx:
        _check_streaming(dev)


# ---------------------------------------------------------------------------------------------------------------------
# 8. above the model
def _language_dir(tmp):
    """PhoneSet.xml / tonelist.txt written from the inventory tests/golden/am_dataset.pt carries (PinYin)."""
    fx = torch.load(os.path.join(GOLDEN, "am_dataset.pt"), weights_only=False)
    d = os.path.join(tmp, "PinYin")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "PhoneSet.xml"), "w") as f:
        f.write("<phoneSet>" + "".join("<phone><name>%s</name></phone>" % p for p in fx["phones"]) + "</phoneSet>")
    with open(os.path.join(d, "tonelist.txt"), "w") as f:
        f.write("\n".join(fx["tones_file"]) + "\n")
    return d


def _fp_config(tmp, params=None):
    unit = dict(_fix()["fpdict"]["unit"], language_dir=_language_dir(tmp))
    params = dict(params if params is not None else {"FP": True, "outputs_per_step": 3})
    return {"model_type": "sambert", "linguistic_unit": unit, "Model": {"KanTtsSAMBERT": {"params": params}}}


def test_get_fpdict_ids_equal_the_reference(tmp_path):
    from kantts.utils.ling_unit import KanTtsLinguisticUnit, get_fpdict

    config = _fp_config(str(tmp_path))
    got = get_fpdict(config)
    ref = _fix()["fpdict"]["ids"]
    assert sorted(got) == [1, 2, 3]
    for c in (1, 2, 3):
        assert got[c].shape == (3, 4) and torch.equal(torch.from_numpy(got[c]).long(), ref[c]), c
    unit = KanTtsLinguisticUnit(config)
    assert unit.fp_enable and unit._fpadd_lfeat_type_list == ["sy", "emo_category"]
    plain = dict(config, Model={"KanTtsSAMBERT": {"params": {}}})
    assert not hasattr(KanTtsLinguisticUnit(plain), "_fpadd_lfeat_type_list")


def _tok(sy, emo="emotion_neutral", tone="tone1"):
    return "{%s$%s$s_both$word_both$%s$F7}" % (sy, tone, emo)


def test_fp_dataset_and_collate(tmp_path):
    from kantts.datasets.dataset import AM_Dataset, get_am_datasets, get_fp_label
    from kantts.datasets.device_batching import make_train_loader

    config = _fp_config(str(tmp_path))
    root = str(tmp_path / "data")
    for d in ("mel", "duration", "f0", "energy", "frame_f0", "frame_uv"):
        os.makedirs(os.path.join(root, d))
    # fpadd lines (the filler tokens carry emotion_disgust) and the labels the reference's get_fp_label gives them,
    # "~" slot included; the fprm line of an utterance has one token per label but the last
    fx = _fix()["fplabel"]
    for ln, lb in zip(fx["lines"], fx["labels"]):  # incl. the ambiguous lines: runs at index 0 / 1, long and adjacent runs
        assert get_fp_label(ln).tolist() == lb, ln
    assert len(fx["lines"]) >= 12 and sorted(max(lb) for lb in fx["labels"][:3]) == [1, 2, 3]
    phones = torch.load(os.path.join(GOLDEN, "am_dataset.pt"), weights_only=False)["phones"][:5]  # symbols of the inventory
    utts = [("u%d" % i, phones[:len(lb) - 1], ln.split(" "), lb)
            for i, (ln, lb) in enumerate(zip(fx["lines"][:3], fx["labels"][:3]))]
    rs = np.random.RandomState(3)
    with open(os.path.join(root, "am_fprm_train.lst"), "w") as f, open(os.path.join(root, "am_fpadd_train.lst"), "w") as g:
        for name, syms, add, labels in utts:
            f.write("%s\t%s\n" % (name, " ".join(_tok(s) for s in syms)))
            g.write("%s\t%s\n" % (name, " ".join(add)))
            assert get_fp_label(" ".join(add)).tolist() == labels, name
            n_dur = len(add)  # the durations describe the sequence WITH the fillers
            dur = rs.randint(1, 5, size=n_dur)
            np.save(os.path.join(root, "duration", name + ".npy"), dur)
            np.save(os.path.join(root, "mel", name + ".npy"), rs.randn(int(dur.sum()), 80).astype(np.float32))
            for d in ("f0", "energy"):
                np.save(os.path.join(root, d, name + ".npy"), rs.randn(n_dur).astype(np.float32))
        f.write("u3\t%s\n" % _tok(phones[0]))  # no fpadd twin: dropped with a warning
    ds = AM_Dataset(config, os.path.join(root, "am_fprm_train.lst"), root)
    assert ds.fp_enable and len(ds) == 3
    items = [ds[i] for i in range(3)]
    for (name, syms, add, labels), item in zip(utts, items):
        assert item[6].tolist() == labels and len(item[0][0]) == len(syms) + 1, name
    batch = ds.collate_fn(items)
    assert batch["fp_label"].dtype == torch.int64
    max_in = max(len(u[3]) for u in utts)
    assert batch["fp_label"].tolist() == [u[3] + [0] * (max_in - len(u[3])) for u in utts]  # padded with 0
    assert batch["valid_input_lengths"].tolist() == [len(u[3]) - 1 for u in utts]
    assert tuple(batch["input_lings"].shape) == (3, max_in, 4)
    max_dur = max(len(u[2]) for u in utts) + 1
    assert tuple(batch["durations"].shape) == (3, max_dur)
    assert tuple(batch["pitch_contours"].shape) == (3, max_dur) and tuple(batch["energy_contours"].shape) == (3, max_dur)
    # the lists an FP configuration reads
    with open(os.path.join(root, "am_fprm_valid.lst"), "w") as f, open(os.path.join(root, "am_fpadd_valid.lst"), "w") as g:
        f.write("u2\t%s\n" % " ".join(_tok(s) for s in utts[2][1]))
        g.write("u2\t%s\n" % " ".join(utts[2][2]))
    train_set, valid_set = get_am_datasets(os.path.join(root, "fprm_metafile.txt"), root, config, False)
    assert len(train_set) == 3 and len(valid_set) == 1
    # --device_corpus has no fp_label stream: refused
    with pytest.raises(NotImplementedError, match="device_corpus"):
        make_train_loader("am", ds, None, "cpu", 2, mode="hbm")
    assert make_train_loader("am", ds, "host", "cpu", 2, mode="off") == "host"


def _trainer(dev, tmp, graph=False, params_extra=None):
    from kantts.models import model_builder
    from kantts.train.loss import criterion_builder
    from kantts.train.trainer import Sambert_Trainer

    cfg = dict(_fix()["cfg"])
    cfg.update(params_extra or {})
    config = _fp_config(str(tmp), params=cfg)
    config["Model"]["KanTtsSAMBERT"].update(
        optimizer={"type": "Adam", "params": {"lr": 0.001, "betas": [0.9, 0.98], "eps": 1e-9, "weight_decay": 0.0}},
        scheduler={"type": "NoamLR", "params": {"warmup_steps": 4000}})
    config.update(grad_norm=1.0, batch_size=3, log_interval_steps=1, Loss={
        "MelReconLoss": {"enable": True, "params": {"loss_type": "mae"}},
        "ProsodyReconLoss": {"enable": True, "params": {"loss_type": "mae"}},
        "FpCELoss": {"enable": True, "params": {"loss_type": "ce", "weight": [1, 4, 4, 8]}}})
    torch.manual_seed(0)
    model, opt, sch = model_builder(config, device=dev)
    crit = criterion_builder(config, dev)
    b = _fix()["train"]["batch"]
    batch = {"input_lings": b["inputs_ling"], "input_emotions": b["inputs_emotion"], "input_speakers": b["inputs_speaker"],
             "valid_input_lengths": b["input_lengths"], "valid_output_lengths": b["output_lengths"],
             "mel_targets": b["mel_targets"], "durations": b["duration_targets"], "pitch_contours": b["pitch_targets"],
             "energy_contours": b["energy_targets"], "attn_priors": None, "fp_label": b["fp_label"]}
    tr = Sambert_Trainer(config, model, opt, sch, crit, torch.device(dev), None, [batch], None, max_steps=10 ** 6,
                         save_dir=str(tmp), save_interval=10 ** 6, valid_interval=10 ** 6, log_interval=1, grad_clip=1.0,
                         graph=graph)
    return tr, batch


def _check_trainer(dev, tmp):
    from collections import defaultdict

    tr, batch = _trainer(dev, tmp)
    net = tr.model["KanTtsSAMBERT"]
    assert sorted(net.fp_dict) == [1, 2, 3] and tuple(net.fp_dict[1].shape) == (1, 3, 4)  # attached by the builder
    net.train()  # dropout on: the counter-based masks of the predictor and the encoder
    before = {k: v.detach().clone() for k, v in net.FP_predictor.named_parameters()}
    total = tr.train_step(batch)
    assert bool(torch.isfinite(total))
    assert any(not torch.equal(before[k], v.detach()) for k, v in net.FP_predictor.named_parameters())
    net.eval()
    tr.eval_step(batch)
    sums = defaultdict(float)
    tr._flush_losses(sums, "train")
    tr._flush_losses(sums, "eval")
    for k in ("train/fp_loss", "eval/fp_loss", "train/TotalLoss", "eval/TotalLoss", "train/mel_loss", "eval/dur_loss"):
        assert k in sums and np.isfinite(sums[k]), (k, dict(sums))
    assert sums["train/fp_loss"] > 0 and sums["eval/fp_loss"] > 0


@pytest.mark.parametrize("leg", LEGS)
def test_eager_trainer_step_with_fp_loss(leg, tmp_path):
    ctx, dev = _leg(leg)
    with _precision("fp32"), ctx:
        _check_trainer(dev, tmp_path)


def test_refusals(tmp_path):
    from kantts.models.sambert.kantts_sambert import KanTtsSAMBERT

    with kernel_source_on_cpu():
        cfg = dict(_fix()["cfg"], SE=True, speaker_units=192)
        with pytest.raises(NotImplementedError, match="SE"):
            KanTtsSAMBERT(cfg)
        with pytest.raises(NotImplementedError, match="read back"):
            _trainer("cpu", tmp_path, graph=True)
        m = _fp_model("cpu")
        m.fp_dict = None
        with pytest.raises(RuntimeError, match="fp_dict"):
            m(**{k: v for k, v in _fix()["infer"]["batch"].items()})
