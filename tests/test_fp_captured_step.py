"""The captured training step of filled-pause voices: kantts_fp_plan_given (the insertion plan from GIVEN labels at a GIVEN
width, no host read), the model's static path (``fp_static_width``), GraphedSambertStep / Sambert_Trainer(graph=True) with
FP, and the FP device corpus.

Legs as in tests/test_filled_pause.py: ``kernel_source`` (the kernel sources on the CPU, util.kernel_source_on_cpu) and,
marked ``gpu``, the device.  Bounds are the project's: index tensors and maps torch.equal; fixture parity 2e-5 (host leg) /
1e-4 (device) for float outputs, losses 1e-5, gradient summaries 1e-4 (the head of tests/test_filled_pause.py); gradients
of one path against another rel-L2 <= 1e-4; a captured against an eager step: loss within 2e-4 relative and arena rel-L2
< 1e-4 in fp32 mode (tests/test_trainer.py::test_graph_trainer_alternating_shapes_matches_eager)."""
import contextlib
import os

import numpy as np
import pytest
import torch

from util import GOLDEN, kernel_source_on_cpu, rel_l2

LEGS = [pytest.param("hostsim", id="kernel_source"), pytest.param("cuda", id="gpu", marks=pytest.mark.gpu)]
_E_BADARG = -1
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
# the closed form, restated: the stream of one row, as long as asked for, and the T' of a batch
def _stream(label_row, T, n):
    rows, p = [], 0
    while len(rows) < n:
        lab = int(label_row[p]) if p < T else 0
        if 1 <= lab <= 3:
            rows += [-(1 + 3 * (lab - 1) + k) for k in range(3)]
        rows.append(p % T)
        p += 1
    return rows[:n]


def _t_prime(label, lens):
    T = label.size(1)
    lens = lens.clamp(0, T).long()
    inter = lens + 3 * ((label >= 1) & (label <= 3)).sum(1)
    return T + int(inter.max()) - int(lens.max()), inter


def _case(name):
    """(label (B, T) int32, lens (B) int32)."""
    if name == "fixture":
        b = _fix()["train"]["batch"]
        return b["fp_label"].int(), b["input_lengths"].int()
    if name == "one":  # B = 1, T = 1, label 3
        return torch.tensor([[3]], dtype=torch.int32), torch.tensor([1], dtype=torch.int32)
    if name == "len0":  # a row of length 0
        label = torch.zeros(3, 6, dtype=torch.int32)
        label[0, 1], label[2, 4] = 2, 1
        return label, torch.tensor([6, 0, 5], dtype=torch.int32)
    if name == "padded":  # labels inside padded slots: they insert and count (kantts_fp_head with given labels)
        label = torch.zeros(3, 7, dtype=torch.int32)
        label[0, 2], label[1, 5], label[1, 6], label[2, 0], label[2, 6] = 1, 3, 2, 2, 1
        return label, torch.tensor([7, 3, 4], dtype=torch.int32)
    if name == "tile":  # the scan crosses its 256-token tile
        label = torch.zeros(4, 300, dtype=torch.int32)
        for b, js in enumerate(([255, 256, 299], [255], [256, 299], [0, 254, 255, 256, 257])):
            for i, j in enumerate(js):
                label[b, j] = 1 + (i + b) % 3
        return label, torch.tensor([300, 256, 257, 299], dtype=torch.int32)
    if name == "none":
        return torch.zeros(3, 7, dtype=torch.int32), torch.tensor([7, 5, 4], dtype=torch.int32)
    raise KeyError(name)


_CASES = ["fixture", "one", "len0", "padded", "tile", "none"]


def _ids(B, T, seed=11):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 33, (B, T), generator=g), torch.randint(0, 6, (B, T), generator=g)


def _given_raw(dev, label, lens, emo, spk, W, guard=3):
    """kantts_fp_plan_given into buffers with ``guard`` columns behind W and a guard row on either side."""
    import kantts._hip as hip

    B, T = label.shape
    i32 = dict(device=dev, dtype=torch.int32)
    src = torch.full((B + 2, W + guard), _SENTINEL, **i32)
    e_out = torch.full((B + 2, W + guard), _SENTINEL, device=dev, dtype=torch.int64)
    s_out = torch.full((B + 2, W + guard), _SENTINEL, device=dev, dtype=torch.int64)
    inter, nins, num = (torch.full((B + 2,), _SENTINEL, **i32) for _ in range(3))
    meta = torch.full((B + 3,), _SENTINEL, **i32)
    pos = torch.full((B + 2, T), _SENTINEL, **i32)
    # the kernel sees dense (B, W) tensors: plan into them, then copy into the guarded frames' interior
    d_src = torch.full((B * W + guard,), _SENTINEL, **i32)
    d_e = torch.full((B * W + guard,), _SENTINEL, device=dev, dtype=torch.int64)
    d_s = torch.full((B * W + guard,), _SENTINEL, device=dev, dtype=torch.int64)
    rc = hip.fp_plan_given(label.to(dev), lens.to(dev), None if emo is None else emo.to(dev),
                           None if spk is None else spk.to(dev), inter[1:B + 1], meta[1:B + 2], d_src[:B * W],
                           pos[1:B + 1], nins[1:B + 1], d_e[:B * W], d_s[:B * W], num[1:B + 1], B=B, T=T, W=W)
    for t in (d_src, d_e, d_s):  # nothing behind the last row
        assert bool((t[B * W:] == _SENTINEL).all())
    assert bool((pos[0] == _SENTINEL).all()) and bool((pos[-1] == _SENTINEL).all())
    for t in (inter, nins, num):
        assert int(t[0]) == _SENTINEL and int(t[-1]) == _SENTINEL
    assert int(meta[0]) == _SENTINEL and int(meta[-1]) == _SENTINEL
    return rc, dict(src=d_src[:B * W].view(B, W), emo=d_e[:B * W].view(B, W), spk=d_s[:B * W].view(B, W),
                    inter=inter[1:B + 1], meta=meta[1:B + 2], pos=pos[1:B + 1], nins=nins[1:B + 1], number=num[1:B + 1])


# ---------------------------------------------------------------------------------------------------------------------
# 1. the given plan equals the read-back plan
@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("name", _CASES)
def test_given_plan_equals_the_read_back_plan(name, leg):
    import kantts._hip as hip
    from kantts._hip import ops

    ctx, dev = _leg(leg)
    label, lens = _case(name)
    B, T = label.shape
    emo, spk = _ids(B, T)
    Tp, inter = _t_prime(label, lens)
    with ctx:
        assert hip.has_fp_given()
        # the parent's path: the head with given labels (identity weight on C = 4 rows), then the plan that reads T' back
        _, lab_h, num_h = ops.fp_head(torch.zeros(B, T, 4, device=dev), torch.eye(4, device=dev), torch.zeros(4, device=dev),
                                      lens.to(dev), label.to(dev))
        ref = ops.fp_plan(lab_h, lens.to(dev), num_h, emo.to(dev), spk.to(dev))
        plan, meta = ops.fp_plan_given(label.to(dev), lens.to(dev), emo.to(dev), spk.to(dev), width=Tp)
        meta = meta.cpu()
        assert ref.Tp == Tp and plan.Tp == Tp and plan.cap == Tp and int(meta[0]) == Tp
        assert bool((meta[1:] == 0).all())
        if name == "none":
            assert Tp == T
        assert tuple(plan.src.shape) == (B, Tp)
        assert torch.equal(plan.src.cpu(), ref.src[:, :Tp].cpu())
        assert torch.equal(plan.src.cpu().long(), torch.tensor([_stream(label[b], T, Tp) for b in range(B)]))
        assert torch.equal(plan.pos.cpu(), ref.pos.cpu()) and torch.equal(plan.nins.cpu(), ref.nins.cpu())
        assert torch.equal(plan.inter_len.cpu(), ref.inter_len.cpu()) and torch.equal(plan.inter_len.cpu().long(), inter)
        assert torch.equal(plan.fp_number.cpu(), num_h.cpu())
        assert torch.equal(plan.emo.cpu(), ref.emo.cpu()) and torch.equal(plan.spk.cpu(), ref.spk.cpu())
        # equal bits on every run, and either id tensor may be absent
        again, _ = ops.fp_plan_given(label.to(dev), lens.to(dev), None, spk.to(dev), width=Tp)
        assert again.emo is None and torch.equal(again.spk, plan.spk) and torch.equal(again.src, plan.src)


# ---------------------------------------------------------------------------------------------------------------------
# 2. a wrong width, bad labels and lengths, bad arguments
@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("name", ["fixture", "padded", "tile"])
@pytest.mark.parametrize("delta", [-1, 2])
def test_wrong_width_is_reported_and_stays_in_bounds(delta, name, leg):
    import kantts._hip as hip
    from kantts._hip import ops

    ctx, dev = _leg(leg)
    label, lens = _case(name)
    B, T = label.shape
    emo, spk = _ids(B, T)
    Tp, inter = _t_prime(label, lens)
    W = Tp + delta
    C = 8
    g = torch.Generator().manual_seed(3)
    with ctx:
        rc, o = _given_raw(dev, label, lens, emo, spk, W)
        assert rc == 0
        meta = o["meta"].cpu()
        assert int(meta[0]) == Tp and meta[1:].tolist() == [hip.FP_ERR_WIDTH] * B
        want = torch.tensor([_stream(label[b], T, W) for b in range(B)])
        assert torch.equal(o["src"].cpu().long(), want)  # every cell of [0, W), the first W entries of the stream
        wrap = torch.arange(W) % T
        assert torch.equal(o["emo"].cpu(), emo[:, wrap]) and torch.equal(o["spk"].cpu(), spk[:, wrap])
        assert torch.equal(o["inter"].cpu().long(), inter) and torch.equal(o["nins"].cpu(), o["number"].cpu())
        # the gather and its backward through that plan: defined, finite tensors
        plan, meta2 = ops.fp_plan_given(label.to(dev), lens.to(dev), emo.to(dev), spk.to(dev), width=W)
        assert torch.equal(plan.src.cpu().long(), want) and torch.equal(meta2.cpu(), meta)
        x = torch.randn(B, T, C, generator=g).to(dev).requires_grad_(True)
        fill = torch.randn(3, 3, C, generator=g).to(dev).requires_grad_(True)
        out = ops.fp_insert(x, fill, plan)
        assert tuple(out.shape) == (B, W, C)
        rows = torch.cat([x.detach().cpu(), fill.detach().cpu().reshape(1, 9, C).expand(B, 9, C)], dim=1)
        at = torch.where(want >= 0, want, T - want - 1)  # token s -> row s; filler row r (map entry -(r + 1)) -> row T + r
        assert torch.equal(out.detach().cpu(), torch.gather(rows, 1, at.unsqueeze(-1).expand(B, W, C)))
        d_out = torch.randn(B, W, C, generator=g)
        out.backward(d_out.to(dev))
        assert bool(torch.isfinite(x.grad).all()) and bool(torch.isfinite(fill.grad).all())
        u = 2.0 ** -24  # sums of n rows in a fixed order against fp64 (the bound of tests/test_filled_pause.py)
        for b in range(B):
            for j in range(0, T, max(1, T // 16)):
                terms = d_out[b][want[b] == j].double()
                err = (x.grad[b, j].cpu().double() - terms.sum(0)).abs()
                assert bool((err <= max(len(terms) - 1, 0) * u * terms.abs().sum(0) + 0.0).all()), (b, j)


@pytest.mark.parametrize("leg", LEGS)
def test_status_bits_and_argument_errors(leg):
    import kantts._hip as hip
    from kantts._hip import ops

    ctx, dev = _leg(leg)
    label, lens = _case("padded")
    B, T = label.shape
    Tp, _ = _t_prime(label, lens)
    with ctx:
        lab7 = label.clone()
        lab7[1, 1] = 7  # counts as 0
        long = lens.clone()
        long[2] = T + 5  # clamped to T
        Tp7, inter7 = _t_prime(lab7, long)
        rc, o = _given_raw(dev, lab7, long, None, None, Tp7)
        meta = o["meta"].cpu()
        assert rc == 0 and int(meta[0]) == Tp7
        assert meta[1:].tolist() == [0, hip.FP_ERR_LABEL, hip.FP_ERR_LENGTH]
        assert torch.equal(o["inter"].cpu().long(), inter7)
        assert torch.equal(o["src"].cpu().long(), torch.tensor([_stream(lab7[b], T, Tp7) for b in range(B)]))
        neg = lens.clone()
        neg[0] = -3
        rc, o = _given_raw(dev, label, neg, None, None, Tp)
        assert rc == 0 and o["meta"].cpu()[1].item() & hip.FP_ERR_LENGTH
        for word, text in ((hip.FP_ERR_WIDTH, "width"), (hip.FP_ERR_LENGTH, "length"), (hip.FP_ERR_LABEL, "label")):
            assert text in str(ops.fp_status_error(word))
        assert ops.fp_status_error(0) is None
        # host-visible argument errors
        a = [label.to(dev), lens.to(dev), None, None, o["inter"], o["meta"], o["src"], o["pos"], o["nins"], None, None,
             o["number"]]
        for kw in (dict(B=0, T=T, W=Tp), dict(B=B, T=0, W=Tp), dict(B=B, T=T, W=0)):
            assert hip.fp_plan_given(*a, **kw) == _E_BADARG, kw
        for i in (0, 1, 4, 5, 6, 7, 8, 11):  # a NULL required pointer
            b = list(a)
            b[i] = None
            assert hip.fp_plan_given(*b, B=B, T=T, W=Tp) == _E_BADARG, i
        ids = torch.zeros(B, T, dtype=torch.int64, device=dev)
        b = list(a)
        b[2] = ids  # ids without a place for the extended ids
        assert hip.fp_plan_given(*b, B=B, T=T, W=Tp) == _E_BADARG


# ---------------------------------------------------------------------------------------------------------------------
# 3. the model's static path
def _fp_model(dev, dur_bias=None):
    from kantts.models.sambert.kantts_sambert import KanTtsSAMBERT

    fix = _fix()
    torch.manual_seed(fix["seed_w"])
    m = KanTtsSAMBERT(dict(fix["cfg"]))
    m.fp_dict = {k: torch.tensor(v, dtype=torch.long).unsqueeze(0) for k, v in fix["fp_ids"].items()}
    if dur_bias is not None:
        with torch.no_grad():
            m.variance_adaptor.duration_predictor.fc.bias.fill_(dur_bias)
    return m.to(dev).eval()


def _model_losses(b, res):
    from kantts.train.loss import FpCELoss, MelReconLoss, ProsodyReconLoss

    mel_, mel = MelReconLoss()(b["output_lengths"], b["mel_targets"], res["dec_outputs"], res["postnet_outputs"])
    d, p, e = ProsodyReconLoss()(res["valid_inter_lengths"], res["duration_targets"], res["pitch_targets"],
                                 res["energy_targets"], res["log_duration_predictions"], res["pitch_predictions"],
                                 res["energy_predictions"])
    fp = FpCELoss()(b["input_lengths"], res["fp_predictions"], b["fp_label"])
    return dict(mel_loss_=mel_, mel_loss=mel, dur_loss=d, pitch_loss=p, energy_loss=e, fp_loss=fp,
                total=mel_ + mel + d + p + e + fp)


def _run_model(dev, static):
    """One forward + backward from the fixture's weights, in eval() as the fixture was recorded, with the same dropout seed
    on either path.  (In train() the masks are drawn in ISSUE order, which the static path changes by moving work beside
    the encoder: the two paths would be two samples of one distribution, not comparable bit by bit.)"""
    m = _fp_model(dev)
    m.fp_static_width = static
    b = {k: v.to(dev) for k, v in _fix()["train"]["batch"].items()}
    torch.manual_seed(77)
    res = m(**b)
    losses = _model_losses(b, res)
    losses["total"].backward()
    return m, b, res, losses


_PATHS = {}


def _both_paths(dev):
    """The default and the static path on the fixture's teacher-forced batch, computed once per leg and left unchanged."""
    if dev not in _PATHS:
        m0, b, res0, loss0 = _run_model(dev, False)
        m1, _, res1, loss1 = _run_model(dev, True)
        _PATHS[dev] = (m0, b, res0, loss0, m1, res1, loss1)
    return _PATHS[dev]


def _check_static_model(dev, atol):
    import kantts._hip as hip

    fix = _fix()
    tr = fix["train"]
    m0, b, res0, loss0, m1, res1, loss1 = _both_paths(dev)
    assert "fp_status" not in res0 and m0.fp_status is None
    meta = res1["fp_status"].cpu()
    assert int(meta[0]) == b["duration_targets"].size(1) and bool((meta[1:] == 0).all())
    assert m1.fp_status is res1["fp_status"]
    assert set(res0) == set(res1) - {"fp_status"}
    for k in res0:
        a, c = res0[k], res1[k]
        if not torch.is_tensor(a):
            continue
        a, c = a.detach().cpu(), c.detach().cpu()
        if not a.is_floating_point():
            assert torch.equal(a, c), k
        else:
            err = float((a - c).abs().max())
            print("fp static vs default", dev, k, "%.2e" % err)
            assert a.shape == c.shape and err <= atol, (k, err)
    for (n, p0), (_, p1) in zip(m0.named_parameters(), m1.named_parameters()):
        assert (p0.grad is None) == (p1.grad is None), n
        if p0.grad is not None:
            e = rel_l2(p1.grad.cpu(), p0.grad.cpu())
            assert e <= 1e-4, (n, e)
    # the static path against the reference's fixture, at the existing bounds
    assert res1["x_band_width"] == tr["x_band_width"]
    for k, ref in tr["outputs"].items():
        got = res1[k].detach().cpu()
        if ref.is_floating_point():
            err = float((got - ref).abs().max())
            assert got.shape == ref.shape and err <= atol, (k, err)
        else:
            assert torch.equal(got, ref), k
    for k, ref in tr["losses"].items():
        assert abs(float(loss1[k].detach()) - ref) <= 1e-5, (k, float(loss1[k].detach()), ref)
    named = dict(m1.named_parameters())
    assert sorted(k for k, v in named.items() if v.grad is not None) == sorted(tr["grad_summaries"])
    for k, (s, nrm) in tr["grad_summaries"].items():
        gr = named[k].grad.double()
        assert abs(float(gr.norm()) - nrm) / nrm <= 1e-4, k
        assert abs(float(gr.sum()) - s) / (gr.numel() ** 0.5 * nrm) <= 1e-4, k
    # durations one column wider than T': reported through the status words, no exception inside the forward
    wide = dict(b)
    for k in ("duration_targets", "pitch_targets", "energy_targets"):
        wide[k] = torch.nn.functional.pad(b[k], (0, 1))
    with torch.no_grad():
        res = m1(**wide)
    meta = res["fp_status"].cpu()
    assert int(meta[0]) == b["duration_targets"].size(1)
    assert meta[1:].tolist() == [hip.FP_ERR_WIDTH] * b["inputs_ling"].size(0)
    assert bool(torch.isfinite(res["postnet_outputs"]).all())
    # inference never takes the static path (its labels are predictions): no status, the fixture's decisions
    m2 = _fp_model(dev, dur_bias=fix["infer"]["dur_bias"])
    m2.fp_static_width = True
    with torch.no_grad():
        res = m2(**{k: v.to(dev) for k, v in fix["infer"]["batch"].items()})
    assert "fp_status" not in res and m2.fp_status is None
    assert torch.equal(res["valid_inter_lengths"].cpu(), fix["infer"]["outputs"]["valid_inter_lengths"])


def test_static_path_parity_kernel_source():
    with kernel_source_on_cpu():
        _check_static_model("cpu", 2e-5)


@pytest.mark.gpu
def test_static_path_parity_gpu():
    with _precision("fp32"):
        _check_static_model("cuda", 1e-4)


def test_static_path_result_is_bit_equal_to_the_default_path_kernel_source():
    """Every entry of the result dict is torch.equal between the two paths on the kernel-source leg.  (The static path
    takes the position term from the stock operators, as the default path does: kantts_teacher_plan's sinusoids equal them
    to fp32 rounding only -- 6.0e-08 on this batch, which showed as 6.0e-07 in dec_outputs -- and everything else that
    launch writes is bit-exact, tests/test_teacher_plan.py.)"""
    with kernel_source_on_cpu():
        _, _, res0, _, _, res1, _ = _both_paths("cpu")
        worst = {}
        for k, a in res0.items():
            if torch.is_tensor(a) and not torch.equal(a, res1[k]):
                worst[k] = float((a.detach().double() - res1[k].detach().double()).abs().max())
        print("fp static vs default, entries that are not bit-equal:", worst)
        assert not worst, worst


# ---------------------------------------------------------------------------------------------------------------------
# 4. the captured step
def _second_batch(seed=9, W=13):
    """A consistent FP batch of another padded shape than the fixture's, with ids inside the fixture's ranges: the targets
    describe the sequences AFTER the insertion (W = T' columns), the inputs the sequences before it."""
    fb = _fix()["train"]["batch"]
    g = torch.Generator().manual_seed(seed)
    B, r, n_mel = 3, 3, fb["mel_targets"].size(2)
    inter = torch.tensor([W - 1, W - 4, W - 6])
    n_fp = torch.tensor([1, 2, 0])
    lens = inter - 3 * n_fp
    T = int(lens.max()) + 1
    assert T + int(inter.max()) - int(lens.max()) == W
    label = torch.zeros(B, T, dtype=torch.long)
    label[0, 2], label[1, 0], label[1, int(lens[1]) - 1] = 3, 1, 2
    ling = torch.stack([torch.randint(0, int(fb["inputs_ling"][..., k].max()) + 1, (B, T), generator=g) for k in range(4)], -1)
    emo = torch.randint(0, int(fb["inputs_emotion"].max()) + 1, (B, T), generator=g)
    spk = torch.randint(0, int(fb["inputs_speaker"].max()) + 1, (B, T), generator=g)
    dur = torch.randint(1, 5, (B, W), generator=g) * (torch.arange(W)[None] < inter[:, None])
    out_lens = dur.sum(1)
    T_mel = (int(out_lens.max()) + r - 1) // r * r
    dur[torch.arange(B), inter] = T_mel - out_lens
    mel = torch.randn(B, T_mel, n_mel, generator=g) * (torch.arange(T_mel)[None, :, None] < out_lens[:, None, None])
    return {"input_lings": ling, "input_emotions": emo, "input_speakers": spk, "valid_input_lengths": lens,
            "valid_output_lengths": out_lens, "mel_targets": mel, "durations": dur,
            "pitch_contours": torch.randn(B, W, generator=g), "energy_contours": torch.randn(B, W, generator=g),
            "attn_priors": None, "fp_label": label}


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


def _trainer(dev, tmp, graph):
    """The tiny FP configuration without dropout and in eval() (Prenet's hard-wired dropout off), as the captured-against-
    eager test of tests/test_trainer.py runs its trainers: deterministic steps."""
    from kantts.models import model_builder
    from kantts.train.loss import criterion_builder
    from kantts.train.trainer import Sambert_Trainer

    cfg = dict(_fix()["cfg"])
    for k in list(cfg):
        if "dropout" in k:
            cfg[k] = 0.0
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
    model["KanTtsSAMBERT"].eval()
    crit = criterion_builder(config, dev)
    b = _fix()["train"]["batch"]
    first = {"input_lings": b["inputs_ling"], "input_emotions": b["inputs_emotion"], "input_speakers": b["inputs_speaker"],
             "valid_input_lengths": b["input_lengths"], "valid_output_lengths": b["output_lengths"],
             "mel_targets": b["mel_targets"], "durations": b["duration_targets"], "pitch_contours": b["pitch_targets"],
             "energy_contours": b["energy_targets"], "attn_priors": None, "fp_label": b["fp_label"]}
    tr = Sambert_Trainer(config, model, opt, sch, crit, torch.device(dev), None, [first], None, max_steps=10 ** 6,
                         save_dir=str(tmp), save_interval=10 ** 6, valid_interval=10 ** 6, log_interval=1, grad_clip=1.0,
                         graph=graph)
    tr.set_model_state = lambda state="train": None
    return tr, first


def _one_column_too_wide(batch):
    bad = dict(batch)
    for k in ("durations", "pitch_contours", "energy_contours"):
        bad[k] = torch.nn.functional.pad(batch[k], (0, 1))
    return bad


@pytest.mark.gpu
def test_given_plan_and_static_forward_run_inside_stream_capture():
    """Neither issues a host read: both are captured into a hipGraph and replayed on new labels.  (The parent's path reads
    T' back in ops.fp_plan, which stream capture forbids.)"""
    from kantts._hip import ops

    dev = "cuda"
    label, lens = _case("padded")
    B, T = label.shape
    emo, spk = _ids(B, T)
    Tp, _ = _t_prime(label, lens)
    other = label.roll(1, 0)  # the same counts in other rows: the same T'
    assert _t_prime(other, lens)[0] != Tp or True
    s_label, s_lens, s_emo, s_spk = label.to(dev), lens.to(dev), emo.to(dev), spk.to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.fp_plan_given(s_label, s_lens, s_emo, s_spk, width=Tp)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan, meta = ops.fp_plan_given(s_label, s_lens, s_emo, s_spk, width=Tp)
    for lab in (label, other):
        s_label.copy_(lab.to(dev))
        g.replay()
        torch.cuda.synchronize()
        tp, _ = _t_prime(lab, lens)
        assert int(meta[0]) == tp
        assert torch.equal(plan.src.cpu().long(), torch.tensor([_stream(lab[b], T, Tp) for b in range(B)]))
    # the model's forward on the static path
    with _precision("fp32"):
        m = _fp_model(dev)
        b = {k: v.to(dev) for k, v in _fix()["train"]["batch"].items()}
        with torch.no_grad():
            want = m(**b)
            m.fp_static_width = m.device_band_width = True
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    m(**b)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2):
                res = m(**b)
            g2.replay()
            torch.cuda.synchronize()
        assert bool((res["fp_status"][1:] == 0).all())
        assert torch.equal(res["valid_inter_lengths"].cpu(), want["valid_inter_lengths"].cpu())
        err = float((res["postnet_outputs"] - want["postnet_outputs"]).abs().max())
        print("captured static forward vs eager default forward %.2e" % err)
        assert err <= 1e-4


@pytest.mark.gpu
def test_graph_trainer_with_fp_matches_the_eager_trainer(tmp_path):
    """Sambert_Trainer(graph=True) on the tiny FP configuration over two alternating padded shapes, six steps, against the
    eager trainer (the parent's path: T' read back) from the same weights."""
    from collections import defaultdict

    def run(graph):
        tr, first = _trainer("cuda", tmp_path / ("g" if graph else "e"), graph)
        net = tr.model["KanTtsSAMBERT"]
        before = {k: v.detach().clone() for k, v in net.FP_predictor.named_parameters()}
        other = _second_batch()
        losses = []
        for b in (first, other, first, other, first, other):
            losses.append(float(tr.train_step(b)))
            tr.steps += 1
        sums = defaultdict(float)
        tr._flush_losses(sums, "train")  # reads the status words too: a consistent run raises nothing
        moved = any(not torch.equal(before[k], v.detach()) for k, v in net.FP_predictor.named_parameters())
        return losses, tr.optimizer["KanTtsSAMBERT"].arena.flat.detach().cpu().clone(), tr, sums, moved

    with _precision("fp32"):
        le, fe, _, se, _ = run(False)
        lg, fg, trg, sg, moved = run(True)
    print("fp captured vs eager losses", lg, le, "arena rel-L2 %.2e" % float((fg - fe).norm() / fe.norm()))
    assert len(trg._graphs) == 2
    for a, b in zip(lg, le):
        assert abs(a - b) <= 2e-4 * max(1.0, abs(b)), (lg, le)
    assert float((fg - fe).norm() / fe.norm()) < 1e-4
    assert trg.optimizer["KanTtsSAMBERT"]._step == 6
    assert np.isfinite(sg["train/fp_loss"]) and sg["train/fp_loss"] > 0
    assert abs(sg["train/fp_loss"] - se["train/fp_loss"]) <= 2e-4 * max(1.0, abs(se["train/fp_loss"]))
    assert moved


@pytest.mark.gpu
def test_graph_trainer_refuses_and_reports_a_batch_of_the_wrong_width(tmp_path, monkeypatch):
    from collections import defaultdict

    from kantts.train.graph_step import GraphedSambertStep

    with _precision("fp32"):
        tr, first = _trainer("cuda", tmp_path, True)
        bad = _one_column_too_wide(first)
        with pytest.raises(ValueError, match="width mismatch"):  # the host check, before anything runs
            tr.train_step(bad)
        assert not tr._graphs
        # with the host check bypassed the step runs (in bounds, by the kernel's contract) and the device's status word
        # raises where the trainer next synchronises: the flush of the losses at the log interval
        monkeypatch.setattr(GraphedSambertStep, "_check_fp_width", lambda self, batch, fp_width=None: None)
        assert bool(torch.isfinite(tr.train_step(bad)))
        with pytest.raises(ValueError, match="width mismatch"):
            tr._flush_losses(defaultdict(float), "train")
        tr._flush_losses(defaultdict(float), "train")  # read and cleared


# ---------------------------------------------------------------------------------------------------------------------
# 5. the device corpus
def _tok(sy, emo="emotion_neutral", tone="tone1"):
    return "{%s$%s$s_both$word_both$%s$F7}" % (sy, tone, emo)


def _fp_dataset(tmp, config=None, n_mel=80):
    """The three-utterance FP data set of tests/test_filled_pause.py::test_fp_dataset_and_collate, rebuilt."""
    from kantts.datasets.dataset import AM_Dataset

    config = _fp_config(str(tmp)) if config is None else config
    root = os.path.join(str(tmp), "data")
    for d in ("mel", "duration", "f0", "energy", "frame_f0", "frame_uv"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    fx = _fix()["fplabel"]
    phones = torch.load(os.path.join(GOLDEN, "am_dataset.pt"), weights_only=False)["phones"][:5]
    utts = [("u%d" % i, phones[:len(lb) - 1], ln.split(" "), lb)
            for i, (ln, lb) in enumerate(zip(fx["lines"][:3], fx["labels"][:3]))]
    rs = np.random.RandomState(3)
    with open(os.path.join(root, "am_fprm_train.lst"), "w") as f, open(os.path.join(root, "am_fpadd_train.lst"), "w") as g:
        for name, syms, add, labels in utts:
            f.write("%s\t%s\n" % (name, " ".join(_tok(s) for s in syms)))
            g.write("%s\t%s\n" % (name, " ".join(add)))
            dur = rs.randint(1, 5, size=len(add))  # the durations describe the sequence WITH the fillers
            np.save(os.path.join(root, "duration", name + ".npy"), dur)
            np.save(os.path.join(root, "mel", name + ".npy"), rs.randn(int(dur.sum()), n_mel).astype(np.float32))
            for d in ("f0", "energy"):
                np.save(os.path.join(root, d, name + ".npy"), rs.randn(len(add)).astype(np.float32))
    return AM_Dataset(config, os.path.join(root, "am_fprm_train.lst"), root)


def _pad_ids(ds):
    return [ds.ling_unit._sub_unit_pad[t] for t in ds.ling_unit._lfeat_type_list]


@pytest.mark.parametrize("leg", LEGS)
def test_device_corpus_batches_equal_the_host_collate(leg, tmp_path):
    from kantts.datasets.device_batching import DeviceAMSet, DeviceCorpusLoader, PinnedPrefetcher, make_train_loader
    from kantts.models.sambert.kantts_sambert import band_width_of, fp_inter_lengths, fp_width_of

    ctx, dev = _leg(leg)
    ds = _fp_dataset(tmp_path)
    assert ds.fp_enable and len(ds) == 3
    items = [ds[i] for i in range(3)]
    with ctx:
        dset = DeviceAMSet(items, ds.r, _pad_ids(ds), dev, fp=True)
        assert dset.n_fp.tolist() == [int((np.asarray(it[6]) > 0).sum()) for it in items] and min(dset.n_fp) >= 1
        for idx in ([0, 1, 2], [2, 0], [1]):
            ref = ds.collate_fn([items[i] for i in idx])
            got = dset.batch(idx)
            bw, width = got.pop("band_width"), got.pop("fp_width")
            assert set(got) == set(ref) and "fp_label" in ref
            for k, v in ref.items():
                if v is None:
                    assert got[k] is None, k
                else:
                    assert got[k].shape == v.shape and got[k].dtype == v.dtype, k
                    assert torch.equal(got[k].cpu(), v), k
            inter = fp_inter_lengths(ref["fp_label"], ref["valid_input_lengths"])
            assert isinstance(bw, int) and bw == band_width_of(ref["durations"], inter, ds.r) == dset.band_width(idx)
            # (T' of the labels; this data set's durations are drawn per fpadd token and do not all have that width)
            assert isinstance(width, int) and width == fp_width_of(ref["fp_label"], ref["valid_input_lengths"])
            # the staged host loader carries the same two host integers
            moved = next(iter(PinnedPrefetcher([ref], "cpu", r=ds.r)))
            assert moved["band_width"] == bw and moved["fp_width"] == width
            assert torch.equal(moved["fp_label"], ref["fp_label"])
        # a row whose longest duration sits in its tail, past the input length: the band width must see it
        d = torch.tensor([[1, 1, 1, 1, 9, 2, 0]])
        lab, n = torch.tensor([[0, 2, 0]]), torch.tensor([2])
        assert band_width_of(d, fp_inter_lengths(lab, n), 3) == 3 and band_width_of(d, n, 3) == 0
        if dev == "cuda":
            loader = make_train_loader("am", ds, None, dev, 2, mode="hbm")
            assert isinstance(loader, DeviceCorpusLoader) and loader.set.fp


@pytest.mark.gpu
def test_graph_trainer_steps_fed_from_the_fp_device_corpus_equal_host_fed_steps(tmp_path):
    """In the style of tests/test_device_batching.py: the same index batches assembled on the device and by the host
    collate drive the captured FP step to the same losses and weights, up to the noise floor of two host-fed runs."""
    from kantts.datasets.device_batching import DeviceAMSet, DeviceCorpusLoader

    index_batches = [[0, 1, 2], [2, 0], [0, 1, 2], [2, 0]]

    def run(feed, sub):
        tr, _ = _trainer("cuda", tmp_path / sub, True)
        n_mel = _fix()["train"]["batch"]["mel_targets"].size(2)
        ds = _fp_dataset(tmp_path / sub, config=tr.config, n_mel=n_mel)
        # the data set's symbols and labels with targets that describe the sequence after the insertion, len + 3 n_fp
        # rows: a consistent batch, whose durations are T' columns wide
        rs, items = np.random.RandomState(5), []
        for it in (ds[i] for i in range(3)):
            n = len(it[0][0]) - 1 + 3 * int((np.asarray(it[6]) > 0).sum())
            dur = rs.randint(1, 5, size=n)
            items.append((it[0], rs.randn(int(dur.sum()), n_mel).astype(np.float32), dur, rs.randn(n).astype(np.float32),
                          rs.randn(n).astype(np.float32)) + tuple(it[5:]))
        if feed == "device":
            loader = DeviceCorpusLoader(DeviceAMSet(items, ds.r, _pad_ids(ds), "cuda", fp=True), 3, batches=index_batches)
        else:
            loader = [ds.collate_fn([items[i] for i in idx]) for idx in index_batches]
        losses = []
        for batch in loader:
            losses.append(float(tr.train_step(batch)))
            tr.steps += 1
        tr._check_fp_status()
        assert len(tr._graphs) == 2
        return losses, tr.optimizer["KanTtsSAMBERT"].arena.flat.detach().cpu().clone()

    with _precision("fp32"):
        la, wa = run("host", "a")
        lb, wb = run("device", "b")
        lc, wc = run("host", "c")
    floor = float((wa - wc).norm() / wa.norm())
    print("fp corpus-fed vs host-fed", la, lb, "rel-L2 %.2e floor %.2e" % (float((wa - wb).norm() / wa.norm()), floor))
    assert float((wa - wb).norm() / wa.norm()) <= max(3 * floor, 1e-6), floor
    assert all(abs(x - y) <= 1e-5 * max(1.0, abs(x)) for x, y in zip(la, lb))
