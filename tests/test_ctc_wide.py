"""kantts_ctc_attn_wide (csrc/ctc.hip): the alignment CTC for up to 1023 tokens -- the widths of byte-input voices --
against the reference's formulation executed with stock PyTorch (kantts/train/loss.py:481-508 of the reference, restated
below as in tests/test_ctc.py), in float64 (the exact answer) and in float32 (what the reference itself computes).

Legs as in tests/test_device_corpus_mas_se.py: ``kernel_source`` (the kernel sources on the CPU) and, marked ``gpu``, the
device.  Tolerances are those of tests/test_ctc.py: loss 2e-5 relative; gradient max(1e-4 of its largest entry, four times
the error ATen's own float32 path makes against float64 on the same input); exactly zero past each item's T and S.

The guard test lays ``grad`` and the workspace into flat sentinel buffers with a guard item in front of and behind them:
no cell outside may change."""
import contextlib
import ctypes

import pytest
import torch
import torch.nn.functional as F

from util import kernel_source_on_cpu

LEGS = [pytest.param("hostsim", id="kernel_source"), pytest.param("cuda", id="gpu", marks=pytest.mark.gpu)]
_SENTINEL = -777.0
_E_BADARG = -1
_REF = {}


def _leg(leg):
    return (kernel_source_on_cpu(), "cpu") if leg == "hostsim" else (contextlib.nullcontext(), "cuda")


def reference_attention_ctc(attn_logprob, in_lens, out_lens, blank_logprob=-1):
    """kantts/train/loss.py:488-508 (the reference's loop, verbatim semantics, stock torch ops on the CPU)."""
    ctc = torch.nn.CTCLoss(zero_infinity=True)
    padded = F.pad(attn_logprob, pad=(1, 0, 0, 0, 0, 0, 0, 0), value=blank_logprob)
    total = 0.0
    for bid in range(attn_logprob.shape[0]):
        target = torch.arange(1, int(in_lens[bid]) + 1).unsqueeze(0)
        cur = padded[bid].permute(1, 0, 2)[: int(out_lens[bid]), :, : int(in_lens[bid]) + 1]
        cur = torch.log_softmax(cur[None], dim=3)[0]
        total = total + ctc(cur, target, input_lengths=out_lens[bid:bid + 1], target_lengths=in_lens[bid:bid + 1])
    return total / attn_logprob.shape[0]


def _ragged(B, T1, T2, seed=3):
    """Seeded ragged lengths of a full byte batch; item 0 fills the batch."""
    g = torch.Generator().manual_seed(seed)
    il = torch.randint(T2 // 3, T2 + 1, (B,), generator=g).tolist()
    ol = [min(T1, s + int(torch.randint(0, T1 - T2, (1,), generator=g))) for s in il]
    il[0], ol[0] = T2, T1
    return il, ol


def _reference(B, T1, T2, in_lens, out_lens, seed=0, scale=2.0):
    """The seeded input of a case with the reference's loss and gradients (float64, and ATen's float32 error against it):
    computed once per case of this file, shared by the legs and never written to."""
    key = (B, T1, T2, tuple(in_lens), tuple(out_lens), seed)
    if key not in _REF:
        g = torch.Generator().manual_seed(seed)
        x = scale * torch.randn(B, 1, T1, T2, generator=g)
        il, ol = torch.tensor(in_lens), torch.tensor(out_lens)
        xr = x.double().requires_grad_(True)
        ref = reference_attention_ctc(xr, il, ol)
        ref.backward()
        x32 = x.clone().requires_grad_(True)
        reference_attention_ctc(x32, il, ol).backward()
        err_aten = float((x32.grad.double() - xr.grad).abs().max())
        _REF[key] = (x, il, ol, float(ref.detach()), xr.grad, err_aten)
    return _REF[key]


def _assert_case(got_loss, gd, ref, what=""):
    """got_loss: the batch mean; gd (B, 1, T1, T2): d mean / d logits on the host."""
    x, il, ol, ref_loss, ref_grad, err_aten = ref
    T1, T2 = x.shape[2:]
    gmax = float(ref_grad.abs().max())
    err = float((gd.double() - ref_grad).abs().max())
    bound = max(1e-4 * max(gmax, 1e-6), 4.0 * err_aten)
    print("%s loss %.6f ref %.6f; gradient err %.3e bound %.3e (gmax %.3e, ATen fp32 err %.3e)" % (
        what, got_loss, ref_loss, err, bound, gmax, err_aten))
    assert abs(got_loss - ref_loss) <= 2e-5 * max(1.0, abs(ref_loss)), (got_loss, ref_loss)
    assert err <= bound, (err, gmax, err_aten)
    for b in range(x.shape[0]):  # frames past the utterance / classes past its tokens receive no gradient
        assert float(gd[b, 0, int(ol[b]):].abs().max() if int(ol[b]) < T1 else 0.0) == 0.0
        assert float(gd[b, 0, :, int(il[b]):].abs().max() if int(il[b]) < T2 else 0.0) == 0.0


def _check_loss_module(dev, case):
    """Through AttentionCTCLoss (unchanged signature): hip.ctc_attn sends these widths to the wide entry."""
    from kantts.train.loss import AttentionCTCLoss

    ref = _reference(*case)
    x, il, ol = ref[:3]
    xd = x.to(dev).requires_grad_(True)
    got = AttentionCTCLoss()(xd, il.to(dev), ol.to(dev))
    (2.5 * got).backward()
    _assert_case(float(got.detach()), xd.grad.cpu() / 2.5, ref, str(case[:3]))


CASES = [(1, 520, 512, [512], [520]),               # 1025 states: the first count the narrow form refuses
         (2, 530, 513, [513, 3], [530, 9]),         # a short item beside a wide one
         (2, 40, 600, [600, 20], [40, 40])]         # T < S: loss 0, gradient 0 for item 0; item 1 is live
GPU_CASES = [(2, 830, 800, [800, 799], [830, 800]),  # T == S for item 1
             (1, 1030, 1023, [1023], [1030]),        # the widest accepted form
             (8, 1500, 800) + _ragged(8, 1500, 800),  # the full byte batch
             (1, 4200, 512, [512], [4200])]          # more than 16 KB of row normalisers: the launcher raises the LDS limit


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%d" % c[:3])
def test_wide_ctc_equals_the_reference_loop(case, leg):
    import kantts._hip as hip

    ctx, dev = _leg(leg)
    with ctx:
        assert hip.has_ctc_wide()
        _check_loss_module(dev, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_CASES, ids=lambda c: "%dx%dx%d" % c[:3])
def test_wide_ctc_equals_the_reference_loop_at_byte_widths_gpu(case):
    _check_loss_module("cuda", case)


def _raw(dev, entry, x, il, ol, guard=True):
    """One call of ``entry`` with ``grad`` and the workspace inside sentinel buffers (a guard item on either side).
    Returns (code, loss (B,), grad (B, 1, T1, T2)) on the host after checking the guards."""
    import kantts._hip as hip

    B, _, T1, T2 = x.shape
    n_ws = int(hip.lib().kantts_ctc_attn_workspace(B, T1, T2))
    assert n_ws == B * 2 * T1 * (2 * T2 + 1)
    per_g, per_w = T1 * T2, n_ws // B
    gbuf = torch.full(((B + 2) * per_g,), _SENTINEL, device=dev)
    wbuf = torch.full(((B + 2) * per_w,), _SENTINEL, device=dev)
    lbuf = torch.full((B + 2,), _SENTINEL, device=dev)
    xd = x.to(dev).contiguous()
    i32 = lambda v: v.to(torch.int32).to(dev)  # noqa: E731
    ild, old = i32(il), i32(ol)
    g = hip.CtcArgs()
    g.logits, g.in_lens, g.out_lens = hip.ptr(xd, torch.float32), hip.ptr(ild, torch.int32), hip.ptr(old, torch.int32)
    g.ws, g.loss, g.grad = hip.ptr(wbuf[per_w:]), hip.ptr(lbuf[1:]), hip.ptr(gbuf[per_g:])
    g.B, g.T1, g.T2, g.blank, g.grad_scale = B, T1, T2, -1.0, 1.0 / B
    rc = getattr(hip.lib(), entry)(ctypes.byref(g), hip.stream())
    gh, wh, lh = gbuf.cpu(), wbuf.cpu(), lbuf.cpu()
    for name, h, per in (("grad", gh, per_g), ("workspace", wh, per_w), ("loss", lh, 1)):
        assert bool((h[:per] == _SENTINEL).all()), "cells in front of %s were written" % name
        assert bool((h[(B + 1) * per:] == _SENTINEL).all()), "cells behind %s were written" % name
    return rc, lh[1:B + 1], gh[per_g:(B + 1) * per_g].view(B, 1, T1, T2)


@pytest.mark.parametrize("leg", LEGS)
def test_wide_entry_stays_inside_grad_and_workspace(leg):
    """The widest row the kernel-source leg runs, ragged, and the narrow shape of tests/test_ctc.py through the wide entry."""
    ctx, dev = _leg(leg)
    with ctx:
        for case in (CASES[1], (3, 20, 6, [6, 3, 1], [20, 11, 5])):
            ref = _reference(*case)
            x, il, ol = ref[:3]
            rc, loss, grad = _raw(dev, "kantts_ctc_attn_wide", x, il, ol)
            assert rc == 0
            assert bool((grad != _SENTINEL).all())  # every cell of grad is written: zeros outside the live region
            _assert_case(float(loss.mean()), grad, ref, "raw %s" % (case[:3],))


@pytest.mark.parametrize("leg", LEGS)
def test_wide_entry_limits(leg):
    import kantts._hip as hip

    ctx, dev = _leg(leg)
    with ctx:
        L = hip.lib()
        z = torch.zeros(8, device=dev)
        zi = torch.zeros(2, dtype=torch.int32, device=dev)

        def args(B, T1, T2, **null):
            g = hip.CtcArgs()
            for name in ("logits", "ws", "loss", "grad"):
                setattr(g, name, None if name in null else hip.ptr(z))
            for name in ("in_lens", "out_lens"):
                setattr(g, name, None if name in null else hip.ptr(zi))
            g.B, g.T1, g.T2, g.blank, g.grad_scale = B, T1, T2, -1.0, 1.0
            return ctypes.byref(g)

        assert L.kantts_ctc_attn_wide(args(1, 4, 1024), hip.stream()) == hip.E_UNSUPPORTED  # 2049 states
        assert L.kantts_ctc_attn_wide(args(1, 24577, 4), hip.stream()) == hip.E_UNSUPPORTED  # the T1 rule of the narrow entry
        assert L.kantts_ctc_attn_wide(args(0, 4, 1024), hip.stream()) == 0
        assert L.kantts_ctc_attn_wide(None, hip.stream()) == _E_BADARG
        assert L.kantts_ctc_attn_wide(args(-1, 4, 4), hip.stream()) == _E_BADARG
        for name in ("logits", "in_lens", "out_lens", "ws", "loss", "grad"):
            assert L.kantts_ctc_attn_wide(args(1, 2, 4, **{name: True}), hip.stream()) == _E_BADARG, name
        assert L.kantts_ctc_attn(args(1, 4, 512), hip.stream()) == hip.E_UNSUPPORTED  # the narrow entry is what it was
        assert L.kantts_ctc_attn_workspace(8, 1500, 800) == 8 * 2 * 1500 * 1601
        if dev == "cuda":
            torch.cuda.synchronize()
        assert bool((z == 0).all())


def test_dispatch_by_width_names_the_missing_entry_point(monkeypatch):
    """hip.ctc_attn: up to 511 tokens the unchanged entry, wider the wide one; a library (or the emulated ABI) without the
    wide entry is told apart from a kernel failure: the error names the width and the entry point."""
    import kantts._hip as hip

    with kernel_source_on_cpu() as real:
        calls = []

        class Lib:  # the loaded library object with the two launches recorded
            def __getattr__(self, name):
                fn = getattr(real, name)
                if name in ("kantts_ctc_attn", "kantts_ctc_attn_wide"):
                    return lambda *a: (calls.append(name), fn(*a))[1]
                return fn

        monkeypatch.setattr(hip, "lib", lambda: Lib())
        il, ol = torch.tensor([5], dtype=torch.int32), torch.tensor([9], dtype=torch.int32)
        hip.ctc_attn(torch.zeros(1, 9, 511), il, ol, -1.0, 1.0)
        hip.ctc_attn(torch.zeros(1, 9, 512), il, ol, -1.0, 1.0)
        assert calls == ["kantts_ctc_attn", "kantts_ctc_attn_wide"]
        with pytest.raises(RuntimeError, match="1024 tokens"):
            hip.ctc_attn(torch.zeros(1, 9, 1024), il, ol, -1.0, 1.0)

        class Old:  # the same library with the wide symbol removed
            def __getattr__(self, name):
                if name == "kantts_ctc_attn_wide":
                    raise AttributeError(name)
                return getattr(real, name)

        monkeypatch.setattr(hip, "lib", lambda: Old())
        assert not hip.has_ctc_wide()
        with pytest.raises(RuntimeError, match=r"600 tokens.*kantts_ctc_attn_wide"):
            hip.ctc_attn(torch.zeros(1, 9, 600), il, ol, -1.0, 1.0)
        loss, grad = hip.ctc_attn(torch.zeros(1, 9, 6), il, ol, -1.0, 1.0)  # narrow widths are served as before
        assert loss.shape == (1,) and grad.shape == (1, 9, 6)
        monkeypatch.undo()  # before the kernel-source routing is taken down: it restores what it found


def test_emulated_abi_without_the_wide_entry_says_so(emulated_cabi):
    import kantts._hip as hip

    assert not hasattr(emulated_cabi, "kantts_ctc_attn_wide") and not hip.has_ctc_wide()
    il, ol = torch.tensor([5], dtype=torch.int32), torch.tensor([9], dtype=torch.int32)
    with pytest.raises(RuntimeError, match=r"600 tokens.*kantts_ctc_attn_wide"):
        hip.ctc_attn(torch.zeros(1, 9, 600), il, ol, -1.0, 1.0)
