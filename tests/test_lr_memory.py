"""The regulated hand-over to the decoder as one launch each way (csrc/seq.hip: kantts_lr_memory_fwd / _bwd, ops.lr_memory)
against the composition it replaces (three ops.lr_gather, + pos_enc, the LFR reshape, torch.cat; reference
kantts_sambert.py:455-500, :995-1003): memory, the frame-level tensors and all three input gradients bit for bit, under a
random d_memory.  Run on the kernel SOURCE on the CPU (tests/hipemu) and on the device."""
import contextlib
import os

import pytest
import torch
import torch.nn.functional as F

import torch_oracle as O
from util import _Patch, kernel_source_on_cpu

HOSTSIM = os.path.exists(os.environ.get("HIPEMU_CXX", "/opt/rocm/lib/llvm/bin/clang++"))
B, N, R, TP = 3, 5, 3, 12
# sequence 0: a zero duration, 10 regulated frames: shorter than Tp and no multiple of r (frames 10, 11 are uncovered, the
#             group 9..11 straddles the end)
# sequence 1: 13 regulated frames (the last token runs past Tp), valid length 11: the mask cuts inside a token and a group
# sequence 2: valid length 0
DURS = [[2, 0, 3, 1, 4], [3, 3, 3, 2, 2], [1, 2, 0, 1, 1]]
VALID = [10, 11, 0]


class _CountingLib:
    """The loaded library with a count of the calls per entry point."""

    def __init__(self, real):
        self._real, self.calls, self.rcs = real, {}, {}

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def counted(*a):
            rc = fn(*a)
            self.calls[name] = self.calls.get(name, 0) + 1
            self.rcs.setdefault(name, []).append(rc)
            return rc

        return counted


@contextlib.contextmanager
def _counting():
    import kantts._hip as hip
    import kantts._hip.ops as ops
    import kantts._hip.ops_bf16 as ops_bf16

    lib = _CountingLib(ops.lib())
    p = _Patch()
    try:
        for mod in (hip, ops, ops_bf16):
            p.setattr(mod, "lib", lambda: lib)
        yield lib
    finally:
        p.undo()


def _composition(ops, aug, spk, emo, idx, cs, valid, pos_enc, r):
    text = ops.lr_gather(aug, idx, cs, valid) + pos_enc
    fs = ops.lr_gather(spk, idx, cs, valid)
    fe = ops.lr_gather(emo, idx, cs, valid)
    b, ds, de = aug.shape[0], spk.shape[-1], emo.shape[-1]
    mem = torch.cat([text.reshape(b, -1, r * text.shape[-1]), fs.reshape(b, -1, r * ds)[:, :, :ds],
                     fe.reshape(b, -1, r * de)[:, :, :de]], dim=-1)
    return mem, text, fs, fe


def _case(device, dt, ds, de, declined=False, padded=False, use_valid=True):
    with _counting() as lib:
        _case_body(lib, device, dt, ds, de, declined, padded, use_valid)


def _case_body(lib, device, dt, ds, de, declined, padded, use_valid):
    from kantts._hip import E_UNSUPPORTED, ops

    g = torch.Generator().manual_seed(7 + dt)
    durs = torch.tensor(DURS, dtype=torch.int64, device=device)
    valid = torch.tensor(VALID, dtype=torch.int64, device=device) if use_valid else None
    idx, _, cs, _ = ops.lr_index(durs, TP)
    pos_enc = torch.randn(B, TP, dt, generator=g)
    pos_enc[:, -2:, : dt // 2] = -0.0  # 0 + (-0) = +0 in the masked frames, in both forms
    pos_enc = pos_enc.to(device)
    leaves = [torch.randn(B, N, c, generator=g).to(device).requires_grad_(True) for c in (dt, ds, de)]
    cot = torch.randn(B, TP // R, R * dt + ds + de + (4 if padded else 0), generator=g).to(device)

    def grads(mem):
        # ``padded``: the gradient arrives as the leading columns of a wider buffer (row pitch D + 4), read where it lies
        out = F.pad(mem, (0, 4)) if padded else mem
        return torch.autograd.grad((out * cot).sum(), leaves)

    ref = _composition(ops, *leaves, idx, cs, valid, pos_enc, R)
    ref_g = grads(ref[0])
    before = dict(lib.calls)
    got = ops.lr_memory(*leaves, idx, cs, valid, pos_enc, R)
    got_g = grads(got[0])
    new = {k: v - before.get(k, 0) for k, v in lib.calls.items() if v != before.get(k, 0)}
    if declined:  # the entry is asked, declines, and the composition runs
        assert lib.rcs["kantts_lr_memory_fwd"] == [E_UNSUPPORTED]
        assert new == {"kantts_lr_memory_fwd": 1, "kantts_lr_gather_fwd": 3, "kantts_lr_gather_bwd": 3}
    else:
        assert new == {"kantts_lr_memory_fwd": 1, "kantts_lr_memory_bwd": 1}
    assert got[0].shape == (B, TP // R, R * dt + ds + de)
    for name, a, b in zip(("memory", "LR_text", "LR_spk", "LR_emo", "d_aug", "d_spk", "d_emo"), got + got_g, ref + ref_g):
        assert a.shape == b.shape and torch.equal(a, b), name
    # what the test set out to cover is there: uncovered frames, a mask inside a group, an empty sequence
    assert int(idx[0, 10]) == -1 and int(cs[1, -1]) > TP and VALID[1] % R and VALID[2] == 0
    if use_valid:
        assert float(ref_g[0][2].abs().max()) == 0.0 and float(ref_g[0][1, -1].abs().max()) == 0.0


def _all(device):
    cfg = O.sambert_config()
    dt, ds, de = cfg["encoder_projection_units"], cfg["speaker_units"], cfg["emotion_units"]
    _case(device, dt, ds, de)
    _case(device, dt, ds, de, padded=True)
    _case(device, dt, ds, de, use_valid=False)
    _case(device, 4, 4, 4)                    # the smallest widths the launch accepts
    _case(device, 4, 8, 12, padded=True)      # three different widths
    _case(device, 6, 4, 4, declined=True)     # a width that is no multiple of 4: the composition runs


@pytest.mark.skipif(not HOSTSIM, reason="the host build of the kernel sources needs the ROCm clang")
def test_frame_level_gradients_are_added_by_the_regulator_backward():
    """Gradients that arrive through LR_text / LR_spk / LR_emo (no training step has any) reach the inputs too."""
    with kernel_source_on_cpu():
        from kantts._hip import ops

        g = torch.Generator().manual_seed(3)
        durs = torch.tensor(DURS, dtype=torch.int64)
        valid = torch.tensor(VALID, dtype=torch.int64)
        idx, _, cs, _ = ops.lr_index(durs, TP)
        pos_enc = torch.randn(B, TP, 8, generator=g)
        leaves = [torch.randn(B, N, 8, generator=g).requires_grad_(True) for _ in range(3)]
        cots = [torch.randn(s, generator=g) for s in ((B, TP // R, 40), (B, TP, 8), (B, TP, 8), (B, TP, 8))]
        res = []
        for fn in (ops.lr_memory, lambda *a: _composition(ops, *a)):
            outs = fn(*leaves, idx, cs, valid, pos_enc, R)
            res.append(torch.autograd.grad(sum((o * c).sum() for o, c in zip(outs, cots)), leaves))
        for a, b in zip(*res):
            torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-6)  # (two partial sums added in another order)


@pytest.mark.skipif(not HOSTSIM, reason="the host build of the kernel sources needs the ROCm clang")
def test_lr_memory_equals_the_composition_kernel_source():
    with kernel_source_on_cpu():
        _all("cpu")


@pytest.mark.gpu
def test_lr_memory_equals_the_composition_gpu():
    _all("cuda")


def _training_step_launches(device):
    """One tiny teacher-forced training step: the decoder's memory is formed by exactly one launch, its gradient taken back
    by exactly one, the regulator's own launches and torch.cat do not run at that site."""
    from torch.utils._python_dispatch import TorchDispatchMode

    from kantts.models.sambert.kantts_sambert import KanTtsSAMBERT
    from kantts.train.loss import MelReconLoss, ProsodyReconLoss

    cats = []

    class Watch(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if func.overloadpacket is torch.ops.aten.cat:
                width = sum(int(t.shape[-1]) for t in args[0])
                cats.append(width)
            return func(*args, **(kwargs or {}))

    cfg = O.sambert_config(tiny=True)
    torch.manual_seed(0)
    m = KanTtsSAMBERT(dict(cfg)).to(device).train()
    batch = {k: v.to(device) for k, v in O.synthetic_sambert_batch(B=3, T_in=12, min_len=6, dur_hi=6).items()}
    with _counting() as lib, Watch():
        res = m(**batch)
        mel_, mel = MelReconLoss()(batch["output_lengths"], batch["mel_targets"], res["dec_outputs"], res["postnet_outputs"])
        d, p, e = ProsodyReconLoss()(batch["input_lengths"], res["duration_targets"], res["pitch_targets"],
                                     res["energy_targets"], res["log_duration_predictions"], res["pitch_predictions"],
                                     res["energy_predictions"])
        (mel_ + mel + d + p + e).backward()
    r = m.mel_decoder.r
    d_mem = r * cfg["encoder_projection_units"] + cfg["speaker_units"] + cfg["emotion_units"]
    assert res["LR_text_outputs"].shape[1] == batch["mel_targets"].shape[1]
    assert lib.calls.get("kantts_lr_memory_fwd") == 1 and lib.calls.get("kantts_lr_memory_bwd") == 1
    assert "kantts_lr_gather_fwd" not in lib.calls and "kantts_lr_gather_bwd" not in lib.calls
    assert d_mem not in cats, cats  # no concatenation forms the decoder's memory
    assert m.text_encoder.ling_proj.weight.grad is not None and m.emo_tokenizer.weight.grad is not None


@pytest.mark.skipif(not HOSTSIM, reason="the host build of the kernel sources needs the ROCm clang")
def test_training_step_forms_the_memory_in_one_launch_each_way_kernel_source():
    with kernel_source_on_cpu():
        _training_step_launches("cpu")


@pytest.mark.gpu
def test_training_step_forms_the_memory_in_one_launch_each_way_gpu():
    _training_step_launches("cuda")
