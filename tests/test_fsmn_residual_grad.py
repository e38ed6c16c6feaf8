"""One FSMN layer (FFN -> memory block -> dropout (+ x)): the layer input x has two readers, the FFN's first contraction and
the residual add.  In bf16 mode the add's gradient is handed to the ``res`` port of that contraction's input-gradient launch
(ops_bf16.ResGradToken) instead of being summed by an elementwise launch of autograd's; fp32 mode leaves autograd's sum.

Both forms compute fp32(dz W) + d_res with one fp32 add (the epilogue adds the residual to the rounded-to-fp32 result of
the contraction, alpha = 1), so input and parameter gradients are compared bit for bit.  Measured pair (folded, parent), kernel
source on the CPU and MI355X, B = 2, T = 50, K = 41, dropout 0.1: maximum difference 0.0 in every gradient at widths 256
and 80 in bf16 mode, where the hand-over runs, and in fp32 mode once the weight gradients' atomic K slices are one (see
_run: with the library's slice count two runs of the SAME fp32 path differ by one ulp on the device)."""
import itertools
import os

import pytest
import torch

import torch_oracle as O
from util import kernel_source_on_cpu

HOSTSIM = os.path.exists(os.environ.get("HIPEMU_CXX", "/opt/rocm/lib/llvm/bin/clang++"))
B, T, D, K = 2, 50, 256, 41


def _run(device, width, precision, fold):
    import kantts._hip as hip
    import kantts._hip.ops as ops
    import kantts.models.sambert.fsmn as fsmn
    from kantts.models.utils import SeqInfo

    cfg = O.sambert_config()
    made = []

    def token():
        made.append(real())
        return made[-1]

    torch.manual_seed(11)
    enc = fsmn.FsmnEncoderV2(K, 1, width, D, cfg["postnet_ffn_inner_dim"], dropout=0.1, shift=0).to(device).train()
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(B, T, width, generator=g).to(device)
    cot = torch.randn(B, T, D, generator=g).to(device)
    info = SeqInfo(torch.tensor([T, 37], device=device), T)
    before, real, real_sk = hip.get_precision(), fsmn.ResGradToken, ops._splitk_for
    # fp32 mode sums a weight gradient's K slices with float atomics, in an order that changes from run to run on the device
    # (two runs of the SAME path differed by one ulp, 9.5e-7 at 19, in ffn_lst.0.w_1.weight); with one slice the order is
    # fixed, and the comparison below can ask for equal bits in both modes
    ops._splitk_for = lambda *a: 1
    fsmn.ResGradToken = token if fold else (lambda: None)  # parent path: no hand-over, autograd sums the two gradients
    hip.set_precision(precision)
    try:
        ops._seed_counter = itertools.count(1000)
        hip.rng_state("cpu" if device == "cpu" else device).zero_()
        x = x0.clone().requires_grad_(True)
        y = enc(x, info)
        (y * cot).sum().backward()
    finally:
        hip.set_precision(before)
        fsmn.ResGradToken = real
        ops._splitk_for = real_sk
    grads = {"x": x.grad.detach().cpu()}
    grads.update({n: p.grad.detach().cpu() for n, p in enc.named_parameters()})
    return y.detach().cpu(), grads, made


def _case(device, width, precision):
    y0, g0, _ = _run(device, width, precision, fold=False)
    y1, g1, made = _run(device, width, precision, fold=True)
    assert torch.equal(y0, y1)
    assert sorted(g0) == sorted(g1) and "ffn_lst.0.w_1.weight" in g0 and "memory_block_lst.0.conv_dw.weight" in g0
    for n in g0:
        diff = float((g0[n] - g1[n]).abs().max())
        print("%s width %d %s: max |folded - parent| = %g (max |parent| %g)" % (precision, width, n, diff,
                                                                               float(g0[n].abs().max())))
        assert torch.equal(g0[n], g1[n]), n
    assert float(g0["x"].abs().max()) > 0
    # the hand-over ran exactly where it can: the residual layer (width == D) on the bf16 kernels, and was consumed
    want = precision == "bf16" and width == D
    assert [t.armed for t in made] == ([want] if width == D else [])
    assert all(t.dres is None for t in made)


CASES = [(D, "bf16"), (D, "fp32"), (80, "bf16"), (80, "fp32")]  # 80 = the postnet's first layer (num_mels): no residual


@pytest.mark.skipif(not HOSTSIM, reason="the host build of the kernel sources needs the ROCm clang")
@pytest.mark.parametrize("width,precision", CASES)
def test_fsmn_layer_gradients_with_the_residual_add_folded_kernel_source(width, precision):
    with kernel_source_on_cpu():
        _case("cpu", width, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("width,precision", CASES)
def test_fsmn_layer_gradients_with_the_residual_add_folded_gpu(width, precision):
    _case("cuda", width, precision)
