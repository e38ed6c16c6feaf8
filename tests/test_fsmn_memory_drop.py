"""The FSMN memory block of a training step as one launch each way (csrc/fsmn_drop.hip: kantts_fsmn_memory_drop_fwd / _bwd,
ops.fsmn_memory_drop) against the pair of launches it replaces: kantts_fsmn_dwconv_fwd + kantts_dropout2_add forward,
kantts_dropout2_add + kantts_fsmn_dwconv_bwd backward.

Equal bits are asked for everywhere.  The fused kernels keep the pair's arithmetic per output -- acc = centre, fmaf(w[k],
x[o + k], acc) for k = 0..40 (flipped taps backward), the length mask, * keep1, * keep2, + res -- and the last three stay
three roundings on the device as well: dropout2_add_kernel compiles to v_pk_mul / v_pk_mul / v_pk_add (its multiplies and its
add sit in different basic blocks), and the new epilogue adds the residual with contraction switched off, which gives the
same three instructions.

One difference is part of the contract and not of the arithmetic: the masked gradient dym is written as ZERO in the rows at
or after lens[b], where the pair's dropout2_add writes keep1 * keep2 * dy.  The filter gradient never reads those rows (and
dx is zero there in both forms), so the comparison takes the pair's masked dy with those rows zeroed; the filter gradients
computed from the two are compared as they are.

Every case runs the kernel sources on the CPU (tests/hipemu) and on the device."""
import contextlib
import itertools
import os

import pytest
import torch

import torch_oracle as O
from util import _Patch, kernel_source_on_cpu

HOSTSIM = os.path.exists(os.environ.get("HIPEMU_CXX", "/opt/rocm/lib/llvm/bin/clang++"))
hostsim = pytest.mark.skipif(not HOSTSIM, reason="the host build of the kernel sources needs the ROCm clang")
K, B = 41, 2
E_BADARG = -1  # KANTTS_E_BADARG (include/kantts_hip.h)
# T = 150: three 64-frame tiles, the last one partial, and a sequence that ends inside the first tile (37);
# T = 7: shorter than the halo, and an empty sequence.  C: the two shipped widths, and one that is no multiple of the
# 64-channel block (132 = two blocks and a single quad).
SHAPES = [(150, (150, 37), 128), (150, (150, 37), 256), (150, (150, 37), 132), (7, (7, 0), 128), (7, (7, 0), 256),
          (7, (7, 0), 132)]
LEFT_PADS = (37, 20, 40, 0)  # postnet, predictors, all taps on one side (both sides)
DROPS = ((0.1, 0.1), (0.1, 0.0), (0.0, 0.1))
SEEDS = (0x1234567, 0x7654321)
RNG_OFFSET = 98765  # the device-resident offset the kernels must add to the seeds


def _guarded(rows, C, device, fill, guard):
    """(tensor (B, T, C) that is rows 1 .. rows of a (rows + 2, C) buffer, the buffer): one guard row before and after."""
    buf = torch.full((rows + 2, C), float(guard), dtype=torch.float32)
    buf[1:-1] = fill.reshape(rows, C) if torch.is_tensor(fill) else float(fill)
    buf = buf.to(device)
    return buf[1:-1], buf


class _Lib:
    """The two forms through the C ABI, on whatever library is installed (device or kernel sources on the CPU)."""

    def __init__(self, device, T, C):
        import kantts._hip as hip

        self.hip, self.device, self.T, self.C = hip, device, T, C
        self.off = torch.tensor([RNG_OFFSET], dtype=torch.int64, device=device)

    def _rc(self, rc, what):
        assert rc == 0, "%s returned %d" % (what, rc)

    def new(self):
        return torch.empty(B, self.T, self.C, dtype=torch.float32, device=self.device)

    def fused_fwd(self, c, w, res, lens, y, lp, p1, p2):
        h = self.hip
        return h.lib().kantts_fsmn_memory_drop_fwd(h.ptr(c), h.ptr(w), h.ptr(res), h.ptr(lens), h.ptr(y), B, self.T, self.C,
                                                   w.shape[-1], lp, p1, SEEDS[0], p2, SEEDS[1], h.ptr(self.off), h.stream())

    def fused_bwd(self, dy, w, lens, dx, dym, lp, p1, p2):
        h = self.hip
        return h.lib().kantts_fsmn_memory_drop_bwd(h.ptr(dy), h.ptr(w), h.ptr(lens), h.ptr(dx), h.ptr(dym), B, self.T,
                                                   self.C, w.shape[-1], lp, p1, SEEDS[0], p2, SEEDS[1], h.ptr(self.off),
                                                   h.stream())

    def drop2(self, x, res, y, p1, p2):
        h = self.hip
        self._rc(h.lib().kantts_dropout2_add(h.ptr(x), h.ptr(res), h.ptr(y), x.numel(), p1, SEEDS[0], p2, SEEDS[1],
                                             h.ptr(self.off), h.stream()), "dropout2_add")

    def pair_fwd(self, c, w, res, lens, lp, p1, p2):
        h = self.hip
        m, y = self.new(), self.new()
        self._rc(h.lib().kantts_fsmn_dwconv_fwd(h.ptr(c), h.ptr(w), None, h.ptr(lens), h.ptr(m), B, self.T, self.C, K, lp,
                                                h.stream()), "fsmn_dwconv_fwd")
        self.drop2(m, res, y, p1, p2)
        return y

    def pair_bwd(self, dy, c, w, lens, lp, p1, p2):
        h = self.hip
        dym, dx = self.new(), self.new()
        self.drop2(dy, None, dym, p1, p2)
        self._rc(h.lib().kantts_fsmn_dwconv_bwd(h.ptr(dym), h.ptr(c), h.ptr(w), h.ptr(lens), h.ptr(dx), None, None, 0, B,
                                                self.T, self.C, K, lp, h.stream()), "fsmn_dwconv_bwd (dx)")
        return dx, dym

    def filter_grad(self, dym, c, w, lens, lp):
        h = self.hip
        n = int(h.lib().kantts_fsmn_dwconv_bwd_ws(B, self.T, self.C, K))
        ws = torch.empty(max(n, 1), dtype=torch.float32, device=self.device)
        dw = torch.zeros_like(w)
        self._rc(h.lib().kantts_fsmn_dwconv_bwd(h.ptr(dym), h.ptr(c), h.ptr(w), h.ptr(lens), None, h.ptr(dw), h.ptr(ws), n,
                                                B, self.T, self.C, K, lp, h.stream()), "fsmn_dwconv_bwd (dw)")
        return dw


def _inputs(T, lens, C, device):
    g = torch.Generator().manual_seed(1000 * T + C)
    c, res, dy = (torch.randn(B, T, C, generator=g) for _ in range(3))
    w = 0.2 * torch.randn(C, K, generator=g)
    row = torch.arange(T)[None, :, None] >= torch.tensor(lens)[:, None, None]  # rows at or after lens[b]
    return c, res, dy, w.to(device), torch.tensor(lens, dtype=torch.int64, device=device), row


def _entry_points_case(device, T, lens_l, C):
    """1. y, dx, dym and the filter gradient of the one-launch form against the pair, bit for bit: every left_pad, both
    dropouts and each alone, with and without the residual, a non-zero device RNG offset."""
    L = _Lib(device, T, C)
    c, res, dy, w, lens, pad_rows = _inputs(T, lens_l, C, device)
    c, res, dy, pad_rows = c.to(device), res.to(device), dy.to(device), pad_rows.to(device)
    masked = 0
    for lp, (p1, p2), r in itertools.product(LEFT_PADS, DROPS, (res, None)):
        tag = "T %d C %d left_pad %d p (%g, %g) res %s" % (T, C, lp, p1, p2, r is not None)
        y = L.new()
        assert L.fused_fwd(c, w, r, lens, y, lp, p1, p2) == 0, tag
        y_ref = L.pair_fwd(c, w, r, lens, lp, p1, p2)
        print("%s: max |y - pair| = %g" % (tag, float((y - y_ref).abs().max())))
        assert torch.equal(y, y_ref), tag
        if r is None:  # backward has no residual port: once per (left_pad, p)
            dx, dym = L.new(), L.new()
            assert L.fused_bwd(dy, w, lens, dx, dym, lp, p1, p2) == 0, tag
            dx_ref, dym_pair = L.pair_bwd(dy, c, w, lens, lp, p1, p2)
            dym_ref = torch.where(pad_rows, torch.zeros_like(dym_pair), dym_pair)
            print("%s: max |dx - pair| = %g, max |dym - pair| = %g" % (tag, float((dx - dx_ref).abs().max()),
                                                                      float((dym - dym_ref).abs().max())))
            assert torch.equal(dx, dx_ref), tag
            assert torch.equal(dym, dym_ref), tag
            assert torch.equal(L.filter_grad(dym, c, w, lens, lp), L.filter_grad(dym_pair, c, w, lens, lp)), tag
            masked += int((dym_pair[:, : max(lens_l)] == 0).sum())
        # the masks are there, and the offset is added: without it the masks differ
        assert float(y_ref.abs().max()) > 0 or max(lens_l) == 0
    assert masked > 0
    L.off.zero_()
    y0 = L.new()
    assert L.fused_fwd(c, w, res, lens, y0, 37, 0.1, 0.1) == 0
    L.off.fill_(RNG_OFFSET)
    y1 = L.new()
    assert L.fused_fwd(c, w, res, lens, y1, 37, 0.1, 0.1) == 0
    assert not torch.equal(y0, y1)


def _contract_case(device, T, lens_l, C):
    """2. Nothing outside the contract is touched: guard rows before and after every tensor (NaN for inputs, a sentinel for
    outputs), c and dy NaN in the rows at or after lens[b] (res is read at every row: it stays finite), outputs pre-filled
    with NaN.  Outputs come back finite, the guards unchanged."""
    L = _Lib(device, T, C)
    c0, res0, dy0, w, lens, pad_rows = _inputs(T, lens_l, C, device)
    nan = float("nan")
    c0 = torch.where(pad_rows, torch.full_like(c0, nan), c0)
    dy0 = torch.where(pad_rows, torch.full_like(dy0, nan), dy0)
    c, _ = _guarded(B * T, C, device, c0, nan)
    dy, _ = _guarded(B * T, C, device, dy0, nan)
    res, _ = _guarded(B * T, C, device, res0, nan)
    c, dy, res = (t.view(B, T, C) for t in (c, dy, res))
    SENT = 12345.0
    for lp, r in itertools.product(LEFT_PADS, (res, None)):
        outs = [_guarded(B * T, C, device, nan, SENT) for _ in range(3)]
        (y, _), (dx, _), (dym, _) = outs
        assert L.fused_fwd(c, w, r, lens, y.view(B, T, C), lp, 0.1, 0.1) == 0
        assert L.fused_bwd(dy, w, lens, dx.view(B, T, C), dym.view(B, T, C), lp, 0.1, 0.1) == 0
        for name, (t, buf) in zip(("y", "dx", "dym"), outs):
            assert bool(torch.isfinite(t).all()), "%s left_pad %d" % (name, lp)
            assert bool((buf[0] == SENT).all()) and bool((buf[-1] == SENT).all()), "%s guard, left_pad %d" % (name, lp)
        pad = pad_rows.to(device).expand(B, T, C)
        assert float(dx.view(B, T, C)[pad].abs().sum()) == 0.0 and float(dym.view(B, T, C)[pad].abs().sum()) == 0.0
        want = (res if r is not None else torch.zeros_like(res))[pad]
        assert torch.equal(y.view(B, T, C)[pad], want)  # a padded row passes the residual through


def _declines_case(device):
    """What the launches decline (the host runs the pair then) and what they refuse, before any launch."""
    import kantts._hip as hip

    T, C = 20, 64
    L = _Lib(device, T, C)
    c, res, dy, w, lens, _ = _inputs(T, (20, 9), C, device)
    c, dy = c.to(device), dy.to(device)
    y = L.new()
    assert L.fused_fwd(c, w[:, :3].contiguous(), None, lens, y, 1, 0.1, 0.1) == hip.E_UNSUPPORTED  # K != 41
    big = torch.zeros(B * T * C + 4, dtype=torch.float32, device=device)
    odd = big[1:1 + B * T * C].view(B, T, C)  # 4 bytes off a 16-byte boundary
    assert L.fused_fwd(odd, w, None, lens, y, 20, 0.1, 0.1) == hip.E_UNSUPPORTED
    assert L.fused_bwd(dy, w, lens, y, odd, 20, 0.1, 0.1) == hip.E_UNSUPPORTED
    L6 = _Lib(device, T, 6)  # C % 4 != 0
    assert L6.fused_fwd(c, w[:6].contiguous(), None, lens, y, 20, 0.1, 0.1) == hip.E_UNSUPPORTED
    assert L.fused_fwd(c, w, None, lens, y, 41, 0.1, 0.1) == E_BADARG  # left_pad outside the filter
    assert L.fused_fwd(c, w, None, lens, y, 20, 1.0, 0.1) == E_BADARG
    assert L.fused_bwd(dy, w, lens, y, None, 20, 0.1, 0.1) == E_BADARG


# ---------------------------------------------------------------------------------------------- module level
class _CountingLib:
    """The installed library with every call counted by entry point (and, for the memory block's backward, whether the call
    asked for dx: the FIR launch, or only for the filter gradient)."""

    def __init__(self, real):
        self._real, self.calls = real, {}

    def __getattr__(self, name):
        fn = getattr(self._real, name)  # AttributeError for an entry point the library does not have
        if not name.startswith("kantts_"):
            return fn

        def counted(*a):
            key = name
            if name == "kantts_fsmn_dwconv_bwd":
                key = name + (":dx" if a[4] is not None else ":dw")
            self.calls[key] = self.calls.get(key, 0) + 1
            return fn(*a)

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


LAYERS, MT, MD = 2, 50, 256


def _run_module(device, width, precision, fused):
    import kantts._hip as hip
    import kantts._hip.ops as ops
    import kantts.models.sambert.fsmn as fsmn
    from kantts.models.utils import SeqInfo

    cfg = O.sambert_config()
    torch.manual_seed(11)
    enc = fsmn.FsmnEncoderV2(K, LAYERS, width, MD, cfg["postnet_ffn_inner_dim"], dropout=0.1, shift=[0, 17])
    enc = enc.to(device).train()
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(B, MT, width, generator=g).to(device)
    cot = torch.randn(B, MT, MD, generator=g).to(device)
    info = SeqInfo(torch.tensor([MT, 37], device=device), MT)
    before, real_sk, was = hip.get_precision(), ops._splitk_for, ops.FSMN_MEMORY_DROP["on"]
    ops._splitk_for = lambda *a: 1  # one K slice per weight gradient: a fixed summation order (test_fsmn_residual_grad.py)
    ops.FSMN_MEMORY_DROP["on"] = fused
    hip.set_precision(precision)
    try:
        ops._seed_counter = itertools.count(1000)
        hip.rng_state("cpu" if device == "cpu" else device).fill_(77)
        with _counting() as lib:
            x = x0.clone().requires_grad_(True)
            y = enc(x, info)
            (y * cot).sum().backward()
            if device != "cpu":
                torch.cuda.synchronize()
    finally:
        hip.set_precision(before)
        ops._splitk_for = real_sk
        ops.FSMN_MEMORY_DROP["on"] = was
        hip.rng_state("cpu" if device == "cpu" else device).zero_()
    grads = {"x": x.grad.detach().cpu()}
    grads.update({n: p.grad.detach().cpu() for n, p in enc.named_parameters()})
    return y.detach().cpu(), grads, lib.calls


def _module_case(device, width, precision):
    """3. FsmnEncoderV2 in training mode, the switch on against the switch off: output, input gradient and every parameter
    gradient bit for bit; one FIR-family launch per layer and direction, no dropout2_add but the encoder's first."""
    y0, g0, n0 = _run_module(device, width, precision, fused=False)
    y1, g1, n1 = _run_module(device, width, precision, fused=True)
    assert torch.equal(y0, y1)
    assert sorted(g0) == sorted(g1) and "memory_block_lst.1.conv_dw.weight" in g0
    for n in g0:
        print("%s width %d %s: max |one launch - pair| = %g (max |pair| %g)" % (
            precision, width, n, float((g0[n] - g1[n]).abs().max()), float(g0[n].abs().max())))
        assert torch.equal(g0[n], g1[n]), n
    assert float(g0["x"].abs().max()) > 0

    def fsmn_calls(n):
        return {k: v for k, v in n.items() if "fsmn" in k or "dropout2" in k}

    # the encoder's first dropout runs forward and (the input asks for its gradient) backward
    assert fsmn_calls(n0) == {"kantts_fsmn_dwconv_fwd": LAYERS, "kantts_fsmn_dwconv_bwd:dx": LAYERS,
                              "kantts_fsmn_dwconv_bwd:dw": LAYERS, "kantts_fsmn_dwconv_bwd_ws": LAYERS,
                              "kantts_dropout2_add": 2 + 2 * LAYERS}
    assert fsmn_calls(n1) == {"kantts_fsmn_memory_drop_fwd": LAYERS, "kantts_fsmn_memory_drop_bwd": LAYERS,
                              "kantts_fsmn_dwconv_bwd:dw": LAYERS, "kantts_fsmn_dwconv_bwd_ws": LAYERS,
                              "kantts_dropout2_add": 2}


MODULE_CASES = [(MD, "bf16"), (MD, "fp32"), (80, "bf16"), (80, "fp32")]  # 80: the first layer has no residual
_ids = ["T%d-C%d" % (s[0], s[2]) for s in SHAPES]


@hostsim
@pytest.mark.parametrize("T,lens,C", SHAPES, ids=_ids)
def test_entry_points_equal_the_pair_kernel_source(T, lens, C):
    with kernel_source_on_cpu():
        _entry_points_case("cpu", T, lens, C)


@pytest.mark.gpu
@pytest.mark.parametrize("T,lens,C", SHAPES, ids=_ids)
def test_entry_points_equal_the_pair_gpu(T, lens, C):
    _entry_points_case("cuda", T, lens, C)


@hostsim
@pytest.mark.parametrize("T,lens,C", SHAPES, ids=_ids)
def test_nothing_outside_the_contract_is_touched_kernel_source(T, lens, C):
    with kernel_source_on_cpu():
        _contract_case("cpu", T, lens, C)


@pytest.mark.gpu
@pytest.mark.parametrize("T,lens,C", SHAPES, ids=_ids)
def test_nothing_outside_the_contract_is_touched_gpu(T, lens, C):
    _contract_case("cuda", T, lens, C)


@hostsim
def test_declined_and_refused_arguments_kernel_source():
    with kernel_source_on_cpu():
        _declines_case("cpu")


@pytest.mark.gpu
def test_declined_and_refused_arguments_gpu():
    _declines_case("cuda")


@hostsim
@pytest.mark.parametrize("width,precision", MODULE_CASES)
def test_encoder_with_one_launch_per_layer_and_direction_kernel_source(width, precision):
    with kernel_source_on_cpu():
        _module_case("cpu", width, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("width,precision", MODULE_CASES)
def test_encoder_with_one_launch_per_layer_and_direction_gpu(width, precision):
    _module_case("cuda", width, precision)
