"""kantts_pnca_bwd_seam: the cross-row half of a PNCA block's backward and the row-local half of the block below it in ONE
launch (csrc/pnca_block.hip: pnca_bwd_seam_kernel), and the host path that links two blocks of a stack, issues the seam from
the upper block's attention node and lets the lower block's feed-forward node adopt -- or refuse -- what it left.

The seam kernel runs the two bodies of the launches it replaces, the second on the dx tile the first has just produced, so
the oracle is ``kantts_pnca_attn_qkv_bwd`` followed by ``kantts_pnca_block_bwd`` on the same back end and every comparison
of what the launches write is BIT FOR BIT (integer views).  Direct cases run on the kernel SOURCES compiled for the host
(tests/hipemu, unmarked) and on the device (``gpu``); the host-level cases also on the numpy model of the C ABI, which has
no such entry point and must keep the two launches.  Output buffers are oversized and NaN-filled: a write past the bound, or
a word one form writes and the other leaves, shows as a difference.
"""
import contextlib
import ctypes
import itertools

import pytest
import torch

from util import emulation, kernel_source_on_cpu

BACKENDS = ["hostsim", pytest.param("gpu", marks=pytest.mark.gpu)]
E_BADARG, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3
PAD = 257


@contextlib.contextmanager
def _backend(name):
    import kantts._hip as hip

    if name == "gpu":
        hip.lib()
        hip.rng_state("cuda").zero_()
        yield "cuda"
    elif name == "emulated":
        with emulation():
            hip.rng_state("cpu").zero_()
            yield "cpu"
    else:
        with kernel_source_on_cpu():
            hip.rng_state("cpu").zero_()
            yield "cpu"


def _sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(_bits(a), _bits(b)), "%s: the seam and the two launches differ" % what


def test_codes_are_the_headers():
    import os
    import re

    from util import ROOT

    header = open(os.path.join(ROOT, "include", "kantts_hip.h")).read()
    for name, val in (("BADARG", E_BADARG), ("UNSUPPORTED", E_UNSUPPORTED), ("WORKSPACE", E_WORKSPACE)):
        assert int(re.search(r"#define\s+KANTTS_E_%s\s+\(?(-?\d+)" % name, header).group(1)) == val
    assert "int kantts_pnca_bwd_seam(const kantts_pnca_attn_bwd_args* upper, const kantts_pnca_block_bwd_args* lower" in header


# ---------------------------------------------------------------------------------------------- direct C-ABI cases
class _Problem:
    """Operands of one seam (host copies): the upper block's cross-row half and the lower block's row-local half."""

    OUT = (("dqkv", 384, torch.float32), ("dhkv", 256, torch.float32), ("dx", 128, torch.float32),
           ("dz", 1024, torch.bfloat16), ("g1", 128, torch.float32), ("d_ox", 128, torch.float32),
           ("d_oh", 128, torch.float32))

    def __init__(self, B, L, lens, bw, p, seeded, masks, dres, bw_on_device, seed=0):
        self.B, self.L, self.M, self.bw, self.p, self.seeded, self.bw_on_device = B, L, B * L, bw, p, seeded, bw_on_device
        g = torch.Generator().manual_seed(1234 + seed)
        M = self.M

        def rn(*s, scale=1.0):
            return torch.randn(*s, generator=g) * scale

        self.t = dict(
            qkv=rn(M, 384, scale=0.6), hkv=rn(M, 256, scale=0.6), ox=rn(M, 128), oh=rn(M, 128), d_ox=rn(M, 128), d_oh=rn(M, 128),
            lse_x=1.0 + rn(B, 8, L, scale=0.3), lse_h=1.0 + rn(B, 8, L, scale=0.3), x=rn(M, 128), mean0=rn(M, scale=0.1),
            rstd0=1.0 + rn(M, scale=0.1).abs(), gamma0=1.0 + rn(128, scale=0.1), dres=rn(M, 128) if dres else None,
            hid=rn(M, 1024).to(torch.bfloat16), y1=rn(M, 128), mean1=rn(M, scale=0.1), rstd1=1.0 + rn(M, scale=0.1).abs(),
            gamma1=1.0 + rn(128, scale=0.1),
            lens=torch.tensor(lens, dtype=torch.int32))
        self.w = dict(wqkv=rn(384, 128, scale=0.09), wfcx=rn(128, 128, scale=0.09), wfch=rn(128, 128, scale=0.09),
                      w1=rn(1024, 128, 1, scale=0.09), w2=rn(128, 1024, 1, scale=0.03))
        mask = None
        if masks:  # rows at or after their sequence's length, and one row inside the first sequence
            pos = torch.arange(L).view(1, L)
            mask = (pos >= torch.tensor(lens).view(B, 1)).view(M)
            mask[min(3, M - 1)] = True
            mask = mask.to(torch.uint8)
        self.mask = mask

    def on(self, dev):
        import kantts._hip.ops_bf16 as ops_bf16

        t = {k: (None if v is None else v.to(dev)) for k, v in self.t.items()}
        w = {k: v.to(dev) for k, v in self.w.items()}
        _, _, wt2, wt1 = ops_bf16.ffn_frag_weights(w["w1"], w["w2"])
        t.update(wqkvT=ops_bf16.frag_major(w["wqkv"].t()), wfcxT=ops_bf16.frag_major(w["wfcx"].t()),
                 wfchT=ops_bf16.frag_major(w["wfch"].t()), wt2=wt2, wt1=wt1)
        t["mask"] = None if self.mask is None else self.mask.to(dev)
        t["bw_dev"] = torch.tensor([self.bw], dtype=torch.int32, device=dev) if self.bw_on_device else None
        t["seed_dev"] = torch.tensor([987654321], dtype=torch.int64, device=dev) if self.seeded else None
        return t

    def buffers(self, dev):
        """NaN-filled output buffers with PAD elements behind their bound: name -> (buffer, view of the front)."""
        out = {}
        for name, cols, dt in self.OUT:
            buf = torch.full((self.M * cols + PAD,), float("nan"), device=dev, dtype=dt)
            out[name] = (buf, buf[:self.M * cols].view(self.M, cols))
        n = ((self.M + 31) // 32) * 256
        for name in ("ws_u", "ws_l"):
            buf = torch.full((n + PAD,), float("nan"), device=dev)
            out[name] = (buf, buf[:n])
        return out

    def structs(self, t, o):
        """(kantts_pnca_attn_bwd_args of the upper block, kantts_pnca_block_bwd_args of the lower one)."""
        import kantts._hip as hip

        p, bw = self.p, self.bw
        gu, _ = hip._pnca_attn_bwd_args(
            t["qkv"], t["hkv"], 256, t["ox"], t["oh"], t["d_ox"], t["d_oh"], t["lse_x"], t["lse_h"], self.B, self.L, t["lens"],
            t["bw_dev"], 0 if self.bw_on_device else bw, 0 if self.bw_on_device else bw, p, 11, 12, t["wqkvT"], t["x"],
            t["mean0"], t["rstd0"], t["gamma0"], t["dres"], t["mask"], o["dqkv"][1], o["dhkv"][1], o["dx"][1])
        gl, _ = hip._pnca_block_bwd_args(
            o["dx"][1], t["hid"], t["y1"], t["mean1"], t["rstd1"], t["gamma1"], t["mask"], t["wt2"], t["wt1"], t["wfcxT"],
            t["wfchT"], 1.0 / (1.0 - p) if p > 0 else 1.0, p, 13, p, 14, o["dz"][1], o["g1"][1], o["d_ox"][1], o["d_oh"][1])
        gu.ws, gu.ws_floats = hip.ptr(o["ws_u"][1]), o["ws_u"][1].numel()
        gl.ws, gl.ws_floats = hip.ptr(o["ws_l"][1]), o["ws_l"][1].numel()
        gu.seed_dev = gl.seed_dev = hip.ptr(t["seed_dev"])
        return gu, gl


def _untouched(o):
    return all(bool(torch.isnan(buf.float()).all()) for buf, _ in o.values())


_S1, _S2, _S3 = (1, 32, (32,)), (1, 33, (33,)), (2, 40, (40, 23))
# shape, band, probability, seed_dev, row masks, dres, band width in device memory
_DIRECT = [
    (_S1, 0, 0.0, False, False, False, False),
    (_S1, 5, 0.1, True, True, True, False),
    (_S1, 16, 0.1, False, True, False, True),
    (_S2, 5, 0.1, False, True, False, False),
    (_S2, 16, 0.0, True, False, True, False),
    (_S2, 0, 0.1, True, False, True, True),
    (_S3, 0, 0.1, True, True, True, False),
    (_S3, 5, 0.1, True, True, True, True),
    (_S3, 16, 0.1, False, False, False, False),
    (_S3, 16, 0.0, False, True, False, True),
    (_S3, 5, 0.0, False, False, True, False),
]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", _DIRECT, ids=lambda c: "M%d-bw%d%s-p%g%s%s%s" % (
    c[0][0] * c[0][1], c[1], "dev" if c[6] else "", c[2], "-seed" if c[3] else "", "-mask" if c[4] else "",
    "-dres" if c[5] else ""))
def test_seam_equals_the_two_launches(backend, case):
    import kantts._hip as hip

    (B, L, lens), bw, p, seeded, masks, dres, bw_on_device = case
    with _backend(backend) as dev:
        L_ = hip.lib()
        assert hip.pnca_bwd_seam_entry_point()
        prob = _Problem(B, L, lens, bw, p, seeded, masks, dres, bw_on_device)
        t = prob.on(dev)
        ref, got = prob.buffers(dev), prob.buffers(dev)
        gu, gl = prob.structs(t, ref)
        assert L_.kantts_pnca_attn_qkv_bwd(ctypes.byref(gu), hip.stream()) == 0
        assert L_.kantts_pnca_block_bwd(ctypes.byref(gl), hip.stream()) == 0
        gu, gl = prob.structs(t, got)
        assert L_.kantts_pnca_bwd_seam(ctypes.byref(gu), ctypes.byref(gl), hip.stream()) == 0
        _sync(dev)
        for name in ref:
            buf, front = got[name]
            _same_bits(buf, ref[name][0], name)
            assert bool(torch.isnan(buf[front.numel():].float()).all()), name + ": guard band"
            assert not bool(torch.isnan(front.float()).any()), name
        assert float(got["dx"][1].abs().max()) > 0 and float(got["d_ox"][1].abs().max()) > 0
        if masks:
            rows = t["mask"].bool()
            assert float(got["dx"][1][rows].abs().max()) == 0 and float(got["g1"][1][rows].abs().max()) == 0


@pytest.mark.parametrize("backend", BACKENDS)
def test_refusals_launch_nothing(backend):
    import kantts._hip as hip

    with _backend(backend) as dev:
        L_ = hip.lib()
        prob = _Problem(2, 40, (40, 23), 5, 0.1, True, True, True, False)
        t = prob.on(dev)
        o = prob.buffers(dev)
        other = torch.full((prob.M, 128), float("nan"), device=dev)

        def run(change):
            gu, gl = prob.structs(t, o)
            change(gu, gl)
            rc = L_.kantts_pnca_bwd_seam(ctypes.byref(gu), ctypes.byref(gl), hip.stream())
            _sync(dev)
            assert _untouched(o) and bool(torch.isnan(other).all())
            return rc

        assert L_.kantts_pnca_bwd_seam(None, None, hip.stream()) == E_BADARG
        assert run(lambda gu, gl: setattr(gl, "dy", hip.ptr(other))) == E_BADARG  # lower->dy != upper->dx
        assert run(lambda gu, gl: setattr(gl, "M", prob.M - 1)) == E_BADARG       # mismatched M
        assert run(lambda gu, gl: (setattr(gu, "bw_x", 17), setattr(gu, "bw_h", 17))) == E_UNSUPPORTED
        assert run(lambda gu, gl: setattr(gu, "ws_floats", gu.ws_floats - 1)) == E_WORKSPACE
        assert run(lambda gu, gl: setattr(gl, "ws_floats", gl.ws_floats - 1)) == E_WORKSPACE
        assert run(lambda gu, gl: setattr(gl, "F", 512)) == E_UNSUPPORTED
        assert run(lambda gu, gl: setattr(gl, "hid", None)) == E_BADARG
        assert run(lambda gu, gl: (setattr(gu, "L", 0), setattr(gl, "M", 0))) == 0  # nothing to do


# ---------------------------------------------------------------------------------------------- host level: a stack of blocks
SB, SL, SLENS, SBW = 2, 40, (40, 23), 5


class _Stack:
    def __init__(self, dev):
        from kantts.models.sambert import PNCABlock
        from kantts.models.utils import SeqInfo

        g = torch.Generator().manual_seed(5)
        torch.manual_seed(5)
        self.dev = dev
        self.blocks = [PNCABlock(128, 160, 8, 16, 1024, (1, 1), 0.1, 0.1, 0.1).to(dev) for _ in range(3)]
        self.final = torch.nn.LayerNorm(128, eps=1e-6).to(dev)
        with torch.no_grad():  # biases and LayerNorm vectors away from their 0 / 1 initial values
            for blk in self.blocks:
                blk.train()
                for _, p in blk.named_parameters():
                    if p.dim() == 1:
                        p.add_(torch.randn(p.shape, generator=g).to(dev) * 0.1)
        self.x0 = (torch.randn(SB, SL, 128, generator=g) * 0.7).to(dev)
        self.hk0 = torch.randn(SB, SL, 3 * 256, generator=g).to(dev)
        self.cot = torch.randn(SB, SL, 128, generator=g).to(dev)
        self.info = SeqInfo(torch.tensor(SLENS, dtype=torch.int64, device=dev), SL)

    def run(self, seam_on, second_consumer=False):
        """One forward + backward of the stack; returns (call counts, activations' gradients, LayerNorm vector gradients,
        weight gradients)."""
        import kantts._hip as hip
        import kantts._hip.ops as ops
        import kantts._hip.ops_bf16 as ops_bf16

        ops._seed_counter = itertools.count(1000)
        hip.rng_state(self.dev).zero_()
        for blk in self.blocks:
            blk.zero_grad()
        x = self.x0.clone().requires_grad_(True)
        hk = self.hk0.clone().requires_grad_(True)
        counts = dict(block=0, attn=0, seam=0)
        real = (ops_bf16.pnca_block_bwd, hip.pnca_attn_qkv_bwd, hip.pnca_bwd_seam)

        def counted(key, fn):
            def call(*a, **k):
                counts[key] += 1
                return fn(*a, **k)
            return call

        ops_bf16.pnca_block_bwd, hip.pnca_attn_qkv_bwd = counted("block", real[0]), counted("attn", real[1])
        hip.pnca_bwd_seam = counted("seam", real[2])
        was = ops_bf16.PNCA_BWD_SEAM["on"]
        ops_bf16.PNCA_BWD_SEAM["on"] = seam_on
        try:
            h = x * 1.0  # a non-leaf, as in the decoder
            outs = []
            for i, blk in enumerate(self.blocks):
                nxt = self.blocks[i + 1].pnca_attn.layer_norm if i + 1 < len(self.blocks) else self.final
                h, _, _ = blk(h, None, mask=self.info, x_band_width=SBW, h_band_width=SBW, hkv=hk[:, :, 256 * i:256 * (i + 1)],
                              private_input=i > 0, next_ln=nxt)
                outs.append(h)
            loss = (h * self.cot).sum()
            if second_consumer:
                loss = loss + 0.5 * outs[1].sum()
            loss.backward()
            _sync(self.dev)
        finally:
            ops_bf16.pnca_block_bwd, hip.pnca_attn_qkv_bwd, hip.pnca_bwd_seam = real
            ops_bf16.PNCA_BWD_SEAM["on"] = was
        acts = dict(x=x.grad.detach().cpu().clone(), hk=hk.grad.detach().cpu().clone())
        vec, mat = {}, {}
        for i, blk in enumerate(self.blocks):
            for n, p in blk.named_parameters():
                if p.grad is None:
                    continue
                (vec if "layer_norm" in n else mat)["%d.%s" % (i, n)] = p.grad.detach().cpu().clone()
        return counts, acts, vec, mat


def _stack_case(backend, second_consumer, want_on):
    import kantts._hip as hip

    with _backend(backend) as dev:
        hip.set_precision("bf16")
        try:
            st = _Stack(dev)
            c_off, a_off, v_off, m_off = st.run(False, second_consumer)
            _, a_off2, v_off2, m_off2 = st.run(False, second_consumer)
            c_on, a_on, v_on, m_on = st.run(True, second_consumer)
        finally:
            hip.set_precision("fp32")
    assert c_off == dict(block=3, attn=3, seam=0)
    assert c_on == want_on
    for name in a_off:
        assert float(a_off[name].abs().max()) > 0
        _same_bits(a_on[name], a_off[name], name + ".grad")
    assert len(v_off) == 3 * 4  # gamma / beta of the two LayerNorms of each block
    for name in v_off:
        _same_bits(v_on[name], v_off[name], name)
    assert m_off and set(m_off) == set(m_on)
    for name in m_off:
        # weight gradients pass through the token-split atomics of the contraction: two runs of ONE form differ by their
        # order, and the seam may differ from the two launches by no more than that (zero where the launch uses one slice)
        bound = float((m_off[name].double() - m_off2[name].double()).abs().max())
        err = float((m_on[name].double() - m_off[name].double()).abs().max())
        print("%s: on vs off %.3e, off vs off %.3e" % (name, err, bound))
        assert err <= bound, "%s: %.3e > %.3e" % (name, err, bound)


@pytest.mark.parametrize("backend", BACKENDS)
def test_stack_of_three_blocks(backend):
    """block_bwd of the top block, one seam per block boundary, attn_qkv_bwd of the bottom block."""
    _stack_case(backend, False, dict(block=1, attn=1, seam=2))


@pytest.mark.parametrize("backend", BACKENDS)
def test_second_consumer_refuses_the_deposit(backend):
    """Block 1's output also feeds the loss directly: the gradient its feed-forward node receives is not the dx the seam
    above it wrote, the deposit is dropped and that node launches its own row-local half."""
    _stack_case(backend, True, dict(block=2, attn=1, seam=2))


@pytest.mark.parametrize("second_consumer", [False, True])
def test_emulated_abi_keeps_the_two_launches(second_consumer):
    """The numpy model of the C ABI has no kantts_pnca_bwd_seam: same launches, same results with the switch on."""
    import kantts._hip as hip

    with _backend("emulated"):
        assert not hip.pnca_bwd_seam_entry_point()
    _stack_case("emulated", second_consumer, dict(block=3, attn=3, seam=0))
