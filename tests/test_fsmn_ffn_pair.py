"""csrc/ffn_pair.hip at the FSMN feed-forward shapes: (256, 256, 512) (postnet layers, 80-token tiles) and (128, 128, 256)
(pitch / energy predictor layers, 32-token tiles), k = 1 both ways.

Every case runs on the kernel SOURCES compiled for the host (tests/hipemu, unmarked) and on the device (``gpu``).
Expected values of the direct calls are an fp64 evaluation, written here, on the bf16-rounded operands:
  hidden / dz (bf16)   rel-L2 < 2e-3 and fewer than 2 % of the bf16 elements differ (the bounds of test_gpu_bf16_ops.py;
                       an fp32 evaluation in 32-wide k blocks is 3.6e-5 / 2.3e-7 from fp64: the cap is the bf16 ulp)
  out / dx (fp32)      rel-L2 < 1e-4 against fp64 computed FROM THE KERNEL'S OWN hidden / dz (the project's fp32 bound)
"""
import contextlib
import itertools

import pytest
import torch

from util import kernel_source_on_cpu, rel_l2

BF = torch.bfloat16
# (K1, N, F, BM): BM is the token tile height csrc/ffn_pair.hip uses at that shape
SHAPES = [(256, 256, 512, 80), (128, 128, 256, 32)]
BACKENDS = ["hostsim", pytest.param("gpu", marks=pytest.mark.gpu)]


def _ms(bm):
    return [5, bm - 1, bm, bm + 1, 2 * bm + 19]  # tail only, one row short, the exact tile, one row into the next, ragged


CASES = [(k1, n, f, bm, m) for (k1, n, f, bm) in SHAPES for m in _ms(bm)]
IDS = ["%dx%dx%d-M%d" % (k1, n, f, m) for (k1, n, f, bm, m) in CASES]


@contextlib.contextmanager
def _backend(name):
    import kantts._hip as hip

    if name == "gpu":
        hip.lib()
        hip.rng_state("cuda").zero_()
        yield "cuda"
    else:
        with kernel_source_on_cpu():
            hip.rng_state("cpu").zero_()
            yield "cpu"


_ops_cache = {}


def _operands(k1, n, f, m):
    """bf16-rounded operands (as fp32 tensors) and their fp64 copies; made once per shape and shared, never modified."""
    key = (k1, n, f, m)
    if key not in _ops_cache:
        g = torch.Generator().manual_seed(1000 * k1 + f + m)
        rb = lambda t: t.to(BF).float()  # noqa: E731
        o = dict(x=rb(torch.randn(m, k1, generator=g)), w1=rb(torch.randn(f, k1, generator=g) * 0.08),
                 w2=rb(torch.randn(n, f, generator=g) * 0.05), b1=torch.randn(f, generator=g) * 0.3,
                 dy=rb(torch.randn(m, n, generator=g)), res=torch.randn(m, k1, generator=g))
        _ops_cache[key] = o
    return _ops_cache[key]


def _check_hidden(got, want64, what):
    want = want64.to(BF)
    r = rel_l2(got.float(), want64)
    d = float((got != want).float().mean())
    print("%s: rel-L2 %.3e, differing bf16 elements %.3e" % (what, r, d))
    assert r < 2e-3, (what, r)
    assert d < 0.02, (what, d)


def _fwd(dev, o, k1, n, f, m, *, drop_p=0.0, seed=0, write_hid=True, pad=3):
    """Direct forward-form call on oversized, NaN-filled outputs: returns (out, hid) INCLUDING the rows past m."""
    import kantts._hip as hip
    from kantts._hip.ops_bf16 import frag_major

    x, w1, w2, b1 = (o[k].to(dev) for k in ("x", "w1", "w2", "b1"))
    out = torch.full((m + pad, n), float("nan"), device=dev)
    hid = torch.full((m + pad, f), float("nan"), device=dev, dtype=BF) if write_hid else None
    assert hip.ffn_pair(x, frag_major(w1), frag_major(w2), out, M=m, T=m, F=f, bias1=b1, relu=True, drop1_p=drop_p,
                        drop1_seed=seed, t_out=hid)
    return out.cpu(), None if hid is None else hid.cpu()


def _bwd(dev, o, hid, k1, n, f, m, *, alpha1=1.0, pad=3):
    """Direct backward-form call: dz = gate_{hid > 0}(dy W2) * alpha1 (bf16), dx = dz W1 + res (fp32)."""
    import kantts._hip as hip
    from kantts._hip.ops_bf16 import frag_major

    dy, w1, w2, res = (o[k].to(dev) for k in ("dy", "w1", "w2", "res"))
    dx = torch.full((m + pad, k1), float("nan"), device=dev)
    dz = torch.full((m + pad, f), float("nan"), device=dev, dtype=BF)
    # the images of the TRANSPOSED weights: phase 1 streams W2^T (F, N), phase 2 W1^T (K1, F)
    assert hip.ffn_pair(dy, frag_major(w2.t().contiguous()), frag_major(w1.t().contiguous()), dx, M=m, T=m, F=f,
                        alpha1=alpha1, gate=hid.to(dev), t_out=dz, res=res)
    return dx.cpu(), dz.cpu()


def _two_launch_fwd(dev, o, k1, n, f, m, drop_p, seed):
    import kantts._hip as hip

    x, w1, w2, b1 = (o[k].to(dev) for k in ("x", "w1", "w2", "b1"))
    hid = torch.empty((m, f), device=dev, dtype=BF)
    out = torch.empty((m, n), device=dev)
    assert hip.bgemm_nt([(x, k1, w1.to(BF), k1, k1, 0)], m, f, hid, f, bias=b1, relu=True, drop_p=drop_p, drop_seed=seed)
    assert hip.bgemm_nt([(hid, f, w2.to(BF), f, f, 0)], m, n, out, n)
    return out.cpu(), hid.cpu()


def _two_launch_bwd(dev, o, hid, k1, n, f, m, alpha1):
    import kantts._hip as hip

    dy, w1, w2, res = (o[k].to(dev) for k in ("dy", "w1", "w2", "res"))
    dz = torch.empty((m, f), device=dev, dtype=BF)
    dx = torch.empty((m, k1), device=dev)
    assert hip.bgemm_nt([(dy, n, w2.to(BF), f, n, 0)], m, f, dz, f, b_kn=True, a_drop_ld=n, gate=hid.to(dev), ldg=f,
                        alpha=alpha1)
    assert hip.bgemm_nt([(dz, f, w1.to(BF), k1, f, 0)], m, k1, dx, k1, b_kn=True, a_drop_ld=f, res=res, ldr=k1)
    return dx.cpu(), dz.cpu()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("k1,n,f,bm,m", CASES, ids=IDS)
def test_direct_forward_and_backward_against_fp64(backend, k1, n, f, bm, m):
    o = _operands(k1, n, f, m)
    x, w1, w2, b1, dy, res = (o[k].double() for k in ("x", "w1", "w2", "b1", "dy", "res"))
    with _backend(backend) as dev:
        out, hid = _fwd(dev, o, k1, n, f, m)
        out_nohid, _ = _fwd(dev, o, k1, n, f, m, write_hid=False)
        dx, dz = _bwd(dev, o, hid[:m].contiguous(), k1, n, f, m)
    # ownership: rows past M of the oversized buffers keep their NaN fill
    for name, t in (("out", out), ("hid", hid), ("dx", dx), ("dz", dz), ("out (no hidden write)", out_nohid)):
        assert torch.isnan(t[m:].float()).all(), "%s: a row past M was written" % name
        assert not torch.isnan(t[:m].float()).any(), "%s: a row below M was not written" % name
    _check_hidden(hid[:m], torch.relu(x @ w1.t() + b1), "hidden")
    r = rel_l2(out[:m], hid[:m].double() @ w2.t())
    print("out: rel-L2 %.3e" % r)
    assert r < 1e-4, r
    # t_out = None (inference): the same output, bit for bit
    assert torch.equal(out[:m], out_nohid[:m])
    h64 = hid[:m].double()
    _check_hidden(dz[:m], torch.where(h64 > 0, dy @ w2, torch.zeros((), dtype=torch.float64)), "dz")
    r = rel_l2(dx[:m], dz[:m].double() @ w1 + res)
    print("dx: rel-L2 %.3e" % r)
    assert r < 1e-4, r


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("k1,n,f,bm,m", CASES, ids=IDS)
def test_dropout_masks_equal_the_two_launch_chain(backend, k1, n, f, bm, m):
    """drop1_p = 0.1 forward, alpha1 = 1 / 0.9 backward, against kantts_bgemm_nt x 2 on the same back end with the same
    seed: the same zero pattern of the hidden tensor (same masks: the index arithmetic m*F + f at F = 512 / 256)."""
    o = _operands(k1, n, f, m)
    x, w1, w2, b1, dy, res = (o[k].double() for k in ("x", "w1", "w2", "b1", "dy", "res"))
    seed, a1 = 4242 + m, 1.0 / 0.9
    with _backend(backend) as dev:
        out, hid = _fwd(dev, o, k1, n, f, m, drop_p=0.1, seed=seed)
        out2, hid2 = _two_launch_fwd(dev, o, k1, n, f, m, 0.1, seed)
        dx, dz = _bwd(dev, o, hid[:m].contiguous(), k1, n, f, m, alpha1=a1)
        dx2, dz2 = _two_launch_bwd(dev, o, hid[:m].contiguous(), k1, n, f, m, a1)
    hid, out, dx, dz = hid[:m], out[:m], dx[:m], dz[:m]
    assert torch.equal(hid == 0, hid2 == 0), "the hidden tensor's zero pattern differs from the two-launch form's"
    pre = torch.relu(x @ w1.t() + b1)
    kept = (hid2 != 0).double()
    dropped = float(((pre > 0) & (hid == 0)).double().sum() / (pre > 0).double().sum())
    print("dropped share of the positive hidden units: %.3f" % dropped)
    assert 0.03 < dropped < 0.25  # the mask is a p = 0.1 dropout mask and not, say, all ones
    _check_hidden(hid, pre * kept * a1, "hidden (dropout)")
    assert rel_l2(out, hid.double() @ w2.t()) < 1e-4
    assert rel_l2(out, out2) < 1e-4 + 2e-3  # the two hidden tensors are each within 2e-3 of fp64
    assert torch.equal(dz == 0, dz2 == 0)
    _check_hidden(dz, torch.where(hid.double() > 0, (dy @ w2) * a1, torch.zeros((), dtype=torch.float64)), "dz (dropout)")
    assert rel_l2(dx, dz.double() @ w1 + res) < 1e-4
    assert rel_l2(dx, dx2) < 1e-4 + 2e-3


@pytest.mark.parametrize("backend", BACKENDS)
def test_declined_shapes_leave_the_outputs_untouched(backend):
    import kantts._hip as hip
    from kantts._hip.ops_bf16 import frag_major

    m = 40
    g = torch.Generator().manual_seed(3)
    with _backend(backend) as dev:
        def call(k1, n, f, **kw):
            x = torch.randn(m, k1, generator=g).to(dev)
            kt = kw.get("KT", 1)
            w1 = frag_major(torch.randn(kt * f, k1, generator=g).to(dev))
            w2 = frag_major(torch.randn(n, f, generator=g).to(dev))
            out = torch.full((m, n), 7.0, device=dev)
            hid = torch.full((m, f), 7.0, device=dev, dtype=BF)
            if kw.pop("with_ln", False):
                kw["ln"] = (torch.ones(n, device=dev), torch.zeros(n, device=dev), 1e-6, torch.full((m, n), 7.0, device=dev),
                            torch.full((m,), 7.0, device=dev), torch.full((m,), 7.0, device=dev))
            ok = hip.ffn_pair(x, w1, w2, out, M=m, T=m, F=f, relu=True, t_out=hid, **kw)
            touched = bool((out != 7.0).any() or (hid != 7.0).any())
            if "ln" in kw:
                touched = touched or any(bool((t != 7.0).any()) for t in kw["ln"][3:])
            return ok, touched

        assert call(256, 256, 1024) == (False, False)                # not an instantiated geometry
        assert call(256, 256, 512, KT=3, pad=1) == (False, False)    # taps at 256 wide
        assert call(256, 256, 512, with_ln=True) == (False, False)   # the LayerNorm epilogue is LayerNorm(128)
        assert call(256, 256, 512)[0] and call(128, 128, 256)[0]     # (the plain calls are taken)


def _encoder_run(dev, args, pair_on):
    """FsmnEncoderV2 forward + backward in bf16 mode, training; returns (output, input gradient, parameter gradients)
    and the launches counted per feed-forward net."""
    import kantts._hip as hip
    from kantts._hip import ops, ops_bf16
    from kantts.models.sambert.fsmn import FsmnEncoderV2

    B, T, lens = 3, 37, [37, 28, 1]
    torch.manual_seed(7)
    enc = FsmnEncoderV2(*args).to(dev).train()
    g = torch.Generator().manual_seed(8)
    x = torch.randn(B, T, args[2], generator=g).to(dev).requires_grad_(True)
    cot = torch.randn(B, T, args[3], generator=g).to(dev)
    mask = (torch.arange(T)[None, :] >= torch.tensor(lens)[:, None]).to(dev)
    calls = []
    real_pair, real_nt = ops_bf16.ffn_pair, ops_bf16.bgemm_nt

    def pair(*a, **kw):
        ok = real_pair(*a, **kw)
        calls.append(("pair", bool(ok), int(a[0].shape[-1]), "bwd" if kw.get("gate") is not None else "fwd"))
        return ok

    def nt(*a, **kw):
        calls.append(("nt",))
        return real_nt(*a, **kw)

    prev = hip.get_precision()
    ops_bf16.PAIR["fsmn"], ops_bf16.ffn_pair, ops_bf16.bgemm_nt = pair_on, pair, nt
    hip.set_precision("bf16")
    ops._seed_counter = itertools.count(900)
    hip.rng_state(dev).zero_()
    try:
        y = enc(x, mask)
        n_fwd = len(calls)
        grads = torch.autograd.grad((y * cot).sum(), [x] + list(enc.parameters()))
    finally:
        ops_bf16.PAIR["fsmn"], ops_bf16.ffn_pair, ops_bf16.bgemm_nt = True, real_pair, real_nt
        hip.set_precision(prev)
    names = ["output", "d input"] + ["d " + k for k, _ in enc.named_parameters()]
    return names, [y.detach().cpu()] + [q.detach().cpu() for q in grads], calls[:n_fwd], calls[n_fwd:]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("args", [(41, 3, 80, 256, 512, 0.1, 17), (41, 3, 96, 128, 256, 0.1, 0)], ids=["postnet", "predictor"])
def test_encoder_with_the_pair_equals_the_two_launch_form(backend, args):
    """PAIR["fsmn"] on against off, seeds reset: output, input gradient and every parameter gradient to rel-L2 < 1e-3 (at
    most the 2 % cap of one-ulp flips, 2^-8, in a hidden tensor: sqrt(0.02) * 3.9e-3 = 5.5e-4 per layer).  Layers 2-3 take one
    kantts_ffn_pair each way, layer 1 (80 / 96 wide) the two kantts_bgemm_nt launches inside the same node."""
    with _backend(backend) as dev:
        names, on, fwd_calls, bwd_calls = _encoder_run(dev, args, True)
        _, off, fwd_off, bwd_off = _encoder_run(dev, args, False)
    width = args[3]
    for calls, way in ((fwd_calls, "fwd"), (bwd_calls, "bwd")):
        pairs = [c for c in calls if c[0] == "pair"]
        assert pairs == [("pair", True, width, way)] * 2, (way, pairs)       # layers 2-3: one launch each, accepted
        assert sum(c[0] == "nt" for c in calls) == 2, (way, calls)            # layer 1: the two-launch fallback
    assert not any(c[0] == "pair" for c in fwd_off + bwd_off)
    assert sum(c[0] == "nt" for c in fwd_off) == 6 and sum(c[0] == "nt" for c in bwd_off) == 6
    worst = 0.0
    for name, a, b in zip(names, on, off):
        r = rel_l2(a, b)
        worst = max(worst, r)
        print("%-40s rel-L2 on / off %.3e" % (name, r))
        assert r < 1e-3, (name, r)
    print("worst rel-L2 on / off: %.3e" % worst)
