"""The two-problem launches of the pitch / energy predictors and the lockstep path built on them.

Every case runs on the kernel SOURCES compiled for the host (tests/hipemu, unmarked) and on the device (``gpu``).
A pair launch runs, per problem, the code of its single launch with that problem's operands, so the oracle of every entry
point is its two single launches on the same back end, compared BIT FOR BIT on oversized NaN-filled buffers (a row written
past M, or left unwritten below it, shows as a difference).  The two problems always differ in weights, inputs, dropout
probabilities and seeds.
"""
import contextlib
import ctypes
import itertools

import pytest
import torch

from util import kernel_source_on_cpu, rel_l2

BF = torch.bfloat16
BACKENDS = ["hostsim", pytest.param("gpu", marks=pytest.mark.gpu)]
MS = [5, 31, 32, 33, 83]  # tail only, one row short of the 32-row tile, the tile, one row into the next, ragged
PAD = 3
B, T, LENS = 3, 37, (37, 20, 1)


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


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(_bits(a), _bits(b)), "%s: the pair launch and the single launch differ" % what


def _nan(shape, dev, dtype=torch.float32):
    return torch.full(shape, float("nan"), device=dev, dtype=dtype)


def _rand(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


# ---------------------------------------------------------------------------------------------- kantts_bgemm_nt_pair
def _bgemm_problems(kind, m, dev, seed):
    """Two problems of one form; returns [(segs, M, N, c, ldc, kwargs)] x 2 factories over fresh NaN-filled outputs."""
    g = torch.Generator().manual_seed(seed)
    probs = []
    for i in range(2):
        if kind == "up":  # FSMN first layer: fp32 A (96 wide), ReLU, bias, dropout, bf16 result
            x, w, b = _rand(g, m, 96).to(dev), _rand(g, 256, 96, scale=0.1).to(BF).to(dev), _rand(g, 256).to(dev)
            kw = dict(bias=b, relu=True, drop_p=(0.1, 0.3)[i], drop_seed=(77, 4242)[i])
            probs.append(lambda x=x, w=w, kw=kw: ([(x, 96, w, 96, 96, 0)], m, 256, _nan((m + PAD, 256), dev, BF), 256, kw))
        elif kind == "proj":  # LSTM input projection: 128 -> 512 with bias, written into half of a (M, 1024) buffer
            x, w, b = _rand(g, m, 128).to(dev), _rand(g, 512, 128, scale=0.1).to(BF).to(dev), _rand(g, 512).to(dev)
            probs.append(lambda x=x, w=w, b=b, i=i: ([(x, 128, w, 128, 128, 0)], m, 512,
                                                     (_nan((m + PAD, 1024), dev), 512 * i), 1024, dict(bias=b)))
        else:  # LSTM input gradient: b_kn, a K segment per direction, fp32 residual
            d0, d1 = _rand(g, m, 512).to(dev), _rand(g, m, 512).to(dev)
            w0, w1 = (_rand(g, 512, 128, scale=0.1).to(BF).to(dev) for _ in range(2))
            r = _rand(g, m, 128).to(dev)
            probs.append(lambda d0=d0, d1=d1, w0=w0, w1=w1, r=r: (
                [(d0, 512, w0, 128, 512, 0), (d1, 512, w1, 128, 512, 0)], m, 128, _nan((m + PAD, 128), dev), 128,
                dict(b_kn=True, res=r, ldr=128)))
    return probs


def _out_of(c):
    return c[0] if isinstance(c, tuple) else c


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("kind", ["up", "proj", "dx"])
def test_bgemm_nt_pair_equals_two_single_launches(backend, kind, m):
    import kantts._hip as hip

    with _backend(backend) as dev:
        probs = _bgemm_problems(kind, m, dev, 100 + m)
        single = [p() for p in probs]
        for s in single:
            assert hip.bgemm_nt(*s[:5], **s[5])
        pair = [p() for p in probs]
        assert hip.bgemm_nt_pair(*pair)
        for i, (s, q) in enumerate(zip(single, pair)):
            _same_bits(_out_of(s[3]), _out_of(q[3]), "%s, problem %d" % (kind, i))
            rows = _out_of(s[3])[:m].float()
            live = rows[:, 512 * i:512 * i + 512] if kind == "proj" else rows
            assert not torch.isnan(live).any() and torch.isnan(_out_of(s[3])[m:].float()).all()
        assert not torch.equal(_bits(_out_of(pair[0][3])), _bits(_out_of(pair[1][3])))  # (two different problems)


@pytest.mark.parametrize("backend", BACKENDS)
def test_bgemm_nt_pair_declines_unequal_problems(backend):
    import kantts._hip as hip

    with _backend(backend) as dev:
        a = _bgemm_problems("proj", 33, dev, 1)[0]()
        for other in (_bgemm_problems("proj", 32, dev, 2)[1](),   # another M
                      _bgemm_problems("up", 33, dev, 3)[1](),     # another N
                      _bgemm_problems("dx", 33, dev, 4)[1]()):    # another operand form (b_kn)
            assert hip.bgemm_nt_pair(a, other) is False
            assert torch.isnan(_out_of(a[3])).all() and torch.isnan(_out_of(other[3]).float()).all()


# ---------------------------------------------------------------------------------------------- kantts_ffn_pair2
def _ffn_operands(m, seed):
    g = torch.Generator().manual_seed(seed)
    rb = lambda t: t.to(BF).float()  # noqa: E731
    return [dict(x=rb(_rand(g, m, 128)), w1=rb(_rand(g, 256, 128, scale=0.08)), w2=rb(_rand(g, 128, 256, scale=0.05)),
                 b1=_rand(g, 256, scale=0.3), dy=rb(_rand(g, m, 128)), res=_rand(g, m, 128)) for _ in range(2)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("m", MS)
def test_ffn_pair2_equals_two_single_launches(backend, m):
    import kantts._hip as hip
    from kantts._hip.ops_bf16 import frag_major

    ops_ = _ffn_operands(m, 500 + m)
    ps, seeds, a1s = (0.1, 0.25), (4242 + m, 17), (1.0 / 0.9, 1.0 / 0.75)
    with _backend(backend) as dev:
        def fwd(i):
            o = ops_[i]
            out, hid = _nan((m + PAD, 128), dev), _nan((m + PAD, 256), dev, BF)
            return ((o["x"].to(dev), frag_major(o["w1"].to(dev)), frag_major(o["w2"].to(dev)), out),
                    dict(M=m, T=m, F=256, bias1=o["b1"].to(dev), relu=True, drop1_p=ps[i], drop1_seed=seeds[i], t_out=hid))

        single, pair = [fwd(0), fwd(1)], [fwd(0), fwd(1)]
        for a, kw in single:
            assert hip.ffn_pair(*a, **kw)
        assert hip.ffn_pair2(*pair)
        for i in range(2):
            _same_bits(single[i][0][3], pair[i][0][3], "forward output, problem %d" % i)
            _same_bits(single[i][1]["t_out"], pair[i][1]["t_out"], "hidden, problem %d" % i)
            assert torch.isnan(pair[i][0][3][m:]).all() and not torch.isnan(pair[i][0][3][:m]).any()
        hids = [single[i][1]["t_out"][:m].contiguous() for i in range(2)]
        assert 0.03 < float((hids[0] == 0).float().mean()) < 0.97  # ReLU and dropout zeros, not a constant tensor

        def bwd(i):
            o = ops_[i]
            dx, dz = _nan((m + PAD, 128), dev), _nan((m + PAD, 256), dev, BF)
            return ((o["dy"].to(dev), frag_major(o["w2"].t().contiguous().to(dev)), frag_major(o["w1"].t().contiguous().to(dev)),
                     dx), dict(M=m, T=m, F=256, alpha1=a1s[i], gate=hids[i], t_out=dz, res=o["res"].to(dev)))

        single, pair = [bwd(0), bwd(1)], [bwd(0), bwd(1)]
        for a, kw in single:
            assert hip.ffn_pair(*a, **kw)
        assert hip.ffn_pair2(*pair)
        for i in range(2):
            _same_bits(single[i][0][3], pair[i][0][3], "dx, problem %d" % i)
            _same_bits(single[i][1]["t_out"], pair[i][1]["t_out"], "dz, problem %d" % i)
            assert torch.isnan(pair[i][0][3][m:]).all() and not torch.isnan(pair[i][0][3][:m]).any()
        # a forward and a backward problem, or two row counts, do not share a launch
        f0, b1 = fwd(0), bwd(1)
        assert hip.ffn_pair2(f0, b1) is False
        assert torch.isnan(f0[0][3]).all() and torch.isnan(b1[0][3]).all()


@pytest.mark.parametrize("backend", BACKENDS)
def test_ffn_pair2_declines_other_geometries_and_unequal_rows(backend):
    import kantts._hip as hip
    from kantts._hip.ops_bf16 import frag_major

    g = torch.Generator().manual_seed(9)
    with _backend(backend) as dev:
        def prob(m, k1, n, f):
            out = _nan((m, n), dev)
            return ((_rand(g, m, k1).to(dev), frag_major(_rand(g, f, k1).to(dev)), frag_major(_rand(g, n, f).to(dev)), out),
                    dict(M=m, T=m, F=f, relu=True))

        for a, b in ((prob(40, 128, 128, 256), prob(41, 128, 128, 256)), (prob(40, 256, 256, 512), prob(40, 256, 256, 512))):
            assert hip.ffn_pair2(a, b) is False
            assert torch.isnan(a[0][3]).all() and torch.isnan(b[0][3]).all()


# ---------------------------------------------------------------------------------------------- fsmn_memory_drop_*_pair
@pytest.mark.parametrize("backend", BACKENDS)
def test_fsmn_memory_drop_pairs_equal_two_single_launches(backend):
    import kantts._hip as hip
    from kantts._hip import ops

    C, K, lp = 128, 41, 20
    g = torch.Generator().manual_seed(41)
    host = [dict(c=_rand(g, B, T, C), w=_rand(g, C, K, scale=0.1), res=_rand(g, B, T, C), dy=_rand(g, B, T, C)) for _ in range(2)]
    cfgs = [(0.1, 11, 0.2, 12), (0.3, 913, 0.05, 7)]  # (p1, seed1, p2, seed2): both dropouts on, all different
    with _backend(backend) as dev:
        lens = torch.tensor(LENS, dtype=torch.int64, device=dev)
        t = [{k: v.to(dev) for k, v in h.items()} for h in host]
        rng = hip.rng_ptr(torch.device(dev))
        L = ops.lib()
        ys = [_nan((B + 1, T, C), dev) for _ in range(2)]
        for o, y, (p1, s1, p2, s2) in zip(t, ys, cfgs):
            assert L.kantts_fsmn_memory_drop_fwd(ops.ptr(o["c"]), ops.ptr(o["w"]), ops.ptr(o["res"]), ops.ptr(lens), ops.ptr(y),
                                                 B, T, C, K, lp, p1, s1, p2, s2, rng, ops.stream()) == 0
        ys2 = [_nan((B + 1, T, C), dev) for _ in range(2)]
        a, b = (ops._fsmn_drop_args(o["c"], o["w"], o["res"], y, None, *cfg) for o, y, cfg in zip(t, ys2, cfgs))
        assert L.kantts_fsmn_memory_drop_fwd_pair(ctypes.byref(a), ctypes.byref(b), ops.ptr(lens), B, T, C, K, lp, rng,
                                                  ops.stream()) == 0
        for i in range(2):
            _same_bits(ys[i], ys2[i], "forward, problem %d" % i)
            assert torch.isnan(ys2[i][B:]).all() and not torch.isnan(ys2[i][:B]).any()
        assert not torch.equal(_bits(ys2[0]), _bits(ys2[1]))
        dxs, dyms = ([_nan((B + 1, T, C), dev) for _ in range(2)] for _ in range(2))
        for o, dx, dym, (p1, s1, p2, s2) in zip(t, dxs, dyms, cfgs):
            assert L.kantts_fsmn_memory_drop_bwd(ops.ptr(o["dy"]), ops.ptr(o["w"]), ops.ptr(lens), ops.ptr(dx), ops.ptr(dym), B, T,
                                                 C, K, lp, p1, s1, p2, s2, rng, ops.stream()) == 0
        dxs2, dyms2 = ([_nan((B + 1, T, C), dev) for _ in range(2)] for _ in range(2))
        a, b = (ops._fsmn_drop_args(o["dy"], o["w"], None, dx, dym, *cfg) for o, dx, dym, cfg in zip(t, dxs2, dyms2, cfgs))
        assert L.kantts_fsmn_memory_drop_bwd_pair(ctypes.byref(a), ctypes.byref(b), ops.ptr(lens), B, T, C, K, lp, rng,
                                                  ops.stream()) == 0
        for i in range(2):
            _same_bits(dxs[i], dxs2[i], "dx, problem %d" % i)
            _same_bits(dyms[i], dyms2[i], "dym, problem %d" % i)
            assert torch.isnan(dxs2[i][B:]).all() and not torch.isnan(dxs2[i][:B]).any()
            assert float((dyms2[i][1, LENS[1]:] != 0).sum()) == 0  # rows past a sequence's length are zero
        # a filter length the fused kernel does not have: declined before anything is launched
        a, b = (ops._fsmn_drop_args(o["dy"], o["w"], None, dx, dym, *cfg) for o, dx, dym, cfg in zip(t, dxs2, dyms2, cfgs))
        assert L.kantts_fsmn_memory_drop_bwd_pair(ctypes.byref(a), ctypes.byref(b), ops.ptr(lens), B, T, C, 11, 5, rng,
                                                  ops.stream()) == hip.E_UNSUPPORTED


# ---------------------------------------------------------------------------------------------- the recurrence
@pytest.mark.parametrize("backend", BACKENDS)
def test_bilstm_pair_equals_two_single_launches(backend):
    import kantts._hip as hip
    from kantts._hip import ops

    H, G = 128, 512
    g = torch.Generator().manual_seed(128)
    host = [dict(gx=_rand(g, B, T, 2 * G), whh=_rand(g, 2, G, H, scale=0.1), bhh=_rand(g, 2, G, scale=0.2),
                 dout=_rand(g, B, T, 2 * H)) for _ in range(2)]
    with _backend(backend) as dev:
        lens = torch.tensor(LENS, dtype=torch.int32, device=dev)
        t = [{k: v.to(dev) for k, v in h.items()} for h in host]
        L = ops.lib()

        def bufs():
            # one NaN-filled sequence more than the launch is told of: past sequence B - 1 of `out`, past (direction 1,
            # sequence B - 1) of the tensors indexed (direction, sequence, ...)
            return [dict(out=_nan((B + 1, T, 2 * H), dev), gates=_nan((2 * B + 1, T, G), dev), cst=_nan((2 * B + 1, T, H), dev),
                         dg=_nan((2 * B + 1, T, G), dev)) for _ in range(2)]

        s, q = bufs(), bufs()
        for o, u in zip(t, s):
            assert L.kantts_lstm_fwd(ops.ptr(o["gx"]), ops.ptr(o["whh"]), ops.ptr(o["bhh"]), ops.ptr(lens), ops.ptr(u["out"]),
                                     ops.ptr(u["gates"]), ops.ptr(u["cst"]), B, T, H, 2, 0, 1, ops.stream()) == 0
            assert L.kantts_lstm_bwd(ops.ptr(o["dout"]), ops.ptr(o["whh"]), ops.ptr(lens), ops.ptr(u["gates"]), ops.ptr(u["cst"]),
                                     ops.ptr(u["dg"]), B, T, H, 2, 0, 1, ops.stream()) == 0
        args = []
        for o, u in zip(t, q):
            a = hip.BiLstmArgs()
            a.gx, a.out, a.gates_save, a.c_save = ops.ptr(o["gx"]), ops.ptr(u["out"]), ops.ptr(u["gates"]), ops.ptr(u["cst"])
            a.dout, a.dgates = ops.ptr(o["dout"]), ops.ptr(u["dg"])
            for d in range(2):  # per-direction pointers: nothing is stacked for the pair
                a.whh[d], a.bhh[d] = ops.ptr(o["whh"][d]), ops.ptr(o["bhh"][d])
            args.append(a)
        assert L.kantts_bilstm_pair_fwd(ctypes.byref(args[0]), ctypes.byref(args[1]), ops.ptr(lens), B, T, H, 1, ops.stream()) == 0
        assert L.kantts_bilstm_pair_bwd(ctypes.byref(args[0]), ctypes.byref(args[1]), ops.ptr(lens), B, T, H, 1, ops.stream()) == 0
        for i in range(2):
            for k in ("out", "gates", "cst", "dg"):
                _same_bits(s[i][k], q[i][k], "%s, problem %d" % (k, i))
            out = q[i]["out"]
            assert torch.isnan(out[B:]).all() and not torch.isnan(out[:B]).any()
            assert float(out[1, LENS[1]:].abs().sum()) == 0 and float(out[1, :LENS[1]].abs().sum()) > 0
            assert not torch.isnan(q[i]["dg"][:2 * B]).any()  # (zeros at and after a sequence's length)
            for k in ("gates", "cst", "dg"):
                assert torch.isnan(q[i][k][2 * B:]).all(), k
        assert not torch.equal(_bits(q[0]["out"]), _bits(q[1]["out"]))
        # fp32 recurrent products have no two-problem form
        assert L.kantts_bilstm_pair_fwd(ctypes.byref(args[0]), ctypes.byref(args[1]), ops.ptr(lens), B, T, H, 0,
                                        ops.stream()) == hip.E_UNSUPPORTED


# ---------------------------------------------------------------------------------------------- the lockstep path
def _predictors_run(dev, paired):
    """Two predictors at the benchmark's widths, training mode, bf16; returns names and [pitch, energy, d input, d params]."""
    import kantts._hip as hip
    from kantts._hip import ops, ops_bf16
    from kantts.models.sambert.adaptors import VarFsmnRnnNARPredictor, paired_nar_predictors

    torch.manual_seed(5)
    mods = [VarFsmnRnnNARPredictor(96, 41, 3, 128, 256, 0.1, 0, 128).to(dev).train() for _ in range(2)]
    g = torch.Generator().manual_seed(6)
    x = torch.randn(B, T, 96, generator=g).to(dev).requires_grad_(True)
    cots = [torch.randn(B, T, generator=g).to(dev) for _ in range(2)]
    mask = (torch.arange(T)[None, :] >= torch.tensor(LENS)[:, None]).to(dev)
    calls = []
    real = {n: getattr(ops_bf16, n) for n in ("bgemm_nt_pair", "ffn_pair2", "bgemm_nt", "ffn_pair")}

    def counted(name):
        def f(*a, **kw):
            calls.append(name)
            return real[name](*a, **kw)
        return f

    prev = hip.get_precision()
    for n in real:
        setattr(ops_bf16, n, counted(n))
    ops_bf16.PAIR["predictors"] = paired
    hip.set_precision("bf16")
    ops._seed_counter = itertools.count(900)
    hip.rng_state(dev).zero_()
    try:
        p, e = paired_nar_predictors(mods[0], mods[1], x, mask)
        params = [q for m in mods for q in m.parameters()]
        grads = torch.autograd.grad((p * cots[0]).sum() + (e * cots[1]).sum(), [x] + params)
    finally:
        for n, f in real.items():
            setattr(ops_bf16, n, f)
        ops_bf16.PAIR["predictors"] = True
        hip.set_precision(prev)
    names = ["pitch", "energy", "d input"] + ["d %s.%s" % (w, k) for w, m in zip(("pitch", "energy"), mods)
                                                for k, _ in m.named_parameters()]
    return names, [t.detach().cpu() for t in (p, e) + tuple(grads)], calls


@pytest.mark.parametrize("backend", BACKENDS)
def test_paired_path_equals_the_two_separate_predictors(backend):
    """PAIR["predictors"] on against off, same seeds.  Predictions, the gradient of the shared input and the FIR filter
    gradients (partial sums + an ordered reduction: no float atomics) are the same bits.  Every other parameter gradient
    -- weights and biases alike -- leaves kantts_bgemm_tn or the segmented GEMM through fp32 atomics: held to the larger of
    three times the unpaired path's own run-to-run rel-L2, measured here, and 1e-6 (the rule of tests/test_ddp_gloo.py)."""
    with _backend(backend) as dev:
        names, off, calls_off = _predictors_run(dev, False)
        _, off2, _ = _predictors_run(dev, False)
        _, on, calls_on = _predictors_run(dev, True)
    # the lockstep path issues every contraction of the predictors' chain once for both: per way 2 + 2 first-layer
    # projections, 2 + 2 layer pairs, forward 2 LSTM input projections, backward 2 shares of the LSTM input gradient
    assert calls_on.count("bgemm_nt_pair") == 4 + 2 + 2 and calls_on.count("ffn_pair2") == 4, calls_on
    assert calls_on.count("bgemm_nt") == 0 and calls_on.count("ffn_pair") == 0, calls_on
    assert calls_off.count("bgemm_nt_pair") == 0 and calls_off.count("ffn_pair2") == 0, calls_off
    worst = 0.0
    for name, a, b, b2 in zip(names, on, off, off2):
        exact = name in ("pitch", "energy", "d input") or name.endswith("conv_dw.weight")
        noise = rel_l2(b, b2)
        r = rel_l2(a, b)
        print("%-52s on / off rel-L2 %.3e   off / off %.3e%s" % (name, r, noise, "   (bits)" if exact else ""))
        if exact:
            assert torch.equal(_bits(a), _bits(b)), name
        else:
            assert r <= max(3.0 * noise, 1e-6), (name, r, noise)
            worst = max(worst, r)
    print("worst on / off rel-L2 of the gradients that go through atomics: %.3e" % worst)
    assert float(on[0].abs().sum()) > 0 and float(on[2].abs().sum()) > 0


@pytest.mark.parametrize("backend", BACKENDS)
def test_other_modes_run_the_two_separate_calls(backend):
    """eval, fp32 mode and unequal modules do not take the paired launches."""
    import kantts._hip as hip
    from kantts._hip import ops_bf16
    from kantts.models.sambert.adaptors import VarFsmnRnnNARPredictor, _predictors_pairable

    with _backend(backend) as dev:
        torch.manual_seed(5)
        a, b = (VarFsmnRnnNARPredictor(96, 41, 3, 128, 256, 0.1, 0, 128).to(dev).train() for _ in range(2))
        c = VarFsmnRnnNARPredictor(96, 41, 3, 128, 256, 0.2, 0, 128).to(dev).train()
        x = torch.randn(B, T, 96).to(dev)
        prev = hip.get_precision()
        try:
            hip.set_precision("bf16")
            assert _predictors_pairable(a, b, x)
            assert not _predictors_pairable(a, c, x)  # another dropout probability
            with torch.no_grad():
                assert not _predictors_pairable(a, b, x)
            b.eval()
            assert not _predictors_pairable(a, b, x)
            b.train()
            ops_bf16.PAIR["predictors"] = False
            assert not _predictors_pairable(a, b, x)
            ops_bf16.PAIR["predictors"] = True
            hip.set_precision("fp32")
            assert not _predictors_pairable(a, b, x)
        finally:
            ops_bf16.PAIR["predictors"] = True
            hip.set_precision(prev)
