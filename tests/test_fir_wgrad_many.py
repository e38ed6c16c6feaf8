"""kantts_fsmn_dw41_many: the 41-tap filter gradient of many memory blocks in two launches, and the host path that records
the problems of a backward pass and issues them at the flush of the deferred weight gradients.

The many-problem launches run, per problem, the workgroup bodies of the single-problem launches with that problem's
operands, so the oracle is ``kantts_fsmn_dwconv_bwd(dx = NULL)`` on the same back end and every comparison is BIT FOR BIT
(int32 views).  Every case runs on the kernel SOURCES compiled for the host (tests/hipemu, unmarked) and on the device
(``gpu``).  Buffers are oversized and NaN-filled behind their bound (a write past it, or a word left unwritten in front of
it, shows as a difference); ``dw`` starts from non-zero values (the reduce adds); rows of dy / x at or after a sequence's
length hold NaN (they must not be read into the result).
"""
import contextlib
import ctypes
import itertools

import pytest
import torch

from util import kernel_source_on_cpu

BACKENDS = ["hostsim", pytest.param("gpu", marks=pytest.mark.gpu)]
K, PAD = 41, 257
E_BADARG, E_WORKSPACE = -1, -3
# (B, T, C, left_pad, lens | None)
SHAPES = [
    (2, 130, 64, 20, (130, 77)),   # crosses the 128-frame chunk and leaves a 2-frame tail
    (3, 37, 128, 40, (37, 20, 0)),  # an empty sequence
    (1, 1, 256, 0, None),          # one frame, no lengths
    (2, 64, 72, 20, (64, 64)),     # a ragged channel group (72 = 64 + 8)
    (2, 50, 64, 17, (90, 13)),     # a length above T: clamped to T
]


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
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(_bits(a), _bits(b)), "%s: the many-problem call and the single call differ" % what


def _sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


class _Problem:
    """Operands of one filter gradient (host copies) and fresh device buffers per run."""

    def __init__(self, shape, seed):
        import kantts._hip as hip

        self.B, self.T, self.C, self.lp, lens = shape
        g = torch.Generator().manual_seed(seed)
        self.dy = torch.randn(self.B, self.T, self.C, generator=g)
        self.x = torch.randn(self.B, self.T, self.C, generator=g)
        self.lens = None if lens is None else torch.tensor(lens, dtype=torch.int64)
        for b, n in enumerate(lens or ()):
            self.dy[b, min(n, self.T):] = float("nan")
            self.x[b, min(n, self.T):] = float("nan")
        self.dw0 = torch.randn(self.C * K, generator=g) + 3.0  # (non-zero: the reduce adds)
        self.ws_n = int(hip.lib().kantts_fsmn_dwconv_bwd_ws(self.B, self.T, self.C, K))
        assert self.ws_n == self.B * ((self.T + 127) // 128) * self.C * K

    def on(self, dev):
        """(dy, x, lens, dw view (C, K), dw buffer, ws buffer) on ``dev``; dw / ws NaN-filled behind their bounds."""
        dwbuf = torch.full((self.C * K + PAD,), float("nan"))
        dwbuf[:self.C * K] = self.dw0
        dwbuf = dwbuf.to(dev)
        ws = torch.full((self.ws_n + PAD,), float("nan"), device=dev)
        lens = None if self.lens is None else self.lens.to(dev)
        return self.dy.to(dev), self.x.to(dev), lens, dwbuf[:self.C * K].view(self.C, K), dwbuf, ws

    def single(self, dev):
        import kantts._hip as hip

        dy, x, lens, dw, dwbuf, ws = self.on(dev)
        w = torch.zeros(self.C, K, device=dev)  # (the filter itself: only the input gradient reads it)
        rc = hip.lib().kantts_fsmn_dwconv_bwd(hip.ptr(dy), hip.ptr(x), hip.ptr(w), hip.ptr(lens), None, hip.ptr(dw),
                                              hip.ptr(ws), self.ws_n, self.B, self.T, self.C, K, self.lp, hip.stream())
        assert rc == 0
        _sync(dev)
        return dwbuf, ws

    def entry(self, bufs):
        dy, x, lens, dw, _, ws = bufs
        return (dy, x, lens, dw, ws, self.ws_n, self.B, self.T, self.C, self.lp)

    def check(self, bufs, ref, what):
        """The buffers of a many-problem run against those of the single call: result, workspace and both NaN tails."""
        dwbuf, ws = bufs[4], bufs[5]
        _same_bits(dwbuf, ref[0], what + " dw")
        _same_bits(ws, ref[1], what + " workspace")
        n = self.C * K
        assert not torch.isnan(dwbuf[:n]).any() and torch.isnan(dwbuf[n:]).all(), what
        assert not torch.isnan(ws[:self.ws_n]).any() and torch.isnan(ws[self.ws_n:]).all(), what
        assert not torch.equal(dwbuf[:n].cpu(), self.dw0), what  # (something was added)


def _problems(n, seed=0):
    return [_Problem(SHAPES[i % len(SHAPES)], 1000 * seed + i) for i in range(n)]


def _struct_array(entries):
    import kantts._hip as hip

    arr = (hip.FirDwProblem * max(len(entries), 1))()
    for g, (dy, x, lens, dw, ws, ws_n, B, T, C, lp) in zip(arr, entries):
        g.dy, g.x, g.lens, g.dw_accum, g.workspace = hip.ptr(dy), hip.ptr(x), hip.ptr(lens), hip.ptr(dw), hip.ptr(ws)
        g.ws_floats, g.B, g.T, g.C, g.left_pad = ws_n, B, T, C, lp
    return arr


def test_cap_is_the_headers():
    import os
    import re

    import kantts._hip as hip
    from util import ROOT

    header = open(os.path.join(ROOT, "include", "kantts_hip.h")).read()
    cap = int(re.search(r"#define\s+KANTTS_FIR_DW_MAX\s+(\d+)", header).group(1))
    assert cap == hip.FIR_DW_MAX and cap >= 16
    assert ctypes.sizeof(hip.FirDwProblem) == 5 * 8 + 8 + 4 * 4


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("nprob", [1, 4, 16])
def test_one_call_equals_the_single_calls(backend, nprob):
    """nprob problems mixed in ONE call of the entry point (1, 4, the cap): shapes, left_pad, lengths and data differ."""
    import kantts._hip as hip

    assert hip.FIR_DW_MAX == 16
    with _backend(backend) as dev:
        probs = _problems(nprob, seed=nprob)
        refs = [p.single(dev) for p in probs]
        bufs = [p.on(dev) for p in probs]
        arr = _struct_array([p.entry(b) for p, b in zip(probs, bufs)])
        assert hip.lib().kantts_fsmn_dw41_many(arr, nprob, hip.stream()) == 0
        _sync(dev)
        for i, (p, b, r) in enumerate(zip(probs, bufs, refs)):
            p.check(b, r, "problem %d of %d" % (i, nprob))


@pytest.mark.parametrize("backend", BACKENDS)
def test_host_chunks_above_the_cap_and_at_a_repeated_dw(backend):
    """fir_dw_many with 19 problems (16 + 3), the last two adding into ONE dw: a repeated dw starts a new call, so its two
    adds are ordered as two single calls are."""
    import kantts._hip as hip

    with _backend(backend) as dev:
        probs = _problems(18, seed=7)
        refs = [p.single(dev) for p in probs]
        bufs = [p.on(dev) for p in probs]
        entries = [p.entry(b) for p, b in zip(probs, bufs)]
        again = probs[-1].on(dev)
        entries.append(probs[-1].entry(again[:3] + bufs[-1][3:5] + again[5:]))  # the same operands into the same dw again
        hip.fir_dw_many(entries)
        _sync(dev)
        for i, (p, b, r) in enumerate(zip(probs[:-1], bufs, refs)):
            p.check(b, r, "problem %d of 19" % i)
        p, n = probs[-1], probs[-1].C * K
        twice = p.on(dev)
        w = torch.zeros(p.C, K, device=dev)
        for _ in range(2):
            assert hip.lib().kantts_fsmn_dwconv_bwd(hip.ptr(twice[0]), hip.ptr(twice[1]), hip.ptr(w), hip.ptr(twice[2]), None,
                                                    hip.ptr(twice[3]), hip.ptr(twice[5]), p.ws_n, p.B, p.T, p.C, K, p.lp,
                                                    hip.stream()) == 0
        _sync(dev)
        _same_bits(bufs[-1][4], twice[4], "two adds into one dw")
        assert not torch.equal(_bits(twice[4][:n]), _bits(refs[-1][0][:n]))


@pytest.mark.parametrize("backend", BACKENDS)
def test_error_codes_and_skipped_problems(backend):
    import kantts._hip as hip

    with _backend(backend) as dev:
        L = hip.lib()
        probs = _problems(3, seed=3)
        bufs = [p.on(dev) for p in probs]
        entries = [p.entry(b) for p, b in zip(probs, bufs)]

        def run(es, n=None):
            rc = L.kantts_fsmn_dw41_many(_struct_array(es), len(es) if n is None else n, hip.stream())
            _sync(dev)
            return rc

        def untouched():
            return all(torch.equal(b[4][:p.C * K].cpu(), p.dw0) and torch.isnan(b[5]).all() for p, b in zip(probs, bufs))

        assert L.kantts_fsmn_dw41_many(None, 0, hip.stream()) == 0  # nothing to do, nothing launched
        assert run(entries, 0) == 0 and untouched()
        assert L.kantts_fsmn_dw41_many(None, 1, hip.stream()) == E_BADARG
        assert run(entries, hip.FIR_DW_MAX + 1) == E_BADARG and run(entries, -1) == E_BADARG
        for field in (0, 1, 3):  # dy, x, dw: a NULL operand in the LAST problem stops the whole call
            bad = list(entries)
            bad[2] = bad[2][:field] + (None,) + bad[2][field + 1:]
            assert run(bad) == E_BADARG and untouched()
        for field in (6, 7, 8):  # B, T negative; C zero
            bad = list(entries)
            bad[1] = bad[1][:field] + (0 if field == 8 else -1,) + bad[1][field + 1:]
            assert run(bad) == E_BADARG and untouched()
        short = list(entries)
        short[2] = short[2][:5] + (probs[2].ws_n - 1,) + short[2][6:]
        assert run(short) == E_WORKSPACE and untouched()
        nows = list(entries)
        nows[0] = nows[0][:4] + (None,) + nows[0][5:]
        assert run(nows) == E_WORKSPACE and untouched()
        # B == 0 / T == 0: skipped (no workspace needed), the others run
        skip = [entries[0][:4] + (None, 0, 0) + entries[0][7:], entries[1], entries[2][:4] + (None, 0, 1, 0) + entries[2][8:]]
        assert run(skip) == 0
        ref = probs[1].single(dev)
        probs[1].check(bufs[1], ref, "the problem between two skipped ones")
        for i in (0, 2):
            assert torch.equal(bufs[i][4][:probs[i].C * K].cpu(), probs[i].dw0) and torch.isnan(bufs[i][5]).all()


# ---------------------------------------------------------------------------------------------- autograd path
class _FlushHere(torch.autograd.Function):
    """Identity; backward flushes the deferred weight gradients (what ops.wgrad_flush_point does through the side stream,
    for the host back end, which has no streams)."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        import kantts._hip as hip

        hip.deferred_tn.flush()
        return g


AB, AT, AC = 3, 150, 72
ALENS = (150, 41, 0)


def _run_stack(dev, mode):
    """A plain memory block, a memory block with dropouts and residual, and the two-problem form of the pitch / energy
    predictors on top; ``mode``: "off" (every filter gradient at its layer), "on" (recorded, issued at the join), "mid" (a
    flush point between the pair and the two layers below it).  Returns every gradient and how many problems were pending
    after backward()."""
    import kantts._hip as hip
    import kantts._hip.ops as ops

    g = torch.Generator().manual_seed(21)
    x = torch.randn(AB, AT, AC, generator=g).to(dev).requires_grad_(True)
    ws = [(torch.randn(AC, K, generator=g) * 0.1).to(dev).requires_grad_(True) for _ in range(4)]
    cots = [torch.randn(AB, AT, AC, generator=g).to(dev) for _ in range(2)]
    lens = torch.tensor(ALENS, dtype=torch.int64, device=dev)
    ops._seed_counter = itertools.count(1000)
    hip.rng_state(dev).zero_()
    gpu = dev != "cpu"
    try:
        if mode != "off":
            if gpu:
                ops.wgrad_overlap.enable(True)  # side stream + deferred weight gradients, as the captured step has them
            else:
                hip.deferred_tn.enabled = True
        y = ops.fsmn_memory(x, ws[0], lens, 20)
        y = ops.fsmn_memory_drop(y, ws[1], lens, 20, 0.1, 0.2, res=y)
        if mode == "mid":
            y = ops.wgrad_flush_point(y) if gpu else _FlushHere.apply(y)
        ya, yb = ops.fsmn_memory_drop2([y, y * 0.5], [ws[2], ws[3]], lens, 40, [(0.1, 11, 0.1, 12), (0.3, 13, 0.0, 0)],
                                       ress=(y, None))
        ((ya * cots[0]).sum() + (yb * cots[1]).sum()).backward()
        pending = len(hip.deferred_tn.firs)
        ops.wgrad_overlap.join()
        assert not hip.deferred_tn.firs
        _sync(dev)
    finally:
        hip.deferred_tn.discard()
        if gpu:
            ops.wgrad_overlap.enable(False)
        hip.deferred_tn.enabled = False
    return [x.grad] + [w.grad for w in ws], pending


@pytest.mark.parametrize("backend", BACKENDS)
def test_recorded_filter_gradients_equal_the_in_line_ones(backend):
    """Every gradient of the stack bit for bit, deferred_tn off / on / on with a flush in the middle of backward."""
    import kantts._hip as hip

    with _backend(backend) as dev:
        assert hip.fir_dw_many_entry_point() and hip.predictor_pair_entry_points()
        ref, n_off = _run_stack(dev, "off")
        on, n_on = _run_stack(dev, "on")
        mid, n_mid = _run_stack(dev, "mid")
        assert (n_off, n_on, n_mid) == (0, 4, 2)  # the pair's two problems left at the flush point
        for name, a, b, c in zip(["x", "w0", "w1", "wa", "wb"], ref, on, mid):
            assert float(a.abs().max()) > 0 and not torch.isnan(a).any(), name
            _same_bits(a, b, name + " (recorded)")
            _same_bits(a, c, name + " (recorded, flushed in the middle)")
