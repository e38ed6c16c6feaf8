"""The backward chain of a stack of PNCA decoder blocks at the benchmark shape (B = 32, L = 204: M = 6528 rows), dropout on,
alone on the chip: one launch per half (2 n launches: pnca_block_bwd, pnca_attn_qkv_bwd per block) against the seam form
(n + 1 launches: the cross-row half of block i and the row-local half of block i - 1 in one, csrc/pnca_block.hip:
pnca_bwd_seam_kernel).  Forward and backward pass are captured in a hipGraph each; only the backward graph is timed.  Weight
gradients and the LayerNorm row sums are recorded (deferred_tn) and dropped, the accumulators come from the zero pool: what
is replayed is the chain of input-gradient launches and nothing else.  The two forms alternate, `rounds` times.
Usage: python scripts/pnca_bwd_chain_bench.py [reps] [rounds]"""
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "kan-tts_amd")]
import torch  # noqa: E402

import kantts._hip as hip  # noqa: E402
import kantts._hip.ops as ops  # noqa: E402
import kantts._hip.ops_bf16 as ops_bf16  # noqa: E402
from kantts.models.sambert import PNCABlock  # noqa: E402
from kantts.models.utils import SeqInfo  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
dev = "cuda"
hip.set_precision("bf16")
torch.manual_seed(0)
B, L, NB = 32, 204, 12
blocks = torch.nn.ModuleList([PNCABlock(128, 160, 8, 16, 1024, (1, 1), 0.1, 0.1, 0.1) for _ in range(NB)]).to(dev).train()
final_ln = torch.nn.LayerNorm(128, eps=1e-6).to(dev)
g = torch.Generator().manual_seed(1)
x0 = torch.randn(B, L, 128, generator=g).to(dev)
hkv = torch.randn(B, L, NB * 256, generator=g).to(dev)
cot = torch.randn(B, L, 128, generator=g).to(dev)
lens = torch.tensor([204 - 3 * i for i in range(B)], device=dev)
info = SeqInfo(lens, L)
ops.zero_pool.enable(1 << 24, dev)
if not hip.pnca_bwd_seam_entry_point():
    print("the loaded library has no kantts_pnca_bwd_seam: both columns are the two-launch form")


def forward(n):
    x = x0.clone().requires_grad_(True)
    h = x * 1.0
    for i in range(n):
        nxt = blocks[i + 1].pnca_attn.layer_norm if i + 1 < n else final_ln
        h, _, _ = blocks[i](h, None, mask=info, x_band_width=5, h_band_width=5, hkv=hkv[:, :, 256 * i:256 * (i + 1)],
                            private_input=i > 0, next_ln=nxt)
    return x, h


def captured_backward(n, seam):
    """(hipGraph of the backward pass of an n-block stack, launches counted on the host, dx)."""
    ops_bf16.PNCA_BWD_SEAM["on"] = seam
    counts = dict(block=0, attn=0, seam=0)
    real = (ops_bf16.pnca_block_bwd, hip.pnca_attn_qkv_bwd, hip.pnca_bwd_seam)

    def counted(key, fn):
        def call(*a, **k):
            counts[key] += 1
            return fn(*a, **k)
        return call

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(2):  # warm the allocator and the weight images
            x, y = forward(n)
            (dx,) = torch.autograd.grad(y, x, cot)
        torch.cuda.synchronize()
        ops.zero_pool.reset()
        # The forward pass is captured too, into a graph of its own whose memory pool the backward graph shares: what backward
        # reads (the saved activations) then lives in the graphs' private pool for as long as the graphs do.  (Activations of an
        # eager forward pass are released when the captured backward drops them, and the next capture empties the allocator's
        # cache: a replay would read unmapped memory.)  Replays alternate forward, backward; only the backward graph is timed.
        ops._seed_counter = itertools.count(1000)  # both forms draw the same dropout masks
        gf = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gf, stream=s):
            x, y = forward(n)
        ops_bf16.pnca_block_bwd, hip.pnca_attn_qkv_bwd = counted("block", real[0]), counted("attn", real[1])
        hip.pnca_bwd_seam = counted("seam", real[2])
        hip.deferred_tn.enabled = True
        try:
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, pool=gf.pool(), stream=s):
                (dx,) = torch.autograd.grad(y, x, cot)
        finally:
            hip.deferred_tn.discard()
            hip.deferred_tn.enabled = False
            ops_bf16.pnca_block_bwd, hip.pnca_attn_qkv_bwd, hip.pnca_bwd_seam = real
            ops_bf16.PNCA_BWD_SEAM["on"] = True
    return (gf, gr), s, counts, dx, (x, y)


def replay(graphs, s, n_rep):
    """Mean time of the backward graph over n_rep replays of (forward graph, backward graph), us."""
    gf, gr = graphs
    with torch.cuda.stream(s):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n_rep)]
        for e0, e1 in ev:
            gf.replay()
            e0.record()
            gr.replay()
            e1.record()
        torch.cuda.synchronize()
    return sum(e0.elapsed_time(e1) for e0, e1 in ev) / n_rep * 1e3


for n in (2, 12):
    off, on = captured_backward(n, False), captured_backward(n, True)
    replay(off[0], off[1], 3)
    replay(on[0], on[1], 3)
    same = torch.equal(off[3].view(torch.int32), on[3].view(torch.int32))
    print("blocks %2d  two launches per block: %s   seam: %s   dx bit-equal: %s" % (n, off[2], on[2], same))
    for r in range(rounds):
        t_off, t_on = replay(off[0], off[1], reps), replay(on[0], on[1], reps)
        seams = max(1, on[2]["seam"])
        print("blocks %2d round %d  two launches per block %8.1f us   seam form %8.1f us   saved %6.1f us = %5.2f us per seam"
              % (n, r, t_off, t_on, t_off - t_on, (t_off - t_on) / seams))
