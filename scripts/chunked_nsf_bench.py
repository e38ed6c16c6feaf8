"""What the streamed NSF excitation costs a chunked vocoder step (ChunkedNSFVocoder, csrc/nsf_source.hip).

Shipped 24 kHz geometry (upsample_scales 8, 5, 3, 2, kernels 16, 10, 6, 4, 512 channels, 7 harmonics + fundamental, random
init), S = 4 slots, 8 frames per step, graph replay, one process.

  step        ChunkedNSFVocoder.step against ChunkedVocoder.step of the same generator built WITHOUT nsf_params (with
              --parent-lib PATH, a libkantts_hip.so built from the parent commit, the plain vocoder captures its graphs
              through that library).  The two legs alternate; a PAIR is --reps steps of each (host clock around step +
              synchronize), --pairs pairs; per leg the median over the pairs of the per-pair medians, and their range.
  launches    the two new launches alone (kantts_nsf_source_rows, kantts_nsf_downs_rows) and, for scale, the four up-layer
              launches they feed, each group captured as a graph of its own: device events around --burst back-to-back
              replays (time per replay), --pairs times.

    python scripts/chunked_nsf_bench.py [--parent-lib PATH] [--mode bf16|fp32]     # -> profiles/chunked_nsf.json
    python scripts/chunked_nsf_bench.py --trace     # 50 eager steps: the program of a rocprofv3 --kernel-trace --stats run
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kan-tts_amd"))
OUT = os.path.join(ROOT, "profiles", "chunked_nsf.json")
GEOM = dict(in_channels=80, channels=512, upsample_scales=[8, 5, 3, 2], upsample_kernal_sizes=[16, 10, 6, 4])
NSF = {"nb_harmonics": 7, "sampling_rate": 24000}
S, TC = 4, 8


def _spread(ts):
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--burst", type=int, default=200)
    ap.add_argument("--mode", default="bf16")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--copy-to", default=None, help="directory that also receives the JSON")
    args = ap.parse_args()

    import torch

    import kantts._hip as hip
    from kantts.models.hifigan.chunked import ChunkedVocoder
    from kantts.models.hifigan.chunked_nsf import ChunkedNSFVocoder
    from kantts.models.hifigan.hifigan import Generator

    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    hip.set_precision(args.mode)
    torch.manual_seed(0)
    G_nsf = Generator(nsf_params=NSF, **GEOM).eval().cuda()
    torch.manual_seed(0)
    G_plain = Generator(**GEOM).eval().cuda()
    g = torch.Generator().manual_seed(1)
    feats = torch.randn(S, 82, TC, generator=g)
    feats[:, -2] = 80.0 + 300.0 * torch.rand(S, TC, generator=g)
    feats[:, -1] = (torch.rand(S, TC, generator=g) > 0.3).float()
    feats = feats.cuda()
    mel = feats[:, :80].contiguous()

    if args.trace:
        v = ChunkedNSFVocoder(G_nsf, slots=S, graph=False)
        with torch.no_grad():
            for _ in range(50):
                v.step(feats)
        torch.cuda.synchronize()
        return

    mine = hip.lib()
    if args.parent_lib:
        parent = ctypes.CDLL(args.parent_lib)
        for name in hip.EXPORTED_SYMBOLS:
            if hasattr(parent, name):
                fn, ref = getattr(parent, name), getattr(mine, name)
                fn.argtypes, fn.restype = ref.argtypes, ref.restype
        hip._lib = parent  # every wrapper goes through hip.lib(), which hands out this global
    plain = ChunkedVocoder(G_plain, slots=S, graph=True)
    with torch.no_grad():
        plain.step(mel), plain.step(mel)  # captured through the parent's library; replays need no library
    hip._lib = mine
    nsf = ChunkedNSFVocoder(G_nsf, slots=S, graph=True)
    with torch.no_grad():
        nsf.step(feats), nsf.step(feats)

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    legs = dict(plain=lambda: plain.step(mel), nsf=lambda: nsf.step(feats))
    per_pair = {k: [] for k in legs}
    with torch.no_grad():
        for fn in legs.values():
            for _ in range(10):
                timed(fn)
        for _ in range(args.pairs):
            for k, fn in legs.items():
                per_pair[k].append(statistics.median(timed(fn) for _ in range(args.reps)))
    step = {k: _spread(v) for k, v in per_pair.items()}
    step["added_ms"] = step["nsf"]["median_ms"] - step["plain"]["median_ms"]
    step["added_share_of_nsf_step"] = step["added_ms"] / step["nsf"]["median_ms"]
    print("step: plain %.3f [%.3f, %.3f] ms, nsf %.3f [%.3f, %.3f] ms, added %.3f ms (%.1f %% of the NSF step)" % (
        step["plain"]["median_ms"], step["plain"]["min_ms"], step["plain"]["max_ms"], step["nsf"]["median_ms"],
        step["nsf"]["min_ms"], step["nsf"]["max_ms"], step["added_ms"], 100 * step["added_share_of_nsf_step"]), flush=True)

    # ---- the launches alone, as graphs of their own
    hop = nsf.hop
    e = torch.empty(S, TC * hop, 1, device="cuda")
    outs = [torch.empty(S, TC * hop // u, C, device="cuda") for u, _, C, _, _ in nsf._downs]
    f0, uv = feats[:, -2].contiguous(), feats[:, -1].contiguous()

    def new_launches():
        hip.nsf_source(f0, uv, nsf._nsf_state[0], nsf._nsf_state[1], nsf._src_w, e, S=S, Tc=TC, hop=hop, H1=nsf.H1, sr=nsf.sr,
                       alpha=nsf.alpha, sigma=nsf.sigma, bias=nsf._src_b)
        hip.nsf_downs(e, nsf._nsf_hist[0], nsf._nsf_hist[1], nsf._downs, outs, S=S, Tc=TC, hop=hop, hist_ss=nsf._hist_ss)

    xs, mul = [], 1
    for s, Cout, upl, _ in nsf.stages:
        xs.append(torch.randn(S, TC * mul, upl.Cin, device="cuda"))
        mul *= s

    def up_layers():
        for (s, Cout, upl, _), x, r in zip(nsf.stages, xs, outs):
            nsf._conv(upl, x, 0, res=r)

    def graph_of(fn):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, capture_error_mode="thread_local"):
            fn()
        return gr

    launches = {}
    with torch.no_grad():
        graphs = dict(source_and_downs=graph_of(new_launches), up_layers=graph_of(up_layers))
        ts = {k: [] for k in graphs}
        for k, gr in graphs.items():
            for _ in range(20):
                gr.replay()
        torch.cuda.synchronize()
        for _ in range(args.pairs):
            for k, gr in graphs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.burst):
                    gr.replay()
                b.record()
                torch.cuda.synchronize()
                ts[k].append(a.elapsed_time(b) / args.burst)
        launches = {k: _spread(v) for k, v in ts.items()}
    launches["ratio_source_and_downs_over_up_layers"] = (launches["source_and_downs"]["median_ms"]
                                                         / launches["up_layers"]["median_ms"])
    print("launches (per replay, back to back): source + downs %.4f ms, the four up-layers %.4f ms" % (
        launches["source_and_downs"]["median_ms"], launches["up_layers"]["median_ms"]), flush=True)

    d = dict(config=dict(geometry=GEOM, nsf_params=NSF, slots=S, frames_per_step=TC, precision=args.mode, reps=args.reps,
                         pairs=args.pairs, burst=args.burst, parent_lib=bool(args.parent_lib),
                         device=torch.cuda.get_device_name(0)),
             step=step, launches=launches)
    for path in [OUT] + ([os.path.join(args.copy_to, os.path.basename(OUT))] if args.copy_to else []):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        json.dump(d, open(path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
