"""What the excitation costs a chunked step of a non-causal NSF vocoder (ChunkedNCNSFVocoder, csrc/nsf_source_sym.hip).

Shipped 16 kHz geometry (hifigan_noncausal_nsf_v1_16k: upsample_scales 10, 5, 2, 2, kernels 20, 11, 4, 4, 256 channels,
residual kernels 3 / 7 / 11 with dilations 1, 3, 5, 7, 7 harmonics + fundamental, random init), S = 4 slots, 8 frames per
step, graph replay, one process, every slot open and in mid-utterance.

  step        ChunkedNCNSFVocoder.step against ChunkedNCVocoder.step of the same generator built WITHOUT nsf_params.  The
              two legs alternate; a PAIR is --reps steps of each (host clock around step + synchronize), --pairs pairs; per
              leg the median over the pairs of the per-pair medians, and their range.
  launches    the two new launches alone (kantts_nsf_source_end_rows, kantts_nsf_downs_sym_rows), captured as a graph of
              their own: device events around --burst back-to-back replays (time per replay), --pairs times.

    python scripts/chunked_nc_nsf_bench.py [--mode bf16|fp32]     # -> profiles/chunked_nc_nsf.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kan-tts_amd"))
OUT = os.path.join(ROOT, "profiles", "chunked_nc_nsf.json")
GEOM = dict(in_channels=80, channels=256, upsample_scales=[10, 5, 2, 2], upsample_kernal_sizes=[20, 11, 4, 4],
            resblock_kernel_sizes=[3, 7, 11], resblock_dilations=[[1, 3, 5, 7]] * 3, causal=False)
NSF = {"nb_harmonics": 7, "sampling_rate": 16000}
S, TC = 4, 8


def _spread(ts):
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--burst", type=int, default=200)
    ap.add_argument("--mode", default="bf16")
    ap.add_argument("--copy-to", default=None, help="directory that also receives the JSON")
    args = ap.parse_args()

    import torch

    import kantts._hip as hip
    from kantts.models.hifigan.chunked_nc import ChunkedNCVocoder
    from kantts.models.hifigan.chunked_nc_nsf import ChunkedNCNSFVocoder
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
    rows = [TC] * S

    plain = ChunkedNCVocoder(G_plain, slots=S, graph=True)
    nsf = ChunkedNCNSFVocoder(G_nsf, slots=S, graph=True)

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    legs = dict(plain=lambda: plain.step(mel, rows=rows), nsf=lambda: nsf.step(feats, rows=rows))
    per_pair = {k: [] for k in legs}
    with torch.no_grad():
        for fn in legs.values():
            for _ in range(30):  # past the delay: every layer's window is inside the utterance
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

    # ---- the two launches alone, as a graph of their own (state half 0 -> half 1, every slot open)
    hop = nsf.hop
    e = torch.empty(S, TC * hop, 1, device="cuda")
    outs = [torch.empty(S, TC * hop // u, C, device="cuda") for u, _, C, _, _ in nsf._downs]
    f0, uv = feats[:, -2].contiguous(), feats[:, -1].contiguous()
    cnt = torch.tensor(rows, dtype=torch.int32, device="cuda")
    pos = dict(end=nsf._end, pos_in=nsf._arena_i32[0, 0, nsf._pos_off:], pos_ss=nsf.arena.shape[2])

    def new_launches():
        hip.nsf_source_end(f0, uv, nsf._nsf_state[0], nsf._nsf_state[1], nsf._src_w, e, S=S, Tc=TC, hop=hop, H1=nsf.H1,
                           sr=nsf.sr, alpha=nsf.alpha, sigma=nsf.sigma, bias=nsf._src_b, rows=cnt, **pos)
        hip.nsf_downs_sym(e, nsf._nsf_hist[0], nsf._nsf_hist[1], nsf._downs, nsf.lags, outs, S=S, Tc=TC, hop=hop,
                          hist_rows=nsf._hh, hist_ss=nsf._hist_ss, rows=cnt, **pos)

    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            new_launches()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, capture_error_mode="thread_local"):
            new_launches()
        for _ in range(20):
            gr.replay()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.pairs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.burst):
                gr.replay()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) / args.burst)
    launches = dict(source_and_downs=_spread(ts))
    print("launches (per replay, back to back): source + downs %.4f ms" % launches["source_and_downs"]["median_ms"], flush=True)

    d = dict(config=dict(geometry=GEOM, nsf_params=NSF, slots=S, frames_per_step=TC, precision=args.mode, reps=args.reps,
                         pairs=args.pairs, burst=args.burst, device=torch.cuda.get_device_name(0)),
             step=step, launches=launches)
    for path in [OUT] + ([os.path.join(args.copy_to, os.path.basename(OUT))] if args.copy_to else []):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        json.dump(d, open(path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
