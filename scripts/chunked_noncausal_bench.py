"""A step of ChunkedNCVocoder against a step of ChunkedVocoder on the causal twin of the same geometry.

Geometry: the shipped non-causal configurations (channels 256, scales 10 x 5 x 2 x 2, kernels 20 / 11 / 4 / 4, residual
kernels 3 / 7 / 11 with dilations (1, 3, 5, 7)).  The causal twin has ``causal=True`` and kernel 10 in the second stage:
ChunkedVocoder takes upsampling kernels that are multiples of the stride only, and with 10 the stage has the same J = 3
polyphase taps as the non-causal one -- so both steps have the same launches with the same contraction sizes per layer.

The method of scripts/chunked_vocoder_rows_bench.py: graph replay, one process, the legs of a point alternating, a warm-up of
every shape (which captures the graphs), medians of --reps synchronised repetitions (host clock around call + synchronize)
with p10 / p90.  Both legs pass per-slot counts (``rows``), as continuous batching does.

    python scripts/chunked_noncausal_bench.py [--reps 200] [--precision bf16]     # -> profiles/chunked_noncausal.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kan-tts_amd"))
OUT = os.path.join(ROOT, "profiles", "chunked_noncausal.json")
GEOM = dict(channels=256, upsample_scales=[10, 5, 2, 2], resblock_kernel_sizes=[3, 7, 11],
            resblock_dilations=[[1, 3, 5, 7]] * 3)


def _summary(ts):
    q = statistics.quantiles(ts, n=10)
    return dict(median_ms=statistics.median(ts), p10_ms=q[0], p90_ms=q[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", default="bf16,fp32")
    ap.add_argument("--copy-to", default=None, help="directory that also receives the JSON")
    args = ap.parse_args()

    import torch

    import kantts._hip as hip
    from kantts.models.hifigan.chunked import ChunkedVocoder
    from kantts.models.hifigan.chunked_nc import ChunkedNCVocoder
    from kantts.models.hifigan.hifigan import Generator

    torch.manual_seed(0)
    G_nc = Generator(causal=False, upsample_kernal_sizes=[20, 11, 4, 4], **GEOM).eval().cuda()
    G_c = Generator(causal=True, upsample_kernal_sizes=[20, 10, 4, 4], **GEOM).eval().cuda()
    d = dict(config=dict(geometry=GEOM, noncausal_kernels=[20, 11, 4, 4], causal_twin_kernels=[20, 10, 4, 4], reps=args.reps,
                         device=torch.cuda.get_device_name(0)), points={})

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def race(legs):
        for fn in legs.values():
            for _ in range(args.warmup):
                timed(fn)
        ts = {k: [] for k in legs}
        for _ in range(args.reps):
            for k, fn in legs.items():
                ts[k].append(timed(fn))
        return {k: _summary(t) for k, t in ts.items()}

    with torch.no_grad():
        for prec in args.precision.split(","):
            hip.set_precision(prec)
            for S in (1, 8):
                nc, c = ChunkedNCVocoder(G_nc, slots=S, graph=True), ChunkedVocoder(G_c, slots=S, graph=True)
                for Tc in (8, 16):
                    mel = torch.randn(S, 80, Tc, device="cuda")
                    rows = torch.full((S,), Tc, dtype=torch.int32, device="cuda")
                    r = race(dict(causal=lambda: c.step(mel, rows=rows), noncausal=lambda: nc.step(mel, rows=rows)))
                    r["ratio_noncausal_over_causal"] = r["noncausal"]["median_ms"] / r["causal"]["median_ms"]
                    r["noncausal_inside_causal_p10_p90"] = (r["causal"]["p10_ms"] <= r["noncausal"]["median_ms"]
                                                            <= r["causal"]["p90_ms"])
                    # a convolution launch per layer and, per stage, sin(h) + h and the mean over the stacks; tanh and the
                    # two layout copies at the ends: the same code path (ChunkedVocoder._run) in both classes
                    r["launches_per_step"] = dict(causal=len(c.layers) + 2 * len(c.stages) + 3,
                                                  noncausal=len(nc.layers) + 2 * len(nc.stages) + 3)
                    r["state_floats_per_slot"] = dict(causal=c.state_floats, noncausal=nc.state_floats)
                    steps_to_first = nc.delay_samples // (Tc * nc.hop) + 1
                    r["first_audio"] = dict(flush_frames=nc.flush_frames, delay_samples=nc.delay_samples,
                                            steps_to_first_sample=steps_to_first,
                                            compute_ms_to_first_sample=steps_to_first * r["noncausal"]["median_ms"])
                    d["points"]["%s,S=%d,Tc=%d" % (prec, S, Tc)] = r
                    print("%s S=%d Tc=%2d causal %.3f [%.3f, %.3f] non-causal %.3f [%.3f, %.3f] x%.3f" % (
                        prec, S, Tc, r["causal"]["median_ms"], r["causal"]["p10_ms"], r["causal"]["p90_ms"],
                        r["noncausal"]["median_ms"], r["noncausal"]["p10_ms"], r["noncausal"]["p90_ms"],
                        r["ratio_noncausal_over_causal"]), flush=True)
                del nc, c
    hip.set_precision("fp32")
    for path in [OUT] + ([os.path.join(args.copy_to, os.path.basename(OUT))] if args.copy_to else []):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        json.dump(d, open(path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
