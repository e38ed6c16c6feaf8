"""What a step of the chunked MULTI-BAND vocoder costs (ChunkedMBVocoder, csrc/mb_tail.hip) against a step of ChunkedVocoder on
a single-band generator of the same ``channels``, per second of audio.

Both generators have 512 channels, random weights and a hop of 240 samples (24 kHz: 10 ms frames): the single-band one the
shipped geometry (upsample_scales 8, 5, 3, 2), the multi-band one 4 sub-bands behind upsample_scales 5, 4, 3 (its stack runs
at a quarter of the sample rate).  S = 4 slots, 8 frames per step, graph replay, one process.

  step        the two legs alternate; a PAIR is --reps steps of each (host clock around step + synchronize), --pairs pairs;
              per leg the median over the pairs of the per-pair medians and their range, and the same per second of audio
              (a step produces S * 8 frames * 10 ms).
  launches    launches per step of either leg, counted in one eager step: the library's launches (by entry point) and the two
              torch kernels around them (the channels-first to channels-last copy of the input, and tanh for the single band).

    python scripts/chunked_multiband_bench.py [--mode bf16|fp32]     # -> profiles/chunked_multiband.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kan-tts_amd"))
OUT = os.path.join(ROOT, "profiles", "chunked_multiband.json")
SINGLE = dict(in_channels=80, channels=512, upsample_scales=[8, 5, 3, 2], upsample_kernal_sizes=[16, 10, 6, 4])
MULTI = dict(in_channels=80, channels=512, out_channels=4, upsample_scales=[5, 4, 3], upsample_kernal_sizes=[10, 8, 6])
S, TC, SR = 4, 8, 24000


def _spread(ts):
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--mode", default="bf16")
    ap.add_argument("--copy-to", default=None, help="directory that also receives the JSON")
    args = ap.parse_args()

    import torch

    import kantts._hip as hip
    from kantts._hip import ops
    from kantts.models.hifigan import chunked
    from kantts.models.hifigan.chunked import ChunkedVocoder
    from kantts.models.hifigan.chunked_mb import ChunkedMBVocoder
    from kantts.models.hifigan.hifigan import Generator
    from kantts.models.pqmf import PQMF

    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    hip.set_precision(args.mode)
    torch.manual_seed(0)
    G1 = Generator(**SINGLE).eval().cuda()
    torch.manual_seed(0)
    G4 = Generator(**MULTI).eval().cuda()
    pq = PQMF().cuda()
    mel = torch.randn(S, 80, TC, generator=torch.Generator().manual_seed(1)).cuda()

    # ---- launches of one eager step
    calls = {}

    def counted(mod, name):
        fn = getattr(mod, name)

        def wrapper(*a, **k):
            calls[name] = calls.get(name, 0) + 1
            return fn(*a, **k)

        setattr(mod, name, wrapper)
        return fn

    launches = {}
    for leg, make in (("single_band", lambda: ChunkedVocoder(G1, slots=S, graph=False)),
                      ("multi_band", lambda: ChunkedMBVocoder(G4, pqmf=pq, slots=S, graph=False))):
        saved = [(hip, n, counted(hip, n)) for n in ("sconv", "mb_tail")] + \
                [(chunked.ops, n, counted(chunked.ops, n)) for n in ("sin_add", "mean_many")]
        try:
            calls.clear()
            with torch.no_grad():
                make().step(mel)
        finally:
            for mod, n, fn in saved:
                setattr(mod, n, fn)
        torch_kernels = 1 + (1 if leg == "single_band" else 0)  # the input's channels-last copy; tanh
        launches[leg] = dict(library=dict(calls), torch_kernels=torch_kernels, total=sum(calls.values()) + torch_kernels)
    assert ops is chunked.ops
    print("launches per step:", launches, flush=True)

    # ---- step time, graph replay
    one = ChunkedVocoder(G1, slots=S, graph=True)
    mb = ChunkedMBVocoder(G4, pqmf=pq, slots=S, graph=True)
    assert one.hop == mb.hop == 240
    with torch.no_grad():
        one.step(mel), one.step(mel), mb.step(mel), mb.step(mel)

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    legs = dict(single_band=lambda: one.step(mel), multi_band=lambda: mb.step(mel))
    per_pair = {k: [] for k in legs}
    with torch.no_grad():
        for fn in legs.values():
            for _ in range(10):
                timed(fn)
        for _ in range(args.pairs):
            for k, fn in legs.items():
                per_pair[k].append(statistics.median(timed(fn) for _ in range(args.reps)))
    audio_s = S * TC * 240 / SR
    step = {k: dict(_spread(v), ms_per_second_of_audio=statistics.median(v) / audio_s) for k, v in per_pair.items()}
    step["multi_over_single"] = step["multi_band"]["median_ms"] / step["single_band"]["median_ms"]
    print("step: single-band %.3f ms, multi-band %.3f ms (x %.2f); per second of audio %.3f / %.3f ms" % (
        step["single_band"]["median_ms"], step["multi_band"]["median_ms"], step["multi_over_single"],
        step["single_band"]["ms_per_second_of_audio"], step["multi_band"]["ms_per_second_of_audio"]), flush=True)

    d = dict(config=dict(single_band=SINGLE, multi_band=MULTI, slots=S, frames_per_step=TC, sampling_rate=SR, precision=args.mode,
                         reps=args.reps, pairs=args.pairs, device=torch.cuda.get_device_name(0)),
             step=step, launches=launches)
    for path in [OUT] + ([os.path.join(args.copy_to, os.path.basename(OUT))] if args.copy_to else []):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        json.dump(d, open(path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
