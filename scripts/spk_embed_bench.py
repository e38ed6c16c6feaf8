"""Throughput of the speaker-embedding extractor (kantts.preprocess.se_processor, csrc/spk_embed.hip) on the MI355X.

Workload: 256 synthetic utterances of 2 - 10 s (16 kHz), shipped D-TDNN geometry with the closed-form recipe weights.
  (i)  ``stock``   the stock-torch forward of the package's module on the same GPU, one wav at a time -- what the reference's
                   se_processor does (its fbank is torchaudio's on the host; here both legs take kantts_kaldi_fbank, so
                   the comparison is of the model path alone plus the batching);
  (ii) ``kernels`` SpeakerEmbeddingProcessor.embed: sorted by length, batched under the frame budget, the kernel path.
The two legs run interleaved in one process, ``--reps`` windows each after a warm-up of both; a window is the whole
workload and ends in a device synchronise.  Utterances per second from the median window; launches of one forward pass
from the profiler in an untimed pass.

    python scripts/spk_embed_bench.py                        # -> profiles/spk_embed.json              (needs the GPU)
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/spk_embed_bench.py --kernels-only   # the per-kernel split
    python scripts/spk_embed_bench.py --stats DIR            # folds that run's per-kernel table into the json
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kan-tts_amd"))
OUT = os.path.join(ROOT, "profiles", "spk_embed.json")
N_UTT, SEC_LO, SEC_HI = 256, 2.0, 10.0


def _stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "windows": len(xs)}


def _workload(torch):
    from kantts.preprocess.se_processor.recipe import unit_uniform

    secs = SEC_LO + (SEC_HI - SEC_LO) * unit_uniform("bench/lengths", N_UTT)
    g = torch.Generator().manual_seed(1)
    return [0.1 * torch.randn(int(s * 16000), generator=g) for s in secs]


def _processor(torch, budget):
    from kantts.preprocess.se_processor.D_TDNN import DTDNN
    from kantts.preprocess.se_processor.recipe import recipe_state_dict
    from kantts.preprocess.se_processor.se_processor import SpeakerEmbeddingProcessor

    proc = SpeakerEmbeddingProcessor(frame_budget=budget)
    m = DTDNN()
    m.load_state_dict(recipe_state_dict(m), strict=True)
    proc.model = m.eval().to(proc.device)
    return proc


def _launches(torch, fn):
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def run(reps, budget, kernels_only):
    import torch

    import kantts._hip as hip

    assert torch.cuda.is_available(), "needs the GPU"
    hip.lib()
    wavs = _workload(torch)
    proc = _processor(torch, budget)
    dev_wavs = [w.to(proc.device) for w in wavs]

    def kernels():
        return proc.embed(wavs)

    def stock():
        out = []
        with torch.no_grad():
            for w in dev_wavs:
                feats, _ = proc.features(w[None], [w.numel()])
                out.append(proc.model(feats))
        return torch.cat(out)

    if kernels_only:  # the run rocprofv3 traces
        for _ in range(3):
            kernels()
        torch.cuda.synchronize()
        return None
    a, b = kernels(), stock()
    torch.cuda.synchronize()
    diff = float((a - b).abs().max())
    one = dev_wavs[0]
    feats, frames = proc.features(one[None], [one.numel()])
    launches = {"kernels_forward": _launches(torch, lambda: proc.model.forward_kernels(feats, frames)),
                "stock_forward": _launches(torch, lambda: proc.model(feats))}
    tk, ts = [], []
    for _ in range(reps):
        for leg, acc in ((kernels, tk), (stock, ts)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg()
            torch.cuda.synchronize()
            acc.append(time.perf_counter() - t0)
    frames_total = sum(1 + (w.numel() - 400) // 160 for w in wavs)
    return {"workload": dict(utterances=N_UTT, seconds=[SEC_LO, SEC_HI], fbank_frames=frames_total, frame_budget=budget,
                             geometry="shipped (6.85 M parameters), recipe weights, fp32"),
            "kernels_s": _stats(tk), "stock_one_by_one_s": _stats(ts),
            "utterances_per_s": {"kernels": N_UTT / statistics.median(tk), "stock_one_by_one": N_UTT / statistics.median(ts)},
            "ratio_of_medians": statistics.median(ts) / statistics.median(tk),
            "device_launches_per_forward": launches, "max_abs_difference_between_the_legs": diff,
            "output_scale": float(b.abs().max())}


def fold_stats(directory, out):
    """Per-kernel totals of a ``rocprofv3 --kernel-trace --stats`` run of ``--kernels-only`` into the json: from the
    ``*kernel_stats.csv`` files, or from the ``top_kernels`` view of the result database where the tool wrote that."""
    import sqlite3

    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                rows.append({"kernel": r["Name"].split("(")[0][:80], "calls": int(r["Calls"]),
                             "total_ms": float(r["TotalDurationNs"]) / 1e6, "percent": float(r["Percentage"])})
    if not rows:
        for path in glob.glob(os.path.join(directory, "**", "*.db"), recursive=True):
            con = sqlite3.connect(path)
            for name, calls, total_us, _avg, pct in con.execute("select * from top_kernels"):
                rows.append({"kernel": name.split("(")[0][:80], "calls": int(calls), "total_ms": float(total_us) / 1e3,
                             "percent": float(pct)})
    rows.sort(key=lambda r: -r["total_ms"])
    result = json.load(open(out)) if os.path.exists(out) else {}
    result["kernel_split_of_three_passes"] = rows[:8]
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(rows[:8], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--budget", type=int, default=16000)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--stats", default=None)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.stats:
        return fold_stats(a.stats, a.out)
    result = run(a.reps, a.budget, a.kernels_only)
    if result is None:
        return
    print(json.dumps(result, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    prev = json.load(open(a.out)) if os.path.exists(a.out) else {}
    prev.update(result)
    with open(a.out, "w") as f:
        json.dump(prev, f, indent=1)


if __name__ == "__main__":
    main()
