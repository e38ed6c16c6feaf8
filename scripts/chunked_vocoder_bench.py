"""Chunked vocoder step against what the whole-utterance interface offers for the same samples.

V1 class defaults, bf16 mode, S in {1, 8, 32} slots x Tc in {4, 8, 16} frames.  Per point, in one process, the legs
alternating, medians over --reps synchronised repetitions after a warm-up of every shape:

  chunk     ChunkedVocoder.step (graph replay), host clock around step + synchronize
  baseline  the unchanged Generator.forward, eager, on a window of 27 + Tc frames per slot (27 = the generator's look-back
            in frames), keeping the last Tc * 256 samples -- the only way to get a chunk without carried state
  baseline_graph   the same window replayed from a torch.cuda.CUDAGraph (information only)

    python scripts/chunked_vocoder_bench.py                       # -> profiles/chunked_vocoder.json (timing table)
    rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- \\
        python scripts/chunked_vocoder_bench.py --trace chunk --steps 10        # (and --steps 20; oneshot likewise)
    python scripts/chunked_vocoder_bench.py --launches chunk=DIR10,DIR20 oneshot=DIR10,DIR20 --trace-steps 10,20

The last form reads the ``*kernel_stats.csv`` files of four profiler runs and writes launches per chunk step / per
one-shot forward (S = 8, Tc = 8) into the same JSON: (calls at 20 steps - calls at 10 steps) / 10, so that warm-up and
capture launches cancel."""
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
OUT = os.path.join(ROOT, "profiles", "chunked_vocoder.json")
LOOKBACK = 27
COPY_TO = None


def _load():
    return json.load(open(OUT)) if os.path.exists(OUT) else {}


def _save(d):
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    json.dump(d, open(OUT, "w"), indent=1, sort_keys=True)
    if COPY_TO:  # --copy-to DIR: a second copy, e.g. in the scratch directory a remote run brings back
        os.makedirs(COPY_TO, exist_ok=True)
        json.dump(d, open(os.path.join(COPY_TO, os.path.basename(OUT)), "w"), indent=1, sort_keys=True)


def _calls(directory):
    files = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_stats.csv under %s" % directory)
    n = 0
    for f in files:
        for row in csv.DictReader(open(f)):
            n += int(row["Calls"])
    return n


def launches(args):
    n1, n2 = (int(v) for v in args.trace_steps.split(","))
    d = _load()
    rec = {}
    for item in args.launches:
        name, dirs = item.split("=")
        a, b = dirs.split(",")
        rec[name] = (_calls(b) - _calls(a)) / float(n2 - n1)
    rec["point"] = "S=8,Tc=8"
    rec["chunk_minus_oneshot"] = rec["chunk"] - rec["oneshot"]
    d["launches"] = rec
    _save(d)
    print(json.dumps(rec))


def trace(args):
    import torch

    import kantts._hip as hip
    from kantts.models.hifigan.chunked import ChunkedVocoder
    from kantts.models.hifigan.hifigan import Generator

    hip.set_precision("bf16")
    torch.manual_seed(0)
    G = Generator().eval().cuda()
    x = torch.randn(8, 80, 8, device="cuda")
    with torch.no_grad():
        if args.trace == "chunk":
            v = ChunkedVocoder(G, slots=8, graph=True)
            for _ in range(args.steps):
                v.step(x)
        else:
            for _ in range(args.steps):
                G(x)
    torch.cuda.synchronize()


def bench(args):
    import torch

    import kantts._hip as hip
    from kantts.models.hifigan.chunked import ChunkedVocoder
    from kantts.models.hifigan.hifigan import Generator

    hip.set_precision("bf16")
    torch.manual_seed(0)
    G = Generator().eval().cuda()
    hop = 256

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def summary(ts):
        q = statistics.quantiles(ts, n=10)
        return dict(median_ms=statistics.median(ts), p10_ms=q[0], p90_ms=q[-1])

    points = {}
    ok = True
    with torch.no_grad():
        for S in (1, 8, 32):
            v = ChunkedVocoder(G, slots=S, graph=True)
            for Tc in (4, 8, 16):
                mel = torch.randn(S, 80, Tc, device="cuda")
                win = torch.randn(S, 80, LOOKBACK + Tc, device="cuda")
                win_static = win.clone()

                def chunk():
                    return v.step(mel)

                def base():
                    return G(win)[..., -Tc * hop:]

                for _ in range(2):
                    G(win_static)
                torch.cuda.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, capture_error_mode="thread_local"):
                    g_out = G(win_static)

                def base_graph(gr=gr, g_out=g_out):
                    win_static.copy_(win)
                    gr.replay()
                    return g_out[..., -Tc * hop:].clone()

                def first_chunk():
                    v.reset()
                    return v.step(mel).cpu()

                legs = dict(chunk=chunk, baseline=base, baseline_graph=base_graph, first_chunk=first_chunk)
                for fn in legs.values():  # warm-up of every shape (captures the chunk step's graphs)
                    for _ in range(args.warmup):
                        timed(fn)
                ts = {k: [] for k in legs}
                for _ in range(args.reps):
                    for k, fn in legs.items():
                        ts[k].append(timed(fn))
                rec = {k: summary(t) for k, t in ts.items()}
                rec["ratio_chunk_over_baseline"] = rec["chunk"]["median_ms"] / rec["baseline"]["median_ms"]
                rec["samples_per_s_per_slot"] = Tc * hop / (rec["chunk"]["median_ms"] * 1e-3)
                rec["reps"] = args.reps
                points["S=%d,Tc=%d" % (S, Tc)] = rec
                ok = ok and rec["chunk"]["median_ms"] <= rec["baseline"]["median_ms"]
                print("S=%2d Tc=%2d  chunk %.3f ms  baseline %.3f ms  (graph %.3f ms)  ratio %.3f  first chunk %.3f ms" % (
                    S, Tc, rec["chunk"]["median_ms"], rec["baseline"]["median_ms"], rec["baseline_graph"]["median_ms"],
                    rec["ratio_chunk_over_baseline"], rec["first_chunk"]["median_ms"]), flush=True)
            del v
    d = _load()
    d["points"] = points
    d["config"] = dict(model="HiFi-GAN V1 class defaults", precision="bf16", lookback_frames=LOOKBACK,
                       device=torch.cuda.get_device_name(0))
    d["chunk_not_above_baseline_everywhere"] = ok
    _save(d)
    print("chunk step not above the baseline at every point:", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace", choices=["chunk", "oneshot"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--launches", nargs="+")
    ap.add_argument("--trace-steps", default="10,20")
    ap.add_argument("--copy-to", default=None, help="directory that also receives the JSON")
    a = ap.parse_args()
    COPY_TO = a.copy_to
    if a.launches:
        launches(a)
    elif a.trace:
        trace(a)
    else:
        sys.exit(bench(a))
