"""What the per-slot row counts of the chunked vocoder cost and return (ChunkedVocoder.step(mel, rows=...), play_many).

The method of scripts/chunked_vocoder_bench.py: V1 class defaults, bf16 mode, graph replay, one process, the legs of a
point alternating, a warm-up of every shape (which captures the graphs), medians of --reps synchronised repetitions (host
clock around call + synchronize) with p10 / p90.

  (a) plain_vs_parent   step(mel) WITHOUT rows, the library of the parent commit against this tree's, S in {1, 8, 32} x
                        Tc in {4, 8, 16}.  Needs --parent-lib PATH (a libkantts_hip.so built from the parent commit): both
                        libraries are loaded into this process, each vocoder captures its graphs through its own, and the
                        replays alternate.  Requirement: this tree's median inside the parent's own p10..p90 band.
  (b) rows_vs_plain     step(mel, rows=[Tc] * S) against step(mel), same points: the price of the counts (host list -> one
                        small copy to the device per step; `rows_dev`: the counts already on the device).
  (c) half_dead         S in {8, 32}, Tc = 8: every second slot at rows = 0 against all slots live: what skipping dead
                        tiles returns.
  (d) play_many         64 seeded utterances of 50..400 frames: play_many on 8 slots, chunk_frames = 8, against the same
                        utterances one by one through synthesize on 1 slot (what infer_hifigan --chunk_frames does without
                        --slots).  Utterances / s and samples / s, medians of --runs whole passes.

    python scripts/chunked_vocoder_rows_bench.py [--parent-lib PATH] [--only a,b,c,d]   # -> profiles/chunked_vocoder_rows.json
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
OUT = os.path.join(ROOT, "profiles", "chunked_vocoder_rows.json")
POINTS = [(S, Tc) for S in (1, 8, 32) for Tc in (4, 8, 16)]


def _summary(ts):
    q = statistics.quantiles(ts, n=10)
    return dict(median_ms=statistics.median(ts), p10_ms=q[0], p90_ms=q[-1])


def _parent_library(hip, path):
    """The parent commit's library with the prototypes of this tree's binding for every entry point it exports."""
    mine = hip.lib()
    L = ctypes.CDLL(path)
    for name in hip.EXPORTED_SYMBOLS:
        if hasattr(L, name):
            fn, ref = getattr(L, name), getattr(mine, name)
            fn.argtypes, fn.restype = ref.argtypes, ref.restype
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only", default="a,b,c,d")
    ap.add_argument("--copy-to", default=None, help="directory that also receives the JSON")
    args = ap.parse_args()
    only = set(args.only.split(","))

    import torch

    import kantts._hip as hip
    from kantts.models.hifigan.chunked import ChunkedVocoder
    from kantts.models.hifigan.hifigan import Generator

    hip.set_precision("bf16")
    torch.manual_seed(0)
    G = Generator().eval().cuda()
    hop = 256
    d = json.load(open(OUT)) if os.path.exists(OUT) else {}
    d["config"] = dict(model="HiFi-GAN V1 class defaults", precision="bf16", reps=args.reps,
                       device=torch.cuda.get_device_name(0))

    def save():
        for path in [OUT] + ([os.path.join(args.copy_to, os.path.basename(OUT))] if args.copy_to else []):
            os.makedirs(os.path.dirname(path), exist_ok=True)
            json.dump(d, open(path, "w"), indent=1, sort_keys=True)

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
        if "a" in only:
            if not args.parent_lib:
                d["plain_vs_parent"] = "not measured (no --parent-lib)"
            else:
                mine, parent = hip.lib(), _parent_library(hip, args.parent_lib)

                def use(L):  # every wrapper goes through hip.lib(), which hands out this global
                    hip._lib = L

                rec, inside = {}, True
                for S, Tc in POINTS:
                    mel = torch.randn(S, 80, Tc, device="cuda")
                    vs = {}
                    for name, L in (("parent", parent), ("this_tree", mine)):
                        use(L)
                        vs[name] = ChunkedVocoder(G, slots=S, graph=True)
                        vs[name].step(mel), vs[name].step(mel)  # captured through L; replays need no library
                    use(mine)
                    r = race({k: (lambda v=v: v.step(mel)) for k, v in vs.items()})
                    r["this_tree_inside_parent_p10_p90"] = r["parent"]["p10_ms"] <= r["this_tree"]["median_ms"] <= r["parent"]["p90_ms"]
                    r["this_tree_not_above_parent_p90"] = r["this_tree"]["median_ms"] <= r["parent"]["p90_ms"]
                    r["ratio_this_tree_over_parent"] = r["this_tree"]["median_ms"] / r["parent"]["median_ms"]
                    inside = inside and r["this_tree_inside_parent_p10_p90"]
                    rec["S=%d,Tc=%d" % (S, Tc)] = r
                    print("(a) S=%2d Tc=%2d parent %.3f [%.3f, %.3f] this tree %.3f  inside: %s" % (
                        S, Tc, r["parent"]["median_ms"], r["parent"]["p10_ms"], r["parent"]["p90_ms"],
                        r["this_tree"]["median_ms"], r["this_tree_inside_parent_p10_p90"]), flush=True)
                    del vs
                d["plain_vs_parent"] = dict(points=rec, every_point_inside_parent_band=inside)
            save()

        if "b" in only or "c" in only:
            recb, recc = {}, {}
            for S in (1, 8, 32):
                v = ChunkedVocoder(G, slots=S, graph=True)
                for Tc in (4, 8, 16):
                    mel = torch.randn(S, 80, Tc, device="cuda")
                    full = [Tc] * S
                    full_dev = torch.tensor(full, dtype=torch.int32, device="cuda")
                    if "b" in only:
                        r = race(dict(plain=lambda: v.step(mel), rows=lambda: v.step(mel, rows=full),
                                      rows_dev=lambda: v.step(mel, rows=full_dev)))
                        r["ratio_rows_over_plain"] = r["rows"]["median_ms"] / r["plain"]["median_ms"]
                        r["ratio_rows_dev_over_plain"] = r["rows_dev"]["median_ms"] / r["plain"]["median_ms"]
                        recb["S=%d,Tc=%d" % (S, Tc)] = r
                        print("(b) S=%2d Tc=%2d plain %.3f rows %.3f (x%.3f) rows on the device %.3f (x%.3f)" % (
                            S, Tc, r["plain"]["median_ms"], r["rows"]["median_ms"], r["ratio_rows_over_plain"],
                            r["rows_dev"]["median_ms"], r["ratio_rows_dev_over_plain"]), flush=True)
                    if "c" in only and Tc == 8 and S > 1:
                        half = torch.tensor([Tc if s % 2 == 0 else 0 for s in range(S)], dtype=torch.int32, device="cuda")
                        r = race(dict(all_live=lambda: v.step(mel, rows=full_dev), half_dead=lambda: v.step(mel, rows=half)))
                        r["ratio_half_dead_over_all_live"] = r["half_dead"]["median_ms"] / r["all_live"]["median_ms"]
                        recc["S=%d,Tc=%d" % (S, Tc)] = r
                        print("(c) S=%2d Tc=%2d all live %.3f half dead %.3f (x%.3f)" % (
                            S, Tc, r["all_live"]["median_ms"], r["half_dead"]["median_ms"],
                            r["ratio_half_dead_over_all_live"]), flush=True)
                del v
            if "b" in only:
                d["rows_vs_plain"] = recb
            if "c" in only:
                d["half_dead"] = recc
            save()

        if "d" in only:
            g = torch.Generator().manual_seed(1)
            lens = torch.randint(50, 401, (64,), generator=g).tolist()
            mels = [torch.randn(80, n, generator=g).cuda() for n in lens]
            samples = sum(lens) * hop
            v8, v1 = ChunkedVocoder(G, slots=8, graph=True), ChunkedVocoder(G, slots=1, graph=True)

            def many():
                return [w for _, w in v8.play_many(mels, chunk_frames=8)]

            def one_by_one():
                return [w for m in mels for w in v1.synthesize(m, chunk_frames=8)]

            legs = dict(play_many=many, one_by_one=one_by_one)
            for fn in legs.values():
                fn()
            torch.cuda.synchronize()
            ts = {k: [] for k in legs}
            for _ in range(args.runs):
                for k, fn in legs.items():
                    ts[k].append(timed(fn))
            rec = dict(utterances=len(lens), frames=sum(lens), slots=8, chunk_frames=8, runs=args.runs)
            for k, t in ts.items():
                ms = statistics.median(t)
                rec[k] = dict(median_ms=ms, all_ms=t, utterances_per_s=len(lens) / (ms * 1e-3), samples_per_s=samples / (ms * 1e-3))
            rec["ratio_play_many_over_one_by_one_throughput"] = rec["one_by_one"]["median_ms"] / rec["play_many"]["median_ms"]
            d["play_many"] = rec
            print("(d) play_many %.1f ms (%.1f utt/s, %.2f M samples/s)  one by one %.1f ms (%.1f utt/s, %.2f M samples/s)  x%.2f" % (
                rec["play_many"]["median_ms"], rec["play_many"]["utterances_per_s"], rec["play_many"]["samples_per_s"] / 1e6,
                rec["one_by_one"]["median_ms"], rec["one_by_one"]["utterances_per_s"],
                rec["one_by_one"]["samples_per_s"] / 1e6, rec["ratio_play_many_over_one_by_one_throughput"]), flush=True)
            save()


if __name__ == "__main__":
    main()
