"""Time to the first mel chunk of a streaming SAM-BERT session against the one-shot forward.

Full 16k model (oracle/torch_oracle.py::sambert_config), bf16 mode, B in {1, 8, 32} utterances of about 600 frames (60
symbols, durations 5..15 frames given), chunk_steps in {4, 8, 16} decoder steps.  Per combination, in one process, the two
legs interleaved, medians over --reps repetitions after a warm-up of both:

  chunked   ChunkedAcoustic.open, then session.step(chunk_steps) until the end; every non-empty chunk is copied to the host
            (that is when it can be handed to the vocoder).  Recorded: open, time from open returning to the first non-empty
            chunk on the host, median time per step, total from open returning to the last chunk.
  oneshot   KanTtsSAMBERT.forward with decode_mode "kernel", postnet_outputs copied to the host.

    python scripts/chunked_acoustic_bench.py            # -> profiles/chunked_acoustic.json

The default mode is a driver: every batch size runs in a child process of its own under ``timeout``, then one more child
counts the device launches of a mid-utterance step; the children are chained, the first failure ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kan-tts_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
OUT = os.path.join(ROOT, "profiles", "chunked_acoustic.json")
BATCHES, CHUNKS = (1, 8, 32), (4, 8, 16)


def _setup(B):
    import torch

    import kantts._hip as hip
    import torch_oracle as O
    from kantts.models.sambert.chunked import ChunkedAcoustic
    from kantts.models.sambert.kantts_sambert import KanTtsSAMBERT
    from kantts.utils.synthetic import inference_utterances

    hip.set_precision("bf16")
    torch.manual_seed(0)
    m = KanTtsSAMBERT(dict(O.sambert_config())).cuda().eval()
    m.mel_decoder.decode_mode = "kernel"
    T_in = 60
    _, ling, emo, spk = inference_utterances(B, seed=1)
    g = torch.Generator().manual_seed(2)
    reps = -(-T_in // ling.size(1))  # the synthetic utterances are up to 80 symbols; tile if a draw was shorter
    args = dict(inputs_ling=ling.repeat(1, reps, 1)[:, :T_in].contiguous().cuda(),
                inputs_emotion=emo.repeat(1, reps)[:, :T_in].contiguous().cuda(),
                inputs_speaker=spk.repeat(1, reps)[:, :T_in].contiguous().cuda(),
                input_lengths=torch.full((B,), T_in, dtype=torch.long).cuda(),
                duration_targets=torch.randint(5, 16, (B, T_in), generator=g).cuda())
    return torch, m, ChunkedAcoustic(m), args


def point(B, reps, warmup):
    torch, m, ca, args = _setup(B)

    def sync():
        torch.cuda.synchronize()

    def chunked(cs):
        sync()
        t0 = time.perf_counter()
        sess = ca.open(**args)
        sync()
        t_open = time.perf_counter()
        first, steps, last = None, [], t_open
        while not sess.finished:
            _, _, mel = sess.step(cs)
            if mel.size(1):
                mel.cpu()
                if first is None:
                    first = time.perf_counter() - t_open
            else:
                sync()
            now = time.perf_counter()
            steps.append(now - last)
            last = now
        return dict(open_ms=1e3 * (t_open - t0), first_chunk_ms=1e3 * first, step_ms=1e3 * statistics.median(steps),
                    total_ms=1e3 * (last - t_open), steps=len(steps), frames=int(sess.frames.max()))

    def oneshot():
        sync()
        t0 = time.perf_counter()
        m(**args)["postnet_outputs"].cpu()
        return 1e3 * (time.perf_counter() - t0)

    rec = {}
    with torch.no_grad():
        for cs in CHUNKS:
            for _ in range(warmup):
                chunked(cs)
                oneshot()
            runs, ones = [], []
            for _ in range(reps):
                runs.append(chunked(cs))
                ones.append(oneshot())
            r = {k: statistics.median(x[k] for x in runs) for k in runs[0]}
            r["oneshot_ms"] = statistics.median(ones)
            r["oneshot_over_open_plus_first_chunk"] = r["oneshot_ms"] / (r["open_ms"] + r["first_chunk_ms"])
            r["open_plus_total_over_oneshot"] = (r["open_ms"] + r["total_ms"]) / r["oneshot_ms"]
            r["reps"] = reps
            rec["B=%d,chunk_steps=%d" % (B, cs)] = r
            print("B=%2d chunk_steps=%2d  open %.2f ms  first chunk +%.2f ms  step %.3f ms  total +%.2f ms | one-shot %.2f ms" % (
                B, cs, r["open_ms"], r["first_chunk_ms"], r["step_ms"], r["total_ms"], r["oneshot_ms"]), flush=True)
    return rec


def launches():
    """Device launches of one mid-utterance step (B = 8, chunk_steps = 8), counted by the profiler."""
    from torch.profiler import ProfilerActivity, profile

    torch, m, ca, args = _setup(8)
    with torch.no_grad():
        for _ in range(2):
            sess = ca.open(**args)
            for _ in range(4):
                sess.step(8)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            sess.step(8)
            torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    return {"point": "B=8,chunk_steps=8", "launches_per_step": n}


def driver(a):
    d = {"config": dict(model="SAM-BERT full 16k configuration, random init", precision="bf16", symbols=60,
                        frames="about 600 (durations 5..15 given)"), "points": {}}
    tmp = OUT + ".part"
    jobs = [["--point", str(B)] for B in BATCHES] + [["--launches"]]
    for job in jobs:
        if os.path.exists(tmp):
            os.remove(tmp)
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps),
               "--warmup", str(a.warmup), "--part", tmp] + job
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print("step %s ended with status %d: stopping" % (" ".join(job), rc))
            return rc
        part = json.load(open(tmp))
        os.remove(tmp)
        if job[0] == "--point":
            d["points"].update(part)
        else:
            d["launches"] = part
        json.dump(d, open(OUT, "w"), indent=1, sort_keys=True)
        if a.copy_to:  # a second copy, e.g. in the scratch directory a remote run brings back
            os.makedirs(a.copy_to, exist_ok=True)
            json.dump(d, open(os.path.join(a.copy_to, os.path.basename(OUT)), "w"), indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--limit", type=int, default=240, help="seconds every child step may take")
    ap.add_argument("--copy-to", default=None, help="directory that also receives the JSON")
    ap.add_argument("--point", type=int, default=None, help="(child) time one batch size")
    ap.add_argument("--launches", action="store_true", help="(child) count the launches of one step")
    ap.add_argument("--part", default=None, help="(child) where the partial result goes")
    a = ap.parse_args()
    if a.point is not None or a.launches:
        res = launches() if a.launches else point(a.point, a.reps, a.warmup)
        json.dump(res, open(a.part, "w"))
        sys.exit(0)
    sys.exit(driver(a))
