"""Continuous batching of SAM-BERT streaming sessions (AcousticSlots) against lockstep sessions (ChunkedAcoustic).

Full 16k model (oracle/torch_oracle.py::sambert_config), bf16 mode, 64 seeded synthetic utterances of 60 symbols whose
frame counts spread over roughly 100..800 (durations given), all requests present at time 0, chunk_steps 8, S in {8, 32}:

  lockstep  ChunkedAcoustic sessions over consecutive groups of S utterances, one after the other (what the library could
            do before the pool): a group's session lasts as long as its longest utterance.
  slots     AcousticSlots(slots=S).play_many over the same utterances in the same order.

Every non-empty chunk is copied to the host (that is when it can be handed to the vocoder): one copy per step for a
lockstep batch, one per advancing slot for the pool.  Reported per leg, medians over --reps repetitions after a warm-up of
both, the legs interleaved: utterances per second, median and worst time from time 0 to an utterance's first mel chunk.

Per-launch check (--launch): kantts_pnca_decode_slots with all sequences in lockstep against kantts_pnca_decode_range over
the same 8 steps of a 32-sequence batch, interleaved A/B five times, each figure the mean of 20 launches between two
device events.  The slots form's median may exceed the range form's by at most the range form's own (max - min).

    python scripts/acoustic_slots_bench.py            # -> profiles/acoustic_slots.json

The default mode is a driver: every point runs in a child process of its own under ``timeout``; the children are chained,
the first failure ends the run."""
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
OUT = os.path.join(ROOT, "profiles", "acoustic_slots.json")
POOLS, CHUNK_STEPS, N_UTT, T_IN, MAX_STEPS = (8, 32), 8, 64, 60, 320


def _model():
    import torch

    import kantts._hip as hip
    import torch_oracle as O
    from kantts.models.sambert.kantts_sambert import KanTtsSAMBERT

    hip.set_precision("bf16")
    torch.manual_seed(0)
    m = KanTtsSAMBERT(dict(O.sambert_config())).cuda().eval()
    m.mel_decoder.decode_mode = "kernel"
    return torch, hip, m


def _utterances(torch, n):
    """``n`` batch-1 requests with the durations given: frame targets spread evenly over 100..800, in a seeded order."""
    from kantts.utils.synthetic import inference_utterances

    _, ling, emo, spk = inference_utterances(n, seed=1)
    reps = -(-T_IN // ling.size(1))  # the synthetic utterances are up to 80 symbols; tile if a draw was shorter
    ling, emo, spk = (t.repeat(*((1, reps) + (1,) * (t.dim() - 2)))[:, :T_IN].contiguous().cuda() for t in (ling, emo, spk))
    g = torch.Generator().manual_seed(2)
    target = torch.linspace(100, 800, n)[torch.randperm(n, generator=g)]
    dur = (target[:, None] / T_IN * (0.6 + 0.8 * torch.rand(n, T_IN, generator=g)) + 0.5).long().clamp(min=1)
    lens = torch.full((n,), T_IN, dtype=torch.long).cuda()
    batch = dict(inputs_ling=ling, inputs_emotion=emo, inputs_speaker=spk, input_lengths=lens, duration_targets=dur.cuda())
    return batch, [int(v) for v in dur.sum(1)]


def point(S, reps, warmup):
    torch, hip, m = _model()
    from kantts.models.sambert.chunked import ChunkedAcoustic
    from kantts.models.sambert.slots import AcousticSlots

    batch, frames = _utterances(torch, N_UTT)
    assert max(frames) <= MAX_STEPS * m.mel_decoder.r, max(frames)
    requests = [{k: v[i:i + 1].contiguous() for k, v in batch.items()} for i in range(N_UTT)]
    ca, pool = ChunkedAcoustic(m), AcousticSlots(m, slots=S, max_steps=MAX_STEPS)

    def lockstep():
        torch.cuda.synchronize()
        t0, first = time.perf_counter(), {}
        for g0 in range(0, N_UTT, S):
            sess = ca.open(**{k: v[g0:g0 + S].contiguous() for k, v in batch.items()})
            for _, hi, mel in sess.stream(CHUNK_STEPS):
                if mel.size(1):
                    mel.cpu()
                    if len(first) < min(g0 + S, N_UTT):
                        now = time.perf_counter() - t0
                        for i in range(g0, min(g0 + S, N_UTT)):
                            first.setdefault(i, now)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, first

    def slots():
        torch.cuda.synchronize()
        t0, first = time.perf_counter(), {}
        for index, _, _, mel in pool.play_many(requests, CHUNK_STEPS):
            mel.cpu()
            first.setdefault(index, time.perf_counter() - t0)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, first

    def summary(runs):
        tot = statistics.median(r[0] for r in runs)
        return dict(utterances_per_s=N_UTT / tot, total_s=tot,
                    first_chunk_median_ms=1e3 * statistics.median(statistics.median(r[1].values()) for r in runs),
                    first_chunk_worst_ms=1e3 * statistics.median(max(r[1].values()) for r in runs),
                    total_s_runs=[r[0] for r in runs])

    with torch.no_grad():
        for _ in range(warmup):
            lockstep()
            slots()
        a, b = [], []
        for _ in range(reps):
            a.append(lockstep())
            b.append(slots())
    rec = dict(lockstep=summary(a), slots=summary(b), reps=reps, frames_min=min(frames), frames_max=max(frames),
               frames_mean=sum(frames) / len(frames))
    rec["slots_over_lockstep_utterances_per_s"] = rec["slots"]["utterances_per_s"] / rec["lockstep"]["utterances_per_s"]
    print("S=%2d  lockstep %.2f utt/s (first chunk median %.1f ms, worst %.1f ms) | slots %.2f utt/s (median %.1f ms, worst "
          "%.1f ms)" % (S, rec["lockstep"]["utterances_per_s"], rec["lockstep"]["first_chunk_median_ms"],
                        rec["lockstep"]["first_chunk_worst_ms"], rec["slots"]["utterances_per_s"],
                        rec["slots"]["first_chunk_median_ms"], rec["slots"]["first_chunk_worst_ms"]), flush=True)
    return {"S=%d" % S: rec}


def launch_check():
    """kantts_pnca_decode_slots (lockstep ranges) against kantts_pnca_decode_range: 8 steps of 32 sequences."""
    torch, hip, m = _model()
    from kantts.models.sambert.chunked import ChunkedAcoustic

    B, t0, t1, n = 32, 64, 64 + CHUNK_STEPS, 20
    batch, _ = _utterances(torch, B)
    batch["duration_targets"] = batch["duration_targets"].clamp(min=6)  # every sequence is alive over [t0, t1)
    with torch.no_grad():
        sess = ChunkedAcoustic(m).open(**batch)
        sess.step(t0)
    dec = m.mel_decoder.mel_dec
    a0 = torch.full((B,), t0, dtype=torch.int32, device="cuda")
    a1 = torch.full((B,), t1, dtype=torch.int32, device="cuda")

    def run(slots):
        kw = dict(slots=(a0, a1)) if slots else dict(steps=(t0, t1))
        rc = hip.pnca_decode_run(sess.dk.w, sess.dk.f, sess.memory, sess.hkv, sess.xkv, sess.out, sess.lens32, sess.ts.bw_dev,
                                 sess.ts.bw_int, sess.d_mel, len(dec.pnca), dec.d_model ** 0.5, dec.ln.eps, **kw)
        assert rc == 0, rc

    def timed(slots):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            run(slots)
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / n  # us per launch

    for s in (False, True):
        timed(s)
    rng, slt = [], []
    for _ in range(5):
        rng.append(timed(False))
        slt.append(timed(True))
    spread = max(rng) - min(rng)
    rec = dict(point="B=32, steps [64, 72), mean of 20 launches per figure", range_us=rng, slots_us=slt,
               range_median_us=statistics.median(rng), slots_median_us=statistics.median(slt), range_spread_us=spread,
               within_bound=statistics.median(slt) - statistics.median(rng) <= spread)
    print("decode launch: range median %.1f us (spread %.1f), slots median %.1f us -> %s" % (
        rec["range_median_us"], spread, rec["slots_median_us"], "within the bound" if rec["within_bound"] else "OVER the bound"),
        flush=True)
    return rec


def driver(a):
    d = {"config": dict(model="SAM-BERT full 16k configuration, random init", precision="bf16", utterances=N_UTT, symbols=T_IN,
                        frames="about 100..800 (durations given)", chunk_steps=CHUNK_STEPS, max_steps=MAX_STEPS), "points": {}}
    tmp = OUT + ".part"
    for job in [["--point", str(S)] for S in POOLS] + [["--launch"]]:
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
            d["decode_launch"] = part
        json.dump(d, open(OUT, "w"), indent=1, sort_keys=True)
        if a.copy_to:  # a second copy, e.g. in the scratch directory a remote run brings back
            os.makedirs(a.copy_to, exist_ok=True)
            json.dump(d, open(os.path.join(a.copy_to, os.path.basename(OUT)), "w"), indent=1, sort_keys=True)
    print(json.dumps(d, sort_keys=True))
    return 0 if d["decode_launch"]["within_bound"] else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--limit", type=int, default=240, help="seconds every child step may take")
    ap.add_argument("--copy-to", default=None, help="directory that also receives the JSON")
    ap.add_argument("--point", type=int, default=None, help="(child) time one pool size")
    ap.add_argument("--launch", action="store_true", help="(child) the per-launch check of the decoder")
    ap.add_argument("--part", default=None, help="(child) where the partial result goes")
    a = ap.parse_args()
    if a.point is not None or a.launch:
        res = launch_check() if a.launch else point(a.point, a.reps, a.warmup)
        json.dump(res, open(a.part, "w"))
        sys.exit(0)
    sys.exit(driver(a))
