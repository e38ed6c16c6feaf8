"""Feeding the captured MAS training step: the host collate with per-utterance host priors behind a PinnedPrefetcher (the
only path a MAS voice had) against the device-resident corpus (DeviceAMSet.batch: the prior from kantts_attn_prior_rows).

    python scripts/mas_corpus_bench.py [--epochs N] [--windows W] [--out profiles/mas_device_corpus.json]

Corpus: synthetic, 256 utterances, 200-800 frames, 20-120 symbols (incl. "~"), r = 3, 80 bins; batch 32, the same eight
index batches every epoch (one captured step per padded shape -- seven: two batches share one --, built before anything
is timed).  The host feeder is the loop a
DataLoader(num_workers=0) over AM_Dataset runs, minus the np.load of the features: per utterance
``beta_binomial_prior_distribution`` (behind its lru_cache of 256), per batch ``am_collate``.  The corpus has exactly 256
utterances, so after one epoch every (P, M) pair sits in that cache -- a real corpus has thousands and misses on almost
every utterance.  Both states are timed: "cold" clears the cache before every epoch, "warm" never does.

Reported: batches per second of each feeder alone (every batch on the device, one synchronisation per epoch); ms per
captured step of the full SAM-BERT MAS model (bf16) fed by each, windows of the three feeders alternating; the prior launch
alone (device events over repeated launches into one buffer) against the bytes it stores, next to a fill of the same
buffer.  No reference run, no network."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "kan-tts_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import kantts._hip as hip  # noqa: E402
from kantts.datasets.batching import am_collate, beta_binomial_prior_distribution  # noqa: E402
from kantts.datasets.device_batching import DeviceAMSet, DeviceCorpusLoader, PinnedPrefetcher  # noqa: E402

R, BATCH, PAD_IDS = 3, 32, [146, 9, 7, 7, 35, 3]


def corpus(n=256, seed=0):
    rng = np.random.RandomState(seed)
    hi = (140, 7, 5, 5, 30, 1)
    items = []
    for _ in range(n):
        nsym, frames = int(rng.randint(20, 121)), int(rng.randint(200, 801))
        ling = [rng.randint(0, hi[k], size=nsym).astype(np.int64) for k in range(6)]
        f0 = (rng.randn(frames) * (rng.rand(frames) > 0.3)).astype(np.float32)
        items.append((ling, rng.randn(frames, 80).astype(np.float32), None, f0, rng.randn(frames).astype(np.float32), None,
                      None, None))
    return items


class HostLoader:
    """AM_Dataset.__getitem__ (the prior per utterance) + collate_fn per batch, in this process."""

    def __init__(self, items, index_batches, cold):
        self.items, self.index_batches, self.cold = items, index_batches, cold

    def __iter__(self):
        if self.cold:
            beta_binomial_prior_distribution.cache_clear()
        for idx in self.index_batches:
            batch = []
            for i in idx:
                it = self.items[i]
                batch.append(it[:5] + (beta_binomial_prior_distribution(len(it[0][0]), len(it[1])),) + it[6:])
            yield am_collate(batch, R, PAD_IDS)


def summary(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "windows": len(xs)}


def same_batches(feeders):
    ref = list(feeders["host_warm"])
    ok, worst = True, 0.0
    for a, b in zip(ref, feeders["device"]):
        for k, v in a.items():
            if v is None:
                ok &= b[k] is None
            elif k == "attn_priors":
                r = v.double().cpu()
                err = (b[k].double().cpu() - r).abs() / (2.0 ** -23 * r + 2.0 ** -126)
                worst = max(worst, float(err.max()))
            else:
                ok &= bool(torch.equal(v.cpu(), b[k].cpu()))
    return {"all_other_fields_bit_equal": bool(ok), "prior_worst_error_over_tolerance": worst}


def trainer(dev):
    import torch_oracle as O
    from kantts.models import model_builder
    from kantts.train.loss import criterion_builder
    from kantts.train.trainer import Sambert_Trainer

    cfg = dict(O.sambert_config(tiny=False), MAS=True)
    config = {"model_type": "sambert", "Model": {"KanTtsSAMBERT": {
        "params": cfg,
        "optimizer": {"type": "Adam", "params": {"lr": 0.001, "betas": [0.9, 0.98], "eps": 1e-9, "weight_decay": 0.0}},
        "scheduler": {"type": "NoamLR", "params": {"warmup_steps": 4000}}}},
        "Loss": {"MelReconLoss": {"enable": True, "params": {"loss_type": "mae"}},
                 "ProsodyReconLoss": {"enable": True, "params": {"loss_type": "mae"}},
                 "AttentionCTCLoss": {"enable": True},
                 "AttentionBinarizationLoss": {"enable": True, "params": {"start_epoch": 0, "warmup_epoch": 100}}},
        "grad_norm": 1.0, "batch_size": BATCH, "log_interval_steps": 10 ** 6}
    torch.manual_seed(0)
    model, opt, sch = model_builder(config, device=dev)
    crit = criterion_builder(config, dev)
    tr = Sambert_Trainer(config, model, opt, sch, crit, torch.device(dev), None, [], None, max_steps=10 ** 9,
                         save_dir=tempfile.mkdtemp(prefix="mas_corpus_bench_"), save_interval=10 ** 9,
                         valid_interval=10 ** 9, log_interval=10 ** 6, grad_clip=1.0, graph=True)
    tr.epoch = 50
    return tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=4, help="epochs (of 8 batches) per timed window")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mas_device_corpus.json"))
    ap.add_argument("--no-step", action="store_true", help="feeders and the prior launch only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mas_corpus_bench needs a GPU: nothing here is measured on a CPU")
    dev = "cuda"
    hip.set_precision("bf16")
    items = corpus()
    order = np.random.RandomState(1).permutation(len(items))
    index_batches = [order[i:i + BATCH].tolist() for i in range(0, len(items), BATCH)]
    dset = DeviceAMSet(items, R, PAD_IDS, dev)
    feeders = {
        "host_cold": PinnedPrefetcher(HostLoader(items, index_batches, cold=True), dev),
        "host_warm": PinnedPrefetcher(HostLoader(items, index_batches, cold=False), dev),
        "device": DeviceCorpusLoader(dset, BATCH, batches=index_batches),
    }
    result = {"corpus": {"utterances": len(items), "frames": "200-800", "symbols": "20-120", "r": R, "num_mels": 80,
                         "batch": BATCH, "batches_per_epoch": len(index_batches),
                         "resident_bytes": int(sum(t.numel() * t.element_size() for t in (dset.ling, dset.mel, dset.f0,
                                                                                           dset.energy, dset.lfact)))},
              "same_batches": same_batches(feeders)}

    # 1. the feeders alone
    def feeder_rate(loader, epochs):
        n = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(epochs):
            for batch in loader:
                n += 1
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)

    epochs = {"host_cold": 1, "host_warm": 4, "device": 40}
    for name, loader in feeders.items():
        feeder_rate(loader, 1)
    rates = {name: [] for name in feeders}
    for _ in range(args.windows):
        for name, loader in feeders.items():
            rates[name].append(feeder_rate(loader, epochs[name]))
    result["feeder_batches_per_s"] = {name: summary(v) for name, v in rates.items()}

    # 2. the prior launch alone, at the widest batch of the corpus
    n_sym, n_mel = dset.n_sym[index_batches[0]], dset.n_mel[index_batches[0]]
    Tin, Tout = int(n_sym.max()), (int(n_mel.max()) + R - 1) // R * R
    d_sym, d_mel = (torch.as_tensor(a, dtype=torch.int32).to(dev) for a in (n_sym, n_mel))
    out = torch.empty(BATCH, Tout, Tin, device=dev)

    def device_us(fn, reps=200):
        for _ in range(20):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / reps

    def launch():
        hip.check(hip.attn_prior_rows_raw(dset.lfact, dset.lfact.numel(), d_sym, d_mel, out, B=BATCH, Tout=Tout, Tin=Tin),
                  "attn_prior_rows")

    us = summary([device_us(launch) for _ in range(args.windows)])
    fill = summary([device_us(lambda: out.zero_()) for _ in range(args.windows)])
    wrapper = summary([device_us(lambda: hip.attn_prior_rows(dset.lfact, n_sym, n_mel, Tout, Tin)) for _ in range(args.windows)])
    t0 = time.perf_counter()
    for p, m in zip(n_sym, n_mel):
        beta_binomial_prior_distribution.__wrapped__(int(p), int(m))
    host_ms = (time.perf_counter() - t0) * 1e3
    result["prior_launch"] = {"shape": [BATCH, Tout, Tin], "bytes_stored": out.numel() * 4,
                              "live_cells": int((n_sym * n_mel).sum()), "us_per_launch": us,
                              "stored_GB_per_s_at_median": out.numel() * 4 / us["median"] * 1e-3,
                              "fill_same_buffer_us": fill, "us_per_call_with_length_upload_and_allocation": wrapper,
                              "host_priors_of_the_same_batch_ms": host_ms}

    # 3. the captured step fed by each
    if not args.no_step:
        tr = trainer(dev)
        for name in ("host_warm", "device"):  # builds the captured steps (one per padded shape); both feeders give the same shapes
            for batch in feeders[name]:
                tr.train_step(batch)
                tr.steps += 1
        torch.cuda.synchronize()
        step_ms = {name: [] for name in feeders}
        for _ in range(args.windows):
            for name, loader in feeders.items():
                n_ep = 1 if name == "host_cold" else args.epochs
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n_ep):
                    for batch in loader:
                        tr.train_step(batch)
                        tr.steps += 1
                torch.cuda.synchronize()
                step_ms[name].append((time.perf_counter() - t0) * 1e3 / (n_ep * len(index_batches)))
        result["captured_step_ms"] = {name: summary(v) for name, v in step_ms.items()}
        result["captured_step_ms"]["captured_steps_built"] = len(tr._graphs)
        result["captured_step_ms"]["model"] = "SAM-BERT full, MAS: True, bf16, batch 32"
    print(json.dumps(result))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
