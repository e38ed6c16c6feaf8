"""sy-BERT pre-training step at the shipped geometry of sybert.yaml: batch 32, 8 encoder blocks (d_model 128, 8 heads, FFN
1024, embeddings 512), mask_ratio 0.3, V = 147, on 256 seeded synthetic sentences of 20 - 120 symbols.

    python scripts/sybert_bench.py step [rounds=5] [out.json]        # step time and feeder rate -> profiles/sybert.json
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/sybert_bench.py head [reps=50]
    python scripts/sybert_bench.py merge DIR [out.json]              # the head's kernel times from that trace, into the json

``step``: per encoder mode (fp32, bf16) three code paths of THIS tree, each with its own trainer from the same seed, warmed
over one epoch (every batch shape) and then timed in turn -- round r runs path 0, 1, 2, each over whole epochs until at
least one second has passed, a host clock around steps that end in a device synchronise:
  resident_fused   DeviceTextSet feeds Textsy_BERT_Trainer.train_step, the head is ops.mlm_head_ce
  resident_stock   the same with the head as ops.linear + SeqCELoss on stock launches (KANTTS_SYBERT_STOCK_HEAD)
  host_fused       the fused step fed by a DataLoader over BERT_Text_Dataset.collate_fn (in-process, num_workers 0: the
                   cost of the host collate itself; a worker pool can hide it behind the step, at a process start per epoch)
Reported: the median over the rounds of the per-step time, min and max as the spread.  ``feeder``: batches per second of
the resident feeder alone and of the host loader alone (no model), same protocol.

``head``: ``reps`` times forward + backward of the head alone at M = 32 x 64 rows, C = 128, V = 147, mask 0.3, fused and
stock in turn; meant to run under rocprofv3.  ``merge`` sums the kernels of each variant per call from the trace's
kernel_stats.csv."""
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kan-tts_amd"))
import torch  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "sybert.json")
N_SENT, BATCH = 256, 32


def config():
    params = dict(max_len=800, embedding_dim=512, encoder_num_layers=8, encoder_num_heads=8, encoder_num_units=128,
                  encoder_ffn_inner_dim=1024, encoder_dropout=0.1, encoder_attention_dropout=0.1, encoder_relu_dropout=0.1,
                  encoder_projection_units=32, mask_ratio=0.3)
    return {"model_type": "sybert",
            "Model": {"KanTtsTextsyBERT": {
                "params": params,
                "optimizer": {"type": "Adam", "params": {"lr": 0.0001, "betas": [0.9, 0.98], "eps": 1e-9, "weight_decay": 0.0}},
                "scheduler": {"type": "NoamLR", "params": {"warmup_steps": 10000}}}},
            "Loss": {"SeqCELoss": {"enable": True, "params": {"loss_type": "ce"}}},
            "batch_size": BATCH, "grad_norm": 1.0, "log_interval_steps": 10 ** 9}


def loaders(cfg, dev):
    from torch.utils.data import DataLoader

    from kantts.datasets.dataset import SyntheticTextDataset
    from kantts.datasets.device_batching import make_train_loader

    ds = SyntheticTextDataset(cfg, N_SENT)
    cfg["Model"]["KanTtsTextsyBERT"]["params"].update(ds.ling_unit.get_unit_size())
    host = DataLoader(ds, shuffle=True, collate_fn=ds.collate_fn, batch_size=BATCH, num_workers=0)
    return ds, host, make_train_loader("bert", ds, host, dev, BATCH, mode="hbm")


def trainer(cfg, dev, loader):
    from kantts.models import model_builder
    from kantts.train.loss import criterion_builder
    from kantts.train.trainer import Textsy_BERT_Trainer

    torch.manual_seed(0)
    model, opt, sch = model_builder(cfg, dev)
    tr = Textsy_BERT_Trainer(cfg, model, opt, sch, criterion_builder(cfg, dev), dev, None, loader, None, save_dir=None,
                             log_interval=10 ** 9, grad_clip=cfg["grad_norm"])
    tr.set_model_state("train")
    return tr


def timed(fn_epoch, least=1.0):
    """Seconds per item of ``fn_epoch`` (which returns the number of items it ran), over whole epochs for >= ``least`` s."""
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while True:
        n += fn_epoch()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= least:
            return dt / n


def spread(xs, scale=1.0):
    return {"median": statistics.median(xs) * scale, "min": min(xs) * scale, "max": max(xs) * scale, "rounds": len(xs)}


def step_mode(rounds, out_path):
    import kantts._hip as hip
    import kantts.models.sambert.kantts_sambert as ks

    dev = torch.device("cuda", 0)
    result = {"geometry": {"batch": BATCH, "sentences": N_SENT, "symbols": "20-120", "encoder_blocks": 8, "d_model": 128,
                           "V": 147, "mask_ratio": 0.3, "host_loader_workers": 0},
              "device": torch.cuda.get_device_name(0), "step_ms": {}, "feeder_batches_per_s": {}}
    for prec in ("fp32", "bf16"):
        hip.set_precision(prec)
        cfg = config()
        ds, host, resident = loaders(cfg, dev)
        paths = {"resident_fused": (trainer(cfg, dev, resident), False), "resident_stock": (trainer(cfg, dev, resident), True),
                 "host_fused": (trainer(cfg, dev, host), False)}

        def epoch(name):
            tr, stock = paths[name]
            ks._SYBERT_STOCK_HEAD = stock
            n = 0
            for batch in tr.train_loader:
                tr.train_step(batch)
                tr.steps += 1
                n += 1
            tr._device_losses.clear()
            return n

        for name in paths:
            epoch(name)  # warm: every batch shape of the corpus
        times = {name: [] for name in paths}
        for _ in range(rounds):
            for name in paths:
                times[name].append(timed(lambda: epoch(name)))
        ks._SYBERT_STOCK_HEAD = False
        result["step_ms"][prec] = {name: spread(v, 1e3) for name, v in times.items()}
        if prec == "fp32":
            def feed(loader):
                n = 0
                for batch in loader:
                    n += 1
                return n

            feed(resident), feed(host)
            rates = {"resident": [], "host": []}
            for _ in range(rounds):
                rates["resident"].append(1.0 / timed(lambda: feed(resident)))
                rates["host"].append(1.0 / timed(lambda: feed(host)))
            result["feeder_batches_per_s"] = {k: spread(v) for k, v in rates.items()}
    hip.set_precision("fp32")
    if os.path.exists(out_path):  # keep the head's kernel times of an earlier ``merge``
        with open(out_path) as f:
            old = json.load(f)
        if "head_kernel_us" in old:
            result["head_kernel_us"] = old["head_kernel_us"]
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result, sort_keys=True))


def head_mode(reps):
    from kantts._hip import ops
    from kantts.train.loss import SeqCELoss

    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    M, C, V = BATCH * 64, 128, 147
    hid = torch.randn(M, C, generator=g).to(dev).requires_grad_(True)
    W = (torch.randn(V, C, generator=g) / C ** 0.5).to(dev).requires_grad_(True)
    b = torch.zeros(V, device=dev, requires_grad=True)
    tg = torch.randint(0, V, (M,), generator=g).to(dev)
    mk = (torch.rand(M, generator=g) < 0.3).float().to(dev)
    crit = SeqCELoss()
    for _ in range(reps):
        for fused in (True, False):
            hid.grad = W.grad = b.grad = None
            if fused:
                loss, _ = ops.mlm_head_ce(hid, W, b, tg, mk, gscale=1.0 / V)
                loss.backward()
            else:
                loss, _ = crit(ops.linear(hid, W, b), tg, mk)
                (loss / V).backward()
    torch.cuda.synchronize()
    print("head: %d x (fused, stock) forward + backward at M %d, C %d, V %d" % (reps, M, C, V))


def merge_mode(trace_dir, out_path, reps):
    found = glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not found:
        raise SystemExit("no *kernel_stats.csv under %s" % trace_dir)
    fused, stock, rows = 0.0, 0.0, {}
    with open(found[0]) as f:
        for row in csv.DictReader(f):
            name, calls, total_ns = row["Name"], int(row["Calls"]), float(row["TotalDurationNs"])
            rows[name] = {"calls": calls, "total_us": total_ns / 1e3}
            if name.startswith("mlm_"):
                fused += total_ns
            else:
                stock += total_ns
    result = {}
    if os.path.exists(out_path):
        with open(out_path) as f:
            result = json.load(f)
    result["head_kernel_us"] = {"reps": reps, "fused_per_call": fused / 1e3 / reps, "stock_per_call": stock / 1e3 / reps,
                                "fused_launches_per_call": sum(v["calls"] for k, v in rows.items() if k.startswith("mlm_")) / reps,
                                "stock_launches_per_call": sum(v["calls"] for k, v in rows.items() if not k.startswith("mlm_")) / reps,
                                "kernels": rows}
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print(json.dumps(result["head_kernel_us"], sort_keys=True))


if __name__ == "__main__":
    a = sys.argv[1:]
    mode = a[0] if a else "step"
    if mode == "merge":
        merge_mode(a[1], a[2] if len(a) > 2 else OUT, int(a[3]) if len(a) > 3 else 50)
        raise SystemExit(0)
    if not torch.cuda.is_available():
        raise SystemExit("sybert_bench.py measures on the GPU; none found")
    if mode == "step":
        step_mode(int(a[1]) if len(a) > 1 else 5, a[2] if len(a) > 2 else OUT)
    elif mode == "head":
        head_mode(int(a[1]) if len(a) > 1 else 50)
    else:
        raise SystemExit("unknown mode %r" % mode)
