"""GAN step of an NSF generator at the hifigan_v1_nsf_24k geometry (channels 512, scales 8 x 5 x 3 x 2 = hop 240, 7 + 1
harmonics at 24 kHz), batch B x (frames * 240) samples -- 34 frames = 8160 samples, the whole number of frames nearest to the
8192 samples of the README's figure for the non-NSF generator.  Three ways to run the same step, INTERLEAVED (round r times
way 0, 1, 2 in turn, so that a drift of the machine hits all three alike):

  eager_host_draws    gan_train_step, SourceModule.excitation: torch.distributions on the device's generator and ~15 stock
                      launches per generator forward (what an NSF generator ran before the device draw existed)
  eager_device_draws  gan_train_step after Generator.enable_device_excitation: kantts_nsf_draw_states + ops.nsf_excite
  captured            GraphedGanStep (one hipGraph replay per step)

    python scripts/nsf_gan_step_bench.py [B=32] [frames=34] [rounds=5] [steps=6] [precision=bf16] [out.json]

Prints one JSON line: per way the median over the rounds of the per-step time (host clock around `steps` steps that end in
a device synchronise), min and max as the spread, and the last losses."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kan-tts_amd"))
import torch

import kantts._hip as hip
from kantts.models import model_builder
from kantts.train.gan_graph_step import GraphedGanStep
from kantts.train.gan_step import gan_train_step
from kantts.train.loss import criterion_builder

SCALES, KERNELS, SR = [8, 5, 3, 2], [16, 10, 6, 4], 24000


def nsf_config(channels=512):
    opt = {"type": "Adam", "params": {"lr": 2e-4, "betas": [0.5, 0.9], "weight_decay": 0.0}}
    sch = {"type": "MultiStepLR", "params": {"gamma": 0.5, "milestones": [200000, 400000, 600000, 800000]}}
    gen = {"channels": channels, "upsample_scales": SCALES, "upsample_kernal_sizes": KERNELS,
           "nsf_params": {"nb_harmonics": 7, "sampling_rate": SR}}
    return {"model_type": "hifigan", "Model": {
        "Generator": {"params": gen, "optimizer": opt, "scheduler": sch},
        "MultiScaleDiscriminator": {"params": {}, "optimizer": opt, "scheduler": sch},
        "MultiPeriodDiscriminator": {"params": {}, "optimizer": opt, "scheduler": sch}},
        "Loss": {"generator_adv_loss": {"enable": True, "params": {}, "weights": 1.0},
                 "discriminator_adv_loss": {"enable": True, "params": {}, "weights": 1.0},
                 "mel_loss": {"enable": True, "params": {}, "weights": 45.0},
                 "feat_match_loss": {"enable": True, "params": {}, "weights": 2.0}},
        "generator_grad_norm": -1, "discriminator_grad_norm": -1, "discriminator_train_start_steps": 0,
        "generator_train_start_steps": 0}


def main():
    a = sys.argv[1:]
    B = int(a[0]) if len(a) > 0 else 32
    frames = int(a[1]) if len(a) > 1 else 34
    rounds = int(a[2]) if len(a) > 2 else 5
    steps = int(a[3]) if len(a) > 3 else 6
    prec = a[4] if len(a) > 4 else "bf16"
    out_path = a[5] if len(a) > 5 else None
    if not torch.cuda.is_available():
        raise SystemExit("nsf_gan_step_bench.py measures on the GPU; none found")
    hip.set_precision(prec)
    hop = 1
    for s in SCALES:
        hop *= s
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 82, frames, generator=g)
    x[:, -1] = (torch.rand(B, frames, generator=g) > 0.25).float()
    x[:, -2] = (60.0 + 340.0 * torch.rand(B, frames, generator=g)) * x[:, -1]
    x = x.cuda()
    y = torch.randn(B, 1, frames * hop, generator=g).clamp(-1, 1).cuda()
    config = nsf_config()
    ways = {}
    for name in ("eager_host_draws", "eager_device_draws", "captured"):
        torch.manual_seed(0)
        model, optimizer, scheduler = model_builder(config, device="cuda")
        crit = criterion_builder(config, device="cuda")
        if name != "eager_host_draws":
            model["generator"].enable_device_excitation(0)
        if name == "captured":
            step = GraphedGanStep(model, optimizer, scheduler, crit, config, y, x)
        else:
            def step(m=model, o=optimizer, s=scheduler, c=crit):
                return gan_train_step(m, o, s, c, config, y, x, steps=1)
        ways[name] = step
    last = {}
    for name, step in ways.items():  # warm every way up
        for _ in range(2):
            last[name] = step()
        torch.cuda.synchronize()
    times = {name: [] for name in ways}
    for _ in range(rounds):
        for name, step in ways.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                last[name] = step()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps * 1e3)
    res = {"B": B, "frames": frames, "samples": frames * hop, "precision": prec, "rounds": rounds, "steps_per_round": steps}
    for name, t in times.items():
        res[name] = {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t),
                     "losses": {k: float(v.detach()) for k, v in last[name].items()}}
    res["max_mem_GB"] = torch.cuda.max_memory_allocated() / 1e9
    line = json.dumps(res)
    print(line)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
