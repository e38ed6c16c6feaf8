"""Byte-input voices (configs/sambert_16k_MAS_byte.yaml): what the wide alignment CTC and the byte-MAS step cost.

    python scripts/byte_voice_bench.py [--windows W] [--parent-lib libkantts_parent.so] [--time-limit S]
                                       [--out profiles/byte_voice.json]

Four measurements, each named for what it is measured against (device events, windows of the arms alternating inside this
one process; medians, minima and maxima over the windows are reported):

  (i)   ctc_wide: kantts_ctc_attn_wide, loss and gradient in one launch, at (B, T1, T2) = (8, 1500, 800) with seeded ragged
        lengths, against the reference's per-utterance loop (torch.nn.CTCLoss(zero_infinity=True), stock ATen on the device,
        forward and backward, same inputs): the only thing a user had for this width.
  (ii)  ctc_narrow: kantts_ctc_attn at the bench shape (32, 612, 64) in this build against the same entry of
        ``--parent-lib`` (a library built from the parent commit), alternating: the same entry, so this shows no change.
        Without ``--parent-lib`` only this build is timed and the field says so.
  (iii) byte_step: the captured against the eager training step of the full byte-MAS configuration (bf16, batch 8, 300 byte
        tokens, about 1100 frames), same trainer class, same batch.
  (iv)  encoder_launches: host-side launch / copy / fill calls of the text encoder's forward and forward + backward at
        that batch's width (every encoder attention sub-layer leaves csrc/enc_attn.hip above 128 tokens) next to the same
        count at a 64-token batch: the price of not having a fused attention sub-layer for long sequences.

The script ends itself after ``--time-limit`` seconds (exit status 3) and needs a GPU: nothing here is measured on a CPU."""
import argparse
import ctypes
import json
import os
import signal
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "kan-tts_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import kantts._hip as hip  # noqa: E402

_LAUNCH_CALLS = ("hipLaunch", "hipExtLaunch", "hipExtModuleLaunch", "hipModuleLaunch", "hipMemcpy", "hipMemset")


def summary(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "windows": len(xs)}


def device_us(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def alternate(arms, windows, reps):
    out = {name: [] for name in arms}
    for _ in range(windows):
        for name, fn in arms.items():
            out[name].append(device_us(fn, reps))
    return {name: summary(v) for name, v in out.items()}


def ragged(B, T1, T2, seed):
    g = torch.Generator().manual_seed(seed)
    il = torch.randint(T2 // 3, T2 + 1, (B,), generator=g)
    ol = torch.minimum(il + torch.randint(0, T1 - T2, (B,), generator=g), torch.tensor(T1))
    il[0], ol[0] = T2, T1
    return il, ol


def aten_loop(x, il, ol):
    """The reference's AttentionCTCLoss (kantts/train/loss.py:481-508) with stock torch on the device, and its backward."""
    ctc = torch.nn.CTCLoss(zero_infinity=True)
    x = x.detach().requires_grad_(True)
    padded = F.pad(x, pad=(1, 0, 0, 0, 0, 0, 0, 0), value=-1)
    total = 0.0
    for bid in range(x.shape[0]):
        target = torch.arange(1, int(il[bid]) + 1, device=x.device).unsqueeze(0)
        cur = padded[bid].permute(1, 0, 2)[: int(ol[bid]), :, : int(il[bid]) + 1]
        cur = torch.log_softmax(cur[None], dim=3)[0]
        total = total + ctc(cur, target, input_lengths=ol[bid:bid + 1], target_lengths=il[bid:bid + 1])
    (total / x.shape[0]).backward()
    return x.grad


def ctc_raw(lib_entry, x, il32, ol32, ws, loss, grad):
    B, _, T1, T2 = x.shape
    g = hip.CtcArgs()
    g.logits, g.in_lens, g.out_lens = x.data_ptr(), il32.data_ptr(), ol32.data_ptr()
    g.ws, g.loss, g.grad = ws.data_ptr(), loss.data_ptr(), grad.data_ptr()
    g.B, g.T1, g.T2, g.blank, g.grad_scale = B, T1, T2, -1.0, 1.0 / B
    ref = ctypes.byref(g)

    def launch():
        rc = lib_entry(ref, hip.stream())
        if rc != 0:
            raise RuntimeError("ctc entry returned %d" % rc)
    return launch, g


def ctc_case(B, T1, T2, seed):
    g = torch.Generator().manual_seed(seed)
    x = (2.0 * torch.randn(B, 1, T1, T2, generator=g)).cuda()
    il, ol = ragged(B, T1, T2, seed + 1)
    n = int(hip.lib().kantts_ctc_attn_workspace(B, T1, T2))
    bufs = (torch.empty(n, device="cuda"), torch.empty(B, device="cuda"), torch.empty_like(x))
    return x, il, ol, il.to(torch.int32).cuda(), ol.to(torch.int32).cuda(), bufs


def measure_ctc_wide(windows):
    B, T1, T2 = 8, 1500, 800
    x, il, ol, il32, ol32, (ws, loss, grad) = ctc_case(B, T1, T2, 0)
    launch, keep = ctc_raw(hip.lib().kantts_ctc_attn_wide, x, il32, ol32, ws, loss, grad)
    ild, old = il.cuda(), ol.cuda()
    launch()
    ref = aten_loop(x, ild, old)
    err = float((grad - ref).abs().max())
    res = alternate({"kantts_ctc_attn_wide_us": launch, "aten_ctc_loop_fwd_bwd_us": lambda: aten_loop(x, ild, old)}, windows, 5)
    res.update(shape=[B, T1, T2], in_lens=il.tolist(), out_lens=ol.tolist(), workspace_bytes=ws.numel() * 4,
               max_abs_gradient_difference_to_aten=err, against="torch.nn.CTCLoss per utterance on the device, forward + backward")
    res["speedup_at_medians"] = res["aten_ctc_loop_fwd_bwd_us"]["median"] / res["kantts_ctc_attn_wide_us"]["median"]
    return res


def measure_ctc_narrow(windows, parent_lib):
    B, T1, T2 = 32, 612, 64
    x, il, ol, il32, ol32, (ws, loss, grad) = ctc_case(B, T1, T2, 1)
    arms, keep = {}, []
    launch, g = ctc_raw(hip.lib().kantts_ctc_attn, x, il32, ol32, ws, loss, grad)
    keep.append(g)
    arms["this_build_us"] = launch
    res = {"shape": [B, T1, T2], "against": "not measured: no --parent-lib"}
    if parent_lib:
        L = ctypes.CDLL(parent_lib)
        L.kantts_ctc_attn.argtypes = [ctypes.POINTER(hip.CtcArgs), ctypes.c_void_p]
        grad2 = torch.empty_like(grad)
        launch2, g2 = ctc_raw(L.kantts_ctc_attn, x, il32, ol32, ws, loss, grad2)
        keep.append(g2)
        launch()
        launch2()
        torch.cuda.synchronize()
        res["bit_equal_gradient"] = bool(torch.equal(grad, grad2))
        arms["parent_build_us"] = launch2
        res["against"] = "kantts_ctc_attn of a library built from the parent commit, alternating in one process"
    res.update(alternate(arms, windows, 50))
    return res


def byte_batch(B=8, T_in=301, seed=5):
    """A byte batch in collate format: 300 byte tokens for the longest item, 3-4 frames per token."""
    from kantts.datasets.batching import beta_binomial_prior_distribution
    from kantts.utils.synthetic import to_collate_format

    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(T_in // 2, T_in, (B,), generator=g)
    lens[0] = T_in - 1
    olens = (lens.float() * (3.0 + torch.rand(B, generator=g))).long()
    T_mel = (int(olens.max()) + 2) // 3 * 3
    valid = torch.arange(T_mel)[None, :] < olens[:, None]
    pri = torch.zeros(B, T_mel, T_in)
    for b in range(B):
        p = beta_binomial_prior_distribution(int(lens[b]) + 1, int(olens[b]))
        pri[b, :p.shape[0], :p.shape[1]] = p
    return to_collate_format(dict(
        inputs_ling=torch.randint(0, 256, (B, T_in, 1), generator=g), inputs_emotion=torch.randint(0, 33, (B, T_in), generator=g),
        inputs_speaker=torch.zeros(B, T_in, dtype=torch.long), input_lengths=lens, output_lengths=olens,
        mel_targets=torch.randn(B, T_mel, 80, generator=g) * valid[:, :, None], duration_targets=None,
        pitch_targets=torch.randn(B, T_mel, generator=g) * (torch.rand(B, T_mel, generator=g) > 0.3) * valid,
        energy_targets=torch.randn(B, T_mel, generator=g) * valid, attn_priors=pri))


def byte_config():
    import torch_oracle as O

    cfg = dict(O.sambert_config(tiny=False), MAS=True, using_byte=True, byte_index=259)
    for k in ("sy", "tone", "syllable_flag", "word_segment"):
        cfg.pop(k, None)
    return cfg


def trainer(graph):
    from kantts.models import model_builder
    from kantts.train.loss import criterion_builder
    from kantts.train.trainer import Sambert_Trainer

    config = {"model_type": "sambert", "Model": {"KanTtsSAMBERT": {
        "params": byte_config(),
        "optimizer": {"type": "Adam", "params": {"lr": 0.001, "betas": [0.9, 0.98], "eps": 1e-9, "weight_decay": 0.0}},
        "scheduler": {"type": "NoamLR", "params": {"warmup_steps": 4000}}}},
        "Loss": {"MelReconLoss": {"enable": True, "params": {"loss_type": "mae"}},
                 "ProsodyReconLoss": {"enable": True, "params": {"loss_type": "mae"}},
                 "AttentionCTCLoss": {"enable": True},
                 "AttentionBinarizationLoss": {"enable": True, "params": {"start_epoch": 0, "warmup_epoch": 100}}},
        "grad_norm": 1.0, "batch_size": 8, "log_interval_steps": 10 ** 6}
    torch.manual_seed(0)
    model, opt, sch = model_builder(config, device="cuda")
    crit = criterion_builder(config, "cuda")
    tr = Sambert_Trainer(config, model, opt, sch, crit, torch.device("cuda"), None, [], None, max_steps=10 ** 9,
                         save_dir=tempfile.mkdtemp(prefix="byte_voice_bench_"), save_interval=10 ** 9,
                         valid_interval=10 ** 9, log_interval=10 ** 6, grad_clip=1.0, graph=graph)
    tr.epoch = 50
    return tr


def measure_step(windows, steps=10):
    batch = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in byte_batch().items()}
    arms = {"eager_ms": trainer(False), "captured_ms": trainer(True)}
    for tr in arms.values():
        for _ in range(3):
            tr.train_step(batch)
            tr.steps += 1
    torch.cuda.synchronize()
    ms = {name: [] for name in arms}
    for _ in range(windows):
        for name, tr in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.train_step(batch)
                tr.steps += 1
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / steps)
    res = {name: summary(v) for name, v in ms.items()}
    res.update(model="SAM-BERT full, MAS: True, using_byte: True, bf16", batch=8, byte_tokens=int(batch["valid_input_lengths"].max()),
               frames=int(batch["mel_targets"].shape[1]), steps_per_window=steps, captured_steps_built=len(arms["captured_ms"]._graphs),
               against="the eager step of the same trainer on the same batch (host clock around steps ending in a synchronise)")
    res["eager_over_captured_at_medians"] = res["eager_ms"]["median"] / res["captured_ms"]["median"]
    return res, arms["eager_ms"].model["KanTtsSAMBERT"]


def host_launches(fn):
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CPU and e.name.startswith(_LAUNCH_CALLS))


def measure_encoder_launches(model):
    from kantts.models.utils import get_mask_from_lengths

    enc = model.text_encoder
    model.train()
    out = {"against": "the same encoder at a 64-token batch (attention sub-layers in csrc/enc_attn.hip)",
           "counted": "host-side launch / copy / fill calls of one call, from the profiler"}
    for name, T in (("byte_batch_301_tokens", 301), ("phoneme_batch_64_tokens", 64)):
        g = torch.Generator().manual_seed(T)
        ling = torch.randint(0, 256, (8, T, 1), generator=g).cuda()
        lens = torch.full((8,), T - 1, dtype=torch.long).cuda()
        masks = get_mask_from_lengths(lens, max_len=T)

        def fwd():
            with torch.no_grad():
                enc(ling, masks)

        def fwd_bwd():
            y = enc(ling, masks)[0]
            y.float().sum().backward()
        out[name] = {"forward": host_launches(fwd), "forward_backward": host_launches(fwd_bwd),
                     "encoder_layers": len(enc.ling_enc.fft)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="a libkantts_hip.so built from the parent commit (measurement ii)")
    ap.add_argument("--time-limit", type=int, default=420, help="seconds after which the script ends itself")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "byte_voice.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("byte_voice_bench needs a GPU: nothing here is measured on a CPU")

    def expired(*_):
        sys.stderr.write("byte_voice_bench: time limit of %d s reached\n" % args.time_limit)
        os._exit(3)

    signal.signal(signal.SIGALRM, expired)
    signal.alarm(args.time_limit)
    hip.set_precision("bf16")
    result = {"device": torch.cuda.get_device_name(0), "precision": "bf16 (the CTC launches are fp32 in either mode)"}
    result["ctc_wide"] = measure_ctc_wide(args.windows)
    result["ctc_narrow"] = measure_ctc_narrow(args.windows, args.parent_lib)
    result["byte_step"], model = measure_step(args.windows)
    result["encoder_launches"] = measure_encoder_launches(model)
    signal.alarm(0)
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
