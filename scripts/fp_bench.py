"""Cost of the filled-pause path (FP: True, csrc/fp.hip) on the MI355X.

Two points, each in a child process of its own under ``timeout`` (the children are chained; the first failure ends the run):

  insert  plan + insert, forward + backward, at the shipped sambert_fp_8k geometry (B = 32, T = 80, C = 32, ~10 % labelled
          tokens): ops.fp_plan + ops.fp_insert and their autograd backward against the REFERENCE'S LOOP restated in torch on
          the device (kantts_sambert.py:794-860: one device scalar read per token, a torch.cat per insertion; autograd
          differentiates the cats).  The restatement lives here, not in the product.  Launches (device kernels + copies,
          counted by the profiler in a separate untimed pass) and host reads of both are recorded.
  step    the eager training step (forward, five reconstruction losses + FpCELoss, backward, clip + Adam on the parameter
          arena, bf16 mode) of the full 16k model with FP: True against the same model with FP: False on a batch of the SAME
          shapes downstream of the insertion (token width T', the same durations / targets): the difference is the
          predictor, the three-filler encoder pass, head / plan / insert, FpCELoss and the host read of T' -- minus the
          baseline's encoder running T' instead of T tokens wide.

  captured  the CAPTURED step of the same FP model (GraphedSambertStep with ``fp_criterion``: the insertion planned from the
          given labels at the width of the duration targets, kantts_fp_plan_given, no host read) against the eager FP step
          above -- both on this commit, the eager leg being the path every FP step took before -- and the same pair for the
          ``FP: False`` twin on the shapes downstream of the insertion, so that what FP still costs inside a captured step
          can be read off.  Device launches per step of all four legs, and the number of distinct captured shapes a pass
          over ``--shape_batches`` seeded batches of this geometry builds (FP adds T' to the key beside the mel length).

Timing: host clock around work that ends in a device synchronise; the two legs of a point interleaved, ``--reps`` windows
each after a warm-up of both; median, minimum and maximum of the windows are recorded.

    python scripts/fp_bench.py                 # -> profiles/filled_pause.json                    (needs the GPU)
    python scripts/fp_bench.py --resources     # -> profiles/filled_pause_kernel_resources.txt    (compiler only)
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kan-tts_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
OUT = os.path.join(ROOT, "profiles", "filled_pause.json")
RES = os.path.join(ROOT, "profiles", "filled_pause_kernel_resources.txt")
B, T, C, P_LABEL = 32, 80, 32, 0.1
FP_IDS = {1: [[5, 4, 0, 0], [17, 4, 1, 1], [140, 6, 2, 4]], 2: [[6, 4, 0, 0], [23, 4, 1, 1], [140, 6, 2, 4]],
          3: [[5, 4, 0, 0], [41, 4, 1, 1], [140, 6, 2, 4]]}


def _stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "windows": len(xs)}


def _labels(torch, seed=3):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(T // 2, T, (B,), generator=g)
    lens[0] = T - 1
    valid = torch.arange(T)[None, :] < lens[:, None]
    label = ((torch.rand(B, T, generator=g) < P_LABEL) * torch.randint(1, 4, (B, T), generator=g)) * valid
    return label.long(), lens


def _window(torch, fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3  # ms per call


_LAUNCH_CALLS = ("hipLaunch", "hipExtLaunch", "hipExtModuleLaunch", "hipModuleLaunch", "hipMemcpy", "hipMemset")


def _launches(torch, fn, host_side=False):
    """Device kernels and copies of one call, from the profiler (untimed pass).  ``host_side``: count the runtime's launch /
    copy / fill CALLS instead of the device records -- work issued on several streams at once came back with device records
    missing (the count changed from run to run), the calls are all there."""
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    if host_side:
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CPU
                   and e.name.startswith(_LAUNCH_CALLS))
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


# ---------------------------------------------------------------------------------------------------------------------
def reference_insert(torch, text_hid, fillers, fp_label, inputs_emotion, inputs_speaker, input_lengths, reads):
    """insert_fp of the reference with given labels (kantts_sambert.py:786-860), restated; ``reads`` counts host reads."""
    en, a, e = fillers[0], fillers[1], fillers[2]
    reads[0] += 1
    max_len_ori = int(input_lengths.max())
    fp_number = torch.sum(fp_label > 0, dim=1)
    inter_lengths = input_lengths + 3 * fp_number
    reads[0] += 1
    delta = int(inter_lengths.max()) - max_len_ori
    Tn = text_hid.shape[1]
    if delta > 0:
        if delta > Tn:
            n, bias = delta // Tn, delta % Tn
            text_hid = torch.cat((text_hid, text_hid.repeat(1, n, 1), text_hid[:, :bias, :]), 1)
            inputs_emotion = torch.cat((inputs_emotion, inputs_emotion.repeat(1, n), inputs_emotion[:, :bias]), 1)
            inputs_speaker = torch.cat((inputs_speaker, inputs_speaker.repeat(1, n), inputs_speaker[:, :bias]), 1)
        else:
            text_hid = torch.cat((text_hid, text_hid[:, :delta, :]), 1)
            inputs_emotion = torch.cat((inputs_emotion, inputs_emotion[:, :delta]), 1)
            inputs_speaker = torch.cat((inputs_speaker, inputs_speaker[:, :delta]), 1)
    rows = list(text_hid.unbind(0))  # (the reference assigns into text_hid[i] in place; autograd wants new tensors)
    for i in range(fp_label.shape[0]):
        for j in range(fp_label.shape[1] - 1, -1, -1):
            reads[0] += 1
            v = int(fp_label[i][j])  # the reference compares the device scalar up to three times; one read here
            if v in (1, 2, 3):
                rows[i] = torch.cat((rows[i][:j], (en, a, e)[v - 1], rows[i][j:-3]), 0)
    return torch.stack(rows), inputs_emotion, inputs_speaker, inter_lengths


def point_insert(reps):
    import torch

    import kantts._hip as hip
    from kantts._hip import ops

    assert torch.cuda.is_available(), "needs the GPU"
    hip.lib()
    label, lens = _labels(torch)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(B, T, C, generator=g).cuda().requires_grad_(True)
    fill = torch.randn(3, 3, C, generator=g).cuda().requires_grad_(True)
    emo, spk = torch.randint(0, 33, (B, T), generator=g).cuda(), torch.zeros(B, T, dtype=torch.long).cuda()
    lab_d, lens_d = label.cuda(), lens.cuda()
    lab32, lens32 = lab_d.int(), lens_d.int()
    number = (lab32 > 0).sum(1).int()
    Tp = ops.fp_plan(lab32, lens32, number, emo, spk).Tp
    cot = torch.randn(B, Tp, C, generator=g).cuda()
    reads = [0]

    def product():
        plan = ops.fp_plan(lab32, lens32, number, emo, spk)
        out = ops.fp_insert(x, fill, plan)
        return torch.autograd.grad(out, (x, fill), cot) + (out, plan)

    def baseline():
        out, e_, s_, inter = reference_insert(torch, x, fill, lab_d, emo, spk, lens_d, reads)
        return torch.autograd.grad(out, (x, fill), cot) + (out, e_, s_, inter)

    gp, gb = product(), baseline()
    same = dict(out=torch.equal(gp[2], gb[2]), emo=torch.equal(gp[3].emo, gb[3]), spk=torch.equal(gp[3].spk, gb[4]),
                inter=torch.equal(gp[3].inter_len.long(), gb[5]),
                d_text_maxabs=float((gp[0] - gb[0]).abs().max()), d_fill_maxabs=float((gp[1] - gb[1]).abs().max()))
    reads[0] = 0
    baseline()
    base_reads = reads[0]
    n_prod, n_base = _launches(torch, product), _launches(torch, baseline)
    for _ in range(3):
        product(), baseline()
    tp, tb = [], []
    for _ in range(reps):
        tp.append(_window(torch, product, 200))
        tb.append(_window(torch, baseline, 2))
    return {"geometry": dict(B=B, T=T, C=C, T_out=Tp, labelled=int((label > 0).sum())),
            "product_ms": _stats(tp), "reference_loop_ms": _stats(tb),
            "ratio_of_medians": statistics.median(tb) / statistics.median(tp),
            "device_launches": {"product": n_prod, "reference_loop": n_base},
            "host_reads": {"product": 1, "reference_loop": base_reads}, "same_results": same}


# ---------------------------------------------------------------------------------------------------------------------
def _fp_batch(torch, fp, seed=3, cuda=True):
    """FP: tokens (B, T) + labels, targets as wide as the sequences after the insertion (T').  Not FP: tokens (B, T') of
    the inter lengths, the same targets."""
    label, lens = _labels(torch, seed)
    inter = lens + 3 * (label > 0).sum(1)
    Tp = T + int(inter.max()) - int(lens.max())
    g = torch.Generator().manual_seed(seed + 2)
    vocab = (147, 10, 8, 8)
    Tw = T if fp else Tp
    ling = torch.stack([torch.randint(0, vocab[k] - 3, (B, Tw), generator=g) for k in range(4)], -1)
    emo, spk = torch.randint(0, 33, (B, Tw), generator=g), torch.zeros(B, Tw, dtype=torch.long)
    g = torch.Generator().manual_seed(seed + 3)
    dur = torch.randint(2, 17, (B, Tp), generator=g) * (torch.arange(Tp)[None, :] < inter[:, None])
    out_lens = dur.sum(1)
    T_mel = -(-int(out_lens.max()) // 3) * 3
    for b in range(B):
        if int(inter[b]) < Tp:
            dur[b, inter[b]] = T_mel - out_lens[b]
        else:
            dur[b, Tp - 1] += T_mel - out_lens[b]
            out_lens[b] = T_mel
    mel = torch.randn(B, T_mel, 80, generator=g) * (torch.arange(T_mel)[None, :, None] < out_lens[:, None, None])
    batch = dict(inputs_ling=ling, inputs_emotion=emo, inputs_speaker=spk, input_lengths=lens if fp else inter,
                 output_lengths=out_lens, mel_targets=mel, duration_targets=dur, pitch_targets=torch.randn(B, Tp, generator=g),
                 energy_targets=torch.randn(B, Tp, generator=g))
    if fp:
        batch["fp_label"] = label
    return {k: v.cuda() for k, v in batch.items()} if cuda else batch


def _step_legs(torch, fps=(True, False)):
    """{fp: (net, opt, batch, eager step)}: the full 16k model, bf16 mode, arena Adam, one batch of the bench geometry."""
    import torch_oracle as O
    from kantts._hip import ops
    from kantts.models.sambert.kantts_sambert import KanTtsSAMBERT
    from kantts.train.loss import FpCELoss, MelReconLoss, ProsodyReconLoss, sambert_loss_sum
    from kantts.train.optim import ArenaAdam, ParamArena

    legs = {}
    for fp in fps:
        cfg = dict(O.sambert_config(), FP=fp)
        torch.manual_seed(0)
        net = KanTtsSAMBERT(cfg).cuda().train()
        if fp:
            net.fp_dict = {k: torch.tensor(v).unsqueeze(0).cuda() for k, v in FP_IDS.items()}
        opt = ArenaAdam(ParamArena(net, bf16_shadow=True), lr=1e-3, betas=(0.9, 0.98), eps=1e-9)
        opt.set_grad_clip(1.0)
        batch = _fp_batch(torch, fp)
        crit = (MelReconLoss(), ProsodyReconLoss(), FpCELoss())

        def step(net=net, opt=opt, batch=batch, fp=fp, crit=crit):
            ops.advance_rng(torch.device("cuda"))
            res = net(**batch)
            total, _ = sambert_loss_sum(crit[0], crit[1], batch, res, prosody_lengths=res["valid_inter_lengths"])
            if fp:
                total = total + crit[2](batch["input_lengths"], res["fp_predictions"], batch["fp_label"])
            opt.zero_grad()
            total.backward()
            opt.step()
            return total

        legs[fp] = (net, opt, batch, step)
    return legs


def _schedule_launches(torch, step, overlap):
    """Device kernels and copies of the schedule ``step`` (a GraphedSambertStep) captured, from one uncaptured run of it
    with the switches the capture had (``overlap``: weight gradients beside the chain / grouped)."""
    from kantts._hip import deferred_tn, ops

    prev = (ops.wgrad_overlap.enabled, deferred_tn.enabled, ops.side_branch.enabled)
    ops.wgrad_overlap.enable(overlap, group_wgrads=overlap)

    def run():
        with torch.cuda.stream(step._cap_stream):
            step._eager_step()

    try:
        step._cap_stream.wait_stream(torch.cuda.current_stream())
        n = _launches(torch, run, host_side=True)
    finally:
        ops.wgrad_overlap.join()
        ops.wgrad_overlap.enabled, deferred_tn.enabled, ops.side_branch.enabled = prev
    return n


def point_captured(reps, shape_batches=64):
    import torch

    import kantts._hip as hip
    from kantts.models.sambert.kantts_sambert import fp_width_of
    from kantts.train.graph_step import GraphedSambertStep
    from kantts.train.loss import FpCELoss, MelReconLoss, ProsodyReconLoss
    from kantts.train.scheduler import NoamLR

    assert torch.cuda.is_available(), "needs the GPU"
    hip.set_precision("bf16")
    # the eager legs on models of their own, the captured legs on twins from the same seed (a captured step switches its
    # model to the static path and its optimizer to device-side state)
    eager, cap = _step_legs(torch), _step_legs(torch)
    steps = {}
    for fp in (True, False):
        steps[("eager", fp)] = eager[fp][3]
        net, opt, batch, _ = cap[fp]
        kw = {}
        if fp:
            kw = dict(fp_criterion=FpCELoss(), fp_width=fp_width_of(batch["fp_label"].cpu(), batch["input_lengths"].cpu()))
        steps[("captured", fp)] = GraphedSambertStep(net, opt, NoamLR(opt, warmup_steps=4000), MelReconLoss(),
                                                     ProsodyReconLoss(), batch, **kw)
    # a third captured leg: the twin with every weight gradient in line, as the FP step is captured (its text encoder runs
    # twice per forward, so its parameters receive two gradients per backward: graph_step.py) -- what that form costs
    net, opt, batch, _ = _step_legs(torch, fps=(False,))[False]
    steps[("captured_inline_wgrad", False)] = GraphedSambertStep(net, opt, NoamLR(opt, warmup_steps=4000), MelReconLoss(),
                                                                 ProsodyReconLoss(), batch, overlap_wgrad=False,
                                                                 group_wgrads=False)
    order = [("eager", True), ("captured", True), ("eager", False), ("captured", False), ("captured_inline_wgrad", False)]
    for _ in range(5):
        last = {k: steps[k]() for k in order}
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v)) for v in last.values()), last
    steps[("captured", True)].check_fp_status()
    t = {k: [] for k in order}
    for _ in range(reps):
        for k in order:
            t[k].append(_window(torch, steps[k], 10))
    # launches per step: the eager legs from the profiler's device records; a captured step is one graph launch, so its
    # NODES are counted by running the schedule it captured once more uncaptured (the same host code on the capture
    # stream) and counting the runtime's launch / copy / fill calls
    launches = {}
    for k in order:
        name = "%s_fp_%s" % (k[0], str(k[1]).lower())
        if k[0] == "eager":
            launches[name] = _launches(torch, steps[k])
            launches[name + "_calls"] = _launches(torch, steps[k], host_side=True)  # the same number: the two counts agree
        else:
            launches[name] = _schedule_launches(torch, steps[k], k[0] == "captured" and not k[1])
    steps[("captured", True)].check_fp_status()
    # distinct captured shapes over a pass of seeded batches of this geometry (host only): the trainer keys its graphs on
    # the shapes of the batch's tensors, to which FP adds T' (durations, pitch, energy) beside T and the mel length
    keys_fp, keys_plain = set(), set()
    for seed in range(100, 100 + shape_batches):
        b = _fp_batch(torch, True, seed=seed, cuda=False)
        keys_fp.add((b["inputs_ling"].size(1), b["duration_targets"].size(1), b["mel_targets"].size(1)))
        keys_plain.add((b["duration_targets"].size(1), b["mel_targets"].size(1)))
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"model": "full 16k SAM-BERT, bf16 mode, arena Adam",
            "geometry": dict(B=B, T=T, T_out=eager[True][2]["duration_targets"].size(1)),
            "fp_true_eager_ms": _stats(t[("eager", True)]), "fp_true_captured_ms": _stats(t[("captured", True)]),
            "fp_false_eager_ms": _stats(t[("eager", False)]), "fp_false_captured_ms": _stats(t[("captured", False)]),
            "fp_false_captured_inline_wgrad_ms": _stats(t[("captured_inline_wgrad", False)]),
            "fp_cost_against_the_inline_wgrad_twin_ms": med[("captured", True)] - med[("captured_inline_wgrad", False)],
            "eager_over_captured_fp_true": med[("eager", True)] / med[("captured", True)],
            "fp_cost_inside_a_captured_step_ms": med[("captured", True)] - med[("captured", False)],
            "device_launches_per_step": launches,
            "captured_shapes": {"batches": shape_batches, "distinct_with_fp": len(keys_fp),
                                "distinct_fp_false_twin": len(keys_plain), "lru": 16}}


def point_step(reps):
    import torch

    import kantts._hip as hip

    assert torch.cuda.is_available(), "needs the GPU"
    hip.set_precision("bf16")
    legs = {fp: leg[3] for fp, leg in _step_legs(torch).items()}
    for _ in range(5):
        a, b_ = legs[True](), legs[False]()
    assert bool(torch.isfinite(a)) and bool(torch.isfinite(b_))
    t = {True: [], False: []}
    for _ in range(reps):
        for fp in (True, False):
            t[fp].append(_window(torch, legs[fp], 10))
    return {"model": "full 16k SAM-BERT, bf16 mode, eager step, arena Adam", "geometry": dict(B=B, T=T),
            "fp_true_ms": _stats(t[True]), "fp_false_ms": _stats(t[False]),
            "difference_of_medians_ms": statistics.median(t[True]) - statistics.median(t[False])}


# ---------------------------------------------------------------------------------------------------------------------
def resources():
    """Registers / LDS / scratch / occupancy of the kernels of csrc/fp.hip as the compiler reports them (no GPU)."""
    csrc = os.path.join(ROOT, "kan-tts_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-comment",
                            "-Rpass-analysis=kernel-resource-usage", "-c", "fp.hip", "-o", os.path.join(tmp, "fp.o")],
                           cwd=csrc, capture_output=True, text=True, check=True)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1)}
            rows.append(cur)
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]+\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    with open(RES, "w") as f:
        f.write("csrc/fp.hip, gfx950, -O3 (hipcc -Rpass-analysis=kernel-resource-usage)\n")
        f.write("%-44s %5s %5s %5s %7s %6s %4s %7s\n" % ("kernel", "SGPR", "VGPR", "AGPR", "scratch", "spills", "occ", "LDS"))
        for r_ in rows:
            name = re.sub(r"^_Z\d+", "", r_["name"]).split("PK")[0]
            f.write("%-44s %5d %5d %5d %7d %6d %4d %7d\n" % (name, r_.get("TotalSGPRs", 0), r_.get("VGPRs", 0), r_.get("AGPRs", 0),
                                                            r_.get("ScratchSize", 0), r_.get("VGPRs Spill", 0),
                                                            r_.get("Occupancy", 0), r_.get("LDS Size", 0)))
    print(open(RES).read())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--point", choices=["insert", "step", "captured"])
    ap.add_argument("--only", choices=["insert", "step", "captured"], help="run this point alone and merge it into --out")
    ap.add_argument("--shape_batches", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.resources:
        return resources()
    if a.point:
        fn = {"insert": point_insert, "step": point_step,
              "captured": lambda reps: point_captured(reps, a.shape_batches)}[a.point]
        print("RESULT " + json.dumps(fn(a.reps)))
        return
    result = {}
    if a.only and os.path.exists(a.out):
        with open(a.out) as f:
            result = json.load(f)
    for point, limit in (("insert", 240), ("step", 300), ("captured", 420)):
        if a.only and point != a.only:
            continue
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--point", point,
                            "--reps", str(a.reps)], capture_output=True, text=True)
        sys.stderr.write(r.stderr[-3000:])
        if r.returncode != 0:
            sys.exit("point %s ended with status %d; nothing further is started" % (point, r.returncode))
        result[point] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        print(point, json.dumps(result[point], indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
