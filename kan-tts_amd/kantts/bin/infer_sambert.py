"""SAM-BERT acoustic-model inference entry point: linguistic symbols -> mel (.npy) + duration / f0 / energy text files.

Mirrors kantts/bin/infer_sambert.py:58-239 of the reference: ``am_synthesis(symbol_seq, fsnet, ling_unit, device)`` and
``am_infer(sentence, ckpt, output_dir, se_file=None, config=None)`` with the same outputs (``feat/<id>_mel.npy`` holds
the post-net mel).  The text front-end (``KanTtsLinguisticUnit``) is not part of the hot path: ``am_infer`` imports it
from the reference package layout if it is installed, or accepts any object with ``encode_symbol_sequence`` /
``get_unit_size`` / ``using_byte`` through ``ling_unit=``.  The model itself runs free-running on the MI355X kernels
(AR duration predictor + AR decoder, kantts/models/sambert).
"""
import argparse
import logging
import os
import time

import numpy as np
import torch
import yaml

logging.basicConfig(format="%(asctime)s, %(levelname)-4s [%(filename)s:%(lineno)d] %(message)s",
                    datefmt="%Y-%m-%d:%H:%M:%S", level=logging.INFO)


def am_inputs(symbol_seq, ling_unit, device, se=None):
    """(inputs_ling, inputs_emotion, inputs_speaker, input_lengths) of one sentence, batch 1."""
    feats = ling_unit.encode_symbol_sequence(symbol_seq)
    # byte-input voices carry one symbol stream in front of emotion and speaker, the others four (reference :62-85)
    n_ling = 1 if ling_unit.using_byte() else 4
    *ling, emo, spk = (torch.from_numpy(np.asarray(f)).long().to(device) for f in feats[:n_ling + 2])
    # the trailing "~" token is dropped from every stream (reference :117-122)
    inputs_ling = torch.stack(ling, dim=-1).unsqueeze(0)[:, :-1, :]
    inputs_emo = emo.unsqueeze(0)[:, :-1]
    if se is not None:
        # SE models (sambert_se_nsf_global_16k.yaml): the utterance-level speaker embedding of --se_file, (1, dim),
        # repeated over the symbols instead of speaker ids (reference :99-106)
        inputs_spk = torch.from_numpy(np.asarray(se).repeat(len(feats[n_ling + 1]), axis=0)).float().to(device).unsqueeze(0)[:, :-1, :]
    else:
        inputs_spk = spk.unsqueeze(0)[:, :-1]
    inputs_len = torch.full((1,), inputs_emo.size(1), dtype=torch.long, device=device)
    return inputs_ling, inputs_emo, inputs_spk, inputs_len


def am_outputs(res):
    """What am_synthesis returns, from the dictionary the model (or a streaming session) returns for one utterance."""
    valid_length = int(res["LR_length_rounded"][0].item())
    dec_outputs = res["dec_outputs"][0, :valid_length, :].cpu().numpy()
    postnet_outputs = res["postnet_outputs"][0, :valid_length, :].cpu().numpy()
    duration_predictions = (torch.exp(res["log_duration_predictions"]) - 1 + 0.5).long().squeeze().cpu().numpy()
    pitch_predictions = res["pitch_predictions"].squeeze().cpu().numpy()
    energy_predictions = res["energy_predictions"].squeeze().cpu().numpy()
    logging.info("x_band_width:%s, h_band_width: %s", res["x_band_width"], res["h_band_width"])
    return dec_outputs, postnet_outputs, duration_predictions, pitch_predictions, energy_predictions


def am_synthesis(symbol_seq, fsnet, ling_unit, device, se=None, chunked=None, chunk_steps=None, chunk_times=None):
    """``chunked`` (a ChunkedAcoustic of ``fsnet``) with ``chunk_steps``: the same outputs through a streaming session;
    the seconds after which each chunk's frames were on the host are appended to ``chunk_times``."""
    inputs_ling, inputs_emo, inputs_spk, inputs_len = am_inputs(symbol_seq, ling_unit, device, se=se)
    if chunked is not None:
        t0 = time.time()
        sess = chunked.open(inputs_ling, inputs_emo, inputs_spk, inputs_len)
        for _, hi, mel in sess.stream(chunk_steps):
            if mel.size(1) and chunk_times is not None:
                mel.cpu()  # the copy to the host is when a chunk can be handed on
                chunk_times.append(time.time() - t0)
        res = sess.result()
    else:
        res = fsnet(inputs_ling, inputs_emo, inputs_spk, inputs_len)
    return am_outputs(res)


def denorm_f0(mel, scale, offset, f0_threshold=30.0, uv_threshold=0.6):
    """The last two channels of an NSF acoustic model's output (frames, n_mels + 2): voicing score -> {0, 1} at
    ``uv_threshold``, f0 -> ``f0 * scale + offset`` Hz floored at ``f0_threshold`` (reference :26-56; mean_std: scale = std,
    offset = mean; global: scale = max - min, offset = min).  In place, like the reference."""
    uv = mel[:, -1]
    mel[:, -1] = np.where(uv < uv_threshold, 0.0, 1.0)
    mel[:, -2] = np.maximum(mel[:, -2] * scale + offset, f0_threshold)
    return mel


def load_am(ckpt, se_file=None, config=None, ling_unit=None):
    """What ``am_infer`` runs with: (device, ling_unit, se, nsf, fsnet) -- the model of ``ckpt`` in eval mode on the
    device, the symbol tables, the speaker embedding of ``se_file`` (SE models) and, for NSF models, the (scale, offset)
    of the f0 de-normalisation (from ``mvn.npy`` beside the config, or the global minimum and maximum)."""
    device = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    if not isinstance(config, dict):
        path = config if config is not None else os.path.join(os.path.dirname(os.path.dirname(ckpt)), "config.yaml")
        with open(path) as f:
            config = yaml.load(f, Loader=yaml.Loader)
    if ling_unit is None:  # symbol tables of this package; the sentences file holds symbol sequences, not raw text
        from kantts.utils.ling_unit import KanTtsLinguisticUnit

        ling_unit = KanTtsLinguisticUnit(config)
    config["Model"]["KanTtsSAMBERT"]["params"].update(ling_unit.get_unit_size())
    se_enable = config["Model"]["KanTtsSAMBERT"]["params"].get("SE", False)
    if se_enable and se_file is None:
        raise ValueError("this checkpoint takes a speaker embedding (SE: True): --se_file is required")
    se = np.load(se_file) if se_enable else None  # (the reference ignores --se_file for models without SE, :177-178)
    # NSF acoustic models predict two more channels behind the mel bins -- normalised f0 and a voicing score -- which the
    # vocoder's source module wants in Hz / as a 0-1 flag (reference :26-56, :180-193, :219-220)
    params = config["Model"]["KanTtsSAMBERT"]["params"]
    nsf = None
    if params.get("NSF", False):
        if params.get("nsf_norm_type", "mean_std") == "mean_std":
            mvn = np.load(os.path.join(os.path.dirname(os.path.dirname(ckpt)), "mvn.npy"))  # rows: mean, std of f0
            nsf = (float(np.asarray(mvn[1:]).reshape(-1)[0]), float(np.asarray(mvn[0:1]).reshape(-1)[0]))
        else:  # "global": f0 was mapped to [0, 1] between a global minimum and maximum
            lo, hi = params.get("nsf_f0_global_minimum", 30.0), params.get("nsf_f0_global_maximum", 730.0)
            nsf = (float(hi) - float(lo), float(lo))
    from kantts.models import model_builder

    model, _, _ = model_builder(config, device)
    fsnet = model["KanTtsSAMBERT"]
    logging.info("Loading checkpoint: %s", ckpt)
    fsnet.load_state_dict(torch.load(ckpt, map_location="cpu")["model"], strict=False)
    fsnet.eval()
    if device.type == "cuda":
        # bf16 mode: each autoregressive loop is one launch (kantts/models/sambert/ar_kernels.py); otherwise one decoder
        # step = one hipGraph replay (kantts/models/sambert/decode_graph.py)
        fsnet.mel_decoder.decode_mode = "kernel"
    return device, ling_unit, se, nsf, fsnet


def am_infer(sentence, ckpt, output_dir, se_file=None, config=None, ling_unit=None, chunk_frames=None, slots=None,
             slot_steps=1024):
    """``slots`` (with ``chunk_frames``): the sentences play through a pool of that many independently advancing streaming
    slots (AcousticSlots.play_many, buffers of ``slot_steps`` decoder steps per slot) instead of one session each; the
    files written are the same."""
    device, ling_unit, se, nsf, fsnet = load_am(ckpt, se_file=se_file, config=config, ling_unit=ling_unit)
    results_dir = os.path.join(output_dir, "feat")
    os.makedirs(results_dir, exist_ok=True)
    chunked, chunk_steps, first_chunk, chunk_ms, totals = None, None, [], [], []
    if chunk_frames is not None:
        r = fsnet.mel_decoder.r
        if chunk_frames < 1 or chunk_frames % r:
            raise ValueError("--chunk_frames must be a positive multiple of outputs_per_step (%d), got %d" % (r, chunk_frames))
        from kantts.models.sambert.chunked import ChunkedAcoustic

        chunked, chunk_steps = ChunkedAcoustic(fsnet), chunk_frames // r  # refuses what it cannot stream, loudly
    if slots is not None:
        if chunk_frames is None:
            raise ValueError("--slots needs --chunk_frames")
        if slots < 1:
            raise ValueError("--slots must be positive, got %d" % slots)
        from kantts.models.sambert.slots import AcousticSlots

        pool = AcousticSlots(fsnet, slots=slots, max_steps=slot_steps)  # refuses what it cannot stream, loudly
    with open(sentence, encoding="utf-8") as f:
        lines = [ln for ln in (line.strip().split("\t") for line in f) if len(ln) >= 2]
    if slots is not None:
        with torch.no_grad():
            requests = [am_inputs(line[1], ling_unit, device, se=se) for line in lines]
            results, t0, first = {}, time.time(), {}
            for index, _, _, mel in pool.play_many(requests, chunk_steps, results=results):
                if index not in first:
                    mel.cpu()  # the copy to the host is when a chunk can be handed on
                    first[index] = time.time() - t0
        for index, line in enumerate(lines):
            logging.info("Inference sentence: %s", line[0])
            _, mel_post, dur, f0, energy = am_outputs(results[index])
            if nsf is not None:
                mel_post = denorm_f0(mel_post, scale=nsf[0], offset=nsf[1])
            np.save("%s/%s_mel.npy" % (results_dir, line[0]), mel_post)
            np.savetxt("%s/%s_dur.txt" % (results_dir, line[0]), dur)
            np.savetxt("%s/%s_f0.txt" % (results_dir, line[0]), f0)
            np.savetxt("%s/%s_energy.txt" % (results_dir, line[0]), energy)
        if first:
            logging.info("Finished inference of %d utterances through %d slots (%d frames per chunk, time from the start to an "
                         "utterance's first chunk: median %.2f ms, worst %.2f ms; total %.2f ms).", len(lines), slots,
                         chunk_frames, 1e3 * float(np.median(list(first.values()))), 1e3 * max(first.values()),
                         1e3 * (time.time() - t0))
        return
    for line in lines:
        logging.info("Inference sentence: %s", line[0])
        with torch.no_grad():
            times = []
            _, mel_post, dur, f0, energy = am_synthesis(line[1], fsnet, ling_unit, device, se=se, chunked=chunked,
                                                        chunk_steps=chunk_steps, chunk_times=times)
        if times:
            first_chunk.append(times[0])
            chunk_ms += list(np.diff([0.0] + times))
            totals.append(times[-1])
        if nsf is not None:
            mel_post = denorm_f0(mel_post, scale=nsf[0], offset=nsf[1])
        np.save("%s/%s_mel.npy" % (results_dir, line[0]), mel_post)
        np.savetxt("%s/%s_dur.txt" % (results_dir, line[0]), dur)
        np.savetxt("%s/%s_f0.txt" % (results_dir, line[0]), f0)
        np.savetxt("%s/%s_energy.txt" % (results_dir, line[0]), energy)
    if chunked is not None and first_chunk:
        logging.info("Finished chunked inference of %d utterances (%d frames per chunk, time to first chunk: median %.2f ms, "
                     "first utterance %.2f ms; median chunk %.2f ms; total %.2f ms per utterance).", len(first_chunk),
                     chunk_frames, 1e3 * float(np.median(first_chunk)), 1e3 * first_chunk[0],
                     1e3 * float(np.median(chunk_ms)), 1e3 * float(np.mean(totals)))


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--sentence", type=str, required=True)
    parser.add_argument("--output_dir", type=str, required=True)
    parser.add_argument("--ckpt", type=str, required=True)
    parser.add_argument("--se_file", type=str, required=False)
    parser.add_argument("--slots", type=int, default=None,
                        help="With --chunk_frames: play the sentences through a pool of this many independently advancing "
                             "streaming slots (continuous batching)")
    parser.add_argument("--slot_steps", type=int, default=1024,
                        help="With --slots: decoder steps the buffers of a slot hold (the longest utterance it can take)")
    parser.add_argument("--chunk_frames", type=int, default=None,
                        help="Infer chunk by chunk through a streaming session, this many mel frames at a time (a multiple "
                             "of outputs_per_step; bf16 mode)")
    args = parser.parse_args()
    if args.chunk_frames is not None and args.chunk_frames < 1:
        parser.error("--chunk_frames must be positive")
    if args.slots is not None and args.chunk_frames is None:
        parser.error("--slots needs --chunk_frames")
    try:
        am_infer(args.sentence, args.ckpt, args.output_dir, args.se_file, chunk_frames=args.chunk_frames, slots=args.slots,
                 slot_steps=args.slot_steps)
    except ValueError as e:
        if "--chunk_frames" not in str(e) and "--slots" not in str(e):
            raise
        parser.error(str(e))
