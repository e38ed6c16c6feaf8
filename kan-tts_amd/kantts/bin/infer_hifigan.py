"""HiFi-GAN inference entry point: mel (.npy, (T, C)) -> 16-bit wav, with the real-time factor the reference logs.

Mirrors kantts/bin/infer_hifigan.py:34-163 of the reference (same function names, arguments, checkpoint layout
``states["model"]["generator"]``, ``<ckpt>/../../config.yaml`` discovery, ``<utt>_gen.wav`` outputs).  The generator
runs on the MI355X kernels (kantts/models/hifigan); wav files are written with scipy (soundfile is not a
dependency here).  NSF generators take (T, C + 2) features whose last column (voiced flag) is re-binarised first, as in
the reference (:52-63, :112-113); multi-band generators are followed by their PQMF synthesis (:47-52, :120-121).

``--chunk_frames N``: the same outputs produced chunk by chunk through kantts.models.hifigan.chunked.ChunkedVocoder
(carried convolution state; causal generators), with the time to the first chunk logged beside
the RTF.  Absent: the whole-utterance path, unchanged.  ``--slots S`` (with ``--chunk_frames``): S utterances at a time,
each slot taking the next file as soon as its utterance ends (``ChunkedVocoder.play_many``); the same files are written.
NSF generators play through kantts.models.hifigan.chunked_nsf.ChunkedNSFVocoder (a streamed sine excitation): utterance i
of the sorted input list gets the noise and initial phases of ``(--seed, i)``, whatever the chunk size and the slots.
Non-causal generators (single band, no source module) play through kantts.models.hifigan.chunked_nc.ChunkedNCVocoder: the
network's look-ahead becomes a delay (logged; 3424 samples for the shipped non-causal geometry) that is flushed at the end.
Non-causal NSF generators (the vocoders of sambert_nsf_16k and sambert_se_nsf_global_16k) play through
kantts.models.hifigan.chunked_nc_nsf.ChunkedNCNSFVocoder: both of the above -- the excitation of ``(--seed, i)``, stopped at
the utterance's end, and the same delay, since the source module adds none.
Multi-band generators play through kantts.models.hifigan.chunked_mb.ChunkedMBVocoder (a PQMF synthesis that holds back the
samples whose future it has not seen): the chunks have variable lengths and add up to the one-shot path's sample count.
"""
import argparse
import glob
import logging
import os
import time

import numpy as np
import torch
import yaml
from scipy.io import wavfile

logging.basicConfig(format="%(asctime)s, %(levelname)-4s [%(filename)s:%(lineno)d] %(message)s",
                    datefmt="%Y-%m-%d:%H:%M:%S", level=logging.INFO)


def count_parameters(model):
    return sum(p.numel() for p in model.parameters() if p.requires_grad)


def _load_config(ckpt, config):
    if isinstance(config, dict):
        return config
    path = config if config is not None else os.path.join(os.path.dirname(os.path.dirname(ckpt)), "config.yaml")
    if not os.path.exists(path):
        raise ValueError("config file not found: {}".format(path))
    with open(path) as f:
        return yaml.load(f, Loader=yaml.Loader)


def load_model(ckpt, config=None):
    config = _load_config(ckpt, config)
    from kantts.models.hifigan.hifigan import Generator

    params = config["Model"]["Generator"]["params"]
    model = Generator(**params)
    states = torch.load(ckpt, map_location="cpu")
    model.load_state_dict(states["model"]["generator"])
    if params.get("out_channels", 1) > 1:  # multi-band generator: PQMF synthesis after it (reference :47-52, :120-121)
        from kantts.models.pqmf import PQMF

        model.pqmf = PQMF(subbands=params["out_channels"], **config.get("pqmf", {}))
    return model


def binarize(mel, threshold=0.6):
    """NSF features: the voiced / unvoiced column (last) predicted by the acoustic model back to {0, 1}."""
    out = np.array(mel, copy=True)
    out[:, -1] = (mel[:, -1] >= threshold).astype(out.dtype)
    return out


def _device():
    return torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")


def _write_wav(output_dir, utt_id, sr, y):
    wavfile.write(os.path.join(output_dir, "%s_gen.wav" % utt_id), sr, (np.clip(y, -1.0, 1.0) * 32767.0).astype(np.int16))


def _load_feats(model, path, device):
    feats = np.load(path)
    if model.nsf_enable:
        feats = binarize(feats)
    return torch.from_numpy(np.ascontiguousarray(feats)).float().to(device)


def _chunked_vocoder(model, slots, device, seed):
    """The chunked player of ``model``; the class refuses what it cannot play, loudly."""
    from kantts.models.hifigan import chunked_vocoder_class

    cls = chunked_vocoder_class(model, lookahead=True)
    vocoder = cls(model, slots=slots, graph=device.type == "cuda", **({"seed": seed} if cls._plays_nsf else {}))
    if cls._plays_noncausal:
        logging.info("Non-causal%s generator: the waveform comes %d samples (%d frames) after the frames it is made of.",
                     " NSF" if model.nsf_enable else "", vocoder.delay_samples, vocoder.flush_frames)
    return vocoder


def _infer_many(model, mel_lst, output_dir, sr, chunk_frames, slots, device, seed=0):
    """The directory through ``slots`` vocoder slots with continuous batching; an utterance's file is written when its last
    chunk has arrived."""
    vocoder = _chunked_vocoder(model, slots, device, seed)
    pcm_len = 0
    with torch.no_grad():
        start = time.time()
        mels = [_load_feats(model, mel, device).transpose(1, 0) for mel in mel_lst]
        parts, got = {}, {}
        for i, wav in vocoder.play_many(mels, chunk_frames=chunk_frames):
            parts.setdefault(i, []).append(wav.reshape(-1).cpu())
            got[i] = got.get(i, 0) + wav.shape[-1]  # in samples: the chunks of a multi-band voice are no multiples of hop
            if got[i] >= mels[i].shape[1] * vocoder.hop:
                y = torch.cat(parts.pop(i)).numpy()
                pcm_len += len(y)
                _write_wav(output_dir, os.path.splitext(os.path.basename(mel_lst[i]))[0], sr, y)
        rtf = (time.time() - start) / max(pcm_len / sr, 1e-9)
    logging.info("Finished chunked generation of %d utterances on %d slots (%d frames per chunk, RTF = %.03f).",
                 len(mel_lst), slots, chunk_frames, rtf)
    return rtf


def hifigan_infer(input_mel, ckpt_path, output_dir, config=None, chunk_frames=None, slots=1, seed=0):
    slots = int(slots)
    if slots < 1:
        raise ValueError("slots must be >= 1")
    if slots > 1 and chunk_frames is None:
        raise ValueError("slots > 1 needs chunk_frames (the slots belong to the chunked vocoder)")
    device = _device()
    config = _load_config(ckpt_path, config)
    os.makedirs(output_dir, exist_ok=True)
    if os.path.isfile(input_mel):
        mel_lst = [input_mel]
    elif os.path.isdir(input_mel):
        mel_lst = sorted(glob.glob(os.path.join(input_mel, "*.npy")))
    else:
        raise ValueError("input_mel should be a file or a directory")
    model = load_model(ckpt_path, config)
    logging.info("Loaded model parameters from %s (%d parameters).", ckpt_path, count_parameters(model))
    model.remove_weight_norm()
    model = model.eval().to(device)
    sr = config["audio_config"]["sampling_rate"]
    if slots > 1:
        return _infer_many(model, mel_lst, output_dir, sr, chunk_frames, slots, device, seed)
    pcm_len = 0
    vocoder, first_chunk = None, []
    if chunk_frames is not None:
        vocoder = _chunked_vocoder(model, 1, device, seed)
    with torch.no_grad():
        start = time.time()
        for index, mel in enumerate(mel_lst):
            utt_id = os.path.splitext(os.path.basename(mel))[0]
            feats = np.load(mel)
            if model.nsf_enable:
                feats = binarize(feats)
            mel_data = torch.from_numpy(np.ascontiguousarray(feats)).float().to(device)
            if vocoder is not None:
                t0, parts = time.time(), []
                key = {"key": index} if model.nsf_enable else {}  # the utterance's excitation, as play_many names it
                for wav in vocoder.synthesize(mel_data.transpose(1, 0), chunk_frames=chunk_frames, **key):
                    parts.append(wav.reshape(-1).cpu())  # the copy to the host is when a chunk can be played
                    if len(parts) == 1:
                        first_chunk.append(time.time() - t0)
                y = torch.cat(parts)
            else:
                y = model(mel_data.transpose(1, 0).unsqueeze(0))  # (T, C) -> (1, C, T)
                if hasattr(model, "pqmf"):
                    y = model.pqmf.synthesis(y)
            y = y.reshape(-1).cpu().numpy()
            pcm_len += len(y)
            wavfile.write(os.path.join(output_dir, "%s_gen.wav" % utt_id), sr,
                          (np.clip(y, -1.0, 1.0) * 32767.0).astype(np.int16))
        rtf = (time.time() - start) / max(pcm_len / sr, 1e-9)
    if vocoder is not None and first_chunk:
        logging.info("Finished chunked generation of %d utterances (%d frames per chunk, RTF = %.03f, time to first chunk: "
                     "median %.2f ms, first utterance %.2f ms).", len(mel_lst), chunk_frames, rtf,
                     1e3 * float(np.median(first_chunk)), 1e3 * first_chunk[0])
    else:
        logging.info("Finished generation of %d utterances (RTF = %.03f).", len(mel_lst), rtf)
    return rtf


def main(argv=None):
    parser = argparse.ArgumentParser(description="Infer hifigan model")
    parser.add_argument("--ckpt", type=str, required=True, help="Path to model checkpoint")
    parser.add_argument("--input_mel", type=str, required=True,
                        help="Path to input mel file or directory containing mel files")
    parser.add_argument("--output_dir", type=str, required=True, help="Path to output directory")
    parser.add_argument("--config", type=str, default=None, help="Path to config file")
    parser.add_argument("--chunk_frames", type=int, default=None,
                        help="Generate chunk by chunk, this many mel frames at a time (carried convolution state)")
    parser.add_argument("--slots", type=int, default=1,
                        help="With --chunk_frames: play this many utterances at a time (continuous batching)")
    parser.add_argument("--seed", type=int, default=0,
                        help="With --chunk_frames on an NSF generator: seed of the excitation's noise and initial phases")
    args = parser.parse_args(argv)
    if args.slots < 1 or (args.slots > 1 and args.chunk_frames is None):
        parser.error("--slots needs --chunk_frames and a value >= 1")
    return hifigan_infer(args.input_mel, args.ckpt, args.output_dir, args.config, chunk_frames=args.chunk_frames,
                         slots=args.slots, seed=args.seed)


if __name__ == "__main__":
    main()
