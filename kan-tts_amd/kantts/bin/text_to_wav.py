"""Text (or linguistic symbols) to wav: the acoustic model, the vocoder and the joining of sub-sentences in one entry point.

Mirrors kantts/bin/text_to_wav.py of the reference: ``text_to_wav(text_file, output_dir, resources_zip_file, am_ckpt,
voc_ckpt, speaker=None, se_file=None, lang="PinYin")`` writes ``symbols.lst``, ``feat/<id>_mel.npy`` (+ ``_dur.txt``,
``_f0.txt``, ``_energy.txt``), ``<id>_mel_gen.wav`` and ``res_wavs/<main>.wav`` under ``output_dir``; ``concat_process``
joins the sub-sentences ``<main>_<sub>`` of a sentence with 0.28 s of silence between them and 0.05 s at the end.  The text
front end (``text_to_mit_symbols``: text -> symbols) is outside the hot path and not part of this package (DESIGN.md section
7): where it cannot be imported, ``text_to_wav`` says so and ``symbols_to_wav`` / ``--symbols`` take the symbols file the
front end would have written (one ``<id>\\t<symbols>`` line per sub-sentence).

``chunk_frames=N`` (``--chunk_frames N --slots S``): the sentences play through ``kantts.models.streaming.StreamingTTS``
instead of through ``am_infer`` then ``hifigan_infer`` -- S utterances at a time, N frames per vocoder step, no mel on the
host or on disk between the two halves; an utterance's wav is written when its last chunk has arrived, the ``feat`` files
afterwards from the pool's results.  bf16 mode (``KANTTS_PRECISION=bf16`` or ``set_precision("bf16")``), as for
``infer_sambert --chunk_frames``.  Wav files are read and written with scipy (soundfile is not a dependency here).
"""
import argparse
import logging
import os
import re
import time
import zipfile

import numpy as np
import torch
import yaml
from scipy.io import wavfile

from kantts.bin import infer_hifigan, infer_sambert
from kantts.bin.infer_hifigan import hifigan_infer
from kantts.bin.infer_sambert import am_infer

logging.basicConfig(format="%(asctime)s, %(levelname)-4s [%(filename)s:%(lineno)d] %(message)s",
                    datefmt="%Y-%m-%d:%H:%M:%S", level=logging.INFO)

SENTENCE_SIL, END_SIL = 0.28, 0.05  # seconds of silence between the sub-sentences of a sentence / behind its last one
_SUB_WAV = re.compile(r"^(\d+)_(\d+)_mel_gen\.wav$")


def concat_process(chunked_dir, output_dir):
    """``<main>_<sub>_mel_gen.wav`` of ``chunked_dir`` -> ``<main>.wav`` in ``output_dir``: the sub-sentences of a sentence
    in the order of their numbers, SENTENCE_SIL seconds of zeros between two of them and END_SIL seconds behind the last."""
    groups = {}
    for name in os.listdir(chunked_dir):
        m = _SUB_WAV.match(name)
        if m:
            groups.setdefault(int(m.group(1)), []).append((int(m.group(2)), name))
    os.makedirs(output_dir, exist_ok=True)
    for main_id, subs in sorted(groups.items()):
        parts, sr = [], None
        for _, name in sorted(subs):
            sr, wav = wavfile.read(os.path.join(chunked_dir, name))
            if parts:
                parts.append(np.zeros(int(SENTENCE_SIL * sr), dtype=wav.dtype))
            parts.append(wav)
        parts.append(np.zeros(int(END_SIL * sr), dtype=parts[-1].dtype))
        wavfile.write(os.path.join(output_dir, "%d.wav" % main_id), sr, np.concatenate(parts, axis=0))


def _stream(symbols_file, output_dir, am_ckpt, voc_ckpt, se_file, chunk_frames, slots, slot_steps, seed, ling_unit):
    """The streaming branch of ``symbols_to_wav``."""
    from kantts.models.streaming import StreamingTTS

    device, ling_unit, se, nsf, fsnet = infer_sambert.load_am(am_ckpt, se_file=se_file, ling_unit=ling_unit)
    voc_config = infer_hifigan._load_config(voc_ckpt, None)
    generator = infer_hifigan.load_model(voc_ckpt, voc_config)
    generator.remove_weight_norm()
    generator = generator.eval().to(device)
    sr = voc_config["audio_config"]["sampling_rate"]
    # lookahead: a non-causal voice streams too, its audio ``flush_frames`` frames late
    tts = StreamingTTS(fsnet, generator, slots=slots, max_steps=slot_steps, chunk_frames=chunk_frames, nsf=nsf, seed=seed,
                       graph=device.type == "cuda", lookahead=True)  # refuses what it cannot stream, loudly
    if tts.flush_frames:
        logging.info("Non-causal generator: the audio of an utterance starts %d frames (%d samples) after its first frame.",
                     tts.flush_frames, tts.vocoder.delay_samples)
    feat_dir = os.path.join(output_dir, "feat")
    os.makedirs(feat_dir, exist_ok=True)
    with open(symbols_file, encoding="utf-8") as f:
        lines = [ln for ln in (line.strip().split("\t") for line in f) if len(ln) >= 2]
    results, parts, first, pcm_len = {}, {}, {}, [0]

    def write_ended():  # an utterance has ended once the pipeline has put its result down
        for index in [i for i in parts if i in results]:
            y = torch.cat(parts.pop(index)).numpy()
            pcm_len[0] += len(y)
            infer_hifigan._write_wav(output_dir, lines[index][0] + "_mel", sr, y)

    with torch.no_grad():
        requests = [infer_sambert.am_inputs(line[1], ling_unit, device, se=se) for line in lines]
        t0 = time.time()
        for index, _, wav in tts.play_many(requests, results=results):
            write_ended()
            parts.setdefault(index, []).append(wav.reshape(-1).cpu())  # the copy to the host is when a chunk can be played
            if index not in first:
                first[index] = time.time() - t0
        write_ended()
        elapsed = time.time() - t0
    for index, line in enumerate(lines):
        _, mel_post, dur, f0, energy = infer_sambert.am_outputs(results[index])
        if nsf is not None:
            mel_post = infer_sambert.denorm_f0(mel_post, scale=nsf[0], offset=nsf[1])
        np.save("%s/%s_mel.npy" % (feat_dir, line[0]), mel_post)
        np.savetxt("%s/%s_dur.txt" % (feat_dir, line[0]), dur)
        np.savetxt("%s/%s_f0.txt" % (feat_dir, line[0]), f0)
        np.savetxt("%s/%s_energy.txt" % (feat_dir, line[0]), energy)
    stats = {"utterances": len(lines), "rtf": elapsed / max(pcm_len[0] / sr, 1e-9),
             "first_audio_median_ms": 1e3 * float(np.median(list(first.values()))) if first else None,
             "first_audio_worst_ms": 1e3 * max(first.values()) if first else None}
    if first:
        logging.info("Finished streaming synthesis of %d utterances through %d slots (%d frames per chunk, RTF = %.03f, time "
                     "from the start to an utterance's first audio chunk: median %.2f ms, worst %.2f ms).", len(lines), slots,
                     chunk_frames, stats["rtf"], stats["first_audio_median_ms"], stats["first_audio_worst_ms"])
    return stats


def symbols_to_wav(symbols_file, output_dir, am_ckpt, voc_ckpt, se_file=None, chunk_frames=None, slots=1, slot_steps=1024,
                   seed=0, ling_unit=None):
    """Everything ``text_to_wav`` does behind the text front end, from the symbols file it would have written.  Without
    ``chunk_frames``: ``am_infer``, then ``hifigan_infer`` over the ``feat`` directory, then ``concat_process`` (returns
    None).  With it: the streaming pipeline, which writes the same files and returns the figures it logs (RTF, time to an
    utterance's first audio chunk)."""
    slots = int(slots)
    if slots < 1:
        raise ValueError("--slots must be positive, got %d" % slots)
    if chunk_frames is None and slots > 1:
        raise ValueError("--slots needs --chunk_frames")
    os.makedirs(os.path.join(output_dir, "res_wavs"), exist_ok=True)
    stats = None
    if chunk_frames is None:
        logging.info("AM is inferring...")
        am_infer(symbols_file, am_ckpt, output_dir, se_file, ling_unit=ling_unit)
        logging.info("Vocoder is inferring...")
        hifigan_infer(os.path.join(output_dir, "feat"), voc_ckpt, output_dir, seed=seed)
    else:
        logging.info("AM and vocoder are streaming...")
        stats = _stream(symbols_file, output_dir, am_ckpt, voc_ckpt, se_file, int(chunk_frames), slots, int(slot_steps),
                        int(seed), ling_unit)
    concat_process(output_dir, os.path.join(output_dir, "res_wavs"))
    logging.info("Symbols to wav finished!")
    return stats


def text_to_wav(text_file, output_dir, resources_zip_file, am_ckpt, voc_ckpt, speaker=None, se_file=None, lang="PinYin",
                chunk_frames=None, slots=1, slot_steps=1024, seed=0):
    """The reference's entry point: text -> symbols through the text front end, then ``symbols_to_wav``."""
    try:
        from kantts.utils.ling_unit import text_to_mit_symbols
    except ImportError:
        raise NotImplementedError(
            "the text front end (kantts.utils.ling_unit.text_to_mit_symbols) is not part of this package: write the symbols "
            "file it produces (one '<id>\\t<symbols>' line per sub-sentence) and call symbols_to_wav / pass --symbols") from None
    os.makedirs(output_dir, exist_ok=True)
    resource_root = os.path.dirname(resources_zip_file)
    resource_dir = os.path.join(resource_root, "resource")
    if not os.path.exists(resource_dir):
        logging.info("Extracting resources...")
        with zipfile.ZipFile(resources_zip_file, "r") as z:
            z.extractall(resource_root)
    with open(text_file, encoding="utf-8") as f:
        texts = f.readlines()
    if speaker is None:
        with open(os.path.join(os.path.dirname(os.path.dirname(am_ckpt)), "config.yaml")) as f:
            speaker = yaml.load(f, Loader=yaml.Loader)["linguistic_unit"]["speaker_list"].split(",")[0]
    logging.info("Converting text to symbols...")
    symbols_file = os.path.join(output_dir, "symbols.lst")
    with open(symbols_file, "w", encoding="utf-8") as f:
        f.writelines(text_to_mit_symbols(texts, resource_dir, speaker, lang))
    return symbols_to_wav(symbols_file, output_dir, am_ckpt, voc_ckpt, se_file=se_file, chunk_frames=chunk_frames, slots=slots,
                          slot_steps=slot_steps, seed=seed)


def main(argv=None):
    parser = argparse.ArgumentParser(description="Text to wav")
    src = parser.add_mutually_exclusive_group(required=True)
    src.add_argument("--txt", type=str, help="Path to text file (needs the text front end and --res_zip)")
    src.add_argument("--symbols", type=str, help="Path to a symbols file: one '<id>\\t<symbols>' line per sub-sentence")
    parser.add_argument("--output_dir", type=str, required=True, help="Path to output directory")
    parser.add_argument("--res_zip", type=str, default=None, help="Path to resource zip file (with --txt)")
    parser.add_argument("--am_ckpt", type=str, required=True, help="Path to am ckpt file")
    parser.add_argument("--voc_ckpt", type=str, required=True, help="Path to voc ckpt file")
    parser.add_argument("--speaker", type=str, default=None, help="The speaker name, default is the first speaker")
    parser.add_argument("--se_file", type=str, default=None, help="The speaker embedding file, default is None")
    parser.add_argument("--lang", type=str, default="PinYin",
                        help="The language of the text, default is PinYin; others: English, British, ZhHK, WuuShanghai, "
                             "Sichuan, Indonesian, Malay, Filipino, Vietnamese, Korean, Russian")
    parser.add_argument("--chunk_frames", type=int, default=None,
                        help="Stream symbols to audio on the device, this many mel frames per vocoder step (a multiple of "
                             "outputs_per_step; bf16 mode)")
    parser.add_argument("--slots", type=int, default=1, help="With --chunk_frames: utterances in flight (continuous batching)")
    parser.add_argument("--slot_steps", type=int, default=1024,
                        help="With --chunk_frames: decoder steps the buffers of a slot hold (the longest utterance it can take)")
    parser.add_argument("--seed", type=int, default=0, help="NSF voices: seed of the excitation's noise and initial phases")
    args = parser.parse_args(argv)
    if args.chunk_frames is not None and args.chunk_frames < 1:
        parser.error("--chunk_frames must be positive")
    if args.slots < 1 or (args.slots > 1 and args.chunk_frames is None):
        parser.error("--slots needs --chunk_frames and a value >= 1")
    if args.txt is not None and args.res_zip is None:
        parser.error("--txt needs --res_zip")
    try:
        if args.symbols is not None:
            return symbols_to_wav(args.symbols, args.output_dir, args.am_ckpt, args.voc_ckpt, se_file=args.se_file,
                                  chunk_frames=args.chunk_frames, slots=args.slots, slot_steps=args.slot_steps, seed=args.seed)
        return text_to_wav(args.txt, args.output_dir, args.res_zip, args.am_ckpt, args.voc_ckpt, args.speaker, args.se_file,
                           args.lang, chunk_frames=args.chunk_frames, slots=args.slots, slot_steps=args.slot_steps,
                           seed=args.seed)
    except ValueError as e:
        if "chunk_frames" not in str(e) and "--slots" not in str(e):
            raise
        parser.error(str(e))


if __name__ == "__main__":
    main()
