"""Speaker embeddings for SE voices: ``wav/*.wav`` -> ``se/<id>.npy`` (1, 192) per recording and ``se/se.npy``, their mean
-- the file AM_Dataset, infer_sambert and text_to_wav ask for.

    python -m kantts.preprocess.se_processor.se_processor --src_voice_dir VOICE --se_model se.model

Kaldi fbank and the D-TDNN extractor run on the device (csrc/spk_embed.hip) over ragged batches: the recordings are sorted
by length and batched under a frame budget, so a corpus of thousands of wavs is a few dozen forward passes, and every
recording gets the embedding it would get alone (the kernels take each item's own length).  Wavs are read with scipy and
must be mono 16 kHz (no resampling here); int16 is scaled to [-1, 1)."""
import argparse
import logging
import os
from glob import glob

import numpy as np
import torch

from .D_TDNN import DTDNN
from .fbank import kaldi_tables, num_frames


def read_wav(path, sample_rate=16000):
    """A mono ``sample_rate`` wav as a float32 array in [-1, 1); anything else is refused."""
    from scipy.io import wavfile

    rate, data = wavfile.read(path)
    if data.ndim == 2 and data.shape[1] == 1:
        data = data[:, 0]
    if data.ndim != 1:
        raise ValueError("%s: %d channels; the speaker-embedding extractor takes mono recordings" % (path, data.shape[1]))
    if rate != sample_rate:
        raise ValueError("%s: %d Hz; the speaker-embedding extractor takes %d Hz recordings (resample first)"
                         % (path, rate, sample_rate))
    if data.dtype == np.int16:
        return data.astype(np.float32) / 32768.0
    if data.dtype == np.int32:
        return (data.astype(np.float64) / 2147483648.0).astype(np.float32)
    if data.dtype == np.uint8:
        return (data.astype(np.float32) - 128.0) / 128.0
    return data.astype(np.float32)


class SpeakerEmbeddingProcessor:
    """``model_factory``: a callable returning the DTDNN to load ``se.model`` into; otherwise ``geometry`` are DTDNN's
    constructor arguments (default: the shipped geometry, embedding size 192).  ``frame_budget``: padded fbank frames
    (items x longest item) one forward pass may hold."""

    def __init__(self, sample_rate=16000, model_factory=None, frame_budget=16000, device=None, **geometry):
        if sample_rate != 16000:
            raise ValueError("SpeakerEmbeddingProcessor: the extractor is a 16 kHz model, got sample_rate = %r" % (sample_rate,))
        self.sample_rate = sample_rate
        self.min_wav_length = self.sample_rate * 30 * 10 / 1000
        self.model_factory = model_factory if model_factory is not None else (lambda: DTDNN(**geometry))
        self.frame_budget = int(frame_budget)
        self.device = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
        self.model = None
        self.se_list = []

    # -- model --------------------------------------------------------------------------------------------------------
    def load_model(self, se_model):
        name = os.path.basename(se_model)
        if name == "se.onnx":
            raise ValueError("[SpeakerEmbeddingProcessor] %s: .onnx extractors are not supported; use the se.model (torch "
                             "state dict) that ships with voices of version 1.0.5 or later" % se_model)
        if name != "se.model":
            raise ValueError("[SpeakerEmbeddingProcessor] --se_model must be a file called se.model, got %s" % se_model)
        model = self.model_factory()
        model.load_state_dict(torch.load(se_model, map_location="cpu"), strict=True)
        self.model = model.eval().to(self.device)
        return self.model

    # -- library entry point ------------------------------------------------------------------------------------------
    def features(self, wav, nsamp, cmn=True):
        """Padded waveforms (B, N) and their sample counts -> (fbank (B, T, 80), frame counts): kantts_kaldi_fbank."""
        from kantts._hip import ops

        frames = [num_frames(n) for n in nsamp]
        wav = wav.to(self.device, torch.float32)
        n32 = torch.tensor([int(n) for n in nsamp], dtype=torch.int32).to(self.device)
        return ops.kaldi_fbank(wav, n32, kaldi_tables(self.device), max(frames), cmn=cmn), frames

    @torch.no_grad()
    def embed(self, wavs, lengths=None):
        """``wavs``: a list of 1-D float waveforms, or a padded (B, N) batch with ``lengths`` (samples per item; default N).
        Returns (B, embedding_size) on the processor's device, in the order given."""
        if self.model is None:
            raise RuntimeError("SpeakerEmbeddingProcessor.embed: no extractor loaded (load_model(se_model) first)")
        if torch.is_tensor(wavs):
            if wavs.dim() != 2:
                raise ValueError("embed: a padded batch is (B, N), got %s" % (tuple(wavs.shape),))
            lengths = [wavs.shape[1]] * wavs.shape[0] if lengths is None else [int(n) for n in lengths]
            wavs = [wavs[i, :n] for i, n in enumerate(lengths)]
        wavs = [torch.as_tensor(w, dtype=torch.float32).reshape(-1) for w in wavs]
        for i, w in enumerate(wavs):
            if w.numel() < self.min_wav_length:
                raise ValueError("embed: item %d has %d samples; the extractor needs at least %d (0.3 s)"
                                 % (i, w.numel(), int(self.min_wav_length)))
        order = sorted(range(len(wavs)), key=lambda i: wavs[i].numel())
        out = torch.empty((len(wavs), self.model.embedding_size), device=self.device)
        start = 0
        while start < len(order):  # the longest item of a batch is its last: grow while items x frames fits the budget
            end = start + 1
            while end < len(order) and (end + 1 - start) * num_frames(wavs[order[end]].numel()) <= self.frame_budget:
                end += 1
            idx = order[start:end]
            nsamp = [wavs[i].numel() for i in idx]
            batch = torch.zeros((len(idx), max(nsamp)), dtype=torch.float32)
            for r, i in enumerate(idx):
                batch[r, :nsamp[r]] = wavs[i]
            feats, frames = self.features(batch, nsamp)
            out[torch.tensor(idx, device=self.device)] = self.model.forward_kernels(feats, frames)
            start = end
        return out

    # -- directory entry point ----------------------------------------------------------------------------------------
    def process(self, src_voice_dir, se_model):
        logging.info("[SpeakerEmbeddingProcessor] Speaker embedding extractor started")
        self.load_model(se_model)
        wav_dir = os.path.join(src_voice_dir, "wav")
        se_dir = os.path.join(src_voice_dir, "se")
        os.makedirs(se_dir, exist_ok=True)
        names, wavs = [], []
        for wav_file in sorted(glob(os.path.join(wav_dir, "*.wav"))):
            wav = read_wav(wav_file, self.sample_rate)
            if wav.shape[0] < self.min_wav_length:
                logging.info("[SpeakerEmbeddingProcessor] %s: shorter than 0.3 s, skipped", wav_file)
                continue
            names.append(os.path.splitext(os.path.basename(wav_file))[0])
            wavs.append(torch.from_numpy(wav))
        if not wavs:
            raise RuntimeError("[SpeakerEmbeddingProcessor] no recording of at least %d samples (0.3 s) under %s: "
                               "nothing to average into se.npy" % (int(self.min_wav_length), wav_dir))
        emb = self.embed(wavs).cpu().numpy()
        self.se_list = [emb[i:i + 1] for i in range(len(names))]
        for name, e in zip(names, self.se_list):
            np.save(os.path.join(se_dir, name + ".npy"), e)
        self.se_average = np.expand_dims(np.mean(np.concatenate(self.se_list, axis=0), axis=0), axis=0)
        np.save(os.path.join(se_dir, "se.npy"), self.se_average)
        logging.info("[SpeakerEmbeddingProcessor] Speaker embedding extracted successfully! (%d recordings)", len(names))
        return self.se_average


def main(argv=None):
    parser = argparse.ArgumentParser(description="Speaker Embedding Processor")
    parser.add_argument("--src_voice_dir", type=str, required=True)
    parser.add_argument("--se_model", required=True)
    args = parser.parse_args(argv)
    logging.basicConfig(format="%(asctime)s %(levelname)-4s [%(filename)s:%(lineno)d] %(message)s",
                        datefmt="%Y-%m-%d:%H:%M:%S", level=logging.INFO)
    SpeakerEmbeddingProcessor().process(args.src_voice_dir, args.se_model)


if __name__ == "__main__":
    main()
