"""Datasets over the on-disk feature layout.  Vocoder: the reader side of
``AudioProcessor.mel_extract``: ``<root>/wav/<utt>.wav`` + ``<root>/mel/<utt>.npy`` (+ ``frame_f0`` / ``frame_uv`` and
``f0/f0_{mean,std}.txt`` for NSF generators), utterance lists in ``train.lst`` / ``valid.lst``.

Same entry points as the reference (kantts/datasets/dataset.py:88-345): ``Voc_Dataset(metafile, root_dir, config)`` with
``__getitem__ -> (wav (T,), mel (frames, C))`` where ``T == frames * hop_length``, ``collate_fn`` (random crop of
``batch_max_steps`` samples, kantts.datasets.batching.voc_collate) and ``get_voc_datasets(config, root_dir)``.  Item
semantics follow the reference exactly (pinned by tests/golden/voc_dataset.pt): utterances not longer than a crop are
zero-padded to one frame more than a crop; longer ones get n_fft samples of reflect padding and are cut to
frames * hop_length; NSF items carry the de-normalised frame f0 and the voiced flag as two extra feature columns.
Two deliberate differences: ``gen_metafile`` only demands the f0 / uv files when the generator is an NSF one (the reference
always does), and ``load_meta_from_dir`` pairs ``<utt>.wav`` with ``<utt>.npy`` (the reference's version pairs it with
a ``.wav`` in the mel directory and returns tuples ``__getitem__`` cannot unpack).

Acoustic model: ``AM_Dataset`` / ``get_am_datasets`` (reference :391-869) over ``raw_metafile.txt`` + the ``mel/
duration/ f0/ energy/ frame_f0/ frame_uv/`` feature files, with the symbol tables of ``kantts.utils.ling_unit`` (native; the
language resource files are looked up as ``ling_unit.language_directory`` describes) and ``am_collate`` for batches --
items and batches pinned to the reference's by tests/golden/am_dataset.pt.  Waveforms must already be at the configured
rate.
"""
import glob
import logging
import os
import random

import numpy as np
import torch

from kantts.datasets.batching import Padder, am_collate, beta_binomial_prior_distribution, voc_collate
from kantts.preprocess.audio_processor.audio_processor import load_wav

DATASET_RANDOM_SEED = 1234


class Voc_Dataset(torch.utils.data.Dataset):
    """(wav, mel) pairs for HiFi-GAN training."""

    def __init__(self, metafile, root_dir, config):
        self.meta = []
        self.config = config
        self.sampling_rate = config["audio_config"]["sampling_rate"]
        self.n_fft = config["audio_config"]["n_fft"]
        self.hop_length = config["audio_config"]["hop_length"]
        self.batch_max_steps = config["batch_max_steps"]
        self.batch_max_frames = self.batch_max_steps // self.hop_length
        nsf = config["Model"]["Generator"]["params"].get("nsf_params", None)
        self.nsf_enable = nsf is not None
        metafile = metafile if isinstance(metafile, list) else [metafile]
        root_dir = root_dir if isinstance(root_dir, list) else [root_dir]
        for meta_file, data_dir in zip(metafile, root_dir):
            if not os.path.exists(meta_file):
                raise ValueError("[Voc_Dataset] meta file: {} not found".format(meta_file))
            if not os.path.exists(data_dir):
                raise ValueError("[Voc_Dataset] data dir: {} not found".format(data_dir))
            self.meta.extend(self.load_meta(meta_file, data_dir))
        if len(self.meta) == 0:
            for d in root_dir:
                self.meta.extend(self.load_meta_from_dir(os.path.join(d, "wav"), os.path.join(d, "mel")))
        self.allow_cache = config.get("allow_cache", False)
        self.caches = {}

    @staticmethod
    def gen_metafile(wav_dir, out_dir, split_ratio=0.98, need_f0=False):
        """train.lst / valid.lst: a seeded shuffle of the utterances whose features exist, split at split_ratio."""
        wav_files = sorted(glob.glob(os.path.join(wav_dir, "*.wav")))
        random.Random(DATASET_RANDOM_SEED).shuffle(wav_files)
        num_train = int(len(wav_files) * split_ratio) - 1
        needed = ["mel"] + (["frame_f0", "frame_uv"] if need_f0 else [])

        def write(path, files):
            with open(path, "w") as f:
                for wav_file in files:
                    index = os.path.splitext(os.path.basename(wav_file))[0]
                    if all(os.path.exists(os.path.join(out_dir, d, index + ".npy")) for d in needed):
                        f.write("{}\n".format(index))

        write(os.path.join(out_dir, "train.lst"), wav_files[:num_train])
        write(os.path.join(out_dir, "valid.lst"), wav_files[num_train:])

    def load_meta(self, metafile, data_dir):
        wav_dir, mel_dir = os.path.join(data_dir, "wav"), os.path.join(data_dir, "mel")
        if not os.path.exists(wav_dir) or not os.path.exists(mel_dir):
            raise ValueError("wav or mel directory not found")
        items = []
        with open(metafile, "r") as f:
            for name in f:
                name = name.strip()
                if name:
                    items.append((os.path.join(wav_dir, name + ".wav"), os.path.join(mel_dir, name + ".npy"),
                                  os.path.join(data_dir, "frame_f0", name + ".npy"),
                                  os.path.join(data_dir, "frame_uv", name + ".npy")))
        return items

    def load_meta_from_dir(self, wav_dir, mel_dir):
        if not os.path.exists(wav_dir) or not os.path.exists(mel_dir):
            raise ValueError("wav or mel directory not found")
        data_dir = os.path.dirname(os.path.normpath(wav_dir))
        items = []
        for wav_file in sorted(glob.glob(os.path.join(wav_dir, "*.wav"))):
            name = os.path.splitext(os.path.basename(wav_file))[0]
            mel_file = os.path.join(mel_dir, name + ".npy")
            if os.path.exists(mel_file):
                items.append((wav_file, mel_file, os.path.join(data_dir, "frame_f0", name + ".npy"),
                              os.path.join(data_dir, "frame_uv", name + ".npy")))
        return items

    def __len__(self):
        return len(self.meta)

    def __getitem__(self, idx):
        if self.allow_cache and idx in self.caches:
            return self.caches[idx]
        wav_file, mel_file, frame_f0_file, frame_uv_file = self.meta[idx]
        wav_data = load_wav(wav_file, self.sampling_rate)
        mel_data = np.load(mel_file)
        if self.nsf_enable:
            # frame f0 is stored mean / std normalised; the generator's source module wants Hz
            f0_dir = os.path.join(os.path.dirname(os.path.dirname(frame_f0_file)), "f0")
            f0_mean = np.loadtxt(os.path.join(f0_dir, "f0_mean.txt"))
            f0_std = np.loadtxt(os.path.join(f0_dir, "f0_std.txt"))
            frame_f0 = np.load(frame_f0_file).reshape(-1, 1) * f0_std + f0_mean
            frame_uv = np.load(frame_uv_file).reshape(-1, 1)
            mel_data = np.concatenate((mel_data, frame_f0, frame_uv), axis=1)
        if mel_data.shape[0] <= self.batch_max_frames:
            # at least one frame more than a crop, zeros after the utterance
            pad = np.zeros((self.batch_max_frames - mel_data.shape[0] + 1, mel_data.shape[1]))
            mel_data = np.concatenate((mel_data, pad), axis=0)
            wav_cache = np.zeros(mel_data.shape[0] * self.hop_length, dtype=np.float32)
            wav_cache[:len(wav_data)] = wav_data
            wav_data = wav_cache
        else:
            wav_data = np.pad(wav_data, (0, self.n_fft), mode="reflect")[:len(mel_data) * self.hop_length]
        assert len(mel_data) * self.hop_length == len(wav_data)
        if self.allow_cache:
            self.caches[idx] = (wav_data, mel_data)
        return wav_data, mel_data

    def collate_fn(self, batch):
        return voc_collate(batch, self.hop_length, self.batch_max_steps)


def get_voc_datasets(config, root_dir, split_ratio=0.98):
    root_dir = [root_dir] if isinstance(root_dir, str) else list(root_dir)
    need_f0 = config["Model"]["Generator"]["params"].get("nsf_params", None) is not None
    train_meta_lst, valid_meta_lst = [], []
    for data_dir in root_dir:
        train_meta, valid_meta = os.path.join(data_dir, "train.lst"), os.path.join(data_dir, "valid.lst")
        if not os.path.exists(train_meta) or not os.path.exists(valid_meta):
            Voc_Dataset.gen_metafile(os.path.join(data_dir, "wav"), data_dir, split_ratio, need_f0=need_f0)
        train_meta_lst.append(train_meta)
        valid_meta_lst.append(valid_meta)
    return Voc_Dataset(train_meta_lst, root_dir, config), Voc_Dataset(valid_meta_lst, root_dir, config)


_FP_FILLER_TAG = 3  # index into EMOTION_TYPES of the tag the preprocessing puts on filler tokens (emotion_disgust)


def _fp_class(before, last):
    """Insertion class of a filler run from the syllables of its last two positions: "ga ..." is the "a" filler (1),
    "ge en_c" the "en" filler (2), anything else the "e" filler (3)."""
    if before == "ga":
        return 1
    return 2 if (before == "ge" and last == "en_c") else 3


def get_fp_label(aug_ling_txt):
    """Insertion label per token of the ``fprm`` line (plus the trailing "~") from the ``fpadd`` line of the same
    utterance, in which the filler tokens are tagged ``emotion_disgust`` (same results as reference dataset.py:348-388,
    pinned by the recorded lines of tests/golden/sambert_tiny_fp.pt).  The rule, token by token with k counted from 0 and
    the "~" slot appended as an untagged token:
      * tagged tokens are fillers and give no label;
      * from k = 2 on, the first untagged token behind a tagged one ENDS the run: it gives no label either, and the token
        after it carries the run's class (``_fp_class`` of the two syllables in front of the ending token) -- also when that
        token is itself tagged;
      * every other token from k = 2 on is labelled 0;
      * the first two tokens are special: unless the line STARTS with a filler both are labelled 0 and token 1 does not
        count as tagged; if it does start with one, token 1 keeps the label of its own tag (none 0, neutral 1, angry 2,
        fear 3, anything else no label)."""
    from kantts.utils.ling_unit import EMOTION_TYPES

    fields = [token.strip("{}").split("$") for token in aug_ling_txt.strip().split(" ")]
    syl = [f[0] for f in fields] + ["~"]
    tag = [f[4] for f in fields] + [EMOTION_TYPES[0]]
    n = len(tag)
    filler = [t == EMOTION_TYPES[_FP_FILLER_TAG] for t in tag]
    starts_with_filler = filler[0]
    if not starts_with_filler and n > 1:
        filler[1] = False
    ends_run = [2 <= k <= n - 2 and not filler[k] and filler[k - 1] for k in range(n)]
    labels = []
    for k in range(n):
        if k >= 1 and ends_run[k - 1]:
            labels.append(_fp_class(syl[k - 3], syl[k - 2]))
        elif ends_run[k]:
            continue
        elif k < 2:
            if not starts_with_filler:
                labels.append(0)
            elif k == 1 and tag[1] in (EMOTION_TYPES[0], EMOTION_TYPES[1], EMOTION_TYPES[2], EMOTION_TYPES[4]):
                labels.append({EMOTION_TYPES[0]: 0, EMOTION_TYPES[1]: 1, EMOTION_TYPES[2]: 2, EMOTION_TYPES[4]: 3}[tag[1]])
        elif not filler[k]:
            labels.append(0)
    return np.array(labels)


class AM_Dataset(torch.utils.data.Dataset):
    """(linguistic ids, mel, durations, pitch, energy, alignment prior, fp label, speaker embedding) per utterance
    (reference dataset.py:391-545).  ``metafile``: path(s) of lines ``<id>\t{sy$tone$flag$ws$emo$spk} ...``; ``root_dir``:
    feature director(ies) with ``mel/ duration/ f0/ energy/ frame_f0/ frame_uv/ [se/se.npy]`` (``<id>.npy`` each; the layout
    AudioProcessor writes).  Behaviour kept from the reference: durations are used iff ``duration/`` exists and the model
    is not MAS (then a beta-binomial prior is attached instead); NSF models get frame-level f0 / voiced flag appended to
    the mel as two extra columns, f0 re-normalised to [global_min, global_max] when ``nsf_norm_type: global``; SE models
    load one speaker embedding per data directory; filled-pause (FP) models read ``fprm`` metafiles (the fillers removed)
    and take each utterance's insertion labels from the ``fpadd`` twin next to it (the same path with "fprm" replaced by
    "fpadd"; an utterance without a twin line is dropped with a warning).  Caching is a plain per-process dict (the
    reference shares a multiprocessing.Manager list)."""

    def __init__(self, config, metafile, root_dir, allow_cache=False, ling_unit=None):
        from kantts.utils.ling_unit import KanTtsLinguisticUnit

        params = config["Model"]["KanTtsSAMBERT"]["params"]
        self.config = config
        self.nsf_enable = bool(params.get("NSF", False))
        self.nsf_norm_type = params.get("nsf_norm_type", "mean_std")
        self.nsf_f0_global_minimum = params.get("nsf_f0_global_minimum", 30.0)
        self.nsf_f0_global_maximum = params.get("nsf_f0_global_maximum", 730.0)
        self.se_enable = bool(params.get("SE", False))
        self.mas_enable = bool(params.get("MAS", False))
        self.fp_enable = bool(params.get("FP", False))
        self.r = params["outputs_per_step"]
        self.with_duration = True
        metafile = metafile if isinstance(metafile, list) else [metafile]
        root_dir = root_dir if isinstance(root_dir, list) else [root_dir]
        self.meta = []
        for meta_file, data_dir in zip(metafile, root_dir):
            if not os.path.exists(meta_file):
                raise ValueError("[AM_Dataset] meta file: {} not found".format(meta_file))
            if not os.path.exists(data_dir):
                raise ValueError("[AM_Dataset] data dir: {} not found".format(data_dir))
            self.meta.extend(self.load_meta(meta_file, data_dir))
        self.ling_unit = ling_unit if ling_unit is not None else KanTtsLinguisticUnit(config)
        self.padder = Padder()
        self.allow_cache = allow_cache
        self.caches = {}
        # duration-free items carry the beta-binomial prior (slot 5) unless this is switched off: a consumer that evaluates
        # the prior itself (the device-resident corpus, device_batching.make_train_loader) then gets ``None`` there and no
        # M x P matrix is computed per utterance; such items are not cached
        self.attach_prior = True

    def __len__(self):
        return len(self.meta)

    def load_meta(self, metafile, data_dir):
        sub = {k: os.path.join(data_dir, k) for k in ("mel", "duration", "f0", "energy", "frame_f0", "frame_uv", "se")}
        # (the last directory decides for the whole dataset, as in the reference)
        self.with_duration = False if self.mas_enable else os.path.exists(sub["duration"])
        se_path = os.path.join(sub["se"], "se.npy")
        if self.se_enable and not os.path.exists(se_path):
            logging.warning("Missing se meta")
            return []
        aug = {}
        if self.fp_enable:  # reference :549-556
            with open(metafile.replace("fprm", "fpadd"), "r") as f:
                for line in f:
                    if line.strip():
                        index, aug_txt = line.strip().split("\t")
                        aug[index] = aug_txt
        items = []
        with open(metafile, "r") as f:
            for line in f:
                line = line.strip()
                if not line:
                    continue
                index, ling_txt = line.split("\t")
                if self.fp_enable and index not in aug:
                    logging.warning("Missing fpadd meta for %s", index)
                    continue
                npy = index + ".npy"
                items.append((ling_txt, os.path.join(sub["mel"], npy),
                              os.path.join(sub["duration"], npy) if self.with_duration else None,
                              os.path.join(sub["f0"], npy), os.path.join(sub["energy"], npy),
                              os.path.join(sub["frame_f0"], npy), os.path.join(sub["frame_uv"], npy), aug.get(index), se_path))
        return items

    def __getitem__(self, idx):
        if self.allow_cache and idx in self.caches:
            item = self.caches[idx]
            return item if self.attach_prior else item[:5] + (None,) + item[6:]
        ling_txt, mel_file, dur_file, f0_file, energy_file, frame_f0_file, frame_uv_file, aug_txt, se_path = self.meta[idx]
        ling_data = self.ling_unit.encode_symbol_sequence(ling_txt)
        mel_data = np.load(mel_file)
        dur_data = np.load(dur_file) if dur_file is not None else None
        f0_data = np.load(f0_file)
        energy_data = np.load(energy_file)
        se_data = np.load(se_path) if self.se_enable else None
        attn_prior = None
        if not self.with_duration and self.attach_prior:
            attn_prior = beta_binomial_prior_distribution(len(ling_data[0]), mel_data.shape[0])
        if self.nsf_enable:
            frame_f0 = np.load(frame_f0_file).reshape(-1, 1)  # stored mean / std normalised
            if self.nsf_norm_type == "global":
                f0_dir = os.path.join(os.path.dirname(os.path.dirname(frame_f0_file)), "f0")
                mean, std = np.loadtxt(os.path.join(f0_dir, "f0_mean.txt")), np.loadtxt(os.path.join(f0_dir, "f0_std.txt"))
                frame_f0 = ((frame_f0 * std + mean) - self.nsf_f0_global_minimum) / (
                    self.nsf_f0_global_maximum - self.nsf_f0_global_minimum)
            mel_data = np.concatenate([mel_data, frame_f0, np.load(frame_uv_file).reshape(-1, 1)], axis=1)
        fp_label = get_fp_label(aug_txt) if (self.fp_enable and aug_txt is not None) else None
        item = (ling_data, mel_data, dur_data, f0_data, energy_data, attn_prior, fp_label, se_data)
        if self.allow_cache and (self.with_duration or self.attach_prior):
            self.caches[idx] = item
        return item

    def collate_fn(self, batch):
        pad_ids = [self.ling_unit._sub_unit_pad[t] for t in self.ling_unit._lfeat_type_list]
        return am_collate(batch, self.r, pad_ids, se=self.se_enable, fp=self.fp_enable)

    @staticmethod
    def gen_metafile(raw_meta_file, out_dir, train_meta_file, valid_meta_file, badlist=None, split_ratio=0.98,
                     se_enable=False):
        """Shuffle the raw metafile with the fixed dataset seed and split it; utterances without mel / frame_f0 /
        frame_uv (or, when ``duration/`` exists, without a duration file) are dropped (reference :626-688)."""
        with open(raw_meta_file, "r") as f:
            lines = f.readlines()
        random.Random(DATASET_RANDOM_SEED).shuffle(lines)  # == random.seed(1234); random.shuffle(lines)
        num_train = int(len(lines) * split_ratio) - 1
        have_dur = os.path.exists(os.path.join(out_dir, "duration"))
        se_missing = se_enable and os.path.exists(os.path.join(out_dir, "se")) and not os.path.exists(
            os.path.join(out_dir, "se", "se.npy"))

        def keep(index):
            if badlist is not None and index in badlist:
                return False
            if not all(os.path.exists(os.path.join(out_dir, d, index + ".npy")) for d in ("frame_f0", "frame_uv", "mel")):
                return False
            if have_dur and not os.path.exists(os.path.join(out_dir, "duration", index + ".npy")):
                return False
            return not se_missing

        for path, part in ((train_meta_file, lines[:num_train]), (valid_meta_file, lines[num_train:])):
            with open(path, "w") as f:
                f.writelines(ln for ln in part if keep(ln.split("\t")[0]))


def get_am_datasets(metafile, root_dir, config, allow_cache, split_ratio=0.98, se_enable=False):
    """(train, valid) AM_Datasets over ``am_train.lst`` / ``am_valid.lst`` of every data directory, generated from the raw
    metafile when missing (reference :831-869; its call passes ``split_ratio, se_enable`` into the positional slots of
    ``badlist, split_ratio`` and would raise a TypeError whenever it actually has to generate the lists -- here the
    arguments go where their names say)."""
    root_dir = root_dir if isinstance(root_dir, list) else [root_dir]
    metafile = metafile if isinstance(metafile, list) else [metafile]
    # FP: the lists of the ``fprm`` metafile; AM_Dataset finds their ``am_fpadd_*`` twins by name (reference :847-854)
    fp = config["Model"]["KanTtsSAMBERT"]["params"].get("FP", False)
    names = ("am_fprm_train.lst", "am_fprm_valid.lst") if fp else ("am_train.lst", "am_valid.lst")
    train_lst, valid_lst = [], []
    for raw_metafile, data_dir in zip(metafile, root_dir):
        train_meta, valid_meta = os.path.join(data_dir, names[0]), os.path.join(data_dir, names[1])
        if not os.path.exists(train_meta) or not os.path.exists(valid_meta):
            AM_Dataset.gen_metafile(raw_metafile, data_dir, train_meta, valid_meta, split_ratio=split_ratio,
                                    se_enable=se_enable)
        train_lst.append(train_meta)
        valid_lst.append(valid_meta)
    return AM_Dataset(config, train_lst, root_dir, allow_cache), AM_Dataset(config, valid_lst, root_dir, allow_cache)


# ---------------------------------------------------------------------------------------------------------------------
# sy-BERT pre-training (reference :873-1130): unlabelled symbol sequences, BERT masking of the sy stream.  This is the HOST
# path -- the validation loader, and the training loader with ``--device_corpus host``; a resident corpus draws its masks on
# the device instead (kantts.datasets.bert_masking / device_batching.DeviceTextSet).  Under equal ``np.random`` / ``random``
# seeds the arrays are the reference's (tests/golden/sybert_tiny.pt): the generators are consumed in its order.
class MaskingActor(object):
    def __init__(self, mask_ratio=0.15):
        self.mask_ratio = mask_ratio

    def _get_random_mask(self, length, p1=0.15):
        """0. / 1. per position: one ``np.random.uniform`` draw of ``length`` values, 1 where it is below ``p1``."""
        draws = np.random.uniform(0, 1, length)
        return (draws < p1).astype(draws.dtype)

    def _input_bert_masking(self, sequence_array, nb_symbol_category, mask_symbol_id, mask, p2=0.8, p3=0.1, p4=0.1):
        """Of the n masked positions, in the order of one ``np.random.shuffle``: the first floor(n p2) read [MASK], the
        next floor(n p3) read ONE ``random.randint`` symbol (drawn only when there is such a position), the rest stay."""
        import math

        out = sequence_array.copy()
        where = np.where(mask == 1)[0]
        order = np.arange(len(where))
        np.random.shuffle(order)
        n2, n3 = int(math.floor(len(where) * p2)), int(math.floor(len(where) * p3))
        if n2 > 0:
            out[where[order[:n2]]] = mask_symbol_id
        if len(where[order[n2:n2 + n3]]) > 0:
            out[where[order[n2:n2 + n3]]] = random.randint(0, nb_symbol_category - 1)
        return out


class BERT_Text_Dataset(torch.utils.data.Dataset):
    """(ling_data, masked sy ids, bert_mask) per sentence.  ``metafile``: path(s) of lines ``<id>\\t{sy$tone$flag$ws...} ...``
    (the ``raw_metafile.txt`` format; only the text is used), ``root_dir``: the director(ies) they belong to.  The mask is
    drawn anew at every ``__getitem__``; with ``allow_cache`` the encoded sentence is kept (a plain per-process dict)."""

    def __init__(self, config, metafile, root_dir, allow_cache=False, ling_unit=None):
        from kantts.utils.ling_unit import KanTtsLinguisticUnit
        from kantts.utils.ling_unit.ling_unit import MASK

        self.config = config
        metafile = metafile if isinstance(metafile, list) else [metafile]
        root_dir = root_dir if isinstance(root_dir, list) else [root_dir]
        self.meta = []
        for meta_file, data_dir in zip(metafile, root_dir):
            if not os.path.exists(meta_file):
                raise ValueError("[BERT_Text_Dataset] meta file: {} not found".format(meta_file))
            if not os.path.exists(data_dir):
                raise ValueError("[BERT_Text_Dataset] data dir: {} not found".format(data_dir))
            self.meta.extend(self.load_meta(meta_file, data_dir))
        self.allow_cache = allow_cache
        self.caches = {}
        self.ling_unit = ling_unit if ling_unit is not None else KanTtsLinguisticUnit(config)
        self.padder = Padder()
        self.masking_actor = MaskingActor(config["Model"]["KanTtsTextsyBERT"]["params"]["mask_ratio"])
        self.mask_id = int(self.ling_unit._streams["sy"].ids[MASK])
        self.nsym = int(self.ling_unit.get_unit_size()["sy"])

    def __len__(self):
        return len(self.meta)

    def encoded(self, idx):
        """The sentence's integer streams (each ends with the id of "~"), without a mask."""
        if self.allow_cache and idx in self.caches:
            return self.caches[idx]
        ling_data = self.ling_unit.encode_symbol_sequence(self.meta[idx])
        if self.allow_cache:
            self.caches[idx] = ling_data
        return ling_data

    def __getitem__(self, idx):
        ling_data = self.encoded(idx)
        bert_mask, masked = self.bert_masking(ling_data)
        return (ling_data, masked, bert_mask)

    def load_meta(self, metafile, data_dir):
        items = []
        with open(metafile, "r") as f:
            for line in f:
                if line.strip():
                    _, ling_txt = line.strip().split("\t")
                    items.append(ling_txt)
        return items

    @staticmethod
    def gen_metafile(raw_meta_file, out_dir, split_ratio=0.98):
        """Shuffle the raw metafile with the fixed dataset seed; ``bert_train.lst`` / ``bert_valid.lst`` in ``out_dir``."""
        with open(raw_meta_file, "r") as f:
            lines = f.readlines()
        random.Random(DATASET_RANDOM_SEED).shuffle(lines)  # == random.seed(1234); random.shuffle(lines)
        num_train = int(len(lines) * split_ratio) - 1
        for name, part in (("bert_train.lst", lines[:num_train]), ("bert_valid.lst", lines[num_train:])):
            with open(os.path.join(out_dir, name), "w") as f:
                f.writelines(part)

    def bert_masking(self, ling_data):
        """(mask (L,) of 0. / 1., masked sy ids): every position but the closing "~" is masked with the configured ratio."""
        mask = self.masking_actor._get_random_mask(len(ling_data[0]), p1=self.masking_actor.mask_ratio)
        mask[-1] = 0
        return mask, self.masking_actor._input_bert_masking(ling_data[0], self.nsym, self.mask_id, mask)

    def collate_fn(self, batch):
        pad_ids = [self.ling_unit._sub_unit_pad[t] for t in self.ling_unit._lfeat_type_list[:4]]
        return bert_collate(batch, pad_ids, self.padder)


class _SyntheticUnit:
    """What BERT_Text_Dataset and the loaders read of a KanTtsLinguisticUnit, for id streams that never were text: every
    stream's inventory ends with pad, "~" and [MASK], as ling_unit._Stream lays it out."""

    _lfeat_type_list = ["sy", "tone", "syllable_flag", "word_segment"]

    def __init__(self, sizes):
        self._sizes = {k: int(sizes[k]) for k in self._lfeat_type_list}
        self._sub_unit_pad = {k: n - 3 for k, n in self._sizes.items()}

    def get_unit_size(self):
        return dict(self._sizes)


class SyntheticTextDataset(BERT_Text_Dataset):
    """BERT_Text_Dataset over ``n`` seeded random sentences of ``lo`` .. ``hi`` symbols (the closing "~" included) instead
    of a metafile: ``train_sybert --synthetic N`` and scripts/sybert_bench.py, which need no language resources.  ``sizes``:
    the four inventory sizes (default: kantts.utils.synthetic.SAMBERT_VOCAB)."""

    def __init__(self, config, n, seed=DATASET_RANDOM_SEED, lo=20, hi=120, sizes=None):
        from kantts.utils.synthetic import SAMBERT_VOCAB

        self.config, self.allow_cache, self.caches = config, False, {}
        self.ling_unit = _SyntheticUnit(sizes or SAMBERT_VOCAB)
        self.padder = Padder()
        self.masking_actor = MaskingActor(config["Model"]["KanTtsTextsyBERT"]["params"]["mask_ratio"])
        size = self.ling_unit.get_unit_size()
        self.nsym, self.mask_id = size["sy"], size["sy"] - 1
        rs = np.random.RandomState(seed)
        self.meta = []
        for _ in range(int(n)):
            L = int(rs.randint(lo, hi + 1))
            self.meta.append([np.append(rs.randint(0, size[k] - 3, size=L - 1), size[k] - 2).astype(np.int32)
                              for k in self.ling_unit._lfeat_type_list])

    def encoded(self, idx):
        return self.meta[idx]


def bert_collate(batch, pad_ids, padder=None):
    """Items of BERT_Text_Dataset -> {"input_lings" (B, T, 4) int64: masked sy | tone | syllable_flag | word_segment,
    "valid_input_lengths" (B) int64: the lengths without the closing "~", "targets" (B, T) int64: the unmasked sy ids,
    "bert_masks" (B, T)} padded to the longest sentence with the streams' pad ids (the mask with 0)."""
    padder = padder or Padder()
    T = max(len(x[0][0]) for x in batch)
    streams = [[x[1] for x in batch]] + [[x[0][k] for x in batch] for k in (1, 2, 3)]
    lings = [padder._prepare_scalar_inputs(s, T, pad).long() for s, pad in zip(streams, pad_ids)]
    return {"input_lings": torch.stack(lings, dim=2),
            "valid_input_lengths": torch.as_tensor([len(x[0][0]) - 1 for x in batch], dtype=torch.long),
            "targets": padder._prepare_scalar_inputs([x[0][0] for x in batch], T, pad_ids[0]).long(),
            "bert_masks": padder._prepare_scalar_inputs([x[2] for x in batch], T, 0.0)}


def get_bert_text_datasets(metafile, root_dir, config, allow_cache, split_ratio=0.98):
    """(train, valid) BERT_Text_Datasets over ``bert_train.lst`` / ``bert_valid.lst`` of every data directory, generated
    from the raw metafile when missing."""
    root_dir = root_dir if isinstance(root_dir, list) else [root_dir]
    metafile = metafile if isinstance(metafile, list) else [metafile]
    train_lst, valid_lst = [], []
    for raw_metafile, data_dir in zip(metafile, root_dir):
        train_meta, valid_meta = os.path.join(data_dir, "bert_train.lst"), os.path.join(data_dir, "bert_valid.lst")
        if not os.path.exists(train_meta) or not os.path.exists(valid_meta):
            BERT_Text_Dataset.gen_metafile(raw_metafile, data_dir, split_ratio)
        train_lst.append(train_meta)
        valid_lst.append(valid_meta)
    return (BERT_Text_Dataset(config, train_lst, root_dir, allow_cache),
            BERT_Text_Dataset(config, valid_lst, root_dir, allow_cache))


logging.getLogger(__name__).addHandler(logging.NullHandler())
