"""sy-BERT pre-training entry point (reference kantts/bin/train_sybert.py:35-222): masked-LM training of the text encoder on
unlabelled symbol sequences.  Same flags, config handling, stage-directory layout (config.yaml, ckpt/, log/), resume
semantics and emergency checkpoint; ``<root_dir>/raw_metafile.txt`` holds lines ``index\\tsymbols``.  The checkpoint is what
``train_sambert --resume_bert_path`` takes.

``--synthetic N`` trains on N seeded random sentences of 20 - 120 symbols (no metafile, no language resources; one epoch).
N counts SENTENCES here -- train_sambert's counts batches -- because both feeders below need a corpus to draw batches from.
``--device_corpus``: "hbm" = the encoded corpus resident in HBM, batches gathered and MASKED on the device
(DeviceTextSet, kantts_bert_mask_rows); "host" = the reference's DataLoader over the host collate, whose masks come from
``np.random`` / ``random``; "auto" = "hbm" on a HIP device whose library has the entry points, else "host".  The validation
loader is always the host collate."""
import argparse
import logging
import os
import sys

import torch
import yaml

from kantts.bin._common import count_parameters, load_config, setup_device
from kantts.models import model_builder
from kantts.train.loss import criterion_builder
from kantts.train.trainer import Textsy_BERT_Trainer


def train(model_config, root_dir, stage_dir, resume_path=None, local_rank=0, synthetic=0, device_corpus="auto"):
    from torch.utils.data import DataLoader

    from kantts.datasets.dataset import SyntheticTextDataset, get_bert_text_datasets
    from kantts.datasets.device_batching import make_train_loader

    if device_corpus not in ("auto", "hbm", "host"):
        raise ValueError("device_corpus must be auto, hbm or host, got %r" % (device_corpus,))
    distributed, device, local_rank, world_size = setup_device()
    if local_rank != 0:
        sys.stdout = open(os.devnull, "w")
        logging.getLogger().disabled = True
    root_dir = root_dir if isinstance(root_dir, list) else [root_dir]
    if local_rank == 0:
        os.makedirs(stage_dir, exist_ok=True)
    config = load_config(model_config, []) if not isinstance(model_config, dict) else dict(model_config)
    if local_rank == 0:
        with open(os.path.join(stage_dir, "config.yaml"), "w") as f:
            yaml.dump(config, f, Dumper=yaml.Dumper, default_flow_style=None)
    if distributed:
        config["rank"], config["distributed"] = torch.distributed.get_rank(), True
    if synthetic:
        train_set, valid_set = SyntheticTextDataset(config, synthetic, seed=1234 + 1000 * config.get("rank", 0)), None
    else:
        meta = [os.path.join(d, "raw_metafile.txt") for d in root_dir]
        train_set, valid_set = get_bert_text_datasets(meta, root_dir, config, config.get("allow_cache", False))
        logging.info("The number of training files = %d.", len(train_set))
        logging.info("The number of validation files = %d.", len(valid_set))
    sampler = {"train": None, "valid": None}
    if distributed:
        from torch.utils.data.distributed import DistributedSampler

        sampler["train"] = DistributedSampler(train_set, num_replicas=world_size, shuffle=True)
        if valid_set is not None:
            sampler["valid"] = DistributedSampler(valid_set, num_replicas=world_size, shuffle=False)
    kw = dict(batch_size=config["batch_size"], num_workers=config.get("num_workers", 0),
              pin_memory=config.get("pin_memory", False))
    train_loader = DataLoader(train_set, shuffle=not distributed, collate_fn=train_set.collate_fn, sampler=sampler["train"], **kw)
    valid_loader = None
    if valid_set is not None:
        valid_loader = DataLoader(valid_set, shuffle=not distributed, collate_fn=valid_set.collate_fn,
                                  sampler=sampler["valid"], **kw)
    if device_corpus != "host":
        train_loader = make_train_loader("bert", train_set, train_loader, device, config["batch_size"],
                                         sampler=sampler["train"], mode=device_corpus)
    config["Model"]["KanTtsTextsyBERT"]["params"].update(train_set.ling_unit.get_unit_size())
    model, optimizer, scheduler = model_builder(config, device, local_rank, distributed)
    criterion = criterion_builder(config, device)
    logging.info("TextsyBERT model parameters count: %d", count_parameters(model["KanTtsTextsyBERT"]))
    trainer = Textsy_BERT_Trainer(config=config, model=model, optimizer=optimizer, scheduler=scheduler, criterion=criterion,
                                  device=device, sampler=sampler, train_loader=train_loader, valid_loader=valid_loader,
                                  max_steps=config.get("train_max_steps"), max_epochs=1 if synthetic else None,
                                  save_dir=stage_dir, save_interval=config.get("save_interval_steps", 10 ** 9),
                                  valid_interval=config.get("eval_interval_steps", 10 ** 9),
                                  log_interval=config.get("log_interval_steps", 10), grad_clip=config.get("grad_norm"))
    if resume_path is not None:
        trainer.load_checkpoint(resume_path, True)
        logging.info("Successfully resumed from %s.", resume_path)
    try:
        trainer.train()
    except (Exception, KeyboardInterrupt) as e:  # noqa: BLE001 - the reference saves an emergency checkpoint here too
        logging.error(e, exc_info=True)
        trainer.save_checkpoint(os.path.join(stage_dir, "ckpt", "checkpoint-%d.pth" % trainer.steps))
        raise
    return trainer


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description="Pre-train the text encoder as a masked language model (sy-BERT)")
    parser.add_argument("--model_config", type=str, required=True, help="model config file")
    parser.add_argument("--root_dir", nargs="+", type=str, default=[], help="root dir of dataset(s), each with raw_metafile.txt")
    parser.add_argument("--stage_dir", type=str, required=True, help="stage dir of checkpoint, log and intermediate results")
    parser.add_argument("--resume_path", type=str, default=None, help="path to resume checkpoint")
    parser.add_argument("--local_rank", type=int, default=0, help="local rank for distributed training")
    parser.add_argument("--synthetic", type=int, default=0, help="train on N seeded synthetic sentences (no dataset)")
    parser.add_argument("--device_corpus", default="auto", choices=["auto", "hbm", "host"],
                        help="the encoded corpus resident in HBM with batches gathered and masked on the device (hbm), the "
                             "reference's DataLoader over the host collate (host), or hbm where the device and the library "
                             "allow it (auto)")
    a = parser.parse_args()
    train(a.model_config, a.root_dir, a.stage_dir, a.resume_path, a.local_rank, a.synthetic, a.device_corpus)
