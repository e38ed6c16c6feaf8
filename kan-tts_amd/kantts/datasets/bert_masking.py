"""The BERT masking of sy-BERT pre-training with counter-based draws: the numpy statement of the rule that
kantts_bert_mask_rows (csrc/sybert.hip, contract in include/kantts_hip.h) evaluates on the device, as
``chunked_nsf.initial_state`` is the host statement of kantts_nsf_draw_states.

The rule restates ``BERT_Text_Dataset.bert_masking`` / ``MaskingActor`` (kantts/datasets/dataset.py): every position but the
closing "~" is masked with probability ``mask_ratio``; of the n masked positions of a sequence floor(0.8 n) read [MASK],
floor(0.1 n) read the sequence's ONE random symbol, the rest keep their id -- which of them is decided by a shuffle there and
by sorting iid 64-bit keys here (the same distribution).  All arithmetic is uint64, wrapping."""
import numpy as np

TAG = 0x53594245
_M64 = (1 << 64) - 1


def mix(seed, blk):
    """kantts_rng_mix of csrc/common.h on uint64 arrays (or Python ints): two rounds of a splitmix finaliser."""
    with np.errstate(over="ignore"):
        z = np.asarray(seed, dtype=np.uint64) + np.asarray(blk, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def threshold(mask_ratio):
    """floor(mask_ratio * 2^24), in fp64."""
    return int(np.floor(np.float64(mask_ratio) * 16777216.0))


def draw(seed, counter, targets, lens, mask_ratio, mask_id, nsym):
    """targets (B, T) int64, lens (B) -- the lengths INCLUDING the closing "~" -- -> (ids (B, T) int64, masks (B, T) fp32) of
    draw number ``counter`` under ``seed``: what one launch of kantts_bert_mask_rows writes when the device words hold
    {seed, counter}."""
    targets = np.asarray(targets, dtype=np.int64)
    B, T = targets.shape
    thr = np.uint64(threshold(mask_ratio))
    ids, masks = targets.copy(), np.zeros((B, T), np.float32)
    base = mix(seed & _M64, TAG)
    j = np.arange(T, dtype=np.uint64)
    for b in range(B):
        key = mix(base, ((int(counter) << 20) | b) & _M64)
        L = min(max(int(lens[b]), 0), T)
        masked = ((mix(key, j) >> np.uint64(40)) < thr) & (np.arange(T) < L - 1)
        pos = np.nonzero(masked)[0]
        n = len(pos)
        n2, n3 = 4 * n // 5, n // 10
        order = pos[np.lexsort((pos, mix(key, np.uint64(1 << 32) + pos.astype(np.uint64))))]  # by (key, position)
        rnd = (int(mix(key, 1 << 33)) >> 32) * int(nsym) >> 32
        ids[b, order[:n2]] = mask_id
        ids[b, order[n2:n2 + n3]] = rnd
        masks[b, pos] = 1.0
    return ids, masks
