"""Device-resident corpus for duration-free (MAS) and speaker-embedding (SE) voices: kantts_attn_prior_rows (the padded
beta-binomial prior of a batch in one launch, from a table of log-factorials), kantts_broadcast_rows_f32 (an utterance's
embedding over its symbols), DeviceAMSet / make_train_loader / AM_Dataset.attach_prior on top of them, and trainer steps fed
from such a corpus.

Legs as in tests/test_fp_captured_step.py: ``kernel_source`` (the kernel sources on the CPU, util.kernel_source_on_cpu) and,
marked ``gpu``, the device.

Bounds.  The prior against ``beta_binomial_prior_distribution(P, M).float()``: every cell within one fp32 rounding of the
fp64 value, |got - ref| <= 2^-23 ref + 2^-126 (the log-space sums carry about 1e-12; the second term allows a flush of fp32
subnormals), and at most 1e-3 of an item's live cells may differ in bits at all; padding exactly zero.  Everything else
is a copy: torch.equal.  Trainer steps: each loss within 1e-5 relative of the host-fed one, weights within
max(3 * floor, 1e-6) in rel-L2, floor = the rel-L2 of two host-fed runs (tests/test_device_batching.py::_feeder_check).

The output of both kernels is a dense (B, rows, width) tensor, so the cells next to an item's live region are its own
padding or the neighbouring item: the guard tests lay the tensor into a flat sentinel buffer with one guard item in front
and behind -- at an offset that is and one that is not 16-byte aligned -- and compare EVERY cell with the expectation."""
import contextlib
import logging
import os

import numpy as np
import pytest
import torch

from util import GOLDEN, kernel_source_on_cpu

LEGS = [pytest.param("hostsim", id="kernel_source"), pytest.param("cuda", id="gpu", marks=pytest.mark.gpu)]
_E_BADARG = -1
_SENTINEL = -777.0
_REF = {}
PAD_IDS = [146, 9, 7, 7, 35, 3]


def _leg(leg):
    return (kernel_source_on_cpu(), "cpu") if leg == "hostsim" else (contextlib.nullcontext(), "cuda")


def _ref(P, M):
    """``beta_binomial_prior_distribution(P, M).float()``, computed once per (P, M) of this file."""
    from kantts.datasets.batching import beta_binomial_prior_distribution

    if (P, M) not in _REF:
        _REF[(P, M)] = beta_binomial_prior_distribution(P, M).float()
    return _REF[(P, M)]


def _round_up(x, m):
    return (x + m - 1) // m * m


def _expected(cases, Tout, Tin):
    ref = torch.zeros(len(cases), Tout, Tin)
    for b, (P, M) in enumerate(cases):
        if P >= 1 and M >= 1:
            ref[b, :M, :P] = _ref(P, M)
    return ref


def _check_prior(got, cases, what=""):
    """got (B, Tout, Tin) on the host against the host function, item by item."""
    B, Tout, Tin = got.shape
    ref = _expected(cases, Tout, Tin)
    for b, (P, M) in enumerate(cases):
        g, r = got[b], ref[b]
        live = torch.zeros(Tout, Tin, dtype=torch.bool)
        live[:M, :P] = True
        assert bool((g[~live] == 0).all()), "%s item %d (%d, %d): padding is not zero" % (what, b, P, M)
        err = (g.double() - r.double()).abs()
        tol = 2.0 ** -23 * r.double() + 2.0 ** -126
        differ = int((g[live] != r[live]).sum())
        worst = float((err / tol).max())
        print("%s prior (P %d, M %d): worst |err| / tol %.3f, %d of %d live cells differ in bits" % (what, P, M, worst, differ, P * M))
        assert bool((err <= tol).all()), "%s item %d (%d, %d): %.3f x the tolerance" % (what, b, P, M, worst)
        assert differ <= 1e-3 * P * M, "%s item %d (%d, %d): %d of %d cells differ in bits" % (what, b, P, M, differ, P * M)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the prior kernel against the host function
_BATCHES = {
    "cell_row_column": [(1, 1), (2, 1), (1, 7)],  # a single cell, a single row, a single column
    "small": [(5, 17), (8, 31), (13, 64)],  # widths that are no multiple of 4; 64 rows
    "tile_edges": [(64, 65), (257, 33)],  # 65 rows; 257 columns; P > M
    "training_shape": [(150, 800)],
    "table_from_cache": [(4100, 2), (3, 3)],  # wider than the LDS window: the table is read through the caches
}


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("name", list(_BATCHES))
def test_prior_kernel_equals_the_host_function(name, leg):
    import kantts._hip as hip

    cases = _BATCHES[name]
    ctx, dev = _leg(leg)
    Tout = _round_up(max(M for _, M in cases), 3)
    Tin = max(P for P, _ in cases) + (1 if name == "training_shape" else 2)  # wider than the longest P; odd and even widths
    with ctx:
        assert hip.has_corpus_prior()
        lfact = hip.log_factorials(max(P + M for P, M in cases), dev)
        assert lfact.dtype == torch.float64 and lfact.numel() == max(P + M for P, M in cases) + 1
        got = hip.attn_prior_rows(lfact, [P for P, _ in cases], [M for _, M in cases], Tout, Tin)
        assert got.shape == (len(cases), Tout, Tin) and got.dtype == torch.float32 and got.device.type == dev
        got = got.cpu()
    _check_prior(got, cases, name)
    if name == "small":  # the rows do NOT sum to 1: the support point k = P is left out, as in the reference
        assert float(got[0, 16, :5].sum()) < 0.5


# ---------------------------------------------------------------------------------------------------------------------
# 2. bounds
def _prior_raw(dev, n_sym, n_mel, Tout, Tin, table_for, offset):
    """kantts_attn_prior_rows into a flat sentinel buffer: one guard item in front of and behind the (B, Tout, Tin) output,
    which starts ``offset`` cells past a 16-byte boundary.  Returns (code, output on the host)."""
    import kantts._hip as hip

    B, L = len(n_sym), Tout * Tin
    buf = torch.full(((B + 2) * L + 8,), _SENTINEL, device=dev)
    assert buf.data_ptr() % 16 == 0
    out = buf[L + offset: L + offset + B * L]
    lfact = hip.log_factorials(table_for, dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32).to(dev)  # noqa: E731
    rc = hip.attn_prior_rows_raw(lfact, lfact.numel(), i32(n_sym), i32(n_mel), out, B=B, Tout=Tout, Tin=Tin)
    host = buf.cpu()
    assert bool((host[: L + offset] == _SENTINEL).all()), "cells in front of the output were written"
    assert bool((host[L + offset + B * L:] == _SENTINEL).all()), "cells behind the output were written"
    return rc, host[L + offset: L + offset + B * L].view(B, Tout, Tin)


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("offset", [0, 1, 3])
def test_prior_kernel_stays_inside_its_output(offset, leg):
    ctx, dev = _leg(leg)
    Tout, Tin = 33, 11
    big = 2 ** 31 - 1
    with ctx:
        # valid input
        rc, got = _prior_raw(dev, [5, 8, 11], [17, 31, 33], Tout, Tin, 44, offset)
        assert rc == 0
        _check_prior(got, [(5, 17), (8, 31), (11, 33)], "valid")
        # P > Tin and M > Tout: clamped to the output
        rc, got = _prior_raw(dev, [Tin + 5, 3, big], [4, Tout + 7, big], Tout, Tin, 44, offset)
        assert rc == 0
        _check_prior(got, [(Tin, 4), (3, Tout), (Tin, Tout)], "clamped")
        # P = 0 / M = 0 (and below): zeros
        rc, got = _prior_raw(dev, [0, 4, -3, 5], [5, 0, 6, -big], Tout, Tin, 44, offset)
        assert rc == 0 and bool((got == 0).all())
        # an item the table does not cover: NaN in its live region, zeros around it, the neighbours' priors as they are
        rc, got = _prior_raw(dev, [5, 8, 3], [17, 31, 4], Tout, Tin, 25, offset)
        assert rc == 0
        assert bool(torch.isnan(got[1, :31, :8]).all())
        assert bool((got[1, 31:] == 0).all()) and bool((got[1, :, 8:] == 0).all())
        _check_prior(got[[0, 2]], [(5, 17), (3, 4)], "next to an uncovered item")
        # ... also when P + M is one past the table's last entry, and not when it is the last entry
        rc, got = _prior_raw(dev, [8, 8], [31, 31], Tout, Tin, 38, offset)
        assert rc == 0 and bool(torch.isnan(got[:, :31, :8]).all())
        rc, got = _prior_raw(dev, [8, 8], [31, 31], Tout, Tin, 39, offset)
        assert rc == 0
        _check_prior(got, [(8, 31), (8, 31)], "table ends at P + M")


@pytest.mark.parametrize("leg", LEGS)
def test_prior_entry_reports_argument_errors(leg, monkeypatch):
    import kantts._hip as hip

    ctx, dev = _leg(leg)
    with ctx:
        lfact = hip.log_factorials(20, dev)
        ns, nm = torch.tensor([3, 4], dtype=torch.int32).to(dev), torch.tensor([5, 6], dtype=torch.int32).to(dev)
        out = torch.full((2, 6, 4), _SENTINEL, device=dev)
        ok = dict(B=2, Tout=6, Tin=4)
        assert hip.attn_prior_rows_raw(None, 21, ns, nm, out, **ok) == _E_BADARG
        assert hip.attn_prior_rows_raw(lfact, 21, None, nm, out, **ok) == _E_BADARG
        assert hip.attn_prior_rows_raw(lfact, 21, ns, None, out, **ok) == _E_BADARG
        assert hip.attn_prior_rows_raw(lfact, 21, ns, nm, None, **ok) == _E_BADARG
        assert hip.attn_prior_rows_raw(lfact, 1, ns, nm, out, **ok) == _E_BADARG
        for bad in (dict(ok, B=0), dict(ok, Tout=0), dict(ok, Tin=0), dict(ok, B=-1)):
            assert hip.attn_prior_rows_raw(lfact, 21, ns, nm, out, **bad) == _E_BADARG
        assert bool((out == _SENTINEL).all())
        assert hip.attn_prior_rows_raw(lfact, 21, ns, nm, out, **ok) == 0
        _check_prior(out.cpu(), [(3, 5), (4, 6)], "after the refusals")
        # the wrapper knows the lengths on the host: a batch the table does not cover never reaches a launch
        monkeypatch.setattr(hip, "attn_prior_rows_raw", lambda *a, **k: pytest.fail("launched"))
        with pytest.raises(ValueError, match="log-factorial table"):
            hip.attn_prior_rows(lfact, [3, 10], [5, 11], 12, 10)
        for n_sym, n_mel in (([3, 0], [5, 6]), ([3, 4], [5, 13]), ([11, 4], [5, 6]), ([3], [5, 6])):
            with pytest.raises(ValueError):
                hip.attn_prior_rows(lfact, n_sym, n_mel, 12, 10)
        # lengths the caller has on the device already: taken as they are, but only int32 tensors of B entries
        for bad in (dict(n_sym_dev=ns.long()), dict(n_mel_dev=nm[:1])):
            with pytest.raises(ValueError, match="int32"):
                hip.attn_prior_rows(lfact, [3, 4], [5, 6], 12, 10, **bad)
        monkeypatch.undo()
        got = hip.attn_prior_rows(lfact, [3, 4], [5, 6], 6, 4, n_sym_dev=ns, n_mel_dev=nm)
        _check_prior(got.cpu(), [(3, 5), (4, 6)], "device lengths")


# ---------------------------------------------------------------------------------------------------------------------
# 3. kantts_broadcast_rows_f32
@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("D", [1, 5, 192])
def test_broadcast_rows_repeats_and_pads(D, leg):
    import kantts._hip as hip

    ctx, dev = _leg(leg)
    Tmax = 7
    g = torch.Generator().manual_seed(D)
    x = torch.randn(4, D, generator=g)
    item, lens = [3, 0, 3, 1, 2], [0, Tmax, 2, 1, 5]  # lengths 0 and Tmax; an item twice
    ref = torch.stack([torch.nn.functional.pad(x[i:i + 1].repeat(n, 1), (0, 0, 0, Tmax - n)) for i, n in zip(item, lens)])
    with ctx:
        t_item, t_lens = torch.tensor(item).to(dev), torch.tensor(lens, dtype=torch.int32).to(dev)
        got = hip.broadcast_rows(x.to(dev), t_item, t_lens, Tmax)
        assert got.shape == ref.shape and got.dtype == torch.float32 and torch.equal(got.cpu(), ref)
        B, L = len(item), Tmax * D
        for offset in (0, 1, 2):
            buf = torch.full(((B + 2) * L + 8,), _SENTINEL, device=dev)
            out = buf[L + offset: L + offset + B * L]
            assert hip.broadcast_rows_raw(x.to(dev), t_item, t_lens, out, n=4, B=B, Tmax=Tmax, D=D) == 0
            host = buf.cpu()
            assert bool((host[: L + offset] == _SENTINEL).all()) and bool((host[L + offset + B * L:] == _SENTINEL).all())
            assert torch.equal(host[L + offset: L + offset + B * L].view(B, Tmax, D), ref)
        # lengths past Tmax are clamped, negative ones and item indices outside the table give zeros: nothing else is read
        wild = torch.tensor([Tmax + 9, -4, 3, 2, 2 ** 31 - 1], dtype=torch.int32).to(dev)
        got = hip.broadcast_rows(x.to(dev), torch.tensor([1, 2, 4, -1, 0]).to(dev), wild, Tmax).cpu()
        assert torch.equal(got[0], x[1:2].repeat(Tmax, 1)) and torch.equal(got[4], x[0:1].repeat(Tmax, 1))
        assert bool((got[1:4] == 0).all())
        out = torch.full((B, Tmax, D), _SENTINEL, device=dev)
        ok = dict(n=4, B=B, Tmax=Tmax, D=D)
        assert hip.broadcast_rows_raw(None, t_item, t_lens, out, **ok) == _E_BADARG
        assert hip.broadcast_rows_raw(x.to(dev), None, t_lens, out, **ok) == _E_BADARG
        assert hip.broadcast_rows_raw(x.to(dev), t_item, None, out, **ok) == _E_BADARG
        assert hip.broadcast_rows_raw(x.to(dev), t_item, t_lens, None, **ok) == _E_BADARG
        for bad in (dict(ok, n=0), dict(ok, B=0), dict(ok, Tmax=0), dict(ok, D=0)):
            assert hip.broadcast_rows_raw(x.to(dev), t_item, t_lens, out, **bad) == _E_BADARG
        assert bool((out == _SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------
# 4. DeviceAMSet against the host collate
def _items(n=6, seed=1, mas=False, se=0, hi=(9, 9, 9, 9, 9, 9), nsym=(5, 15), dur_hi=6):
    """Synthetic items in the manner of tests/test_device_batching.py::_am_items.  ``mas``: slot 2 ``None``, frame-level
    pitch / energy, slot 5 ``None``; ``se``: the size of the (1, D) speaker embedding in slot 7 (0: none)."""
    rng = np.random.RandomState(seed)
    items = []
    lo, up = nsym
    for _ in range(n):
        nsym = int(rng.randint(lo, up))  # incl. the trailing "~"
        dur = rng.randint(1, dur_hi, size=nsym - 1).astype(np.int64)
        frames = int(dur.sum())
        ling = [rng.randint(0, hi[k], size=nsym).astype(np.int64) for k in range(6)]
        feat = frames if mas else nsym
        emb = rng.randn(1, se).astype(np.float32) if se else None
        items.append((ling, rng.randn(frames, 80).astype(np.float32), None if mas else dur,
                      rng.randn(feat).astype(np.float32), rng.randn(feat).astype(np.float32), None, None, emb))
    return items


def _with_host_prior(items):
    """What AM_Dataset.__getitem__ returns by default for duration-free items: the host prior in slot 5."""
    from kantts.datasets.batching import beta_binomial_prior_distribution

    return [it[:5] + (beta_binomial_prior_distribution(len(it[0][0]), len(it[1])),) + it[6:] for it in items]


def _same_batch(got, ref, what=""):
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    for k, v in ref.items():
        if v is None:
            assert got[k] is None, k
            continue
        assert got[k].shape == v.shape and got[k].dtype == v.dtype, (what, k, got[k].shape, got[k].dtype, v.shape, v.dtype)
        if k == "attn_priors":
            lens = zip((ref["valid_input_lengths"] + 1).tolist(), ref["valid_output_lengths"].tolist())
            _check_prior(got[k].cpu(), list(lens), what)
        else:
            assert torch.equal(got[k].cpu(), v), (what, k)


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("kind", ["mas", "se", "mas_se"])
def test_device_set_batches_equal_the_host_collate(kind, leg):
    from kantts.datasets.batching import am_collate
    from kantts.datasets.device_batching import DeviceAMSet

    ctx, dev = _leg(leg)
    mas, se = "mas" in kind, "se" in kind
    items = _items(mas=mas, se=192 if se else 0)
    host_items = _with_host_prior(items) if mas else items
    with ctx:
        ds = DeviceAMSet(items, 3, PAD_IDS, dev, se=se)
        assert len(ds) == 6 and ds.mas == mas
        for idx in ([0, 1, 2], [5, 3, 3, 4], [2]):
            ref = am_collate([host_items[i] for i in idx], 3, PAD_IDS, se=se)
            got = ds.batch(idx)
            if mas:
                assert got.get("band_width") is None and got["durations"] is None
                got.pop("band_width", None)
                assert got["pitch_contours"].shape == ref["mel_targets"].shape[:2]
            else:
                assert isinstance(got.pop("band_width"), int)
            assert all(v is None or v.device.type == dev for v in got.values())
            if se:
                assert got["input_speakers"].dtype == torch.float32 and got["input_speakers"].shape[2] == 192
            _same_batch(got, ref, "%s %s" % (kind, idx))


@pytest.mark.parametrize("leg", LEGS)
def test_device_set_refusals(leg):
    from kantts.datasets.device_batching import DeviceAMSet

    ctx, dev = _leg(leg)
    sup, mas, se = _items(), _items(mas=True), _items(se=5)
    with ctx:
        with pytest.raises(ValueError, match="duration-free"):
            DeviceAMSet(sup[:3] + mas[3:], 3, PAD_IDS, dev)
        with pytest.raises(NotImplementedError, match="FP together with MAS"):
            DeviceAMSet(mas, 3, PAD_IDS, dev, fp=True)
        it = mas[2]
        longer = it[:3] + (np.zeros(_round_up(len(it[1]), 3) + 1, np.float32),) + it[4:]
        with pytest.raises(ValueError, match="pitch"):
            DeviceAMSet(mas[:2] + [longer] + mas[3:], 3, PAD_IDS, dev)
        fits = it[:3] + (np.zeros(_round_up(len(it[1]), 3), np.float32),) + it[4:]  # as long as the padded mel: accepted
        DeviceAMSet(mas[:2] + [fits] + mas[3:], 3, PAD_IDS, dev)
        with pytest.raises(ValueError, match="energy"):
            DeviceAMSet([it[:4] + (np.zeros(len(it[1]) + 3, np.float32),) + it[5:]], 3, PAD_IDS, dev)
        with pytest.raises(ValueError, match="no speaker embedding"):
            DeviceAMSet(se[:4] + [se[4][:7] + (None,)] + se[5:], 3, PAD_IDS, dev, se=True)
        with pytest.raises(ValueError, match="differ in size"):
            DeviceAMSet(se[:5] + [se[5][:7] + (np.zeros((1, 6), np.float32),)], 3, PAD_IDS, dev, se=True)


# ---------------------------------------------------------------------------------------------------------------------
# 5. AM_Dataset on a voice directory
def _language_dir(tmp):
    fx = torch.load(os.path.join(GOLDEN, "am_dataset.pt"), weights_only=False)
    d = os.path.join(tmp, "PinYin")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "PhoneSet.xml"), "w") as f:
        f.write("<phoneSet>" + "".join("<phone><name>%s</name></phone>" % p for p in fx["phones"]) + "</phoneSet>")
    with open(os.path.join(d, "tonelist.txt"), "w") as f:
        f.write("\n".join(fx["tones_file"]) + "\n")
    return d, fx["phones"]


def _tok(sy, emo="emotion_neutral", tone="tone1"):
    return "{%s$%s$s_both$word_both$%s$F7}" % (sy, tone, emo)


def _voice_dataset(tmp, kind, n=5, allow_cache=False):
    """A voice directory as AudioProcessor lays it out, written into ``tmp``: ``kind`` "mas" (no duration/, frame-level
    f0 / energy) or "se" (duration/, se/se.npy)."""
    from kantts.datasets.dataset import AM_Dataset

    lang, phones = _language_dir(str(tmp))
    unit = {"cleaners": "english_cleaners", "language_dir": lang,
            "lfeat_type_list": "sy,tone,syllable_flag,word_segment,emo_category,speaker_category",
            "speaker_list": "F7,F74,M7,FBYN,FRXL,xiaoyu"}
    params = {"outputs_per_step": 3, "MAS": kind == "mas", "SE": kind == "se"}
    config = {"model_type": "sambert", "linguistic_unit": unit, "Model": {"KanTtsSAMBERT": {"params": params}}}
    root = os.path.join(str(tmp), "data_" + kind)
    for d in ("mel", "f0", "energy", "frame_f0", "frame_uv") + (("duration", "se") if kind == "se" else ()):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    rs = np.random.RandomState(7)
    if kind == "se":
        np.save(os.path.join(root, "se", "se.npy"), rs.randn(1, 192).astype(np.float32))
    with open(os.path.join(root, "am_train.lst"), "w") as f:
        for u in range(n):
            name, nsym = "u%d" % u, 3 + u
            f.write("%s\t%s\n" % (name, " ".join(_tok(phones[(u + j) % 9]) for j in range(nsym))))
            dur = rs.randint(2, 6, size=nsym)
            frames = int(dur.sum())
            if kind == "se":
                np.save(os.path.join(root, "duration", name + ".npy"), dur)
            np.save(os.path.join(root, "mel", name + ".npy"), rs.randn(frames, 80).astype(np.float32))
            for d in ("f0", "energy"):
                np.save(os.path.join(root, d, name + ".npy"), rs.randn(frames if kind == "mas" else nsym + 1).astype(np.float32))
    return AM_Dataset(config, os.path.join(root, "am_train.lst"), root, allow_cache=allow_cache)


def test_dataset_attaches_the_host_prior_unless_told_not_to(tmp_path):
    from kantts.datasets.batching import beta_binomial_prior_distribution

    for cache in (False, True):
        ds = _voice_dataset(tmp_path, "mas", allow_cache=cache)
        assert ds.mas_enable and not ds.with_duration and ds.attach_prior is True and len(ds) == 5
        before = [ds[i] for i in range(5)]
        for it in before:  # the default: as before
            assert it[2] is None and torch.equal(it[5], beta_binomial_prior_distribution(len(it[0][0]), len(it[1])))
        ds.attach_prior = False
        beta_binomial_prior_distribution.cache_clear()
        bare = [ds[i] for i in range(5)]
        if not cache:
            assert beta_binomial_prior_distribution.cache_info().misses == 0  # nothing was computed
        for a, b in zip(before, bare):
            assert b[5] is None and len(b) == 8
            for k in (1, 3, 4):
                assert np.array_equal(a[k], b[k])
            assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))
        ds.attach_prior = True
        again = ds[3]
        assert torch.equal(again[5], before[3][5])
        ref = ds.collate_fn(before[:3])
        assert ref["durations"] is None and ref["attn_priors"].shape == ref["mel_targets"].shape[:2] + ref["input_lings"].shape[1:2]
    ds = _voice_dataset(tmp_path, "se")  # nothing to opt out of: the switch changes nothing for supervised items
    ds.attach_prior = False
    assert ds[0][5] is None and ds[0][2] is not None and ds[0][7].shape == (1, 192)


@pytest.mark.gpu
def test_make_train_loader_takes_the_resident_path_for_mas_and_se(tmp_path, monkeypatch, caplog):
    import kantts._hip as hip
    from kantts.datasets.batching import beta_binomial_prior_distribution
    from kantts.datasets.device_batching import DeviceCorpusLoader, PinnedPrefetcher, make_train_loader

    mas, se = _voice_dataset(tmp_path, "mas"), _voice_dataset(tmp_path, "se")
    host_items = [mas[i] for i in range(len(mas))]
    beta_binomial_prior_distribution.cache_clear()
    for mode in ("hbm", "auto"):
        loader = make_train_loader("am", mas, None, "cuda", 2, mode=mode)
        assert isinstance(loader, DeviceCorpusLoader) and loader.set.mas and not loader.set.se
        assert mas.attach_prior is True  # restored
        seen = 0
        for batch in loader:  # an epoch
            assert batch["durations"] is None and batch["attn_priors"].is_cuda and "band_width" not in batch
            seen += batch["mel_targets"].size(0)
        assert seen == len(mas) and len(loader) == 3
    assert beta_binomial_prior_distribution.cache_info().misses == 0  # no host prior from the upload to the last batch
    ordered = DeviceCorpusLoader(loader.set, 2, shuffle=False)
    for k, batch in enumerate(ordered):
        _same_batch(dict(batch), mas.collate_fn(host_items[2 * k: 2 * k + 2]), "mas voice directory")
    loader = make_train_loader("am", se, None, "cuda", 2, mode="hbm")
    assert isinstance(loader, DeviceCorpusLoader) and loader.set.se and not loader.set.mas and se.attach_prior is True
    for k, batch in enumerate(DeviceCorpusLoader(loader.set, 2, shuffle=False)):
        got = dict(batch)
        assert isinstance(got.pop("band_width"), int)
        _same_batch(got, se.collate_fn([se[i] for i in range(2 * k, min(2 * k + 2, len(se)))]), "se voice directory")
    # "pinned" and "off" are what they were
    assert isinstance(make_train_loader("am", mas, [], "cuda", 2, mode="pinned"), PinnedPrefetcher)
    host = object()
    assert make_train_loader("am", mas, host, "cuda", 2, mode="off") is host
    # a library built before the two entry points still serves these voices, through the prefetcher, and says why
    monkeypatch.setattr(hip, "has_corpus_prior", lambda: False)
    for ds in (mas, se):
        with caplog.at_level(logging.WARNING):
            caplog.clear()
            assert isinstance(make_train_loader("am", ds, [], "cuda", 2, mode="hbm"), PinnedPrefetcher)
            assert "kantts_attn_prior_rows" in caplog.text


# ---------------------------------------------------------------------------------------------------------------------
# the streams of a captured step (the tests of this file take streams from torch's pool: what the later tests get moves)
@pytest.mark.gpu
def test_roles_of_a_captured_step_never_share_a_pool_stream():
    """torch's pool hands out 32 streams round-robin, so stream n and stream n + 32 of a process are ONE HIP stream.  The
    helper roles of kantts._hip.ops (attention side stream, branch streams, weight-gradient stream, variance-predictor
    branch) are created through their own code paths with 31 pool allocations between one and the next -- the next
    ``torch.cuda.Stream()`` is then the stream the previous role holds -- and more than two rounds of the pool pass before
    the capture streams: the roles, the current stream and a capture stream stay pairwise distinct."""
    from kantts._hip import deferred_tn, ops

    def a_round_minus_one():
        return [torch.cuda.Stream() for _ in range(31)]

    t = torch.zeros(8, device="cuda")
    was = ops.wgrad_overlap.enabled, ops.side_branch.enabled, deferred_tn.enabled
    burnt = a_round_minus_one()
    try:
        ops._pair_on_two_streams(lambda: None, lambda: None, side_inputs=(t,))  # the attention / plan side stream
        burnt += a_round_minus_one()
        ops.parallel_branches([lambda: None, lambda: None, lambda: None], inputs=(t,))  # the branch streams
        burnt += a_round_minus_one()
        ops.wgrad_overlap.enable(True)
        with ops.wgrad_overlap.side(t):  # the weight-gradient stream
            pass
        burnt += a_round_minus_one()
        with ops.side_branch.fork(t):  # the variance-predictor branch
            pass
        ops.wgrad_overlap.join()
    finally:
        ops.wgrad_overlap.enabled, ops.side_branch.enabled, deferred_tn.enabled = was
    torch.cuda.synchronize()
    assert len({s.cuda_stream for s in burnt}) == 32  # the pool is what this test takes it for
    roles = ops.helper_streams()
    assert len(roles) >= 6 and ops.wgrad_overlap._stream is not None and ops.side_branch._stream is not None
    current = torch.cuda.current_stream().cuda_stream
    ids = [s.cuda_stream for s in roles]
    assert len(set(ids)) == len(ids) and current not in ids, ids
    for _ in range(70):  # more than two rounds of the pool
        cap = ops.distinct_stream()
        assert cap.cuda_stream != current and cap.cuda_stream not in ids
    side = ops._new_side_stream()
    assert side.cuda_stream != current and side.cuda_stream not in ids


# ---------------------------------------------------------------------------------------------------------------------
# 6. trainer steps fed from the resident corpus
_VOCAB_HI = (140, 7, 5, 5, 30, 1)
_INDEX_BATCHES = [[0, 3, 5], [7, 1], [0, 3, 5], [7, 1]]  # four steps over two batch shapes


def _trainer(dev, save_dir, fixture, graph):
    """The tiny configuration of ``fixture`` without dropout and in eval() (Prenet's hard-wired dropout off): deterministic
    steps, as the captured-against-eager tests run their trainers."""
    from kantts.models import model_builder
    from kantts.train.loss import criterion_builder
    from kantts.train.trainer import Sambert_Trainer

    cfg = dict(torch.load(os.path.join(GOLDEN, fixture), weights_only=False)["cfg"])
    for k in list(cfg):
        if "dropout" in k:
            cfg[k] = 0.0
    loss = {"MelReconLoss": {"enable": True, "params": {"loss_type": "mae"}},
            "ProsodyReconLoss": {"enable": True, "params": {"loss_type": "mae"}}}
    if cfg.get("MAS"):
        loss.update(AttentionCTCLoss={"enable": True},
                    AttentionBinarizationLoss={"enable": True, "params": {"start_epoch": 0, "warmup_epoch": 4}})
    config = {"model_type": "sambert", "Model": {"KanTtsSAMBERT": {
        "params": cfg,
        "optimizer": {"type": "Adam", "params": {"lr": 0.001, "betas": [0.9, 0.98], "eps": 1e-9, "weight_decay": 0.0}},
        "scheduler": {"type": "NoamLR", "params": {"warmup_steps": 4000}}}},
        "Loss": loss, "grad_norm": 1.0, "batch_size": 3, "log_interval_steps": 1}
    torch.manual_seed(0)
    model, opt, sch = model_builder(config, device=dev)
    model["KanTtsSAMBERT"].eval()
    crit = criterion_builder(config, dev)
    tr = Sambert_Trainer(config, model, opt, sch, crit, torch.device(dev), None, [], None, max_steps=10 ** 6,
                         save_dir=str(save_dir), save_interval=10 ** 6, valid_interval=10 ** 6, log_interval=1, grad_clip=1.0,
                         graph=graph)
    tr.set_model_state = lambda state="train": None
    tr.epoch = 2  # MAS: a binarisation warm-up ratio of 0.5
    return tr


def _fed_steps(dev, save_dir, fixture, graph, feed, items, se):
    from kantts.datasets.batching import am_collate
    from kantts.datasets.device_batching import DeviceAMSet, DeviceCorpusLoader

    tr = _trainer(dev, save_dir, fixture, graph)
    mas = items[0][2] is None
    assert tr.with_MAS == mas
    if feed == "device":
        loader = DeviceCorpusLoader(DeviceAMSet(items, 3, PAD_IDS, dev, se=se), 3, batches=_INDEX_BATCHES)
    else:
        host_items = _with_host_prior(items) if mas else items
        loader = [am_collate([host_items[i] for i in idx], 3, PAD_IDS, se=se) for idx in _INDEX_BATCHES]
    losses = []
    for batch in loader:
        if feed == "device":
            assert batch["mel_targets"].device.type == dev and (batch["attn_priors"] is not None) == mas
        losses.append(float(tr.train_step(batch)))
        tr.steps += 1
    if graph:
        assert len(tr._graphs) == 2
    return losses, torch.cat([p.detach().reshape(-1).cpu() for p in tr.model["KanTtsSAMBERT"].parameters()])


def _feeder_check(dev, tmp, fixture, graph, items, se=False):
    import kantts._hip as hip

    hip.set_precision("fp32")
    la, wa = _fed_steps(dev, tmp / "a", fixture, graph, "host", items, se)
    lb, wb = _fed_steps(dev, tmp / "b", fixture, graph, "device", items, se)
    floor = 0.0  # the kernel sources on the CPU run on one thread in a fixed order: two host-fed runs are identical
    if dev == "cuda":  # on the device the weight gradients are fp32 atomics whose order differs from run to run
        lc, wc = _fed_steps(dev, tmp / "c", fixture, graph, "host", items, se)
        floor = float((wa - wc).norm() / wa.norm())
    got = float((wa - wb).norm() / wa.norm())
    print("%s graph=%s: host-fed %s corpus-fed %s, weights rel-L2 %.2e, floor %.2e" % (fixture, graph, la, lb, got, floor))
    assert all(np.isfinite(x) for x in la + lb)
    assert all(abs(x - y) <= 1e-5 * max(1.0, abs(x)) for x, y in zip(la, lb)), (la, lb)
    assert got <= max(3 * floor, 1e-6), (got, floor)


def test_eager_mas_steps_fed_from_the_resident_corpus_equal_host_fed_steps_kernel_source(tmp_path):
    # (short utterances: a step of the tiny model takes seconds on this leg whatever the batch holds)
    with kernel_source_on_cpu():
        _feeder_check("cpu", tmp_path, "sambert_tiny_mas.pt", False,
                      _items(n=8, seed=4, mas=True, hi=_VOCAB_HI, nsym=(3, 6), dur_hi=4))


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_mas_steps_fed_from_the_resident_corpus_equal_host_fed_steps_gpu(graph, tmp_path):
    _feeder_check("cuda", tmp_path, "sambert_tiny_mas.pt", graph, _items(n=8, seed=4, mas=True, hi=_VOCAB_HI))


@pytest.mark.gpu
def test_eager_se_steps_fed_from_the_resident_corpus_equal_host_fed_steps_gpu(tmp_path):
    _feeder_check("cuda", tmp_path, "sambert_tiny_se.pt", False, _items(n=8, seed=4, se=192, hi=_VOCAB_HI), se=True)
