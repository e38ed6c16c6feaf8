"""TEST INFRASTRUCTURE -- records tests/golden/spk_embed.pt by running the UNTOUCHED reference DTDNN
(kantts/preprocess/se_processor/D_TDNN.py of the reference tree) on the CPU.

    python scripts/record_spk_embed_golden.py        # needs the reference tree (oracle/ref_harness.REFERENCE_ROOT)

The weights are NOT stored (28 MB at the shipped geometry): they come from the closed-form recipe of
kantts.preprocess.se_processor.recipe (a hash of tensor name and element index), which the tests evaluate again.  The
recipe's state dict is built for the PACKAGE's DTDNN and loaded with ``strict=True`` into the reference's -- that load is
the key-compatibility check.  The file holds data only: the four input feature matrices (250, 199, 201 and 28 frames, from
the same recipe), and per geometry the reference's embedding of every item alone, the state-dict keys and shapes, the
parameter count, and the measured error of the fp32 forward against an fp64 copy of the same module (the figure the
kernel path's tolerance is derived from; tests/test_spk_embed.py).

tests/golden/kaldi_fbank.pt (torchaudio.compliance.kaldi.fbank on the fbank test's waveforms) is written only when
torchaudio imports; it does not on the machines this project is developed on."""
import importlib
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "kan-tts_amd"))
import ref_harness  # noqa: E402
from kantts.preprocess.se_processor.D_TDNN import DTDNN  # noqa: E402
from kantts.preprocess.se_processor.recipe import recipe_state_dict, tensor_from_recipe  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "spk_embed.pt")
OUT_FBANK = os.path.join(ROOT, "tests", "golden", "kaldi_fbank.pt")
FRAMES = (250, 199, 201, 28)
GEOMETRIES = {"shipped": {}, "reduced": dict(embedding_size=16, growth_rate=8, bn_size=2, init_channels=32)}
FBANK_SAMPLES = (4800, 4879, 4880, 4959, 4960, 40240)  # as tests/test_spk_embed.py


def reference_dtdnn():
    """The reference's DTDNN class, imported under a private package name (its own ``kantts`` cannot share a process with
    the package's)."""
    src = os.path.join(ref_harness.REFERENCE_ROOT, "kantts", "preprocess", "se_processor")
    if not os.path.isfile(os.path.join(src, "D_TDNN.py")):
        raise RuntimeError("reference tree not present at %s" % ref_harness.REFERENCE_ROOT)
    pkg = types.ModuleType("_ref_se_processor")
    pkg.__path__ = [src]
    sys.modules["_ref_se_processor"] = pkg
    return importlib.import_module("_ref_se_processor.D_TDNN").DTDNN


def inputs():
    return [tensor_from_recipe("feats/%d" % i, (n, 80), -4.0, 4.0) for i, n in enumerate(FRAMES)]


def fbank_waveform(i, n):
    """Waveform i of the fbank test: two tones and recipe noise, inside [-1, 1]."""
    t = torch.arange(n, dtype=torch.float64) / 16000.0
    x = 0.3 * torch.sin(2 * torch.pi * (220.0 + 90.0 * i) * t) + 0.2 * torch.sin(2 * torch.pi * (1800.0 + 400.0 * i) * t + 0.5)
    return (x + 0.1 * tensor_from_recipe("wav/%d" % i, (n,), -1.0, 1.0).double() + 0.05).float()


def main():
    Ref = reference_dtdnn()
    feats = inputs()
    out = {"frames": list(FRAMES), "feats": feats, "geometries": {}}
    for name, geo in GEOMETRIES.items():
        ours = DTDNN(**geo)
        sd = recipe_state_dict(ours)
        ref = Ref(**geo)
        ref.load_state_dict(sd, strict=True)  # the key-compatibility check
        ref.eval()
        ref64 = Ref(**geo).double()
        ref64.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, strict=True)
        ref64.eval()
        with torch.no_grad():
            emb = [ref(f.clone()[None]) for f in feats]
            emb64 = [ref64(f.double()[None]) for f in feats]
        err = [float((a.double() - b).abs().max()) for a, b in zip(emb, emb64)]
        out["geometries"][name] = dict(
            kwargs=dict(geo), embeddings=torch.cat(emb, 0), fp32_vs_fp64=err, scale=float(torch.cat(emb64, 0).abs().max()),
            params=sum(p.numel() for p in ref.parameters()), keys=[(k, tuple(v.shape)) for k, v in ref.state_dict().items()])
        print(name, "params %d, %d tensors, scale %.3g, fp32 vs fp64 %s" % (
            out["geometries"][name]["params"], len(sd), out["geometries"][name]["scale"], ["%.2e" % e for e in err]))
    torch.save(out, OUT)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    try:
        import torchaudio.compliance.kaldi as kaldi
    except Exception as e:  # noqa: BLE001
        print("torchaudio does not import (%s): %s is not written" % (type(e).__name__, OUT_FBANK))
        return
    wavs = [fbank_waveform(i, n) for i, n in enumerate(FBANK_SAMPLES)]
    torch.save({"samples": list(FBANK_SAMPLES), "fbank": [kaldi.fbank(w[None], num_mel_bins=80) for w in wavs]}, OUT_FBANK)
    print("wrote", OUT_FBANK)


if __name__ == "__main__":
    main()
