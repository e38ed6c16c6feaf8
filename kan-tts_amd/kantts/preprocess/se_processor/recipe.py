"""Closed-form stand-in weights for the D-TDNN extractor: every element is a hash of (tensor name, element index) mapped to
the tensor's init scale, so the same state dict can be rebuilt anywhere without storing it (28 MB at the shipped
geometry) and without depending on any library's random stream.  Used by the fixture recorder, the tests and the bench;
a real voice loads its own ``se.model``."""
import numpy as np
import torch

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def _name_hash(name):
    h = 0xCBF29CE484222325  # FNV-1a, 64 bit
    for ch in name.encode("utf-8"):
        h = ((h ^ ch) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return np.uint64(h)


def unit_uniform(name, n):
    """n values in [0, 1): 24 bits of splitmix64(hash(name) + i * golden), i = 0 .. n - 1, as fp64."""
    with np.errstate(over="ignore"):
        z = _name_hash(name) + np.arange(n, dtype=np.uint64) * _GOLDEN
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float64) / float(1 << 24)


def tensor_from_recipe(name, shape, lo, hi):
    n = int(np.prod(shape)) if len(shape) else 1
    v = lo + (hi - lo) * unit_uniform(name, n)
    return torch.from_numpy(v.astype(np.float32)).reshape(tuple(shape))


def recipe_state_dict(model, tag=""):
    """A state dict for ``model`` (a DTDNN of any geometry), keyed and shaped like ``model.state_dict()``:
      convolution / dense weights: uniform with the variance of the Kaiming-normal init, +-sqrt(6 / fan_in);
      BatchNorm weight in [0.5, 1.5), bias and running_mean in [-0.2, 0.2), running_var in [0.5, 1.5);
      the PoolingBlock biases in [-0.2, 0.2); num_batches_tracked = 1."""
    out = {}
    for key, ref in model.state_dict().items():
        name, shape = tag + key, tuple(ref.shape)
        if key.endswith("num_batches_tracked"):
            out[key] = torch.ones((), dtype=torch.long)
        elif key.endswith("running_var"):
            out[key] = tensor_from_recipe(name, shape, 0.5, 1.5)
        elif key.endswith("running_mean") or key.endswith(".bias"):
            out[key] = tensor_from_recipe(name, shape, -0.2, 0.2)
        elif len(shape) == 1:  # a BatchNorm weight
            out[key] = tensor_from_recipe(name, shape, 0.5, 1.5)
        else:
            bound = (6.0 / float(np.prod(shape[1:]))) ** 0.5
            out[key] = tensor_from_recipe(name, shape, -bound, bound)
    return out
