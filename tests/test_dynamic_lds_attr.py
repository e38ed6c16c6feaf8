"""kantts_allow_dynamic_lds (csrc/prims.h) raises a kernel's dynamic-LDS limit once per DEVICE: the attribute belongs to
the device, so a second device in the same process needs its own call.  Runs on the host build of the kernel sources
(tests/hipemu), whose hip shim has a settable current device and counts hipFuncSetAttribute per (function, device).

The entry point is kantts_upsample_stream at (Cin, Cout, S) = (64, 32, 2) with one token: one workgroup, one live tile,
eight MFMA rendezvous.  The library is loaded from a private copy, so the helper's per-kernel device mask and the shim's
counters start from zero whatever the other tests of the session have launched."""
import ctypes
import os
import shutil
import sys

import numpy as np
import pytest

import util

pytestmark = pytest.mark.skipif(not os.path.exists(os.environ.get("HIPEMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")),
                                reason="the host build of the kernel sources needs the ROCm clang")


def _aligned(nbytes):
    raw = np.zeros(nbytes + 16, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + nbytes]


def test_dynamic_lds_limit_is_raised_once_per_device(tmp_path):
    sys.path.insert(0, os.path.join(util.ROOT, "tests", "hipemu"))
    try:
        import build as hipemu_build
    finally:
        sys.path.pop(0)
    private = str(tmp_path / "libkantts_hostsim_private.so")
    shutil.copy(hipemu_build.build(), private)
    lib = ctypes.CDLL(private)
    lib.kantts_upsample_stream.restype = ctypes.c_int
    lib.kantts_upsample_stream.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int] * 5 + [ctypes.c_float, ctypes.c_int, ctypes.c_void_p]
    lib.hipemu_attr_calls.restype = ctypes.c_int
    lib.hipemu_set_device.argtypes = [ctypes.c_int]

    cin, cout, s = 64, 32, 2
    x = _aligned(1 * cin * 2)                 # (B*T, Cin) bf16
    wp = _aligned(s * cout * 2 * cin * 2)     # (S*Cout, 2*Cin) bf16
    out = _aligned(1 * s * cout * 4)          # (B*T*S, Cout) fp32

    def launch():
        rc = lib.kantts_upsample_stream(x.ctypes.data, wp.ctypes.data, None, None, out.ctypes.data, 1, 1, cin, cout, s, 1.0, 0, None)
        assert rc == 0

    def table():
        fns, devs, counts = (ctypes.c_void_p * 8)(), (ctypes.c_int * 8)(), (ctypes.c_int * 8)()
        n = lib.hipemu_attr_calls(fns, devs, counts, 8)
        assert n <= 8
        return {(fns[i], devs[i]): counts[i] for i in range(n)}

    assert table() == {}
    launch()
    launch()
    lib.hipemu_set_device(1)
    launch()
    t = table()
    kernels = {fn for fn, _ in t}
    assert len(kernels) == 1, t  # one kernel instantiation behind this shape
    (fn,) = kernels
    assert t == {(fn, 0): 1, (fn, 1): 1}
    lib.hipemu_set_device(0)
    launch()
    assert table() == t
