"""ctypes wrapper over tests/support/libslpx_sensbatchcheck.so — TEST INFRASTRUCTURE ONLY.

classify(): which instances of a batched sensitivity call are differentiated at all (csrc/sens_plan.hpp:
sens_classify_instances), on numpy rows.  No device is touched.
"""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np

import sleipnir_amd

HERE = Path(__file__).resolve().parent
LIB_PATH = HERE / "libslpx_sensbatchcheck.so"
_CSRC = HERE.parents[1] / "sleipnir_amd" / "csrc"
SOURCES = [HERE / "sensbatchcheck.cpp", _CSRC / "sens_plan.hpp"]


def build():
    sleipnir_amd.build()
    return _build_probe()


def _build_probe():
    # (host code only; lib() builds the probe alone: libslpx.so is loaded by then)
    cmd = ["/opt/rocm/bin/hipcc", "-O2", "-std=c++23", "-fPIC", "-shared", "--offload-host-only", "-x", "hip",
           str(HERE / "sensbatchcheck.cpp"), "-o", str(LIB_PATH), "-L" + str(sleipnir_amd.LIB_PATH.parent), "-lslpx",
           "-Wl,-rpath," + str(sleipnir_amd.LIB_PATH.parent)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("building sensbatchcheck failed:\n" + res.stdout + res.stderr)
    return LIB_PATH


def _stale():
    if not LIB_PATH.exists():
        return True
    t = LIB_PATH.stat().st_mtime
    return any(t < p.stat().st_mtime for p in SOURCES + [sleipnir_amd.LIB_PATH])


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    sleipnir_amd.lib()  # make sure libslpx.so is loaded first
    if _stale():
        _build_probe()
    L = ctypes.CDLL(str(LIB_PATH))
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    L.sbc_classify.restype = None
    L.sbc_classify.argtypes = [i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp]
    _lib = L
    return L


def classify(x, s, y, z, mu, params, extra=None):
    """status (B) for rows x (B, n), s (B, m_i), y (B, m_e), z (B, m_i), mu (B), params (B, n_p), extra (B, k) or None;
    an array with no columns goes down as NULL, as the C ABI allows."""
    arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in (x, s, y, z, np.reshape(mu, (-1, 1)), params)]
    B = arrays[0].shape[0]
    for a in arrays:
        assert a.ndim == 2 and a.shape[0] == B
    e = None if extra is None else np.ascontiguousarray(extra, dtype=np.float64)
    status = np.full(B, -1, dtype=np.int32)
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None
    lib().sbc_classify(B, arrays[0].shape[1], arrays[2].shape[1], arrays[1].shape[1], arrays[5].shape[1], *(ptr(a) for a in arrays),
                       ptr(e), 0 if e is None else e.shape[1], status.ctypes.data)
    return status
