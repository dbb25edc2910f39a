"""ctypes wrapper over tests/support/libslpx_warmcheck.so — TEST INFRASTRUCTURE ONLY.

A probe of the warm-start launches of slpx::BatchDevice (warmcheck.cpp): batch_warm_start_kernel and
batch_unscale_iterate_kernel through their launch wrappers in libslpx.so, on an `sa.System(problem, B)`, with the iterate,
the scales and the c_i the kernel reads set by the caller.  Never used by the product.
"""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np

import sleipnir_amd

HERE = Path(__file__).resolve().parent
LIB_PATH = HERE / "libslpx_warmcheck.so"
_CSRC = HERE.parents[1] / "sleipnir_amd" / "csrc"
SOURCES = [HERE / "warmcheck.cpp", HERE / "probe_common.hpp", _CSRC / "ipm_batch.hpp", _CSRC / "eq_batch.hpp",
           _CSRC / "batch_lockstep.hpp"]


def build():
    sleipnir_amd.build()
    return _build_probe()


def _build_probe():
    # (lib() builds the probe alone: libslpx.so is loaded by then, and relinking it in place would pull the file out
    # from under the process)
    cmd = ["/opt/rocm/bin/hipcc", "-O2", "-std=c++23", "-fPIC", "-shared", "--offload-arch=gfx950",
           "-x", "hip", str(HERE / "warmcheck.cpp"), "-o", str(LIB_PATH),
           "-L" + str(sleipnir_amd.LIB_PATH.parent), "-lslpx",
           "-Wl,-rpath," + str(sleipnir_amd.LIB_PATH.parent)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("building warmcheck failed:\n" + res.stdout + res.stderr)
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
    sleipnir_amd.lib()  # make sure libslpx.so is loaded first (same arena)
    if _stale():
        _build_probe()
    L = ctypes.CDLL(str(LIB_PATH))
    vp, i32 = ctypes.c_void_p, ctypes.c_int32

    def sig(name, restype, *argtypes):
        fn = getattr(L, name)
        fn.restype = restype
        fn.argtypes = list(argtypes)

    sig("wc_last_error", ctypes.c_char_p)
    sig("wc_create", vp, vp)
    sig("wc_destroy", None, vp)
    sig("wc_dims", i32, vp, vp)
    sig("wc_set_scales", i32, vp, vp)
    sig("wc_set_iterate", i32, vp, vp, vp, vp, vp)
    sig("wc_get_iterate", i32, vp, vp, vp, vp, vp)
    sig("wc_set_ci", i32, vp, vp)
    sig("wc_warm_start", i32, vp, vp, vp, vp, vp, vp, vp, vp)
    sig("wc_unscaled_iterate", i32, vp, vp, vp, vp, vp)
    _lib = L
    return L


class ProbeError(RuntimeError):
    pass


def _check(rc):
    if rc < 0:
        raise ProbeError(lib().wc_last_error().decode())
    return rc


def _f64(a, n):
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    assert a.size == n, (a.size, n)
    return a


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


class WarmProbe:
    """The batched device state on the system behind `system` (an sa.System of batch B)."""

    def __init__(self, system: "sleipnir_amd.System"):
        self.system = system
        self._h = lib().wc_create(system._h)
        if not self._h:
            raise ProbeError(lib().wc_last_error().decode())
        d = np.zeros(7, dtype=np.int64)
        _check(lib().wc_dims(self._h, d.ctypes.data))
        self.B, self.n, self.m_e, self.m_i, self.ns, self.nV, self.off_ci = (int(v) for v in d)

    def close(self):
        if self._h:
            lib().wc_destroy(self._h)
            self._h = None

    def set_scales(self, scales):
        a = _f64(scales, self.B * self.ns)
        _check(lib().wc_set_scales(self._h, a.ctypes.data))

    def set_iterate(self, x, s, y, z):
        B = self.B
        a = [_f64(x, B * self.n), _f64(s, B * self.m_i), _f64(y, B * self.m_e), _f64(z, B * self.m_i)]
        _check(lib().wc_set_iterate(self._h, *(_ptr(v) for v in a)))

    def get_iterate(self):
        B = self.B
        a = [np.zeros((B, k)) for k in (self.n, self.m_i, self.m_e, self.m_i)]
        _check(lib().wc_get_iterate(self._h, *(_ptr(v) for v in a)))
        return a

    def set_ci(self, ci):
        a = _f64(ci, self.B * self.m_i)
        _check(lib().wc_set_ci(self._h, _ptr(a)))

    def warm_start(self, s0, y0, z0, mu0, run, mu_min):
        """-> out [B][3]: first barrier parameter, entries repaired, non-finite input"""
        B = self.B
        blocks = [None if v is None else _f64(v, B * k) for v, k in ((s0, self.m_i), (y0, self.m_e), (z0, self.m_i), (mu0, 1))]
        run = np.ascontiguousarray(run, dtype=np.uint8).reshape(B)
        mu_min = _f64(mu_min, B)
        out = np.zeros((B, 3))
        _check(lib().wc_warm_start(self._h, *(_ptr(v) for v in blocks), run.ctypes.data, mu_min.ctypes.data,
                                   out.ctypes.data))
        return out

    def unscaled_iterate(self, run):
        B = self.B
        run = np.ascontiguousarray(run, dtype=np.uint8).reshape(B)
        a = [np.zeros((B, k)) for k in (self.m_i, self.m_e, self.m_i)]
        _check(lib().wc_unscaled_iterate(self._h, run.ctypes.data, *(_ptr(v) for v in a)))
        return a
