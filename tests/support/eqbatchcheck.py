"""ctypes wrapper over tests/support/libslpx_eqbatchcheck.so — TEST INFRASTRUCTURE ONLY.

A probe of slpx::BatchEqDevice (eqbatchcheck.cpp): the launch wrappers of the batched SQP / Newton drivers from
libslpx.so, driven one method at a time on an `sa.System(problem, B)`, with every per-instance buffer readable and
writable.  Never used by the product.
"""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np

import sleipnir_amd
from tests.support.batchcheck import ERR, ERR_KEYS  # noqa: F401  (the layout of batch_errors_kernel's output)

HERE = Path(__file__).resolve().parent
LIB_PATH = HERE / "libslpx_eqbatchcheck.so"
_CSRC = HERE.parents[1] / "sleipnir_amd" / "csrc"
SOURCES = [HERE / "eqbatchcheck.cpp", HERE / "probe_common.hpp", _CSRC / "eq_batch.hpp", _CSRC / "batch_lockstep.hpp"]

# ebc_get / ebc_put selectors (eqbatchcheck.cpp: BatchEqProbe::buffer)
BUFFERS = ["x", "y", "tx", "ty", "px", "py", "sx", "sy", "Vcur", "tce", "sce", "out", "sys_V", "sys_rhs", "sys_p",
           "sys_y", "sys_in"]


def build():
    sleipnir_amd.build()
    return _build_probe()


def _build_probe():
    # (lib() builds the probe alone: libslpx.so is loaded by then)
    cmd = ["/opt/rocm/bin/hipcc", "-O2", "-std=c++23", "-fPIC", "-shared", "--offload-arch=gfx950",
           "-x", "hip", str(HERE / "eqbatchcheck.cpp"), "-o", str(LIB_PATH),
           "-L" + str(sleipnir_amd.LIB_PATH.parent), "-lslpx",
           "-Wl,-rpath," + str(sleipnir_amd.LIB_PATH.parent)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("building eqbatchcheck failed:\n" + res.stdout + res.stderr)
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
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64

    def sig(name, restype, *argtypes):
        fn = getattr(L, name)
        fn.restype = restype
        fn.argtypes = list(argtypes)

    sig("ebc_last_error", ctypes.c_char_p)
    sig("ebc_create", vp, vp)
    sig("ebc_destroy", None, vp)
    sig("ebc_dims", i32, vp, vp)
    sig("ebc_set_scales", i32, vp, vp)
    sig("ebc_set_iterate", i32, vp, vp, vp)
    sig("ebc_set_params", i32, vp, vp, vp, vp, vp, vp)
    sig("ebc_newton_step", i32, vp, vp)
    for name in ("refresh", "direction", "trial_values"):
        sig("ebc_" + name, i32, vp, vp)
    sig("ebc_soc_step", i32, vp)
    sig("ebc_kkt_fallback", i32, vp, vp, vp)
    sig("ebc_commit", i32, vp)
    sig("ebc_get", i64, vp, ctypes.c_int, vp)
    sig("ebc_put", i32, vp, ctypes.c_int, vp)
    _lib = L
    return L


class ProbeError(RuntimeError):
    pass


def _check(rc):
    if rc < 0:
        raise ProbeError(lib().ebc_last_error().decode())
    return rc


def _f64(a, n):
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    assert a.size == n, (a.size, n)
    return a


class EqBatchProbe:
    """BatchEqDevice on the system behind `system` (an sa.System of batch B, no inequality rows)."""

    def __init__(self, system: "sleipnir_amd.System"):
        self.system = system
        self._h = lib().ebc_create(system._h)
        if not self._h:
            raise ProbeError(lib().ebc_last_error().decode())
        d = np.zeros(7, dtype=np.int64)
        _check(lib().ebc_dims(self._h, d.ctypes.data))
        self.B, self.n, self.m_e, self.dim, self.ns, self.nV, self.n_inputs = (int(v) for v in d)

    def close(self):
        if self._h:
            lib().ebc_destroy(self._h)
            self._h = None

    def set_scales(self, scales):
        a = _f64(scales, self.B * self.ns)
        _check(lib().ebc_set_scales(self._h, a.ctypes.data))

    def set_iterate(self, x, y):
        a, b = _f64(x, self.B * self.n), _f64(y, self.B * self.m_e)
        _check(lib().ebc_set_iterate(self._h, a.ctypes.data, b.ctypes.data if b.size else None))

    def set_params(self, alpha=None, alpha_soc=None, mode=None, first=None, active=None):
        B = self.B
        f = lambda v, dflt: _f64(np.full(B, dflt) if v is None else v, B)
        u8 = lambda v, dflt: np.ascontiguousarray(np.full(B, dflt) if v is None else v, dtype=np.uint8).reshape(B)
        p = dict(alpha=f(alpha, 1.0), alpha_soc=f(alpha_soc, 1.0),
                 mode=np.ascontiguousarray(np.zeros(B) if mode is None else mode, dtype=np.int32).reshape(B),
                 first=u8(first, 0), active=u8(active, 1))
        self.params = p
        _check(lib().ebc_set_params(self._h, *(p[k].ctypes.data for k in ("alpha", "alpha_soc", "mode", "first", "active"))))

    def newton_step(self):
        info = np.zeros(self.B, dtype=np.int32)
        _check(lib().ebc_newton_step(self._h, info.ctypes.data))
        return info

    def _out(self, name, per):
        out = np.zeros(self.B * per)
        _check(getattr(lib(), "ebc_" + name)(self._h, out.ctypes.data))
        return out.reshape(self.B, per)

    def refresh(self):
        return self._out("refresh", len(ERR_KEYS))

    def direction(self):
        return self._out("direction", 1)[:, 0]

    def trial_values(self):
        return self._out("trial_values", 3)

    def soc_step(self):
        _check(lib().ebc_soc_step(self._h))

    def kkt_fallback(self):
        c, t = np.zeros((self.B, len(ERR_KEYS))), np.zeros((self.B, len(ERR_KEYS)))
        _check(lib().ebc_kkt_fallback(self._h, c.ctypes.data, t.ctypes.data))
        return c, t

    def commit(self):
        _check(lib().ebc_commit(self._h))

    def get(self, name):
        """buffer `name` (BUFFERS) as [B, per-instance length]"""
        which = BUFFERS.index(name)
        count = _check(lib().ebc_get(self._h, which, None))
        out = np.zeros(max(count, 1))
        _check(lib().ebc_get(self._h, which, out.ctypes.data))
        return out[:count].reshape(self.B, -1)

    def put(self, name, values):
        which = BUFFERS.index(name)
        count = _check(lib().ebc_get(self._h, which, None))
        a = _f64(values, count)
        if count:
            _check(lib().ebc_put(self._h, which, a.ctypes.data))
