"""ctypes wrapper over tests/support/libslpx_batchcheck.so — TEST INFRASTRUCTURE ONLY.

A probe of slpx::BatchIpmDevice (batchcheck.cpp): the launch wrappers of the batched interior-point driver from
libslpx.so, driven one method at a time on an `sa.System(problem, B)`, with every per-instance buffer readable and
writable.  Never used by the product.
"""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np

import sleipnir_amd

HERE = Path(__file__).resolve().parent
LIB_PATH = HERE / "libslpx_batchcheck.so"
_CSRC = HERE.parents[1] / "sleipnir_amd" / "csrc"
SOURCES = [HERE / "batchcheck.cpp", HERE / "probe_common.hpp", _CSRC / "ipm_batch.hpp", _CSRC / "batch_lockstep.hpp"]

# the per-instance errors of batch_errors_kernel (batch_lockstep.hpp: BatchErr), in order
ERR_KEYS = ["F", "DUAL_INF", "DUAL_1", "Y1", "Z1", "SZ_MAX", "SZ_MIN", "COMP_1", "CE_INF", "CE_1", "CIS_INF", "CIS_1",
            "DUALU_INF", "YU1", "ZU1", "COMPU_INF", "CEU_INF", "CISU_INF",
            "LOGSUM", "V_BAD", "CI_NONPOS", "AETCE2", "CE2", "AITCM2", "CM2", "X_INF", "X_BAD", "S_INF", "S_BAD"]
ERR = {k: i for i, k in enumerate(ERR_KEYS)}

# bc_get / bc_put selectors (batchcheck.cpp: BatchIpmProbe::buffer)
BUFFERS = ["x", "s", "y", "z", "tx", "ts", "ty", "tz", "sx", "ss", "sy", "sz", "p", "ps", "pz", "Vcur", "tce", "tci",
           "sce", "scims", "out", "sys_V", "sys_rhs", "sys_p", "sys_s", "sys_y", "sys_z", "sys_lhs", "sys_ps", "sys_pz"]


def build():
    sleipnir_amd.build()
    return _build_probe()


def _build_probe():
    # (lib() builds the probe alone: libslpx.so is loaded by then, and relinking it in place would pull the file out
    # from under the process)
    cmd = ["/opt/rocm/bin/hipcc", "-O2", "-std=c++23", "-fPIC", "-shared", "--offload-arch=gfx950",
           "-x", "hip", str(HERE / "batchcheck.cpp"), "-o", str(LIB_PATH),
           "-L" + str(sleipnir_amd.LIB_PATH.parent), "-lslpx",
           "-Wl,-rpath," + str(sleipnir_amd.LIB_PATH.parent)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("building batchcheck failed:\n" + res.stdout + res.stderr)
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
    vp, i32, i64, d = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double

    def sig(name, restype, *argtypes):
        fn = getattr(L, name)
        fn.restype = restype
        fn.argtypes = list(argtypes)

    sig("bc_last_error", ctypes.c_char_p)
    sig("bc_create", vp, vp)
    sig("bc_destroy", None, vp)
    sig("bc_dims", i32, vp, vp)
    sig("bc_set_scales", i32, vp, vp)
    sig("bc_set_iterate", i32, vp, vp, vp, vp, vp)
    sig("bc_set_params", i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp)
    sig("bc_get_s_from_ci", i32, vp, vp)
    sig("bc_assemble", i32, vp)
    sig("bc_reset_regularization", i32, vp, d)
    sig("bc_set_regularization", i32, vp, vp, vp)
    sig("bc_get_regularization", i32, vp, vp, vp)
    sig("bc_compute", i32, vp, i32, vp, vp, vp)
    for name in ("refresh", "newton_direction", "trial_values", "soc_step"):
        sig("bc_" + name, i32, vp, vp)
    sig("bc_kkt_fallback", i32, vp, vp, vp)
    sig("bc_commit", i32, vp)
    sig("bc_get", i64, vp, ctypes.c_int, vp)
    sig("bc_put", i32, vp, ctypes.c_int, vp)
    _lib = L
    return L


class ProbeError(RuntimeError):
    pass


def _check(rc):
    if rc < 0:
        raise ProbeError(lib().bc_last_error().decode())
    return rc


def _f64(a, n):
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    assert a.size == n, (a.size, n)
    return a


def _ptr(a):
    return a.ctypes.data if a.size else None


class BatchProbe:
    """BatchIpmDevice on the system behind `system` (an sa.System of batch B)."""

    def __init__(self, system: "sleipnir_amd.System"):
        self.system = system
        self._h = lib().bc_create(system._h)
        if not self._h:
            raise ProbeError(lib().bc_last_error().decode())
        d = np.zeros(8, dtype=np.int64)
        _check(lib().bc_dims(self._h, d.ctypes.data))
        self.B, self.n, self.m_e, self.m_i, self.dim, self.ns, self.nV, self.nnz_lhs = (int(v) for v in d)

    def close(self):
        if self._h:
            lib().bc_destroy(self._h)
            self._h = None

    def set_scales(self, scales):
        a = _f64(scales, self.B * self.ns)
        _check(lib().bc_set_scales(self._h, a.ctypes.data))

    def set_iterate(self, x, s, y, z):
        B = self.B
        a = [_f64(x, B * self.n), _f64(s, B * self.m_i), _f64(y, B * self.m_e), _f64(z, B * self.m_i)]
        _check(lib().bc_set_iterate(self._h, *(_ptr(v) for v in a)))

    def set_params(self, mu, tau=None, alpha=None, alpha_z=None, alpha_soc=None, mode=None, s_from_ci=None,
                   first=None, active=None):
        B = self.B
        f = lambda v, dflt: _f64(np.full(B, dflt) if v is None else v, B)
        u8 = lambda v, dflt: np.ascontiguousarray(np.full(B, dflt) if v is None else v, dtype=np.uint8).reshape(B)
        self.params = dict(mu=f(mu, 0.0), tau=f(tau, 0.99), alpha=f(alpha, 1.0), alpha_z=f(alpha_z, 1.0),
                           alpha_soc=f(alpha_soc, 1.0),
                           mode=np.ascontiguousarray(np.zeros(B) if mode is None else mode, dtype=np.int32).reshape(B),
                           s_from_ci=u8(s_from_ci, 0), first=u8(first, 0), active=u8(active, 1))
        p = self.params
        _check(lib().bc_set_params(self._h, *(p[k].ctypes.data for k in (
            "mu", "tau", "alpha", "alpha_z", "alpha_soc", "mode", "s_from_ci", "first", "active"))))

    def s_from_ci(self):
        out = np.zeros(self.B, dtype=np.uint8)
        _check(lib().bc_get_s_from_ci(self._h, out.ctypes.data))
        return out

    def assemble(self):
        _check(lib().bc_assemble(self._h))

    def reset_regularization(self, gamma_min=1e-10):
        _check(lib().bc_reset_regularization(self._h, float(gamma_min)))

    def set_regularization(self, delta, gamma):
        d, g = _f64(delta, self.B), _f64(gamma, self.B)
        _check(lib().bc_set_regularization(self._h, d.ctypes.data, g.ctypes.data))

    def regularization(self):
        d, g = np.zeros(self.B), np.zeros(self.B)
        _check(lib().bc_get_regularization(self._h, d.ctypes.data, g.ctypes.data))
        return d, g

    def compute(self, spec=True, mask=None):
        info = np.zeros(self.B, dtype=np.int32)
        nf = np.zeros(1, dtype=np.int32)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8).reshape(self.B)
        _check(lib().bc_compute(self._h, int(spec), None if m is None else m.ctypes.data, info.ctypes.data,
                                nf.ctypes.data))
        return info, int(nf[0])

    def _out(self, name, per):
        out = np.zeros(self.B * per)
        _check(getattr(lib(), "bc_" + name)(self._h, out.ctypes.data))
        return out.reshape(self.B, per)

    def refresh(self):
        return self._out("refresh", len(ERR_KEYS))

    def newton_direction(self):
        return self._out("newton_direction", 3)

    def trial_values(self):
        return self._out("trial_values", 4)

    def soc_step(self):
        return self._out("soc_step", 2)

    def kkt_fallback(self):
        c, t = np.zeros((self.B, len(ERR_KEYS))), np.zeros((self.B, len(ERR_KEYS)))
        _check(lib().bc_kkt_fallback(self._h, c.ctypes.data, t.ctypes.data))
        return c, t

    def commit(self):
        _check(lib().bc_commit(self._h))

    def get(self, name):
        """buffer `name` (BUFFERS) as [B, per-instance length]"""
        which = BUFFERS.index(name)
        count = _check(lib().bc_get(self._h, which, None))
        out = np.zeros(max(count, 1))
        _check(lib().bc_get(self._h, which, out.ctypes.data))
        return out[:count].reshape(self.B, -1)

    def put(self, name, values):
        which = BUFFERS.index(name)
        count = _check(lib().bc_get(self._h, which, None))
        a = _f64(values, count)
        if count:
            _check(lib().bc_put(self._h, which, a.ctypes.data))
