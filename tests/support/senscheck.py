"""ctypes wrapper over tests/support/libslpx_senscheck.so — TEST INFRASTRUCTURE ONLY.

The sensitivity plan of a model (csrc/sens_plan.hpp) made on the host, its arrays and the patterns of the model's and the
extended structure by name, and the plan's host executor on numpy arrays (senscheck.cpp).  No device is touched.
dense_reference() restates the formulas of sens_plan.hpp with dense numpy matrices: what the CPU test compares with.
"""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np

import sleipnir_amd

HERE = Path(__file__).resolve().parent
LIB_PATH = HERE / "libslpx_senscheck.so"
_CSRC = HERE.parents[1] / "sleipnir_amd" / "csrc"
SOURCES = [HERE / "senscheck.cpp", _CSRC / "sens_plan.hpp", _CSRC / "sens_rows.h"]


def build():
    sleipnir_amd.build()
    return _build_probe()


def _build_probe():
    # (host code only; lib() builds the probe alone: libslpx.so is loaded by then)
    cmd = ["/opt/rocm/bin/hipcc", "-O2", "-std=c++23", "-fPIC", "-shared", "--offload-host-only", "-x", "hip",
           str(HERE / "senscheck.cpp"), "-o", str(LIB_PATH), "-L" + str(sleipnir_amd.LIB_PATH.parent), "-lslpx",
           "-Wl,-rpath," + str(sleipnir_amd.LIB_PATH.parent)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("building senscheck failed:\n" + res.stdout + res.stderr)
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
    vp = ctypes.c_void_p

    def sig(name, restype, *argtypes):
        fn = getattr(L, name)
        fn.restype = restype
        fn.argtypes = list(argtypes)

    sig("sc_create", vp, vp)
    sig("sc_destroy", None, vp)
    sig("sc_array", ctypes.c_int64, vp, ctypes.c_char_p, vp)
    sig("sc_scalar", ctypes.c_int32, vp, ctypes.c_char_p, vp)
    sig("sc_rhs", None, vp, vp, vp, vp, vp, vp, vp)
    sig("sc_combine", None, vp, vp, vp, vp, vp, vp)
    sig("sc_expand", None, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp)
    sig("sc_vjp", None, vp, vp, vp, vp)
    _lib = L
    return L


def _d(a):
    """A contiguous float64 array with at least one entry to point at."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a if a.size else np.zeros(1)


class SensCheck:
    """The plan of `problem` (a sleipnir_amd.Problem)."""

    def __init__(self, problem):
        self._h = lib().sc_create(problem._h)
        if not self._h:
            raise RuntimeError("senscheck: the plan could not be made")
        for k in ("n", "n_p", "m_e", "m_i", "dim", "dimM", "nV", "nVx"):
            setattr(self, k, self.scalar(k))

    def close(self):
        if self._h:
            lib().sc_destroy(self._h)
            self._h = None

    def array(self, name):
        data = ctypes.c_void_p()
        count = lib().sc_array(self._h, name.encode(), ctypes.byref(data))
        if count < 0:
            raise KeyError(name)
        return np.frombuffer(ctypes.string_at(data, 4 * count) if count else b"", dtype=np.int32).copy()

    def scalar(self, name):
        out = ctypes.c_int64()
        if lib().sc_scalar(self._h, name.encode(), ctypes.byref(out)) != 0:
            raise KeyError(name)
        return int(out.value)

    def pattern(self, name):
        """(colptr, rowidx, offset of its values in the value vector) of model.Ai, ext.Ae, ext.Ai, ext.Hf, ext.Hc"""
        return self.array(name + ".colptr"), self.array(name + ".rowidx"), self.scalar(name.replace(".", ".off_"))

    # ---- the host executor ----
    def rhs(self, Vx, V, s, z):
        M, R = np.zeros((self.n_p, self.dimM)), np.zeros((self.n_p, self.dim))
        Vx, V, s, z = _d(Vx), _d(V), _d(s), _d(z)
        lib().sc_rhs(self._h, Vx.ctypes.data, V.ctypes.data, s.ctypes.data, z.ctypes.data, M.ctypes.data, R.ctypes.data)
        return M, R

    def combine(self, M, R, dp):
        rhs, r_i = np.zeros(self.dim), np.zeros(max(1, self.m_i))
        M, R, dp = _d(M), _d(R), _d(dp)
        lib().sc_combine(self._h, M.ctypes.data, R.ctypes.data, dp.ctypes.data, rhs.ctypes.data, r_i.ctypes.data)
        return rhs, r_i[:self.m_i]

    def expand(self, V, s, z, sol, r_i):
        out = [np.zeros(max(1, k)) for k in (self.n, self.m_i, self.m_e, self.m_i)]
        V, s, z, sol, r_i = _d(V), _d(s), _d(z), _d(sol), _d(r_i)
        lib().sc_expand(self._h, V.ctypes.data, s.ctypes.data, z.ctypes.data, sol.ctypes.data, r_i.ctypes.data,
                        *(a.ctypes.data for a in out))
        return tuple(a[:k] for a, k in zip(out, (self.n, self.m_i, self.m_e, self.m_i)))

    def vjp(self, R, w):
        grad = np.zeros(self.n_p)
        R, w = _d(R), _d(w)
        lib().sc_vjp(self._h, R.ctypes.data, w.ctypes.data, grad.ctypes.data)
        return grad


def dense(colptr, rowidx, values, rows):
    """The CSC matrix as a dense array (values: the slice of the value vector behind the pattern)."""
    A = np.zeros((rows, len(colptr) - 1))
    for c in range(len(colptr) - 1):
        for t in range(colptr[c], colptr[c + 1]):
            A[rowidx[t], c] += values[t]
    return A


def unreduced_dense(sc, Vx):
    """M [n_p, n + m_e + m_i] from the extended structure's blocks as dense matrices."""
    n, n_p = sc.n, sc.n_p
    H = np.zeros((n + n_p, n + n_p))
    for name in ("ext.Hf", "ext.Hc"):
        cp, ri, off = sc.pattern(name)
        H += dense(cp, ri, Vx[off:off + len(ri)], n + n_p)
    cp, ri, off = sc.pattern("ext.Ae")
    Ae = dense(cp, ri, Vx[off:off + len(ri)], sc.m_e)
    cp, ri, off = sc.pattern("ext.Ai")
    Ai = dense(cp, ri, Vx[off:off + len(ri)], sc.m_i)
    return np.hstack([H[n:, :n], Ae[:, n:].T, Ai[:, n:].T])


def dense_reference(sc, Vx, V, s, z, dp, sol, w):
    """dict(M, R, rhs, r_i, dx, ds, dy, dz, grad): sens_plan.hpp's formulas on dense matrices."""
    n, m_e = sc.n, sc.m_e
    M = unreduced_dense(sc, Vx)
    cp, ri, off = sc.pattern("model.Ai")
    Ai = dense(cp, ri, V[off:off + len(ri)], sc.m_i)
    sigma = z / s if sc.m_i else np.zeros(0)
    r_x, r_e, r_i = M[:, :n], M[:, n:n + m_e], M[:, n + m_e:]
    R = np.hstack([-r_x - (r_i * sigma) @ Ai, -r_e])
    rhs, ri_c = dp @ R, dp @ r_i
    dx, dy = sol[:n], -sol[n:]
    ds = Ai @ dx + ri_c
    return dict(M=M, R=R, rhs=rhs, r_i=ri_c, dx=dx, ds=ds, dy=dy, dz=-sigma * ds, grad=R @ w)
