"""ctypes wrapper over tests/support/libslpx_sensadjcheck.so — TEST INFRASTRUCTURE ONLY.

The adjoint part of the sensitivity plan of a model (csrc/sens_plan.hpp): the maps g_src and fp_src, the patterns of the
cost's gradient in the model's and the extended structure, and the host executors of the full vjp on numpy arrays
(sensadjcheck.cpp).  No device is touched.  dense_adjoint() restates the reverse formulas with dense numpy matrices; the
forward side is senscheck.py's.
"""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np

import sleipnir_amd
from tests.support import senscheck

HERE = Path(__file__).resolve().parent
LIB_PATH = HERE / "libslpx_sensadjcheck.so"
_CSRC = HERE.parents[1] / "sleipnir_amd" / "csrc"
SOURCES = [HERE / "sensadjcheck.cpp", _CSRC / "sens_plan.hpp", _CSRC / "sens_rows.h"]
BLOCKS = ("x", "s", "y", "z", "cost")


def build():
    sleipnir_amd.build()
    return _build_probe()


def _build_probe():
    # (host code only; lib() builds the probe alone: libslpx.so is loaded by then)
    cmd = ["/opt/rocm/bin/hipcc", "-O2", "-std=c++23", "-fPIC", "-shared", "--offload-host-only", "-x", "hip",
           str(HERE / "sensadjcheck.cpp"), "-o", str(LIB_PATH), "-L" + str(sleipnir_amd.LIB_PATH.parent), "-lslpx",
           "-Wl,-rpath," + str(sleipnir_amd.LIB_PATH.parent)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("building sensadjcheck failed:\n" + res.stdout + res.stderr)
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

    sig("sa_create", vp, vp)
    sig("sa_destroy", None, vp)
    sig("sa_array", ctypes.c_int64, vp, ctypes.c_char_p, vp)
    sig("sa_scalar", ctypes.c_int32, vp, ctypes.c_char_p, vp)
    sig("sa_adjoint_rhs", None, *([vp] * 10))
    sig("sa_vjp_full", None, *([vp] * 13))
    sig("sa_classify_extras", None, ctypes.c_int32, ctypes.c_int32, vp, vp, vp)
    _lib = L
    return L


def _d(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a if a.size else np.zeros(1)


def _cot(v):
    """v: dict block -> array (missing or None: absent) -> (arrays kept alive, five pointers)"""
    hold = [None if v.get(k) is None else _d(np.atleast_1d(v[k])) for k in BLOCKS]
    return hold, [None if a is None else a.ctypes.data for a in hold]


class SensAdjCheck:
    """The adjoint part of the plan of `problem` (a sleipnir_amd.Problem); `sc`: senscheck.SensCheck of the same problem."""

    def __init__(self, problem, sc):
        self._h = lib().sa_create(problem._h)
        if not self._h:
            raise RuntimeError("sensadjcheck: the plan could not be made")
        self.sc = sc

    def close(self):
        if self._h:
            lib().sa_destroy(self._h)
            self._h = None

    def array(self, name):
        data = ctypes.c_void_p()
        count = lib().sa_array(self._h, name.encode(), ctypes.byref(data))
        if count < 0:
            raise KeyError(name)
        return np.frombuffer(ctypes.string_at(data, 4 * count) if count else b"", dtype=np.int32).copy()

    def scalar(self, name):
        out = ctypes.c_int64()
        if lib().sa_scalar(self._h, name.encode(), ctypes.byref(out)) != 0:
            raise KeyError(name)
        return int(out.value)

    def adjoint_rhs(self, V, s, z, v):
        rhs = np.zeros(self.sc.dim)
        V, s, z = _d(V), _d(s), _d(z)
        hold, ptrs = _cot(v)
        lib().sa_adjoint_rhs(self._h, V.ctypes.data, s.ctypes.data, z.ctypes.data, *ptrs, rhs.ctypes.data)
        return rhs

    def vjp_full(self, Vx, M, R, s, z, w, v):
        grad = np.zeros(self.sc.n_p)
        Vx, M, R, s, z, w = _d(Vx), _d(M), _d(R), _d(s), _d(z), _d(w)
        hold, ptrs = _cot(v)
        lib().sa_vjp_full(self._h, Vx.ctypes.data, M.ctypes.data, R.ctypes.data, s.ctypes.data, z.ctypes.data, w.ctypes.data, *ptrs,
                          grad.ctypes.data)
        return grad

    # the cost's derivatives as dense vectors, from the patterns alone (not from the maps under test)
    def g_dense(self, V):
        cp, off = self.array("model.g.colptr"), self.scalar("model.off_g")
        return np.array([V[off + cp[i]:off + cp[i + 1]].sum() for i in range(self.sc.n)])

    def fp_dense(self, Vx):
        cp, off, n = self.array("ext.g.colptr"), self.scalar("ext.off_g"), self.sc.n
        return np.array([Vx[off + cp[n + q]:off + cp[n + q + 1]].sum() for q in range(self.sc.n_p)])


def classify_extras(B, arrays, widths):
    hold = [None if a is None else _d(a) for a in arrays]
    ptrs = (ctypes.c_void_p * len(hold))(*[None if a is None else a.ctypes.data for a in hold])
    w = np.ascontiguousarray(widths, dtype=np.int32)
    status = np.full(B, -1, dtype=np.int32)
    lib().sa_classify_extras(B, len(hold), ptrs, w.ctypes.data, status.ctypes.data)
    return status


def dense_adjoint(sa, Vx, V, s, z, w, v):
    """dict(rhs, grad): the reverse formulas of sens_plan.hpp on dense matrices; v: dict of the cotangents present."""
    sc = sa.sc
    n, m_e, m_i = sc.n, sc.m_e, sc.m_i
    M = senscheck.unreduced_dense(sc, Vx)
    cp, ri, off = sc.pattern("model.Ai")
    Ai = senscheck.dense(cp, ri, V[off:off + len(ri)], m_i)
    sigma = z / s if m_i else np.zeros(0)
    r_x, r_e, r_i = M[:, :n], M[:, n:n + m_e], M[:, n + m_e:]
    R = np.hstack([-r_x - (r_i * sigma) @ Ai, -r_e])
    get = lambda k, size: np.zeros(size) if v.get(k) is None else np.asarray(v[k], dtype=np.float64).reshape(size)
    vcost = float(get("cost", 1)[0])
    t = get("s", m_i) - sigma * get("z", m_i)
    u = get("x", n) + Ai.T @ t + vcost * sa.g_dense(V)
    rhs = np.concatenate([u, -get("y", m_e)])
    return dict(rhs=rhs, grad=R @ w + r_i @ t + vcost * sa.fp_dense(Vx), R=R, M=M, Ai=Ai, sigma=sigma)
