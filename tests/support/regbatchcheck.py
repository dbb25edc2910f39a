"""ctypes wrapper over tests/support/libslpx_regbatchcheck.so — TEST INFRASTRUCTURE ONLY.

ldlt_run_batch (csrc/ldlt_policy.hpp) with per-problem extra pivots under scripted inertia counters (regbatchcheck.cpp), the
script format of hostcheck.reg_policy.  Needs no device.
"""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np

import sleipnir_amd

HERE = Path(__file__).resolve().parent
LIB_PATH = HERE / "libslpx_regbatchcheck.so"
SOURCES = [HERE / "regbatchcheck.cpp", HERE.parents[1] / "sleipnir_amd" / "csrc" / "ldlt_policy.hpp"]


def build():
    cmd = ["/opt/rocm/bin/hipcc", "-O2", "-std=c++23", "-fPIC", "-shared", "--offload-arch=gfx950",
           "-x", "hip", str(HERE / "regbatchcheck.cpp"), "-o", str(LIB_PATH)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("building regbatchcheck failed:\n" + res.stdout + res.stderr)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists() or any(LIB_PATH.stat().st_mtime < p.stat().st_mtime for p in SOURCES):
        build()
    L = ctypes.CDLL(str(LIB_PATH))
    vp, i32, d = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double
    L.rb_reg_policy_batch.restype = i32
    L.rb_reg_policy_batch.argtypes = [i32, i32, i32, d, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp]
    _lib = L
    return L


def reg_policy_batch(n, m_e, problems, gamma_min=1e-10, skip_first=False, launch_for_nobody=False, extra=None, mask=None):
    """One pass of ldlt_run_batch over `problems` = [((prev_delta, prev_gamma), response), ...] (hostcheck.reg_policy's
    format); extra: the smallest eliminated pivot per problem, or None.  Returns a dict: attempts (per problem, the
    (delta, gamma) judged in order), launch_of (per problem, the launch each attempt was part of), info and memory per
    problem, launches."""
    B = len(problems)
    fa = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    mem = fa([m for m, _ in problems]).reshape(B, 2).copy()
    table = fa([row for _, resp in problems for row in resp]).reshape(-1, 8)
    table_ptr = np.ascontiguousarray(np.cumsum([0] + [len(resp) for _, resp in problems]), dtype=np.int32)
    msk = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    ext = None if extra is None else fa(extra)
    cap = 4096
    attempts = np.zeros((cap, 4))
    info, counts = np.zeros(B, dtype=np.int32), np.zeros(1, dtype=np.int32)
    rows = lib().rb_reg_policy_batch(n, m_e, B, float(gamma_min), int(skip_first), int(launch_for_nobody), mem.ctypes.data,
                                     None if msk is None else msk.ctypes.data, None if ext is None else ext.ctypes.data,
                                     table.ctypes.data, table_ptr.ctypes.data, attempts.ctypes.data, cap, info.ctypes.data,
                                     counts.ctypes.data)
    if rows < 0:
        raise RuntimeError({-1: "reg_policy_batch: an attempt no row of the response answers",
                            -2: "reg_policy_batch: the loop does not end"}[rows])
    att = attempts[:rows]
    return {"attempts": [[(r[1], r[2]) for r in att if int(r[0]) == b] for b in range(B)],
            "launch_of": [[int(r[3]) for r in att if int(r[0]) == b] for b in range(B)],
            "info": [int(v) for v in info], "memory": [tuple(m) for m in mem], "launches": int(counts[0])}
