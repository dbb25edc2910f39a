"""Runs tests/support/warmcheck_host — TEST INFRASTRUCTURE ONLY.

A stand-alone program (warmcheck_host.cpp) around the host instantiation of the warm-start formulas
(sleipnir_amd/csrc/warm_start.h).  build() makes it twice: plain, and with -fsanitize=address,undefined (host code
only; the program has its own main and is run directly, never loaded into python).

reference(): the same formulas restated in numpy, one IEEE operation at a time — what the CPU test compares the
program with, and what the GPU tests compare the kernels with.
"""
from __future__ import annotations

import struct
import subprocess
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
SRCS = [HERE / "warmcheck_host.cpp"]
DEPS = SRCS + [ROOT / "sleipnir_amd" / "csrc" / "warm_start.h", ROOT / "sleipnir_amd" / "csrc" / "ipm_formulas.h"]
BIN = HERE / "warmcheck_host_bin"
BIN_SAN = HERE / "warmcheck_host_san_bin"
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"]
COLUMNS_IN = ("v_u", "d_c", "d_f", "mu_given", "sum", "count", "mu_min", "given_s", "s", "c_i", "given_z", "z")
COLUMNS_OUT = ("scale_s", "unscale_s", "scale_dual", "unscale_dual", "scale_mu", "unscale_mu", "bad", "counts", "mu",
               "slack", "slack_repaired", "dual", "dual_repaired")
KAPPA = 1e10


def _compile(out: Path, extra):
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++23", "--offload-host-only", "-x", "hip", *extra, *(str(s) for s in SRCS),
           "-o", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("building warmcheck_host failed:\n" + res.stdout + res.stderr)
    return out


def build():
    _compile(BIN, ["-O2"])
    _compile(BIN_SAN, SANITIZE)
    return BIN


def binary(sanitized=False) -> Path:
    path = BIN_SAN if sanitized else BIN
    if not path.exists() or any(path.stat().st_mtime < d.stat().st_mtime for d in DEPS):
        _compile(path, SANITIZE if sanitized else ["-O2"])
    return path


def evaluate(table, sanitized=False):
    """table: [rows][12] doubles in the order of COLUMNS_IN.  Returns [rows][13], the host results in the order of
    COLUMNS_OUT."""
    table = np.ascontiguousarray(table, dtype=np.float64).reshape(-1, len(COLUMNS_IN))
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = Path(tmp) / "in.bin", Path(tmp) / "out.bin"
        src.write_bytes(struct.pack("<ii", len(table), 0) + table.tobytes())
        res = subprocess.run([str(binary(sanitized)), str(src), str(dst)], capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"warmcheck_host failed ({res.returncode}):\n{res.stdout}{res.stderr}")
        out = np.frombuffer(dst.read_bytes(), dtype=np.float64)
    assert len(out) == len(table) * len(COLUMNS_OUT)
    return out.reshape(len(table), len(COLUMNS_OUT)).copy()


# ---- the numpy restatement (scalars or arrays; every line one IEEE operation per entry) ----

def _f(v):
    return np.asarray(v, dtype=np.float64)


def scale_s(s_u, d_ci):
    return _f(d_ci) * _f(s_u)


def unscale_s(s, d_ci):
    return _f(s) / _f(d_ci)


def scale_dual(v_u, d_c, d_f):
    q = _f(d_c) / _f(d_f)
    return _f(v_u) / q


def unscale_dual(v, d_c, d_f):
    q = _f(d_c) / _f(d_f)
    return _f(v) * q


def z_reset(z, mu, s):
    """ipm_formulas.h: z_reset, entry by entry."""
    with np.errstate(all="ignore"):
        lo = np.float64(1.0) / np.float64(KAPPA) * mu / s
        hi = np.float64(KAPPA) * mu / s
        return np.where(z < lo, lo, np.where(z > hi, hi, z))


def choose_mu(total, count, mu_given, d_f, mu_min):
    if mu_given > 0.0:
        return max(np.float64(d_f) * np.float64(mu_given), np.float64(mu_min))
    cold = np.float64(0.1) * np.float64(d_f)
    if not count > 0.0:
        return cold
    with np.errstate(all="ignore"):
        mu = np.float64(total) / np.float64(count)
    mu = mu if mu < cold else cold
    return mu if mu > mu_min else np.float64(mu_min)


def slack(given, s, c_i, mu):
    """-> (values, replaced mask)"""
    s, c_i = np.asarray(s, dtype=np.float64), np.asarray(c_i, dtype=np.float64)
    keep = np.logical_and(given, s > 0.0)
    return np.where(keep, s, np.where(c_i > mu, c_i, mu)), ~keep


def dual(given, z, mu, s):
    """-> (values, repaired mask); s: the slacks after slack()"""
    z, s = np.asarray(z, dtype=np.float64), np.asarray(s, dtype=np.float64)
    keep = np.logical_and(given, z > 0.0)
    with np.errstate(all="ignore"):
        z0 = np.where(keep, z, mu / s)
    z1 = z_reset(z0, mu, s)
    return z1, np.logical_or(~keep, z1 != z0)


def instance(scales, m_e, c_i_unit, x, s_u, y_u, z_u, mu_given, mu_min, mu=None):
    """The safeguarded first iterate of one instance (warm_start.h) from the user's-units blocks (None: absent).
    Returns dict(bad, mu, s, y, z, repaired, sum, count).  `mu`: the barrier parameter to repair with in place of this
    function's own — the device's, whose mean is summed in another order (sum and count are numpy's either way)."""
    scales = np.asarray(scales, dtype=np.float64)
    m_i = len(scales) - 1 - m_e
    d_f, d_ce, d_ci = scales[0], scales[1:1 + m_e], scales[1 + m_e:]
    given = [np.asarray(v, dtype=np.float64) for v in (x, s_u, y_u, z_u) if v is not None]
    bad = any(not np.all(np.isfinite(v)) for v in given) or not np.isfinite(mu_given)
    if bad:
        return dict(bad=True)
    total, count = 0.0, 0.0
    if s_u is not None and z_u is not None and m_i:
        s, z = scale_s(s_u, d_ci), scale_dual(z_u, d_ci, d_f)
        rows = np.logical_and(s > 0.0, z > 0.0)
        total, count = float(np.sum((s * z)[rows], dtype=np.longdouble)), float(np.sum(rows))
    mu_own = choose_mu(total, count, mu_given, d_f, mu_min)
    mu = mu_own if mu is None else np.float64(mu)
    y = scale_dual(y_u, d_ce, d_f) if y_u is not None else np.zeros(m_e)
    c_i = d_ci * np.asarray(c_i_unit, dtype=np.float64)
    s, rep_s = slack(s_u is not None, scale_s(s_u, d_ci) if s_u is not None else np.zeros(m_i), c_i, mu)
    z, rep_z = dual(z_u is not None, scale_dual(z_u, d_ci, d_f) if z_u is not None else np.zeros(m_i), mu, s)
    return dict(bad=False, mu=mu_own, s=s, y=y, z=z, repaired=int(np.sum(rep_s) + np.sum(rep_z)), sum=total, count=count)
