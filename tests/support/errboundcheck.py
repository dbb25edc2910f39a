"""Runs tests/support/errboundcheck — TEST INFRASTRUCTURE ONLY.

A stand-alone program (errboundcheck.cpp) around the host side of the error bounds of a solve: the host bodies of
kkt_errbound.h over the row map, and the estimator's state machine.  build() makes it twice: plain, and with
-fsanitize=address,undefined (host code only; the program has its own main and is run directly, never loaded into
python).
"""
from __future__ import annotations

import struct
import subprocess
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
CSRC = ROOT / "sleipnir_amd" / "csrc"
SRCS = [HERE / "errboundcheck.cpp", CSRC / "kkt_plan.cpp"]
DEPS = SRCS + [CSRC / "kkt_errbound.h", CSRC / "kkt_residual.h", CSRC / "kkt_plan.hpp"]
BIN = HERE / "errboundcheck_bin"
BIN_SAN = HERE / "errboundcheck_san_bin"
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"]

# NormEstProbe of kkt_errbound.h
PROBE_NONE, PROBE_UNIFORM, PROBE_UNIT, PROBE_SIGNS, PROBE_ALTERNATING = range(5)


def _compile(out: Path, extra):
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++23", "--offload-host-only", "-x", "hip", *extra, *(str(s) for s in SRCS),
           "-o", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("building errboundcheck failed:\n" + res.stdout + res.stderr)
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


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def rows(colptr, rowidx, lhs, rhs, p, n_dec, delta, gamma, sanitized=False):
    """The host bodies on every row of the system: a dict of r (row_residual), w and sum (row_abs_sum), t (berr_term),
    rho (residual_rounding_bound), each [dim] float64, and terms [dim] int.  lhs over the lower-CSC pattern (every
    diagonal entry present, rows of a column ascending), delta on the first n_dec rows, -gamma on the others."""
    colptr, rowidx = _i32(colptr), _i32(rowidx)
    dim, nnz = len(colptr) - 1, len(rowidx)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64).tobytes()
    payload = struct.pack("<iiiidd", dim, nnz, int(n_dec), 0, float(delta), float(gamma)) + colptr.tobytes() + rowidx.tobytes()
    if (dim + 1 + nnz) % 2:
        payload += b"\0\0\0\0"
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = Path(tmp) / "in.bin", Path(tmp) / "out.bin"
        src.write_bytes(payload + f(lhs) + f(rhs) + f(p))
        res = subprocess.run([str(binary(sanitized)), "rows", str(src), str(dst)], capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"errboundcheck rows failed ({res.returncode}):\n{res.stdout}{res.stderr}")
        out = np.frombuffer(dst.read_bytes(), dtype=np.float64)
    assert len(out) == 6 * dim
    res = {k: out[i * dim:(i + 1) * dim].copy() for i, k in enumerate(("r", "w", "sum", "t", "rho", "terms"))}
    res["terms"] = res["terms"].astype(np.int64)
    return res


def berr_norm1(system_rows):
    """(berr, norm1) as the kernels fold them: the maxima on the bit patterns of the absolute values (a NaN wins)."""
    top = lambda a: np.abs(np.asarray(a, dtype=np.float64)).view(np.uint64).max().view(np.float64)
    return float(top(system_rows["t"])), float(top(system_rows["sum"]))


def sign_vector(v):
    return np.where(np.asarray(v) >= 0.0, 1.0, -1.0)


def probe_vector(kind, j, dim, kept_signs):
    """The probe vector of a command, as est_fill_kernel writes it."""
    i = np.arange(dim, dtype=np.float64)
    if kind == PROBE_UNIFORM:
        return np.full(dim, 1.0 / dim)
    if kind == PROBE_UNIT:
        x = np.zeros(dim)
        x[j] = 1.0
        return x
    if kind == PROBE_SIGNS:
        return kept_signs.copy()
    if kind == PROBE_ALTERNATING:
        return np.where(np.arange(dim) % 2 == 1, -1.0, 1.0) * (1.0 + i / (dim - 1))
    raise ValueError(kind)


def norm_estimate(apply, apply_t, dim, sanitized=False):
    """Drives the product's NormEstState with the operator given as two callables (x -> A x, x -> A^T x) and reduces
    each product the way the device does: ||v||_1 summed in index order, the first index of max |v_i|, sign(v) against
    the kept sign vector, finiteness.  Returns (estimate, solves, probes) with probes = [(kind, j), ...]."""
    proc = subprocess.Popen([str(binary(sanitized)), "normest", str(dim)], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                            stderr=subprocess.PIPE, text=True)
    kept = np.zeros(dim)
    probes = []
    try:
        while True:
            kind, j, transposed, done, solves, est = proc.stdout.readline().split()
            kind, j, done = int(kind), int(j), int(done)
            if done:
                break
            probes.append((kind, j))
            x = probe_vector(kind, j, dim, kept)
            v = np.asarray(apply_t(x) if int(transposed) else apply(x), dtype=np.float64)
            finite = bool(np.all(np.isfinite(v)))
            norm1 = 0.0
            for a in np.abs(v):
                norm1 += float(a)
            argmax = int(np.argmax(np.abs(v))) if finite else 0  # (numpy: the first of equal maxima)
            s = sign_vector(v)
            proc.stdin.write(f"{float(norm1).hex()} {argmax} {int(np.array_equal(s, kept))} {int(finite)}\n")
            proc.stdin.flush()
            if proc.stdout.readline().split() == ["adopt", "1"]:
                kept = s
        proc.stdin.close()
        rc = proc.wait(timeout=30)
        err = proc.stderr.read()
    finally:
        if proc.poll() is None:
            proc.kill()
        for stream in (proc.stdin, proc.stdout, proc.stderr):
            if stream and not stream.closed:
                stream.close()
    if rc != 0:
        raise RuntimeError(f"errboundcheck normest failed ({rc}):\n{err}")
    return float.fromhex(est), int(solves), probes
