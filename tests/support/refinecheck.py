"""Runs tests/support/refinecheck — TEST INFRASTRUCTURE ONLY.

A stand-alone program (refinecheck.cpp) around the host side of the residual / refinement path: the row map and
the host body of row_residual.  build() makes it twice: plain, and with -fsanitize=address,undefined (host code
only; the program has its own main and is run directly, never loaded into python).
"""
from __future__ import annotations

import struct
import subprocess
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
SRCS = [HERE / "refinecheck.cpp", ROOT / "sleipnir_amd" / "csrc" / "kkt_plan.cpp"]
DEPS = SRCS + [ROOT / "sleipnir_amd" / "csrc" / "kkt_residual.h", ROOT / "sleipnir_amd" / "csrc" / "kkt_plan.hpp"]
BIN = HERE / "refinecheck_bin"
BIN_SAN = HERE / "refinecheck_san_bin"
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"]


def _compile(out: Path, extra):
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++23", "--offload-host-only", "-x", "hip", *extra, *(str(s) for s in SRCS),
           "-o", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("building refinecheck failed:\n" + res.stdout + res.stderr)
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


def _run(mode, payload: bytes, sanitized) -> bytes:
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = Path(tmp) / "in.bin", Path(tmp) / "out.bin"
        src.write_bytes(payload)
        res = subprocess.run([str(binary(sanitized)), mode, str(src), str(dst)], capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"refinecheck {mode} failed ({res.returncode}):\n{res.stdout}{res.stderr}")
        return dst.read_bytes()


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def row_map(colptr, rowidx, sanitized=False):
    """The row map of the lower-CSC pattern (colptr, rowidx) after its diagonal was completed.  Returns a dict:
    colptr, rowidx (the completed pattern), user_map (where each given entry went), rowptr, ent, col."""
    colptr, rowidx = _i32(colptr), _i32(rowidx)
    dim, nnz = len(colptr) - 1, len(rowidx)
    out = np.frombuffer(_run("rowmap", struct.pack("<ii", dim, nnz) + colptr.tobytes() + rowidx.tobytes(), sanitized),
                        dtype=np.int32)
    full_nnz = int(out[0])
    at = 1
    res = {}
    for key, count in (("colptr", dim + 1), ("rowidx", full_nnz), ("user_map", nnz), ("rowptr", dim + 1)):
        res[key] = out[at:at + count].copy()
        at += count
    count = int(out[at])
    at += 1
    res["ent"] = out[at:at + count].copy()
    res["col"] = out[at + count:at + 2 * count].copy()
    assert at + 2 * count == len(out)
    return res


def residual(colptr, rowidx, lhs, rhs, p, n_dec, delta, gamma, sanitized=False):
    """(r, r_plain) of the host body of row_residual / row_residual_plain: lhs over the lower-CSC pattern (every
    diagonal entry present), delta on the first n_dec rows, -gamma on the others."""
    colptr, rowidx = _i32(colptr), _i32(rowidx)
    dim, nnz = len(colptr) - 1, len(rowidx)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64).tobytes()
    payload = struct.pack("<iiiidd", dim, nnz, int(n_dec), 0, float(delta), float(gamma)) + colptr.tobytes() + rowidx.tobytes()
    if (dim + 1 + nnz) % 2:
        payload += b"\0\0\0\0"
    out = np.frombuffer(_run("residual", payload + f(lhs) + f(rhs) + f(p), sanitized), dtype=np.float64)
    assert len(out) == 2 * dim
    return out[:dim].copy(), out[dim:].copy()
