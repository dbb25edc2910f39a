"""Runs tests/support/formulacheck — TEST INFRASTRUCTURE ONLY.

A stand-alone program (formulacheck.cpp) around the host instantiation of the interior-point row formulas
(sleipnir_amd/csrc/ipm_formulas.h).  build() makes it twice: plain, and with -fsanitize=address,undefined (host code
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
SRCS = [HERE / "formulacheck.cpp"]
DEPS = SRCS + [ROOT / "sleipnir_amd" / "csrc" / "ipm_formulas.h"]
BIN = HERE / "formulacheck_bin"
BIN_SAN = HERE / "formulacheck_san_bin"
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"]
COLUMNS_IN = ("acc", "tau", "p", "v", "z", "mu", "s", "c", "p_s", "alpha", "prev", "trial")
COLUMNS_OUT = ("ftb_candidate", "z_reset", "soc_rhs_multiplier", "backsub_pz_sinv", "soc_accumulate")


def _compile(out: Path, extra):
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++23", "--offload-host-only", "-x", "hip", *extra, *(str(s) for s in SRCS),
           "-o", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("building formulacheck failed:\n" + res.stdout + res.stderr)
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
    """table: [rows][12] doubles in the order of COLUMNS_IN.  Returns [rows][5], the host results in the order of
    COLUMNS_OUT (backsub_pz_sinv is given 1 / s)."""
    table = np.ascontiguousarray(table, dtype=np.float64).reshape(-1, len(COLUMNS_IN))
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = Path(tmp) / "in.bin", Path(tmp) / "out.bin"
        src.write_bytes(struct.pack("<ii", len(table), 0) + table.tobytes())
        res = subprocess.run([str(binary(sanitized)), str(src), str(dst)], capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"formulacheck failed ({res.returncode}):\n{res.stdout}{res.stderr}")
        out = np.frombuffer(dst.read_bytes(), dtype=np.float64)
    assert len(out) == len(table) * len(COLUMNS_OUT)
    return out.reshape(len(table), len(COLUMNS_OUT)).copy()
