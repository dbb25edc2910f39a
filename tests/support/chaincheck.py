"""The stand-alone program over csrc/chain_ledger.hpp (chaincheck_main.cpp) — TEST INFRASTRUCTURE ONLY.

Built plain and with -fsanitize=address,undefined; it has its own main and is run directly, never loaded into python.
It reads a script of events and prints what the ledger answered, a line per event:

    sweep W   -> "sweep: chained wait_step A this_step B order_by_event E"   (and W workgroups are counted), or
                 "sweep: main order_pending P" / "sweep: restart order_pending P"
    step W    -> "step: chained C wait_step A this_step B"
    touch     -> "touch: order_by_event E"                                    (something is handed the main stream)
    twin, fail, break, save, restore, start HEADROOM [STEP_NUMBER]
              -> "<event>: step_number .. sweep_total .. step_total .. last_step_chained .. pending .. touched .. failures .."
"""
from __future__ import annotations

import subprocess
from pathlib import Path

HERE = Path(__file__).resolve().parent
BIN = HERE / "chaincheck_bin"
BIN_SAN = HERE / "chaincheck_san_bin"
_SOURCES = [HERE / "chaincheck_main.cpp", HERE.parents[1] / "sleipnir_amd" / "csrc" / "chain_ledger.hpp"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"]


def _build_bin(out, extra):
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++23", "--offload-host-only", "-x", "hip", *extra, HERE / "chaincheck_main.cpp", "-o", out]
    res = subprocess.run([str(c) for c in cmd], capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"building {out.name} failed:\n" + res.stdout + res.stderr)


def build():
    _build_bin(BIN, ["-O2"])
    _build_bin(BIN_SAN, SANITIZE)


def binary(sanitized=False) -> Path:
    path = BIN_SAN if sanitized else BIN
    if not path.exists() or any(path.stat().st_mtime < d.stat().st_mtime for d in _SOURCES):
        _build_bin(path, SANITIZE if sanitized else ["-O2"])
    return path


def run(events, sanitized=False):
    """The program's lines for a list of events."""
    res = subprocess.run([str(binary(sanitized))], input="\n".join(events) + "\n", capture_output=True, text=True)
    if res.returncode != 0 or res.stderr.strip():
        raise RuntimeError(f"chaincheck program failed ({res.returncode}):\n{res.stdout}{res.stderr}")
    lines = res.stdout.strip().splitlines()
    assert len(lines) == len(events), (len(lines), len(events))
    return lines
