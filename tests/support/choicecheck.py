"""ctypes wrapper over tests/support/libslpx_choicecheck.so, and the stand-alone program beside it — TEST
INFRASTRUCTURE ONLY.

csrc/switches.hpp and csrc/system_choice.hpp as dictionaries: the switches the environment gives, the options and the
plan route of a system, the launch modes from numbers handed in (choicecheck.cpp, choicecheck_modes.h).  The program
(choicecheck_main.cpp: the launch modes only) is built plain and with -fsanitize=address,undefined; it has its own main
and is run directly, never loaded into python.
"""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np

import sleipnir_amd

HERE = Path(__file__).resolve().parent
LIB_PATH = HERE / "libslpx_choicecheck.so"
BIN = HERE / "choicecheck_bin"
BIN_SAN = HERE / "choicecheck_san_bin"
_CSRC = HERE.parents[1] / "sleipnir_amd" / "csrc"
_CHOICE = [_CSRC / "switches.cpp", _CSRC / "system_choice.cpp"]
_HEADERS = [HERE / "choicecheck_modes.h", _CSRC / "switches.hpp", _CSRC / "system_choice.hpp", _CSRC / "ldlt_symbolic.hpp"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"]

SWITCHES = ["fuse_launches", "fuse_kkt", "fuse_backsub", "ldlt_mf", "ldlt_il", "chain_tape", "ipm_resident", "ipm_lookahead",
            "ipm_pipeline", "twin", "ipm_ride", "mf_solve", "fuse_kkt_store", "il_min_batch", "dense", "task_entries", "single_launch",
            "mf_threads", "relax_zeros", "sn_min_width", "mfma_min_entries"]
OPTIONS = ["task_entries", "supernodal", "multifrontal", "min_supernode_width", "relax_zeros", "balance_supernode_cuts",
           "chain_from_deepest_child", "chain_from_deepest_min_round", "single_problem_task_rules", "mfma_min_entries"]
MODES_IN = ["batch", "dense", "dense_pivoted", "tasks", "factor_lds_bytes", "mf", "mf_n_mfma", "one_reader", "n_sums", "cus", "kkt_ok",
            "backsub_ok", "mf_declined", "mf_lds", "static_lds", "step_1024", "step_512", "solve_1024", "solve_512", "ask_twin",
            "twin_1024", "twin_512", "ask_ride", "riding"]
MODES_OUT = ["dense", "dense_pivoted", "il", "single_launch", "fuse_launches", "fuse_kkt", "fuse_backsub", "fuse_kkt_store", "fuse_solve",
             "slot_handoff", "xg_by_data", "mf", "mf_solve", "mf_mfma", "mf_threads", "twin_threads", "chain_mode", "chain_on", "twin",
             "ride"]


def _run(cmd, what):
    res = subprocess.run([str(c) for c in cmd], capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"building {what} failed:\n" + res.stdout + res.stderr)


def _build_lib():
    _run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++23", "-fPIC", "-shared", "--offload-arch=gfx950", "-x", "hip", HERE / "choicecheck.cpp",
          "-o", LIB_PATH, "-L" + str(sleipnir_amd.LIB_PATH.parent), "-lslpx", "-Wl,-rpath," + str(sleipnir_amd.LIB_PATH.parent)],
         "choicecheck")


def _build_bin(out, extra):
    _run(["/opt/rocm/bin/hipcc", "-std=c++23", "--offload-host-only", "-x", "hip", *extra, HERE / "choicecheck_main.cpp", *_CHOICE,
          "-o", out], out.name)


def build():
    sleipnir_amd.build()
    _build_lib()
    _build_bin(BIN, ["-O2"])
    _build_bin(BIN_SAN, SANITIZE)
    return LIB_PATH


def _stale(path, deps):
    return not path.exists() or any(path.stat().st_mtime < d.stat().st_mtime for d in deps)


def binary(sanitized=False) -> Path:
    path = BIN_SAN if sanitized else BIN
    if _stale(path, [HERE / "choicecheck_main.cpp", *_CHOICE, *_HEADERS]):
        _build_bin(path, SANITIZE if sanitized else ["-O2"])
    return path


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    sleipnir_amd.lib()
    if _stale(LIB_PATH, [HERE / "choicecheck.cpp", *_HEADERS, sleipnir_amd.LIB_PATH]):
        _build_lib()
    L = ctypes.CDLL(str(LIB_PATH))
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    for name, restype, argtypes in (("cc_switches", None, [vp]), ("cc_interleaved", i32, [i32]), ("cc_options", None, [i32, i32, i32, i32, vp]),
                                    ("cc_dense_bound", i32, [i32, i32, ctypes.c_char_p, i32]),
                                    ("cc_plan", i32, [vp, vp, vp, i32, i32, vp, ctypes.c_char_p, i32]), ("cc_modes", None, [vp, vp])):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def switches():
    """Switches::from_environment() now: {member: value}, None for an optional that is empty."""
    out = np.zeros(2 * len(SWITCHES), dtype=np.int64)
    lib().cc_switches(out.ctypes.data)
    return {k: (int(out[2 * i + 1]) if out[2 * i] else None) for i, k in enumerate(SWITCHES)}


def interleaved_for(batch):
    return bool(lib().cc_interleaved(batch))


def options(batch, dim, compiled_model=True, base_task_entries=0):
    """(choose_ldlt_options of default options, pair_list_options of the result), each {field: value}."""
    out = np.zeros(2 * len(OPTIONS), dtype=np.int64)
    lib().cc_options(batch, dim, int(compiled_model), base_task_entries, out.ctypes.data)
    return tuple({k: int(v) for k, v in zip(OPTIONS, half)} for half in (out[:len(OPTIONS)], out[len(OPTIONS):]))


def dense_bound_error(batch, dim):
    """None where the dense factors of `batch` systems of order `dim` are within the bound, else the error's text."""
    msg = ctypes.create_string_buffer(512)
    return msg.value.decode() if lib().cc_dense_bound(batch, dim, msg, 512) else None


def plan(hc, perm=None, batch=1):
    """The plan of the product's route for the model of `hc` (a hostcheck.HostCheck): {dense, dense_pivoted, mf,
    mf_asked}; raises what the route throws."""
    s, k, _ = hc.plans()
    p = None if perm is None else np.ascontiguousarray(perm, dtype=np.int32)
    out = np.zeros(4, dtype=np.int64)
    msg = ctypes.create_string_buffer(512)
    if lib().cc_plan(s, k, None if p is None else p.ctypes.data, 0 if p is None else len(p), batch, out.ctypes.data, msg, 512) != 0:
        raise RuntimeError(msg.value.decode())
    return dict(zip(("dense", "dense_pivoted", "mf", "mf_asked"), (bool(v) for v in out)))


def _row(inputs):
    unknown = set(inputs) - set(MODES_IN)
    assert not unknown, unknown
    return [int(inputs.get(k, 0)) for k in MODES_IN]


def modes(**inputs):
    """LaunchModes after the stages DeviceNlp runs, from MODES_IN (what is not given is 0): {mode: value}."""
    row = np.array(_row(inputs), dtype=np.int64)
    out = np.zeros(len(MODES_OUT), dtype=np.int64)
    lib().cc_modes(row.ctypes.data, out.ctypes.data)
    return {k: int(v) for k, v in zip(MODES_OUT, out)}


def modes_by_program(rows, sanitized=False):
    """The same for a list of input dictionaries, by the stand-alone program."""
    text = "\n".join(" ".join(str(v) for v in _row(r)) for r in rows) + "\n"
    res = subprocess.run([str(binary(sanitized))], input=text, capture_output=True, text=True)
    if res.returncode != 0 or res.stderr.strip():
        raise RuntimeError(f"choicecheck program failed ({res.returncode}):\n{res.stdout}{res.stderr}")
    lines = res.stdout.strip().splitlines()
    assert len(lines) == len(rows)
    return [{k: int(v) for k, v in zip(MODES_OUT, line.split())} for line in lines]
