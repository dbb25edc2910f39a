"""sleipnir_amd — MI355X-native interior-point Newton step behind Sleipnir's
``slp::Problem`` surface.

The product is the C++/HIP library ``libslpx.so`` (sources in ``csrc/``, C-ABI in
``include/slpx.h``).  This Python package is plumbing only: it builds the library
in-tree and exposes the C-ABI through ctypes so that ``tests/`` and ``bench.py``
can drive it.  It never computes anything itself and has no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from pathlib import Path

import numpy as np

_PKG = Path(__file__).resolve().parent
_ROOT = _PKG.parent
# (SLPX_LIB: another build of the library, e.g. for an A/B on one box)
LIB_PATH = Path(os.environ["SLPX_LIB"]).resolve() if os.environ.get("SLPX_LIB") else _PKG / "libslpx.so"

ABI_VERSION = 6  # include/slpx.h: SLPX_ABI_VERSION (struct layouts and entry points below)

c_i32p = ctypes.POINTER(ctypes.c_int32)
c_i64p = ctypes.POINTER(ctypes.c_int64)
c_f64p = ctypes.POINTER(ctypes.c_double)

# include/slpx.h: SLPX_INFO_*
INFO_KEYS = [
    "n", "m_e", "m_i", "nV", "nnz_g", "nnz_Ae", "nnz_Ai", "nnz_Hf", "nnz_Hc", "nnz_lhs", "nnz_L",
    "ldlt_rounds", "ldlt_tasks", "etree_height", "ldlt_pairs", "tape_tasks", "tape_nodes",
    "tape_slots", "tape_edges", "tape_levels", "tape_slot_levels", "assemble_bytes", "rhs_bytes",
    "factor_bytes", "solve_bytes", "sweep_bytes", "struct_singular", "off_g", "off_Ae", "off_Ai",
    "off_Hf", "off_Hc", "graph_nodes", "nonlinear_rows", "tape_global_tasks", "tape_shared_tasks",
    "tape_program_bytes", "ldlt_levels", "ldlt_supernodes", "ldlt_widest_supernode",
    "ldlt_multifrontal", "ldlt_fronts", "ldlt_mfma_fronts", "ldlt_dense",
]

# slpx_op
OPS = {name: i for i, name in enumerate([
    "CONST", "VAR", "ADD", "SUB", "NEG", "MUL", "DIV", "POW", "ABS", "SIGN", "SQRT", "CBRT", "EXP",
    "LOG", "LOG10", "SIN", "COS", "TAN", "ASIN", "ACOS", "ATAN", "ATAN2", "SINH", "COSH", "TANH",
    "ERF", "HYPOT", "MAX", "MIN", "ISNONNEG", "ISPOS"])}


class Options(ctypes.Structure):
    _fields_ = [("tolerance", ctypes.c_double), ("max_iterations", ctypes.c_int32),
                ("timeout", ctypes.c_double), ("feasible_ipm", ctypes.c_int32),
                ("diagnostics", ctypes.c_int32), ("spy", ctypes.c_int32)]


class Report(ctypes.Structure):
    _fields_ = [("iterations", ctypes.c_int32), ("factorizations", ctypes.c_int32),
                ("solves", ctypes.c_int32), ("value_sweeps", ctypes.c_int32),
                ("delta", ctypes.c_double), ("gamma", ctypes.c_double),
                ("final_error", ctypes.c_double), ("t_setup", ctypes.c_double),
                ("t_kkt_build", ctypes.c_double), ("t_kkt_decomp", ctypes.c_double),
                ("t_kkt_solve", ctypes.c_double), ("t_line_search", ctypes.c_double),
                ("t_ad_refresh", ctypes.c_double), ("t_total", ctypes.c_double),
                ("t_compile", ctypes.c_double), ("restorations", ctypes.c_int32),
                ("restoration_iterations", ctypes.c_int32), ("t_restoration_setup", ctypes.c_double),
                ("t_restoration", ctypes.c_double)]


class WarmStart(ctypes.Structure):
    """slpx_warm_start: s, y, z in the user's units (NULL: absent), mu (<= 0: choose)."""
    _fields_ = [("s", ctypes.c_void_p), ("y", ctypes.c_void_p), ("z", ctypes.c_void_p), ("mu", ctypes.c_double)]


class Cotangent(ctypes.Structure):
    """slpx_cotangent: cotangents on x, s, y, z and on the optimal cost (NULL: absent)."""
    _fields_ = [("vx", ctypes.c_void_p), ("vs", ctypes.c_void_p), ("vy", ctypes.c_void_p), ("vz", ctypes.c_void_p),
                ("vcost", ctypes.c_void_p)]


class SensitivityInfo(ctypes.Structure):
    """slpx_sensitivity_info: what one sensitivity call did (include/slpx.h: solution sensitivities)."""
    _fields_ = [("n_p", ctypes.c_int32), ("solves", ctypes.c_int32), ("factorizations", ctypes.c_int32),
                ("refine_steps", ctypes.c_int32), ("n_pos", ctypes.c_int32), ("n_neg", ctypes.c_int32),
                ("n_zero", ctypes.c_int32), ("delta", ctypes.c_double), ("gamma", ctypes.c_double),
                ("berr_max", ctypes.c_double), ("solve_status", ctypes.c_int32), ("t_compile", ctypes.c_double),
                ("t_factor", ctypes.c_double), ("t_total", ctypes.c_double)]


def build(force: bool = False, verbose: bool = False) -> Path:
    """Compile libslpx.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    # (at most 16 jobs: a shared build host may count far more CPUs than one build may use)
    cmd = ["make", "-C", str(_PKG / "csrc"), "-j", str(min(16, os.cpu_count() or 4))]
    if force:
        subprocess.run(cmd + ["clean"], check=True, capture_output=not verbose)
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("building libslpx.so failed:\n" + res.stdout[-4000:] + res.stderr[-4000:])
    return LIB_PATH


_lib = None


def lib() -> ctypes.CDLL:
    """Load libslpx.so (building it first if missing) and declare the C-ABI."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        build()
    L = ctypes.CDLL(str(LIB_PATH))
    vp, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double

    def sig(name, restype, *argtypes):
        fn = getattr(L, name)
        fn.restype = restype
        fn.argtypes = list(argtypes)

    sig("slpx_abi_version", ctypes.c_int)
    if L.slpx_abi_version() != ABI_VERSION:
        raise SlpxError(f"{LIB_PATH} has ABI version {L.slpx_abi_version()}, this binding was written for {ABI_VERSION}")
    sig("slpx_last_error", ctypes.c_char_p)
    sig("slpx_device_count", ctypes.c_int)
    sig("slpx_shard_range", ctypes.c_int, i64, i32, i32, c_i64p, c_i64p)
    sig("slpx_graph_reset", None)
    sig("slpx_graph_size", i64)
    sig("slpx_expr_variable", i32, f64)
    sig("slpx_expr_constant", i32, f64)
    sig("slpx_expr_unary", i32, ctypes.c_int, i32)
    sig("slpx_expr_binary", i32, ctypes.c_int, i32, i32)
    sig("slpx_expr_type", ctypes.c_int, i32)
    sig("slpx_expr_value", f64, i32)
    sig("slpx_expr_set_value", None, i32, f64)
    sig("slpx_expr_gradient_tree", None, i32, vp, i32, vp)
    sig("slpx_problem_create", vp)
    sig("slpx_problem_destroy", None, vp)
    sig("slpx_problem_decision_variable", i32, vp)
    sig("slpx_problem_minimize", None, vp, i32)
    sig("slpx_problem_maximize", None, vp, i32)
    sig("slpx_problem_subject_to_eq", None, vp, i32)
    sig("slpx_problem_subject_to_ineq", None, vp, i32)
    sig("slpx_problem_cost_type", ctypes.c_int, vp)
    sig("slpx_problem_eq_type", ctypes.c_int, vp)
    sig("slpx_problem_ineq_type", ctypes.c_int, vp)
    sig("slpx_problem_dims", None, vp, c_i32p, c_i32p, c_i32p)
    sig("slpx_problem_get_x", None, vp, vp)
    sig("slpx_problem_set_x", None, vp, vp)
    sig("slpx_problem_solve", ctypes.c_int, vp, ctypes.POINTER(Options), ctypes.POINTER(Report))
    sig("slpx_problem_solve_sized", ctypes.c_int, vp, ctypes.POINTER(Options), ctypes.c_uint32, ctypes.POINTER(Report))
    sig("slpx_problem_get_duals", None, vp, vp, vp, vp)
    sig("slpx_problem_restoration_steps", ctypes.c_int, vp, ctypes.POINTER(Options), vp, vp, vp, vp, f64, i32)
    sig("slpx_problem_prebuild_kernels", ctypes.c_int, vp, ctypes.c_char_p)
    sig("slpx_system_create", vp, vp, i32, i32, vp, i32)
    sig("slpx_system_destroy", None, vp)
    sig("slpx_system_set_stream", ctypes.c_int, vp, vp)
    sig("slpx_system_sync", ctypes.c_int, vp)
    sig("slpx_system_info", ctypes.c_int, vp, vp)
    sig("slpx_system_pattern", i32, vp, ctypes.c_int, vp, vp)
    sig("slpx_system_perm", ctypes.c_int, vp, vp)
    sig("slpx_system_set_scaling", ctypes.c_int, vp, vp)
    sig("slpx_system_set_state", ctypes.c_int, vp, vp, vp, vp, vp, vp)
    sig("slpx_tape_sweep", ctypes.c_int, vp, ctypes.c_int)
    sig("slpx_kkt_assemble", ctypes.c_int, vp)
    sig("slpx_kkt_rhs", ctypes.c_int, vp)
    sig("slpx_ldlt_factor", ctypes.c_int, vp, vp, vp, vp)
    sig("slpx_ldlt_compute", ctypes.c_int, vp, vp, vp, vp)
    sig("slpx_ldlt_reset", ctypes.c_int, vp, f64)
    sig("slpx_ldlt_solve", ctypes.c_int, vp)
    sig("slpx_step_backsub", ctypes.c_int, vp)
    sig("slpx_newton_step", ctypes.c_int, vp, ctypes.c_int, vp)
    sig("slpx_system_get", i64, vp, ctypes.c_int, vp)
    sig("slpx_system_set_rhs", ctypes.c_int, vp, vp)
    sig("slpx_system_set_lhs", ctypes.c_int, vp, vp)
    sig("slpx_system_time_step", ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, vp)
    sig("slpx_debug_chain", ctypes.c_int, vp, ctypes.c_int)
    sig("slpx_system_time_fused_step", ctypes.c_int, vp, ctypes.c_int, vp)
    sig("slpx_newton_steps", ctypes.c_int, vp, i32, ctypes.c_int, ctypes.c_int, vp)
    sig("slpx_system_regularization", ctypes.c_int, vp, vp)
    sig("slpx_problem_add_callback", ctypes.c_int, vp, vp, vp)
    sig("slpx_problem_clear_callbacks", ctypes.c_int, vp)
    sig("slpx_problem_system", vp, vp)
    sig("slpx_ldlt_create", vp, i32, i32, vp, vp, i32, i32)
    sig("slpx_ldlt_set_matrix", ctypes.c_int, vp, vp)
    sig("slpx_ipm_direction", ctypes.c_int, vp, f64, vp)
    sig("slpx_ipm_trial", ctypes.c_int, vp, f64, ctypes.c_int, vp)
    sig("slpx_ipm_commit", ctypes.c_int, vp, f64, f64, ctypes.c_int)
    sig("slpx_ipm_errors", ctypes.c_int, vp, vp, vp)
    # an addition within ABI version 6, bound where the library has it
    if hasattr(L, "slpx_problem_solve_batch"):
        sig("slpx_problem_solve_batch", ctypes.c_int, vp, i32, vp, ctypes.POINTER(Options), ctypes.c_uint32, vp, vp, vp,
            vp, vp, vp, vp, vp, ctypes.POINTER(Report))
    if hasattr(L, "slpx_problem_batch_stats"):
        sig("slpx_problem_batch_stats", ctypes.c_int, vp, vp)
    if hasattr(L, "slpx_problem_set_batch_restoration"):
        sig("slpx_problem_set_batch_restoration", ctypes.c_int, vp, ctypes.c_int)
        sig("slpx_problem_batch_restoration_stats", ctypes.c_int, vp, vp)
        sig("slpx_problem_restoration_steps_batch", ctypes.c_int, vp, ctypes.POINTER(Options), ctypes.c_uint32, i32, vp, vp,
            vp, vp, vp, i32, vp)
    if hasattr(L, "slpx_ldlt_residual"):
        sig("slpx_ldlt_residual", ctypes.c_int, vp, vp, vp)
        sig("slpx_ldlt_refine", ctypes.c_int, vp, i32, vp, vp)
        sig("slpx_ldlt_residual_masked", ctypes.c_int, vp, vp, vp, vp)
        sig("slpx_ldlt_refine_masked", ctypes.c_int, vp, i32, vp, vp, vp)
    if hasattr(L, "slpx_ldlt_error_bounds"):
        sig("slpx_ldlt_error_bounds", ctypes.c_int, vp, vp, vp, vp, vp)
        sig("slpx_ldlt_condest", ctypes.c_int, vp, vp, vp, vp, vp)
    if hasattr(L, "slpx_problem_set_parameters"):
        sig("slpx_problem_parameters", i32, vp, vp, i32)
        sig("slpx_problem_parameter_slots_in_order", ctypes.c_int, vp)
        sig("slpx_problem_set_parameters", ctypes.c_int, vp, vp)
        sig("slpx_problem_compile_count", i64, vp)
        sig("slpx_problem_solve_batch_parameters", ctypes.c_int, vp, i32, vp, vp, ctypes.POINTER(Options), ctypes.c_uint32,
            vp, vp, vp, vp, vp, vp, vp, vp, ctypes.POINTER(Report))
        sig("slpx_system_set_parameters", ctypes.c_int, vp, vp, ctypes.c_int)
        sig("slpx_system_parameter_pool_bytes", i64, vp)
    if hasattr(L, "slpx_problem_solve_warm"):
        sig("slpx_problem_solve_warm", ctypes.c_int, vp, ctypes.POINTER(Options), ctypes.c_uint32, ctypes.POINTER(WarmStart),
            ctypes.POINTER(Report))
        sig("slpx_problem_get_iterate", ctypes.c_int, vp, vp, vp, vp, vp, vp)
        sig("slpx_problem_warm_start_repaired", i32, vp)
        sig("slpx_problem_solve_batch_warm", ctypes.c_int, vp, i32, vp, vp, vp, vp, vp, vp, ctypes.POINTER(Options),
            ctypes.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ctypes.POINTER(Report))
    if hasattr(L, "slpx_problem_sensitivity"):
        sig("slpx_problem_sensitivity", ctypes.c_int, vp, vp, vp, vp, vp, ctypes.POINTER(SensitivityInfo))
        sig("slpx_problem_sensitivity_jvp", ctypes.c_int, vp, vp, vp, vp, vp, vp, ctypes.POINTER(SensitivityInfo))
        sig("slpx_problem_sensitivity_vjp", ctypes.c_int, vp, vp, vp, ctypes.POINTER(SensitivityInfo))
        sig("slpx_problem_sensitivity_rhs", ctypes.c_int, vp, vp)
    if hasattr(L, "slpx_problem_sensitivity_vjp_full"):
        sig("slpx_problem_sensitivity_vjp_full", ctypes.c_int, vp, ctypes.POINTER(Cotangent), ctypes.c_uint32, vp,
            ctypes.POINTER(SensitivityInfo))
        sig("slpx_problem_sensitivity_batch_vjp_full", ctypes.c_int, vp, i32, vp, vp, vp, vp, vp, vp, ctypes.POINTER(Cotangent),
            ctypes.c_uint32, vp, vp, vp)
    if hasattr(L, "slpx_problem_sensitivity_batch"):
        rows = (vp, i32, vp, vp, vp, vp, vp, vp)  # problem, B, x, s, y, z, mu, params
        sig("slpx_problem_sensitivity_batch", ctypes.c_int, *rows, vp, vp, vp, vp, vp, vp)
        sig("slpx_problem_sensitivity_batch_jvp", ctypes.c_int, *rows, vp, vp, vp, vp, vp, vp, vp)
        sig("slpx_problem_sensitivity_batch_vjp", ctypes.c_int, *rows, vp, vp, vp, vp)
        sig("slpx_problem_sensitivity_batch_rhs", ctypes.c_int, *rows, vp, vp)
    _lib = L
    return L


def _ptr(a):
    return None if a is None else a.ctypes.data


def _f64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


class SlpxError(RuntimeError):
    pass


def _check(rc):
    if rc < 0:
        raise SlpxError(lib().slpx_last_error().decode())
    return rc


class IterationInfo(ctypes.Structure):
    _fields_ = [("iteration", ctypes.c_int32), ("n", ctypes.c_int32), ("m_e", ctypes.c_int32),
                ("m_i", ctypes.c_int32)] + [(k, ctypes.POINTER(ctypes.c_double)) for k in "xsyzV"] + [
                    ("off", ctypes.c_int64 * 8), ("in_restoration", ctypes.c_int32)]


IterationCallback = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.POINTER(IterationInfo), ctypes.c_void_p)


class Problem:
    """Handle on an slp::Problem living in libslpx (include/slpx.h, slpx_problem_*)."""

    def __init__(self, handle=None):
        self._h = handle if handle is not None else lib().slpx_problem_create()
        if not self._h:
            raise SlpxError(lib().slpx_last_error().decode())

    def close(self):
        if self._h:
            lib().slpx_problem_destroy(self._h)
            self._h = None

    @property
    def dims(self):
        n, me, mi = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        lib().slpx_problem_dims(self._h, ctypes.byref(n), ctypes.byref(me), ctypes.byref(mi))
        return n.value, me.value, mi.value

    def decision_variable(self) -> int:
        return lib().slpx_problem_decision_variable(self._h)

    def minimize(self, expr_id: int):
        lib().slpx_problem_minimize(self._h, expr_id)

    def maximize(self, expr_id: int):
        lib().slpx_problem_maximize(self._h, expr_id)

    def subject_to_eq(self, expr_id: int):
        lib().slpx_problem_subject_to_eq(self._h, expr_id)

    def subject_to_ineq(self, expr_id: int):
        lib().slpx_problem_subject_to_ineq(self._h, expr_id)

    def types(self):
        L = lib()
        return (L.slpx_problem_cost_type(self._h), L.slpx_problem_eq_type(self._h),
                L.slpx_problem_ineq_type(self._h))

    def get_x(self) -> np.ndarray:
        x = np.zeros(self.dims[0])
        lib().slpx_problem_get_x(self._h, x.ctypes.data)
        return x

    def set_x(self, x):
        x = _f64(x)
        lib().slpx_problem_set_x(self._h, x.ctypes.data)

    def solve(self, tolerance=1e-8, max_iterations=5000, timeout=0.0, feasible_ipm=False,
              diagnostics=False, spy=False, warm_start=None):
        """warm_start: None, or a dict with any of s, y, z (arrays in the user's units) and mu — the rest of the iterate
        the solve begins at, x being the variables' values (slpx_problem_solve_warm; include/slpx.h: warm starts)."""
        opt = Options(tolerance, max_iterations, timeout, int(feasible_ipm), int(diagnostics), int(spy))
        rep = Report()
        if warm_start is None:
            status = lib().slpx_problem_solve_sized(self._h, ctypes.byref(opt), ctypes.sizeof(Options), ctypes.byref(rep))
        else:
            L = lib()
            if not hasattr(L, "slpx_problem_solve_warm"):
                raise SlpxError(f"{LIB_PATH} has no slpx_problem_solve_warm")
            n, me, mi = self.dims
            hold = {}
            for k, count in (("s", mi), ("y", me), ("z", mi)):
                v = warm_start.get(k)
                if v is not None:
                    v = np.ascontiguousarray(np.asarray(v, dtype=np.float64).ravel())
                    if v.shape[0] != count:
                        raise ValueError(f"warm_start: {k} must have {count} entries")
                    hold[k] = v
            mu = warm_start.get("mu")
            ws = WarmStart(*(hold[k].ctypes.data if k in hold and hold[k].size else None for k in ("s", "y", "z")),
                           0.0 if mu is None else float(mu))
            status = L.slpx_problem_solve_warm(self._h, ctypes.byref(opt), ctypes.sizeof(Options), ctypes.byref(ws),
                                               ctypes.byref(rep))
        if status == -100:
            raise SlpxError(lib().slpx_last_error().decode())
        return status, {f[0]: getattr(rep, f[0]) for f in Report._fields_}

    def iterate(self):
        """(x, s, y, z, mu) the last solve ended at, in the user's units (slpx_problem_get_iterate)."""
        L = lib()
        if not hasattr(L, "slpx_problem_get_iterate"):
            raise SlpxError(f"{LIB_PATH} has no slpx_problem_get_iterate")
        n, me, mi = self.dims
        x, s, y, z = np.zeros(n), np.zeros(mi), np.zeros(me), np.zeros(mi)
        mu = ctypes.c_double()
        if L.slpx_problem_get_iterate(self._h, *(a.ctypes.data if a.size else None for a in (x, s, y, z)),
                                      ctypes.addressof(mu)) != 0:
            raise SlpxError(L.slpx_last_error().decode())
        return x, s, y, z, mu.value

    def warm_start_repaired(self) -> int:
        """Entries of its warm start the last solve's safeguard replaced or clamped (slpx_problem_warm_start_repaired)."""
        return int(lib().slpx_problem_warm_start_repaired(self._h))

    # ---- solution sensitivities (include/slpx.h): everything in the user's units, rows in the order of parameters() ----
    def _sensitivity_entry(self, name):
        L = lib()
        if not hasattr(L, name):
            raise SlpxError(f"{LIB_PATH} has no {name}")
        return getattr(L, name)

    @staticmethod
    def _sensitivity_info(info):
        return {f[0]: getattr(info, f[0]) for f in SensitivityInfo._fields_}

    def sensitivity(self):
        """The Jacobian of the last solve's end iterate with respect to the parameters (slpx_problem_sensitivity):
        dict(dx (n_p, n), ds (n_p, m_i), dy (n_p, m_e), dz (n_p, m_i), info)."""
        fn = self._sensitivity_entry("slpx_problem_sensitivity")
        n, me, mi = self.dims
        # (the sizes come first, so an error of the call itself — no solve yet, no parameters — is the library's)
        n_p = max(0, lib().slpx_problem_parameters(self._h, None, 0))
        out = {"dx": np.zeros((n_p, n)), "ds": np.zeros((n_p, mi)), "dy": np.zeros((n_p, me)), "dz": np.zeros((n_p, mi))}
        info = SensitivityInfo()
        if fn(self._h, *(out[k].ctypes.data if out[k].size else None for k in ("dx", "ds", "dy", "dz")), ctypes.byref(info)) != 0:
            raise SlpxError(lib().slpx_last_error().decode())
        out["info"] = self._sensitivity_info(info)
        return out

    def sensitivity_jvp(self, dp):
        """The directional derivative of the end iterate along dp (n_p) (slpx_problem_sensitivity_jvp):
        dict(dx (n), ds (m_i), dy (m_e), dz (m_i), info).  iterate() + these is a warm start for parameters + dp."""
        fn = self._sensitivity_entry("slpx_problem_sensitivity_jvp")
        n, me, mi = self.dims
        n_p = max(0, lib().slpx_problem_parameters(self._h, None, 0))
        dp = np.ascontiguousarray(np.asarray(dp, dtype=np.float64).ravel())
        if n_p and dp.shape[0] != n_p:
            raise SlpxError(f"sensitivity_jvp: dp must have {n_p} entries, one per parameter")
        out = {"dx": np.zeros(n), "ds": np.zeros(mi), "dy": np.zeros(me), "dz": np.zeros(mi)}
        info = SensitivityInfo()
        hold = dp if dp.size else np.zeros(1)
        if fn(self._h, hold.ctypes.data, *(out[k].ctypes.data if out[k].size else None for k in ("dx", "ds", "dy", "dz")),
              ctypes.byref(info)) != 0:
            raise SlpxError(lib().slpx_last_error().decode())
        out["info"] = self._sensitivity_info(info)
        return out

    def sensitivity_vjp(self, vx):
        """(dx/dp)^T vx (n_p) for a cotangent vx (n) on x, from one solve (slpx_problem_sensitivity_vjp): (grad, info)."""
        fn = self._sensitivity_entry("slpx_problem_sensitivity_vjp")
        n = self.dims[0]
        n_p = max(0, lib().slpx_problem_parameters(self._h, None, 0))
        vx = np.ascontiguousarray(np.asarray(vx, dtype=np.float64).ravel())
        if vx.shape[0] != n:
            raise SlpxError(f"sensitivity_vjp: vx must have {n} entries, one per decision variable")
        grad = np.zeros(max(1, n_p))
        info = SensitivityInfo()
        if fn(self._h, vx.ctypes.data if vx.size else None, grad.ctypes.data, ctypes.byref(info)) != 0:
            raise SlpxError(lib().slpx_last_error().decode())
        return grad[:n_p], self._sensitivity_info(info)

    @staticmethod
    def _cotangent(who, shapes, x, s, y, z, cost):
        """(slpx_cotangent, the arrays it points into): `shapes` the shape of each of x, s, y, z, cost; None is absent, and
        so is a cotangent on rows the model does not have."""
        c, hold = Cotangent(), []
        for field, name, v in (("vx", "x", x), ("vs", "s", s), ("vy", "y", y), ("vz", "z", z), ("vcost", "cost", cost)):
            if v is None:
                continue
            a = np.ascontiguousarray(np.asarray(v, dtype=np.float64))
            want = shapes[name]
            if a.size != int(np.prod(want)):
                raise SlpxError(f"{who}: the cotangent on {name} must have shape {tuple(want)}")
            # (an empty one still counts as given: the library ignores it, and says "no cotangent" only when all are None)
            hold.append(a if a.size else np.zeros(1))
            setattr(c, field, hold[-1].ctypes.data)
        return c, hold

    def sensitivity_vjp_full(self, x=None, s=None, y=None, z=None, cost=None):
        """The vjp for cotangents on the whole end iterate and on the optimal cost — x (n), s (m_i), y (m_e), z (m_i),
        cost (a number), None: absent — from ONE solve (slpx_problem_sensitivity_vjp_full): (grad (n_p), info)."""
        fn = self._sensitivity_entry("slpx_problem_sensitivity_vjp_full")
        n, me, mi = self.dims
        n_p = max(0, lib().slpx_problem_parameters(self._h, None, 0))
        c, hold = self._cotangent("sensitivity_vjp_full", {"x": (n,), "s": (mi,), "y": (me,), "z": (mi,), "cost": (1,)}, x, s, y, z, cost)
        grad = np.zeros(max(1, n_p))
        info = SensitivityInfo()
        if fn(self._h, ctypes.byref(c), ctypes.sizeof(c), grad.ctypes.data, ctypes.byref(info)) != 0:
            raise SlpxError(lib().slpx_last_error().decode())
        return grad[:n_p], self._sensitivity_info(info)

    def sensitivity_rhs(self):
        """M (n_p, n + m_e + m_i): per parameter r_x = d(grad_x L)/dp, r_e = dc_e/dp, r_i = dc_i/dp at the end iterate
        (slpx_problem_sensitivity_rhs)."""
        fn = self._sensitivity_entry("slpx_problem_sensitivity_rhs")
        n_p = max(0, lib().slpx_problem_parameters(self._h, None, 0))
        M = np.zeros((n_p, sum(self.dims)))
        if fn(self._h, M.ctypes.data if M.size else None) != 0:
            raise SlpxError(lib().slpx_last_error().decode())
        return M

    # ---- batched sensitivities (include/slpx.h): functions of the rows they are given, not of the problem's state ----
    def _batch_rows(self, iterate, parameters, who):
        """(B, n_p, [x, s, y, z, mu, params] as contiguous arrays, their pointers): `iterate` is anything with x, s, y, z,
        mu rows — the dict solve_batch(..., warm_start={}) returns as it is, or an object with those attributes."""
        get = iterate.get if hasattr(iterate, "get") else lambda k: getattr(iterate, k, None)
        n, me, mi = self.dims
        n_p = max(0, lib().slpx_problem_parameters(self._h, None, 0))
        x = get("x")
        if x is None:
            raise ValueError(f"{who}: the iterate has no x")
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
        if x.ndim != 2 or x.shape[1] != n:
            raise ValueError(f"{who}: x must have shape (B, {n})")
        B = x.shape[0]
        hold = [x]
        for k, count in (("s", mi), ("y", me), ("z", mi), ("mu", 1)):
            v = get(k)
            if v is None:
                if count:
                    raise ValueError(f"{who}: the iterate has no {k}")
                v = np.zeros((B, 0))
            v = np.asarray(v, dtype=np.float64)
            if v.size != B * count or (v.ndim == 2 and v.shape != (B, count)):
                raise ValueError(f"{who}: {k} must have shape ({B}, {count})")
            hold.append(np.ascontiguousarray(v.reshape(B, count)))
        rows = np.ascontiguousarray(np.asarray(parameters, dtype=np.float64))
        if rows.ndim != 2 or rows.shape != (B, n_p):
            raise ValueError(f"{who}: parameters must have shape ({B}, {n_p}): one row per instance")
        hold.append(rows)
        return B, n_p, hold, [a.ctypes.data if a.size else None for a in hold]

    def _batch_info(self, info):
        return [self._sensitivity_info(i) for i in info]

    def sensitivity_batch(self, iterate, parameters):
        """The Jacobians of B end iterates with respect to their parameter rows (slpx_problem_sensitivity_batch):
        dict(dx (B, n_p, n), ds (B, n_p, m_i), dy (B, n_p, m_e), dz (B, n_p, m_i), status (B), info: list of B dicts).
        status: 0 computed, 1 skipped (not finite, or s <= 0), 2 not factored; rows of the latter two are NaN."""
        fn = self._sensitivity_entry("slpx_problem_sensitivity_batch")
        B, n_p, hold, ptrs = self._batch_rows(iterate, parameters, "sensitivity_batch")
        n, me, mi = self.dims
        out = {"dx": np.zeros((B, n_p, n)), "ds": np.zeros((B, n_p, mi)), "dy": np.zeros((B, n_p, me)), "dz": np.zeros((B, n_p, mi)),
               "status": np.zeros(B, dtype=np.int32)}
        info = (SensitivityInfo * max(1, B))()
        if fn(self._h, B, *ptrs, *(out[k].ctypes.data if out[k].size else None for k in ("dx", "ds", "dy", "dz", "status")), info) != 0:
            raise SlpxError(lib().slpx_last_error().decode())
        out["info"] = self._batch_info(info[:B])
        return out

    def sensitivity_batch_jvp(self, iterate, parameters, dp):
        """Along dp (B, n_p), one round of solves (slpx_problem_sensitivity_batch_jvp): dict(dx (B, n), ds (B, m_i),
        dy (B, m_e), dz (B, m_i), status, info).  iterate + these is the warm start of the batch with parameters + dp."""
        fn = self._sensitivity_entry("slpx_problem_sensitivity_batch_jvp")
        B, n_p, hold, ptrs = self._batch_rows(iterate, parameters, "sensitivity_batch_jvp")
        dp = np.ascontiguousarray(np.asarray(dp, dtype=np.float64))
        if dp.shape != (B, n_p):
            raise ValueError(f"sensitivity_batch_jvp: dp must have shape ({B}, {n_p})")
        n, me, mi = self.dims
        out = {"dx": np.zeros((B, n)), "ds": np.zeros((B, mi)), "dy": np.zeros((B, me)), "dz": np.zeros((B, mi)),
               "status": np.zeros(B, dtype=np.int32)}
        info = (SensitivityInfo * max(1, B))()
        if fn(self._h, B, *ptrs, dp.ctypes.data if dp.size else None,
              *(out[k].ctypes.data if out[k].size else None for k in ("dx", "ds", "dy", "dz", "status")), info) != 0:
            raise SlpxError(lib().slpx_last_error().decode())
        out["info"] = self._batch_info(info[:B])
        return out

    def sensitivity_batch_vjp(self, iterate, parameters, vx):
        """(dx/dp)^T vx per instance for cotangents vx (B, n), one round of solves (slpx_problem_sensitivity_batch_vjp):
        dict(grad (B, n_p), status, info)."""
        fn = self._sensitivity_entry("slpx_problem_sensitivity_batch_vjp")
        B, n_p, hold, ptrs = self._batch_rows(iterate, parameters, "sensitivity_batch_vjp")
        vx = np.ascontiguousarray(np.asarray(vx, dtype=np.float64))
        if vx.shape != (B, self.dims[0]):
            raise ValueError(f"sensitivity_batch_vjp: vx must have shape ({B}, {self.dims[0]})")
        out = {"grad": np.zeros((B, n_p)), "status": np.zeros(B, dtype=np.int32)}
        info = (SensitivityInfo * max(1, B))()
        if fn(self._h, B, *ptrs, vx.ctypes.data if vx.size else None, out["grad"].ctypes.data if out["grad"].size else None,
              out["status"].ctypes.data if B else None, info) != 0:
            raise SlpxError(lib().slpx_last_error().decode())
        out["info"] = self._batch_info(info[:B])
        return out

    def sensitivity_batch_vjp_full(self, iterate, parameters, x=None, s=None, y=None, z=None, cost=None):
        """The full vjp per instance for cotangent rows x (B, n), s (B, m_i), y (B, m_e), z (B, m_i), cost (B), None:
        absent, one round of solves (slpx_problem_sensitivity_batch_vjp_full): dict(grad (B, n_p), status, info)."""
        fn = self._sensitivity_entry("slpx_problem_sensitivity_batch_vjp_full")
        B, n_p, hold, ptrs = self._batch_rows(iterate, parameters, "sensitivity_batch_vjp_full")
        n, me, mi = self.dims
        c, hold_c = self._cotangent("sensitivity_batch_vjp_full",
                                    {"x": (B, n), "s": (B, mi), "y": (B, me), "z": (B, mi), "cost": (B,)}, x, s, y, z, cost)
        out = {"grad": np.zeros((B, n_p)), "status": np.zeros(B, dtype=np.int32)}
        info = (SensitivityInfo * max(1, B))()
        if fn(self._h, B, *ptrs, ctypes.byref(c), ctypes.sizeof(c), out["grad"].ctypes.data if out["grad"].size else None,
              out["status"].ctypes.data if B else None, info) != 0:
            raise SlpxError(lib().slpx_last_error().decode())
        out["info"] = self._batch_info(info[:B])
        return out

    def sensitivity_batch_rhs(self, iterate, parameters):
        """M (B, n_p, n + m_e + m_i): per instance and parameter r_x, r_e, r_i at its iterate; neither factors nor solves
        (slpx_problem_sensitivity_batch_rhs): dict(M, status)."""
        fn = self._sensitivity_entry("slpx_problem_sensitivity_batch_rhs")
        B, n_p, hold, ptrs = self._batch_rows(iterate, parameters, "sensitivity_batch_rhs")
        out = {"M": np.zeros((B, n_p, sum(self.dims))), "status": np.zeros(B, dtype=np.int32)}
        if fn(self._h, B, *ptrs, out["M"].ctypes.data if out["M"].size else None, out["status"].ctypes.data if B else None) != 0:
            raise SlpxError(lib().slpx_last_error().decode())
        return out

    RESTORATION_MODES = {"handoff": 0, "lockstep": 1}

    def solve_batch(self, x0, tolerance=1e-8, max_iterations=5000, timeout=0.0, feasible_ipm=False, restoration="handoff",
                    parameters=None, warm_start=None):
        """B instances from the rows of x0 (B x n), each as solve() from that start
        (slpx_problem_solve_batch).  Returns a dict of arrays: status, x, s, y, z, cost, iterations,
        restorations, the batch's report, and how the batch ran (slpx_problem_batch_stats): rounds (lockstep
        Newton-step computations), handoffs (instances handed to the batch-1 system for restoration) and
        driver (0 none needed, 1 interior point, 2 SQP, 3 Newton).
        restoration: "handoff" (the default: an instance that asks for feasibility restoration runs it on the batch-1
        system while the batch waits) or "lockstep" (all instances that ask in one round run one restoration phase
        together on the batch system; slpx_problem_set_batch_restoration).  "restoration_lockstep" in the result is
        slpx_problem_batch_restoration_stats: instances restored in lockstep, phases, lockstep restoration rounds,
        instances that used the batch-1 system for the KKT-error fallback.
        parameters: None, or (B x n_p) — instance b is the problem with parameter row b, the order of parameters()
        (slpx_problem_solve_batch_parameters).
        warm_start: None, or a dict with any of s (B x m_i), y (B x m_e), z (B x m_i), mu (B) in the user's units, possibly
        empty: instance b begins there (slpx_problem_solve_batch_warm), and s, y, z of the result are in the user's units
        too, with "mu" (B) and "repaired" (B) added."""
        L = lib()
        if warm_start is not None and not hasattr(L, "slpx_problem_solve_batch_warm"):
            raise SlpxError(f"{LIB_PATH} has no slpx_problem_solve_batch_warm")
        if parameters is not None and not hasattr(L, "slpx_problem_solve_batch_parameters"):
            raise SlpxError(f"{LIB_PATH} has no slpx_problem_solve_batch_parameters")
        if not hasattr(L, "slpx_problem_solve_batch"):
            raise SlpxError(f"{LIB_PATH} has no slpx_problem_solve_batch")
        if restoration not in self.RESTORATION_MODES:
            raise ValueError('restoration: "handoff" or "lockstep"')
        if hasattr(L, "slpx_problem_set_batch_restoration"):
            if L.slpx_problem_set_batch_restoration(self._h, self.RESTORATION_MODES[restoration]) != 0:
                raise SlpxError(L.slpx_last_error().decode())
        elif restoration != "handoff":
            raise SlpxError(f"{LIB_PATH} has no slpx_problem_set_batch_restoration")
        n, me, mi = self.dims
        x0 = np.ascontiguousarray(np.asarray(x0, dtype=np.float64).reshape(-1, n) if n else
                                  np.zeros((len(x0), 0)))
        B = x0.shape[0]
        out = {"status": np.zeros(B, dtype=np.int32), "x": np.zeros((B, n)), "s": np.zeros((B, mi)),
               "y": np.zeros((B, me)), "z": np.zeros((B, mi)), "cost": np.zeros(B),
               "iterations": np.zeros(B, dtype=np.int32), "restorations": np.zeros(B, dtype=np.int32)}
        opt = Options(tolerance, max_iterations, timeout, int(feasible_ipm), 0, 0)
        rep = Report()
        outputs = [out[k].ctypes.data for k in ("status", "x", "s", "y", "z", "cost", "iterations", "restorations")]
        rows = None
        if parameters is not None:
            rows = np.ascontiguousarray(np.asarray(parameters, dtype=np.float64))
            if rows.ndim != 2 or rows.shape[0] != B:
                raise ValueError(f"parameters must have shape ({B}, n_p): one row per instance")
            n_p = len(self.parameters())
            if rows.shape[1] != n_p:
                raise ValueError(f"parameters must have {n_p} columns, the model's parameters")
        if warm_start is not None:
            hold = {}
            for k, count in (("s", mi), ("y", me), ("z", mi), ("mu", 1)):
                v = warm_start.get(k)
                if v is not None:
                    v = np.asarray(v, dtype=np.float64)
                    if v.size != B * count:
                        raise ValueError(f"warm_start: {k} must have shape ({B}, {count})")
                    v = np.ascontiguousarray(v.reshape(B, count))
                    hold[k] = v
            out["mu"] = np.zeros(B)
            out["repaired"] = np.zeros(B, dtype=np.int32)
            rc = L.slpx_problem_solve_batch_warm(
                self._h, B, x0.ctypes.data if B else None, rows.ctypes.data if rows is not None and rows.size else None,
                *(hold[k].ctypes.data if k in hold and hold[k].size else None for k in ("s", "y", "z", "mu")),
                ctypes.byref(opt), ctypes.sizeof(Options),
                *(out[k].ctypes.data for k in ("status", "x", "s", "y", "z", "mu", "cost", "iterations", "restorations",
                                               "repaired")), ctypes.byref(rep))
        elif parameters is None:
            rc = L.slpx_problem_solve_batch(self._h, B, x0.ctypes.data if B else None, ctypes.byref(opt),
                                            ctypes.sizeof(Options), *outputs, ctypes.byref(rep))
        else:
            rc = L.slpx_problem_solve_batch_parameters(self._h, B, x0.ctypes.data if B else None,
                                                       rows.ctypes.data if rows.size else None, ctypes.byref(opt),
                                                       ctypes.sizeof(Options), *outputs, ctypes.byref(rep))
        if rc != 0:
            raise SlpxError(L.slpx_last_error().decode())
        out["report"] = {f[0]: getattr(rep, f[0]) for f in Report._fields_}
        out["rounds"], out["handoffs"], out["driver"] = self.batch_stats()[1:]
        if hasattr(L, "slpx_problem_batch_restoration_stats"):
            out["restoration_lockstep"] = dict(zip(("instances", "phases", "rounds", "fallbacks"), self.batch_restoration_stats()))
        return out

    def parameters(self) -> list:
        """Expression ids of the model's parameters — free variables that are no decision variables and that the cost
        or a constraint reaches — ascending: the order of every parameter vector (slpx_problem_parameters; no device)."""
        L = lib()
        if not hasattr(L, "slpx_problem_parameters"):
            raise SlpxError(f"{LIB_PATH} has no slpx_problem_parameters")
        count = _check(L.slpx_problem_parameters(self._h, None, 0))
        ids = np.zeros(max(count, 1), dtype=np.int32)
        _check(L.slpx_problem_parameters(self._h, ids.ctypes.data, count))
        return [int(v) for v in ids[:count]]

    def parameter_slots_in_order(self) -> bool:
        """Parameter j sits in constant slot j of both tape programs (slpx_problem_parameter_slots_in_order; no device)."""
        return bool(_check(lib().slpx_problem_parameter_slots_in_order(self._h)))

    def set_parameters(self, values):
        """New values for all parameters, in place in every compiled system of the problem: the next solve does not
        compile again (slpx_problem_set_parameters)."""
        L = lib()
        if not hasattr(L, "slpx_problem_set_parameters"):
            raise SlpxError(f"{LIB_PATH} has no slpx_problem_set_parameters")
        v = np.ascontiguousarray(np.asarray(values, dtype=np.float64).ravel())
        n_p = len(self.parameters())
        if v.shape[0] != n_p:
            raise ValueError(f"set_parameters: {n_p} values, one per parameter")
        if L.slpx_problem_set_parameters(self._h, v.ctypes.data if v.size else None) != 0:
            raise SlpxError(L.slpx_last_error().decode())

    def compile_count(self) -> int:
        """How many times this problem built the system solve() runs on (slpx_problem_compile_count)."""
        return int(lib().slpx_problem_compile_count(self._h))

    def batch_stats(self):
        """(batch, rounds, handoffs, driver) of the last solve_batch (slpx_problem_batch_stats)."""
        L = lib()
        if not hasattr(L, "slpx_problem_batch_stats"):
            raise SlpxError(f"{LIB_PATH} has no slpx_problem_batch_stats")
        st = np.zeros(4, dtype=np.int64)
        if L.slpx_problem_batch_stats(self._h, st.ctypes.data) != 0:
            raise SlpxError("no batch has been solved")
        return tuple(int(v) for v in st)

    def batch_restoration_stats(self):
        """(instances restored in lockstep, restoration phases, lockstep restoration rounds, instances that used the
        batch-1 system for a fallback) of the last batch (slpx_problem_batch_restoration_stats)."""
        L = lib()
        if not hasattr(L, "slpx_problem_batch_restoration_stats"):
            raise SlpxError(f"{LIB_PATH} has no slpx_problem_batch_restoration_stats")
        st = np.zeros(4, dtype=np.int64)
        if L.slpx_problem_batch_restoration_stats(self._h, st.ctypes.data) != 0:
            raise SlpxError("no batch has been solved")
        return tuple(int(v) for v in st)

    def restoration_steps_batch(self, x, s, y, z, mu, steps, tolerance=1e-8, max_iterations=5000):
        """The batched twin of restoration_steps: `steps` restoration iterations from each of the B iterates in the rows of
        x (B x n), s (B x m_i), y (B x m_e), z (B x m_i) with mu (B), in lockstep on the batch system
        (slpx_problem_restoration_steps_batch).  Returns (status[B], x, s, y, z)."""
        L = lib()
        if not hasattr(L, "slpx_problem_restoration_steps_batch"):
            raise SlpxError(f"{LIB_PATH} has no slpx_problem_restoration_steps_batch")
        n, me, mi = self.dims
        mu = np.ascontiguousarray(np.atleast_1d(np.asarray(mu, dtype=np.float64)))
        B = mu.shape[0]
        x, s, y, z = (np.array(np.asarray(a, dtype=np.float64).reshape(B, k), dtype=np.float64, copy=True, order="C")
                      for a, k in ((x, n), (s, mi), (y, me), (z, mi)))
        status = np.zeros(B, dtype=np.int32)
        opt = Options(tolerance, max_iterations, 0.0, 0, 0, 0)
        hold = [a if a.size else np.zeros(1) for a in (x, s, y, z)]
        rc = L.slpx_problem_restoration_steps_batch(self._h, ctypes.byref(opt), ctypes.sizeof(Options), B,
                                                    *(a.ctypes.data for a in hold), mu.ctypes.data, int(steps),
                                                    status.ctypes.data)
        if rc != 0:
            raise SlpxError(L.slpx_last_error().decode())
        return status, x, s, y, z

    def restoration_steps(self, x, s, y, z, mu, steps, tolerance=1e-8, max_iterations=5000):
        """feasibility_restoration from the given iterate, `steps` iterations (slpx_problem_restoration_steps)."""
        x, s, y, z = (np.array(a, dtype=np.float64, copy=True) for a in (x, s, y, z))
        opt = Options(tolerance, max_iterations, 0.0, 0, 0, 0)
        status = lib().slpx_problem_restoration_steps(self._h, ctypes.byref(opt), x.ctypes.data, s.ctypes.data,
                                                      y.ctypes.data, z.ctypes.data, float(mu), int(steps))
        if status == -100:
            raise SlpxError(lib().slpx_last_error().decode())
        return status, x, s, y, z

    def add_callback(self, fn):
        """Problem::add_callback (problem.hpp:690-709): fn(info: dict) -> truthy to stop."""

        def trampoline(info_ptr, _user):
            i = info_ptr.contents
            view = lambda p, k: np.ctypeslib.as_array(p, shape=(k,)).copy() if k else np.zeros(0)
            off = list(i.off)
            return int(bool(fn({"iteration": i.iteration, "x": view(i.x, i.n), "s": view(i.s, i.m_i),
                                "y": view(i.y, i.m_e), "z": view(i.z, i.m_i), "f": i.V[off[0]], "off": off,
                                "V": i.V, "in_restoration": bool(i.in_restoration)})))

        cb = IterationCallback(trampoline)
        self._callbacks = getattr(self, "_callbacks", []) + [cb]  # keep the thunks alive
        _check(lib().slpx_problem_add_callback(self._h, ctypes.cast(cb, ctypes.c_void_p), None))

    def prebuild_kernels(self, directory=None) -> int:
        """Cross-compile this model's generated tape kernels for gfx950 into the library's
        jit_cache (slpx_problem_prebuild_kernels; needs no device)."""
        n = lib().slpx_problem_prebuild_kernels(self._h, None if directory is None else str(directory).encode())
        if n < 0:
            raise SlpxError(lib().slpx_last_error().decode())
        return n

    def system(self) -> "System":
        """The system solve() runs on (slpx_problem_system); owned by the problem."""
        h = lib().slpx_problem_system(self._h)
        if not h:
            raise SlpxError(lib().slpx_last_error().decode())
        return System._adopt(h, batch=1, borrowed=True)

    def clear_callbacks(self):
        _check(lib().slpx_problem_clear_callbacks(self._h))
        self._callbacks = []

    def duals(self):
        n, me, mi = self.dims
        s, y, z = np.zeros(mi), np.zeros(me), np.zeros(mi)
        lib().slpx_problem_get_duals(self._h, s.ctypes.data, y.ctypes.data, z.ctypes.data)
        return s, y, z


class System:
    """Compiled Newton system on one GPU (include/slpx.h, slpx_system_* and kernels)."""

    _borrowed = False

    @classmethod
    def _adopt(cls, handle, batch, borrowed=False):
        self = cls.__new__(cls)
        self._h = handle
        self._borrowed = borrowed
        self.batch = batch
        out = np.zeros(len(INFO_KEYS) + 4, dtype=np.int64)
        _check(lib().slpx_system_info(self._h, out.ctypes.data))
        self.info = {k: int(out[i]) for i, k in enumerate(INFO_KEYS)}
        return self

    @classmethod
    def linear_solver(cls, n, m_e, colptr, rowidx, batch=1, device=0):
        """RegularizedLDLT on its own (slpx_ldlt_create): lower-triangular CSC pattern only."""
        cp = np.ascontiguousarray(colptr, dtype=np.int32)
        ri = np.ascontiguousarray(rowidx, dtype=np.int32)
        h = lib().slpx_ldlt_create(int(n), int(m_e), cp.ctypes.data, ri.ctypes.data, int(batch), int(device))
        if not h:
            raise SlpxError(lib().slpx_last_error().decode())
        return cls._adopt(h, batch)

    def set_matrix(self, values):
        a = _f64(values)
        _check(lib().slpx_ldlt_set_matrix(self._h, a.ctypes.data))

    def __init__(self, problem: Problem, batch: int = 1, device: int = 0, perm=None):
        p = None if perm is None else np.ascontiguousarray(perm, dtype=np.int32)
        self._h = lib().slpx_system_create(problem._h, batch, device, _ptr(p), 0 if p is None else len(p))
        if not self._h:
            raise SlpxError(lib().slpx_last_error().decode())
        self.batch = batch
        out = np.zeros(len(INFO_KEYS) + 4, dtype=np.int64)
        _check(lib().slpx_system_info(self._h, out.ctypes.data))
        self.info = {k: int(out[i]) for i, k in enumerate(INFO_KEYS)}

    def close(self):
        if self._h and not self._borrowed:
            lib().slpx_system_destroy(self._h)
        self._h = None

    def pattern(self, which: int):
        nnz = lib().slpx_system_pattern(self._h, which, None, None)
        ncols = self.info["n"] if which != 5 else self.info["n"] + self.info["m_e"]
        colptr = np.zeros(ncols + 1, dtype=np.int32)
        rowidx = np.zeros(max(nnz, 1), dtype=np.int32)
        lib().slpx_system_pattern(self._h, which, colptr.ctypes.data, rowidx.ctypes.data)
        return colptr, rowidx[:nnz]

    def perm(self):
        p = np.zeros(self.info["n"] + self.info["m_e"], dtype=np.int32)
        lib().slpx_system_perm(self._h, p.ctypes.data)
        return p

    def set_stream(self, stream_ptr: int):
        _check(lib().slpx_system_set_stream(self._h, stream_ptr))

    def sync(self):
        _check(lib().slpx_system_sync(self._h))

    def set_scaling(self, scales):
        s = _f64(scales)
        _check(lib().slpx_system_set_scaling(self._h, s.ctypes.data))

    def set_parameters(self, values, per_instance=False):
        """The model's parameters at this system: values (n_p) for every instance, or per_instance (batch x n_p)
        (slpx_system_set_parameters)."""
        v = np.ascontiguousarray(np.asarray(values, dtype=np.float64))
        _check(lib().slpx_system_set_parameters(self._h, v.ctypes.data if v.size else None, int(per_instance)))

    def parameter_pool_bytes(self) -> int:
        """Device memory of the per-instance constant pools (slpx_system_parameter_pool_bytes); 0 before the first
        per-instance install."""
        return int(_check(lib().slpx_system_parameter_pool_bytes(self._h)))

    def set_state(self, x=None, s=None, y=None, z=None, mu=None):
        x, s, y, z, mu = (_f64(a) for a in (x, s, y, z, mu))
        _check(lib().slpx_system_set_state(self._h, _ptr(x), _ptr(s), _ptr(y), _ptr(z), _ptr(mu)))

    def sweep(self, full=True):
        _check(lib().slpx_tape_sweep(self._h, int(full)))

    def assemble(self):
        _check(lib().slpx_kkt_assemble(self._h))

    def rhs(self):
        _check(lib().slpx_kkt_rhs(self._h))

    def factor(self, delta, gamma):
        d = np.full(self.batch, delta, dtype=np.float64) if np.isscalar(delta) else _f64(delta)
        g = np.full(self.batch, gamma, dtype=np.float64) if np.isscalar(gamma) else _f64(gamma)
        stats = np.zeros((self.batch, 5))
        _check(lib().slpx_ldlt_factor(self._h, d.ctypes.data, g.ctypes.data, stats.ctypes.data))
        return stats

    def compute(self):
        info = np.zeros(self.batch, dtype=np.int32)
        reg = np.zeros((self.batch, 2))
        nf = ctypes.c_int32()
        _check(lib().slpx_ldlt_compute(self._h, info.ctypes.data, reg.ctypes.data, ctypes.addressof(nf)))
        return info, reg, nf.value

    def reset_regularization(self, gamma_min=1e-10):
        _check(lib().slpx_ldlt_reset(self._h, gamma_min))

    def solve(self):
        _check(lib().slpx_ldlt_solve(self._h))

    def backsub(self):
        _check(lib().slpx_step_backsub(self._h))

    @staticmethod
    def _mask(mask, batch):
        if mask is None:
            return None
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        if m.shape != (batch,):
            raise ValueError("mask: one entry per problem of the batch")
        return m

    def residual(self, mask=None, out=None):
        """(r, norm): r = rhs - (lhs + diag(delta, -gamma)) p of the factorization in memory, accumulated in
        double-double (slpx_ldlt_residual); r is [batch, dim], norm [batch] = max |r_i| (non-finite if an r_i is).
        mask: only the problems with mask[b] != 0 — the others' rows keep what `out` = (r, norm) held (zeros
        without `out`).  Also on a linear_solver() handle."""
        dim = self.info["n"] + self.info["m_e"]
        r, norm = (np.zeros((self.batch, dim)), np.zeros(self.batch)) if out is None else out
        m = self._mask(mask, self.batch)
        _check(lib().slpx_ldlt_residual_masked(self._h, _ptr(m), r.ctypes.data, norm.ctypes.data))
        return r, norm

    def refine(self, max_steps=1, mask=None):
        """(norms, accepted): up to max_steps steps of iterative refinement of p on the factors in memory
        (slpx_ldlt_refine).  norms is [batch, max_steps + 1]: the residual norm before, then after every step taken or
        tried (NaN beyond); accepted [batch] = steps taken.  Run it before the iterate moves: a Newton step that never
        stored its system has it evaluated at the resident state.  mask as in residual() (rows of the others: NaN, 0)."""
        norms = np.full((self.batch, int(max_steps) + 1), np.nan)
        accepted = np.zeros(self.batch, dtype=np.int32)
        m = self._mask(mask, self.batch)
        _check(lib().slpx_ldlt_refine_masked(self._h, int(max_steps), _ptr(m), norms.ctypes.data, accepted.ctypes.data))
        return norms, accepted

    def error_bounds(self, mask=None, forward=True, out=None):
        """{berr, ferr, solves} of p on the factors in memory (slpx_ldlt_error_bounds), each [batch]: the componentwise
        backward error, the estimated bound on max |p - p*| / max |p|, and the solves the estimate took (shared by the
        batch; at most 11).  forward=False: berr alone, no solve (ferr stays NaN).  p and rhs keep their bits.  mask as
        in residual(): the others' rows keep what `out` = (berr, ferr, solves) held (NaN, NaN, 0 without `out`)."""
        berr, ferr, solves = ((np.full(self.batch, np.nan), np.full(self.batch, np.nan), np.zeros(self.batch, dtype=np.int32))
                              if out is None else out)
        m = self._mask(mask, self.batch)
        _check(lib().slpx_ldlt_error_bounds(self._h, _ptr(m), berr.ctypes.data, ferr.ctypes.data if forward else None,
                                            solves.ctypes.data))
        return {"berr": berr, "ferr": ferr, "solves": solves}

    def condest(self, mask=None, out=None):
        """{norm1, inv_norm1, cond1, solves} of the matrix the factors in memory are factors of (slpx_ldlt_condest):
        its 1-norm, the estimated 1-norm of its inverse (a lower estimate), their product, the solves taken.  mask and
        `out` = (norm1, inv_norm1, solves) as in error_bounds()."""
        norm1, inv_norm1, solves = ((np.full(self.batch, np.nan), np.full(self.batch, np.nan), np.zeros(self.batch, dtype=np.int32))
                                    if out is None else out)
        m = self._mask(mask, self.batch)
        _check(lib().slpx_ldlt_condest(self._h, _ptr(m), norm1.ctypes.data, inv_norm1.ctypes.data, solves.ctypes.data))
        return {"norm1": norm1, "inv_norm1": inv_norm1, "cond1": norm1 * inv_norm1, "solves": solves}

    def newton_step(self, refresh_ad=True):
        info = np.zeros(self.batch, dtype=np.int32)
        _check(lib().slpx_newton_step(self._h, int(refresh_ad), info.ctypes.data))
        return info

    def newton_steps(self, count, refresh_ad=True, forget_regularization=True):
        info = np.zeros(self.batch, dtype=np.int32)
        _check(lib().slpx_newton_steps(self._h, int(count), int(refresh_ad), int(forget_regularization),
                                       info.ctypes.data))
        return info

    def regularization(self) -> np.ndarray:
        """[batch, 2] = (delta, gamma) the last compute / Newton step settled on."""
        reg = np.zeros((self.batch, 2))
        _check(lib().slpx_system_regularization(self._h, reg.ctypes.data))
        return reg

    def get(self, which: str) -> np.ndarray:
        sel = {"V": 0, "lhs": 1, "rhs": 2, "p": 3, "p_s": 4, "p_z": 5, "D": 6, "Lx": 7, "x": 8, "s": 9,
               "y": 10, "z": 11, "zv": 12, "update_blocks": 13}[which]
        count = _check(lib().slpx_system_get(self._h, sel, None))
        out = np.zeros(max(count, 1))
        _check(lib().slpx_system_get(self._h, sel, out.ctypes.data))
        return out[:count].reshape(self.batch, -1)

    # ---- the interior-point iteration around the Newton step, on the resident iterate ----
    IPM_ERROR_KEYS = ["dual_inf_u", "sz_max_u", "ce_inf_u", "cis_inf_u", "y1_u", "z1_u", "dual_inf", "sz_min",
                      "sz_max", "ce_inf", "cis_inf", "y1", "z1", "f", "viol", "logsum", "aetce_sq", "ce_sq",
                      "aitcp_sq", "cp_sq", "x_inf", "s_inf", "finite", "ci_all_pos"]

    def ipm_direction(self, tau):
        out = np.zeros(3)
        _check(lib().slpx_ipm_direction(self._h, float(tau), out.ctypes.data))
        return {"alpha_max": out[0], "alpha_z": out[1], "D_phi": out[2]}

    def ipm_trial(self, alpha, s_from_ci=False):
        out = np.zeros(4)
        _check(lib().slpx_ipm_trial(self._h, float(alpha), int(s_from_ci), out.ctypes.data))
        return {"f": out[0], "viol": out[1], "logsum": out[2], "finite": out[3]}

    def ipm_commit(self, alpha, alpha_z, s_from_ci=False):
        _check(lib().slpx_ipm_commit(self._h, float(alpha), float(alpha_z), int(s_from_ci)))

    def ipm_errors(self, error_scales):
        sc = _f64(error_scales)
        out = np.zeros(24)
        _check(lib().slpx_ipm_errors(self._h, sc.ctypes.data, out.ctypes.data))
        return dict(zip(self.IPM_ERROR_KEYS, out))

    def set_rhs(self, rhs):
        r = _f64(rhs)
        _check(lib().slpx_system_set_rhs(self._h, r.ctypes.data))

    def set_lhs(self, lhs):
        a = _f64(lhs)
        _check(lib().slpx_system_set_lhs(self._h, a.ctypes.data))

    def debug_chain(self, action=0) -> int:
        """Chain failures recovered from so far; action 1 breaks the next chained sweep's hand-over (slpx_debug_chain)."""
        return _check(lib().slpx_debug_chain(self._h, action))

    def time_fused_step(self, iters=10):
        """The launches a single problem's step really makes (slpx_system_time_fused_step)."""
        ms = np.zeros(4, dtype=np.float32)
        _check(lib().slpx_system_time_fused_step(self._h, iters, ms.ctypes.data))
        return {"sweep": float(ms[0]), "kkt_factor_solve": float(ms[1]), "total": float(ms[2]),
                "one_launch": bool(ms[3]), "multifrontal": ms[3] == 2.0}

    def time_step(self, iters=10, refresh_ad=True):
        ms = np.zeros(8, dtype=np.float32)
        _check(lib().slpx_system_time_step(self._h, iters, int(refresh_ad), ms.ctypes.data))
        keys = ["sweep", "assemble", "rhs", "factor", "solve", "backsub", "total", "factorizations"]
        return {k: float(ms[i]) for i, k in enumerate(keys)}


from .dist import Comm, shard_range  # noqa: E402,F401  (multi-GPU plumbing)
