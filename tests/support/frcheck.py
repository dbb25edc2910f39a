"""ctypes wrapper over tests/support/libslpx_frcheck.so — TEST INFRASTRUCTURE ONLY.

A probe of slpx::FrDevice (frcheck.cpp): the launch wrappers of feasibility restoration from libslpx.so, driven one
method at a time on an `sa.System(problem, 1)`, with the sweeps the driver runs between them and every buffer the
kernels read or write readable and writable.  Never used by the product.
"""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np

import sleipnir_amd

HERE = Path(__file__).resolve().parent
LIB_PATH = HERE / "libslpx_frcheck.so"
_CSRC = HERE.parents[1] / "sleipnir_amd" / "csrc"
SOURCES = [HERE / "frcheck.cpp", HERE / "probe_common.hpp", _CSRC / "restoration.hpp", _CSRC / "device.hpp", _CSRC / "device_base.hpp", _CSRC / "device_ldlt.hpp"]

# fc_get / fc_put selectors (frcheck.cpp: FrProbe::buffer)
BUFFERS = ["V", "V_trial", "in", "trial_in", "s", "y", "z", "p", "p_s", "p_z", "lhs_raw", "rhs_raw", "s_ahead", "y_ahead",
           "z_ahead", "second_lhs", "second_rhs", "soc_ce", "soc_c0", "soc_x", "keep_p", "keep_ps0", "keep_pz0", "keep_dpn",
           "keep_psx", "keep_pzx", "pn", "sx", "zx", "dpn", "psx", "pzx", "pn_ahead", "sx_ahead", "zx_ahead", "alpha"]

# FrHost as doubles (restoration.hpp: FrDirOut, IpmTrialOut, FrErrOut)
DIR_KEYS = ["alpha_max", "alpha_z", "D_phi", "eliminated_min_pivot"]
TRIAL_KEYS = ["f", "viol", "logsum", "finite"]
ERR_KEYS = ["dual_inf_u", "sz_max_u", "ce_inf_u", "cis_inf_u", "y1_u", "z1_u", "dual_inf", "sz_min", "sz_max", "ce_inf",
            "cis_inf", "y1", "z1", "f", "viol", "logsum", "aetce_sq", "ce_sq", "aitcp_sq", "cp_sq", "x_inf", "s_inf",
            "finite", "ci_all_pos", "f_outer", "viol_outer", "logsum_outer", "dphi_outer", "eliminated_min_pivot"]


def build():
    sleipnir_amd.build()
    return _build_probe()


def _build_probe():
    # (lib() builds the probe alone: libslpx.so is loaded by then, and relinking it in place would pull the file out
    # from under the process)
    cmd = ["/opt/rocm/bin/hipcc", "-O2", "-std=c++23", "-fPIC", "-shared", "--offload-arch=gfx950",
           "-x", "hip", str(HERE / "frcheck.cpp"), "-o", str(LIB_PATH),
           "-L" + str(sleipnir_amd.LIB_PATH.parent), "-lslpx",
           "-Wl,-rpath," + str(sleipnir_amd.LIB_PATH.parent)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("building frcheck failed:\n" + res.stdout + res.stderr)
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
    vp, i32, i64, d = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double

    def sig(name, restype, *argtypes):
        fn = getattr(L, name)
        fn.restype = restype
        fn.argtypes = list(argtypes)

    sig("fc_last_error", ctypes.c_char_p)
    sig("fc_create", vp, vp)
    sig("fc_destroy", None, vp)
    sig("fc_dims", i32, vp, vp)
    sig("fc_set_outer", i32, vp, vp, vp, vp, vp)
    sig("fc_begin", i32, vp, vp, vp, vp, vp, d, vp, vp, vp, vp)
    sig("fc_build", i32, vp, d, d, i32, i32, i32)
    sig("fc_build_pair", i32, vp, d, d, d)
    sig("fc_expand", i32, vp, d, d, d, i32, i32)
    sig("fc_accept_lookahead", i32, vp)
    sig("fc_trial_point", i32, vp, d)
    sig("fc_trial_metrics", i32, vp, d, d)
    sig("fc_commit", i32, vp, d, d, d)
    sig("fc_errors", i32, vp, i32, d, i32, i32)
    sig("fc_soc_accumulate", i32, vp, d, i32)
    sig("fc_save_direction", i32, vp)
    sig("fc_restore_direction", i32, vp)
    sig("fc_wait_published", i32, vp)
    sig("fc_sweep_full", i32, vp, i32)
    sig("fc_sweep_values_trial", i32, vp)
    sig("fc_sweep_full_lookahead", i32, vp, i32)
    sig("fc_download_state", i32, vp, vp, vp, vp)
    sig("fc_download_direction", i32, vp, vp, vp, vp)
    sig("fc_host", i32, vp, vp)
    sig("fc_get", i64, vp, ctypes.c_int, vp)
    sig("fc_put", i32, vp, ctypes.c_int, vp)
    _lib = L
    return L


class ProbeError(RuntimeError):
    pass


def _check(rc):
    if rc < 0:
        raise ProbeError(lib().fc_last_error().decode())
    return rc


def _f64(a, n):
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    assert a.size == n, (a.size, n)
    if a.size == 0:  # (a valid pointer for the empty blocks: nothing is read through it)
        a = np.zeros(1)
    return a


class FrProbe:
    """FrDevice on the system behind `system` (an sa.System of batch 1)."""

    def __init__(self, system: "sleipnir_amd.System"):
        self.system = system
        self._h = lib().fc_create(system._h)
        if not self._h:
            raise ProbeError(lib().fc_last_error().decode())
        d = np.zeros(10, dtype=np.int64)
        _check(lib().fc_dims(self._h, d.ctypes.data))
        (self.n, self.m_e, self.m_i, self.dim, self.nV, self.nnz_lhs, self.M, self.n_in, self.n_reduces,
         self.host_doubles) = (int(v) for v in d)
        assert self.host_doubles == len(DIR_KEYS) + len(TRIAL_KEYS) + 2 * len(ERR_KEYS)

    def close(self):
        if self._h:
            lib().fc_destroy(self._h)
            self._h = None

    def _call(self, name, *args):
        _check(getattr(lib(), "fc_" + name)(self._h, *args))

    def set_outer(self, x, s, y, z):
        a = [_f64(x, self.n), _f64(s, self.m_i), _f64(y, self.m_e), _f64(z, self.m_i)]
        self._call("set_outer", *(v.ctypes.data for v in a))

    def begin(self, x_r, w, g_outer, s_outer, mu_outer, pn, sx, zx, err_scales):
        a = [_f64(x_r, self.n), _f64(w, self.n), _f64(g_outer, self.n), _f64(s_outer, self.m_i)]
        b = [_f64(pn, self.M), _f64(sx, self.M), _f64(zx, self.M), _f64(err_scales, 1 + self.m_e + self.m_i)]
        self._call("begin", *(v.ctypes.data for v in a), float(mu_outer), *(v.ctypes.data for v in b))

    def build(self, delta, mu, soc=False, rhs_only=False, second=False):
        self._call("build", float(delta), float(mu), int(soc), int(rhs_only), int(second))

    def build_pair(self, delta, delta_second, mu):
        self._call("build_pair", float(delta), float(delta_second), float(mu))

    def expand(self, delta, mu, tau, soc=False, ahead=False):
        self._call("expand", float(delta), float(mu), float(tau), int(soc), int(ahead))

    def accept_lookahead(self):
        self._call("accept_lookahead")

    def trial_point(self, alpha):
        self._call("trial_point", float(alpha))

    def trial_metrics(self, alpha, mu):
        self._call("trial_metrics", float(alpha), float(mu))

    def commit(self, alpha, alpha_z, mu):
        self._call("commit", float(alpha), float(alpha_z), float(mu))

    def errors(self, check_all_V, mu, ahead=False, sums_ride=False):
        self._call("errors", int(check_all_V), float(mu), int(ahead), int(sums_ride))

    def soc_accumulate(self, alpha, first):
        self._call("soc_accumulate", float(alpha), int(first))

    def save_direction(self):
        self._call("save_direction")

    def restore_direction(self):
        self._call("restore_direction")

    def wait_published(self):
        self._call("wait_published")

    def sweep_full(self, with_reduce=True):
        self._call("sweep_full", int(with_reduce))

    def sweep_values_trial(self):
        self._call("sweep_values_trial")

    def sweep_full_lookahead(self, with_reduce=False):
        self._call("sweep_full_lookahead", int(with_reduce))

    def download_state(self):
        out = [np.zeros(max(1, self.M)) for _ in range(3)]
        self._call("download_state", *(v.ctypes.data for v in out))
        return tuple(v[:self.M] for v in out)

    def download_direction(self):
        out = [np.zeros(max(1, self.M)) for _ in range(3)]
        self._call("download_direction", *(v.ctypes.data for v in out))
        return tuple(v[:self.M] for v in out)

    def host(self):
        """FrHost: {"dir": {...}, "trial": {...}, "err": {...}, "err_ahead": {...}}"""
        out = np.zeros(self.host_doubles)
        self._call("host", out.ctypes.data)
        nd, nt, ne = len(DIR_KEYS), len(TRIAL_KEYS), len(ERR_KEYS)
        return {"dir": dict(zip(DIR_KEYS, out[:nd])), "trial": dict(zip(TRIAL_KEYS, out[nd:nd + nt])),
                "err": dict(zip(ERR_KEYS, out[nd + nt:nd + nt + ne])), "err_ahead": dict(zip(ERR_KEYS, out[nd + nt + ne:]))}

    def get(self, name):
        which = BUFFERS.index(name)
        count = _check(lib().fc_get(self._h, which, None))
        out = np.zeros(max(count, 1))
        _check(lib().fc_get(self._h, which, out.ctypes.data))
        return out[:count]

    def put(self, name, values):
        which = BUFFERS.index(name)
        count = _check(lib().fc_get(self._h, which, None))
        a = _f64(values, count)
        if count:
            _check(lib().fc_put(self._h, which, a.ctypes.data))
