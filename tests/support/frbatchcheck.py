"""ctypes wrapper over tests/support/libslpx_frbatchcheck.so — TEST INFRASTRUCTURE ONLY.

A probe of slpx::BatchFrDevice (frbatchcheck.cpp): the launch wrappers of the batched feasibility restoration from
libslpx.so, driven one method at a time on an `sa.System(problem, B)`, with every per-instance buffer the kernels read or
write readable and writable.  Never used by the product.
"""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np

import sleipnir_amd

HERE = Path(__file__).resolve().parent
LIB_PATH = HERE / "libslpx_frbatchcheck.so"
_CSRC = HERE.parents[1] / "sleipnir_amd" / "csrc"
SOURCES = [HERE / "frbatchcheck.cpp", HERE / "probe_common.hpp", _CSRC / "fr_batch.hpp", _CSRC / "batch_lockstep.hpp",
           _CSRC / "restoration.hpp", _CSRC / "device.hpp", _CSRC / "device_base.hpp", _CSRC / "device_ldlt.hpp"]

# fbc_get / fbc_put selectors (frbatchcheck.cpp: BatchFrProbe::buffer) with the length of an instance's slice
BUFFERS = ["x", "s0", "y", "z0", "xr", "w", "g_outer", "s_outer", "pn", "sx", "zx", "p", "ps0", "pz0", "dpn", "psx", "pzx",
           "soc_ce", "soc_c0", "soc_x", "keep_p", "keep_ps0", "keep_pz0", "keep_dpn", "keep_psx", "keep_pzx", "Vcur", "out",
           "vt_keep", "sys_V", "sys_in", "sys_lhs", "sys_rhs", "sys_p"]
# what a launch of the device struct may write of an instance (everything but the batch system's shared scratch)
OWN = BUFFERS[:BUFFERS.index("sys_V")]

DIR_KEYS = ["alpha_max", "alpha_z", "D_phi", "eliminated_min_pivot"]
TRIAL_KEYS = ["f", "viol", "logsum", "finite"]
ERR_KEYS = ["dual_inf_u", "sz_max_u", "ce_inf_u", "cis_inf_u", "y1_u", "z1_u", "dual_inf", "sz_min", "sz_max", "ce_inf",
            "cis_inf", "y1", "z1", "f", "viol", "logsum", "aetce_sq", "ce_sq", "aitcp_sq", "cp_sq", "x_inf", "s_inf",
            "finite", "ci_all_pos", "f_outer", "viol_outer", "logsum_outer", "dphi_outer", "eliminated_min_pivot"]
PARAMS = ["delta", "mu", "tau", "alpha", "alpha_soc", "alpha_z", "mu_outer", "soc", "first", "rhs_only", "active"]


def build():
    sleipnir_amd.build()
    return _build_probe()


def _build_probe():
    cmd = ["/opt/rocm/bin/hipcc", "-O2", "-std=c++23", "-fPIC", "-shared", "--offload-arch=gfx950",
           "-x", "hip", str(HERE / "frbatchcheck.cpp"), "-o", str(LIB_PATH),
           "-L" + str(sleipnir_amd.LIB_PATH.parent), "-lslpx",
           "-Wl,-rpath," + str(sleipnir_amd.LIB_PATH.parent)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("building frbatchcheck failed:\n" + res.stdout + res.stderr)
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
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64

    def sig(name, restype, *argtypes):
        fn = getattr(L, name)
        fn.restype = restype
        fn.argtypes = list(argtypes)

    sig("fbc_last_error", ctypes.c_char_p)
    sig("fbc_create", vp, vp)
    sig("fbc_destroy", None, vp)
    sig("fbc_dims", i32, vp, vp)
    sig("fbc_set_scales", i32, vp, vp)
    sig("fbc_begin", i32, vp, i32, *([vp] * 11))
    sig("fbc_set_params", i32, vp, *([vp] * 11))
    for name in ("sweep", "build", "soc_accumulate", "save_direction", "restore_direction", "commit"):
        sig("fbc_" + name, i32, vp)
    sig("fbc_expand", i32, vp, vp)
    sig("fbc_trial_values", i32, vp, i32, vp)
    sig("fbc_errors", i32, vp, i32, vp)
    sig("fbc_download_instance", i32, vp, i32, *([vp] * 7))
    sig("fbc_get", i64, vp, ctypes.c_int, vp)
    sig("fbc_put", i32, vp, ctypes.c_int, vp)
    _lib = L
    return L


class ProbeError(RuntimeError):
    pass


def _check(rc):
    if rc < 0:
        raise ProbeError(lib().fbc_last_error().decode())
    return rc


def _f64(a, n):
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    assert a.size == n, (a.size, n)
    if a.size == 0:  # (a valid pointer for the empty blocks: nothing is read through it)
        a = np.zeros(1)
    return a


class BatchFrProbe:
    """BatchFrDevice on the system behind `system` (an sa.System of batch B)."""

    def __init__(self, system: "sleipnir_amd.System"):
        self.system = system
        self._h = lib().fbc_create(system._h)
        if not self._h:
            raise ProbeError(lib().fbc_last_error().decode())
        d = np.zeros(11, dtype=np.int64)
        _check(lib().fbc_dims(self._h, d.ctypes.data))
        (self.B, self.n, self.m_e, self.m_i, self.dim, self.ns, self.nV, self.nnz_lhs, self.M, self.n_in,
         self.err_doubles) = (int(v) for v in d)
        assert self.err_doubles == len(ERR_KEYS)
        self.params = {k: np.zeros(self.B, dtype=np.uint8 if k in ("soc", "first", "rhs_only", "active") else np.float64)
                       for k in PARAMS}

    def close(self):
        if self._h:
            lib().fbc_destroy(self._h)
            self._h = None

    def _call(self, name, *args):
        _check(getattr(lib(), "fbc_" + name)(self._h, *args))

    def set_scales(self, scales):
        a = _f64(scales, self.B * self.ns)
        self._call("set_scales", a.ctypes.data)

    def begin(self, b, st):
        """st: a state of fr_reference.random_state (x, s0, y, z0, xr, w, g_outer, s_outer, pn, sx, zx)"""
        a = [_f64(st["x"], self.n), _f64(st["s0"], self.m_i), _f64(st["y"], self.m_e), _f64(st["z0"], self.m_i),
             _f64(st["xr"], self.n), _f64(st["w"], self.n), _f64(st["g_outer"], self.n), _f64(st["s_outer"], self.m_i),
             _f64(st["pn"], self.M), _f64(st["sx"], self.M), _f64(st["zx"], self.M)]
        self._call("begin", int(b), *(v.ctypes.data for v in a))

    def set_params(self, **kw):
        """per-instance arrays (or scalars, broadcast) by name; the others keep their last values; then upload()"""
        for k, v in kw.items():
            self.params[k][:] = v
        self._call("set_params", *(self.params[k].ctypes.data for k in PARAMS))

    def sweep(self):
        self._call("sweep")

    def build(self):
        self._call("build")

    def _scalars(self, name, per, keys, *args):
        out = np.zeros(self.B * per)
        self._call(name, *args, out.ctypes.data)
        return [dict(zip(keys, out[b * per:(b + 1) * per])) for b in range(self.B)]

    def expand(self):
        return self._scalars("expand", 4, DIR_KEYS)

    def trial_values(self, after_expand=False):
        return self._scalars("trial_values", 4, TRIAL_KEYS, int(after_expand))

    def errors(self, check_all_V):
        return self._scalars("errors", len(ERR_KEYS), ERR_KEYS, int(check_all_V))

    def soc_accumulate(self):
        self._call("soc_accumulate")

    def save_direction(self):
        self._call("save_direction")

    def restore_direction(self):
        self._call("restore_direction")

    def commit(self):
        self._call("commit")

    def download_instance(self, b):
        sizes = [self.n, self.m_i, self.m_e, self.m_i, self.M, self.M, self.M]
        out = [np.zeros(max(1, k)) for k in sizes]
        self._call("download_instance", int(b), *(v.ctypes.data for v in out))
        return dict(zip(("x", "s0", "y", "z0", "pn", "sx", "zx"), (v[:k] for v, k in zip(out, sizes))))

    def get(self, name):
        """[B][slice] of buffer `name`"""
        which = BUFFERS.index(name)
        count = _check(lib().fbc_get(self._h, which, None))
        out = np.zeros(max(count, 1))
        _check(lib().fbc_get(self._h, which, out.ctypes.data))
        return out[:count].reshape(self.B, -1) if count else np.zeros((self.B, 0))

    def put(self, name, values):
        which = BUFFERS.index(name)
        count = _check(lib().fbc_get(self._h, which, None))
        a = _f64(values, count)
        if count:
            _check(lib().fbc_put(self._h, which, a.ctypes.data))
