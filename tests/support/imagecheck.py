"""ctypes wrapper over tests/support/libslpx_imagecheck.so — TEST INFRASTRUCTURE ONLY.

The packers of csrc/device_images.hpp run on the plans of a hostcheck handle (imagecheck.cpp): what DeviceNlp's
constructor uploads, and the plan arrays it is made from, as numpy arrays by name.  Never used by the product.
"""
from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np

import sleipnir_amd

HERE = Path(__file__).resolve().parent
LIB_PATH = HERE / "libslpx_imagecheck.so"
_CSRC = HERE.parents[1] / "sleipnir_amd" / "csrc"
SOURCES = [HERE / "imagecheck.cpp", _CSRC / "device_images.hpp", _CSRC / "device_layout.h"]

# the fields of MfCarve (device_layout.h), in order: columns of Images.array("mf.carve", "u4", 16)
CARVE = ["o_arena", "o_invd", "o_x", "o_tab", "o_lvl", "o_ext", "o_src", "o_flags", "o_cent", "o_cptr", "o_cidx", "o_cp", "o_anc",
         "o_fr", "o_cnt", "o_terms"]


def build():
    sleipnir_amd.build()
    return _build_probe()


def _build_probe():
    # (lib() builds the probe alone: libslpx.so is loaded by then, and relinking it in place would pull the file out
    # from under the process)
    cmd = ["/opt/rocm/bin/hipcc", "-O2", "-std=c++23", "-fPIC", "-shared", "--offload-arch=gfx950",
           "-x", "hip", str(HERE / "imagecheck.cpp"), "-o", str(LIB_PATH),
           "-L" + str(sleipnir_amd.LIB_PATH.parent), "-lslpx",
           "-Wl,-rpath," + str(sleipnir_amd.LIB_PATH.parent)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("building imagecheck failed:\n" + res.stdout + res.stderr)
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
    vp, i32, i64, u32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32

    def sig(name, restype, *argtypes):
        fn = getattr(L, name)
        fn.restype = restype
        fn.argtypes = list(argtypes)

    sig("ic_create", vp, vp, vp, vp)
    sig("ic_destroy", None, vp)
    sig("ic_array", i64, vp, ctypes.c_char_p, vp)
    sig("ic_scalar", i32, vp, ctypes.c_char_p, vp)
    sig("ic_template_tables", i32, vp, i32, u32, u32, u32)
    sig("ic_level_tables_throw_at", i32, vp, u32)
    sig("ic_mf_declines_short_task_terms", i32, vp)
    _lib = L
    return L


class Images:
    """The images of the plans of `hc` (a hostcheck.HostCheck, which must outlive this object)."""

    def __init__(self, hc):
        s, k, l = hc.plans()
        self._h = lib().ic_create(s, k, l)
        if not self._h:
            raise RuntimeError("imagecheck: a packer threw")

    def close(self):
        if self._h:
            lib().ic_destroy(self._h)
            self._h = None

    def array(self, name, dtype, cols=None):
        """A copy of the array `name` as `dtype`, reshaped to (-1, cols) if given."""
        data = ctypes.c_void_p()
        nbytes = lib().ic_array(self._h, name.encode(), ctypes.byref(data))
        if nbytes < 0:
            raise KeyError(name)
        a = np.frombuffer(ctypes.string_at(data, nbytes) if nbytes else b"", dtype=dtype).copy()
        return a if cols is None else a.reshape(-1, cols)

    def scalar(self, name):
        out = ctypes.c_int64()
        if lib().ic_scalar(self._h, name.encode(), ctypes.byref(out)) != 0:
            raise KeyError(name)
        return int(out.value)

    def tasks(self, prefix, fields):
        """{field: array} of the per-task struct fields exported under `prefix` (l.tasks, l.mf_tasks, tape.tasks)."""
        return {f: self.array(f"{prefix}.{f}", "u4") for f in fields}

    def template_tables(self, batch, block_threads, n_groups, max_members):
        """pack_template_tables over the families imagecheck.cpp makes of the full tape; returns their number."""
        return lib().ic_template_tables(self._h, batch, block_threads, n_groups, max_members)

    def level_tables_throw_at(self, value):
        return lib().ic_level_tables_throw_at(self._h, value)

    def mf_declines_short_task_terms(self):
        return lib().ic_mf_declines_short_task_terms(self._h)
