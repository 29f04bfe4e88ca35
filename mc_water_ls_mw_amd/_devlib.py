"""What the ctypes wrappers of the stand-alone device libraries share (``structure`` over libmw_sk.so, ``bondorder`` over
libmw_boo.so, ``tetrahedral`` over libmw_tet.so, ``angles`` over libmw_adf.so, ``rings`` over libmw_rings.so, ``quench`` over libmw_quench.so, ``dynamics`` over libmw_md.so, ``npt`` over libmw_npt.so, ``timecorr`` over libmw_tcf.so, ``phonons`` over libmw_hess.so, ``einstein`` over libmw_ti.so): loading, the error check, the one-device life cycle, the plan fields and the checks of the callers' arrays.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from .energy import MwError, _share_hip_runtime_with_torch


class DevLib:
    """One library with the entries ``mw_<prefix>_init / finalize / is_initialised / last_error / last``.  ``what`` names
    it in the not-built message; ``setup(L)`` declares argument types after loading."""

    def __init__(self, prefix, path, what, plan_fields, setup=None):
        self.prefix, self.path, self.what, self.plan_fields, self.setup = prefix, path, what, plan_fields, setup
        self.name = os.path.basename(path)
        self.lib = None
        self.device = None                          # the device this module initialised the library on

    def _entry(self, name):
        return getattr(self.lib, f"mw_{self.prefix}_{name}")

    def load(self, path=None):
        """dlopen the library.  Raises if it has not been built -- there is no fallback."""
        if self.lib is not None:
            return self.lib
        path = path or self.path
        if not os.path.exists(path):
            raise MwError(f"{path} not found: build it with `python -m mc_water_ls_mw_amd.build` ({self.what} has no CPU fallback)")
        _share_hip_runtime_with_torch()
        L = ctypes.CDLL(path)
        getattr(L, f"mw_{self.prefix}_last_error").restype = ctypes.c_char_p
        if self.setup:
            self.setup(L)
        self.lib = L
        return L

    def chk(self, rc):
        if rc != 0:
            raise MwError(self._entry("last_error")().decode())

    def live(self, device=None):
        """The library, initialised on ``device`` (0 by default) if nobody has.  ``device`` given and the library live on
        another one: an error -- it serves one device, and pointers of another must not reach it."""
        L = self.load()
        if not self._entry("is_initialised")():
            self.chk(self._entry("init")(int(device or 0)))
            self.device = int(device or 0)
        elif device is not None and self.device is not None and int(device) != self.device:
            raise MwError(f"{self.name} is initialised on device {self.device}, not on device {int(device)}: "
                          f"call {self.prefix}_finalize() first")
        return L

    def finalize(self):
        """Finalize the library (not live: nothing to do) and forget its device."""
        self.load()
        self.chk(self._entry("finalize")())
        self.device = None

    def plan_out(self):
        return (ctypes.c_int * len(self.plan_fields))()

    def fields(self, out):
        d = dict(zip(self.plan_fields, (int(v) for v in out)))
        d["small"] = bool(d["small"])
        return d

    def last(self):
        """{field: value} of the plan fields for the last call that launched."""
        self.load()
        out = self.plan_out()
        self.chk(self._entry("last")(out, len(out)))
        return self.fields(out)


def check_boxes(cells, pos):
    """``cells`` [nboxes, 3, 3] and ``pos`` [nboxes, nwater, 3], arrays or tensors."""
    if cells.ndim != 3 or tuple(cells.shape[1:]) != (3, 3) or pos.ndim != 3 or pos.shape[0] != cells.shape[0] or pos.shape[2] != 3:
        raise MwError(f"cells {tuple(cells.shape)} / pos {tuple(pos.shape)}: expected [nboxes, 3, 3] and [nboxes, nwater, 3]")


def host_boxes(cells, pos):
    """(cells, pos, single) as contiguous float64 arrays with the leading box axis; ``single``: it was added here."""
    cells = np.ascontiguousarray(cells, dtype=np.float64)
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    single = cells.ndim == 2
    if single:
        cells, pos = cells[None], pos[None]
    check_boxes(cells, pos)
    return cells, pos, single


def check_device_tensors(*named):
    """Every (tensor, dtype, name): a contiguous device tensor of that dtype, all on one device, which is returned."""
    for t, dt, name in named:
        if not (t.is_cuda and t.dtype == dt and t.is_contiguous()):
            raise MwError(f"{name}: expected a contiguous {dt} device tensor")
    dev = named[0][0].device
    if any(t.device != dev for t, _, _ in named):
        raise MwError(f"{', '.join(name for _, _, name in named)} must be on one device")
    return dev
