"""Steinhardt bond-order parameters over the C ABI of ``libmw_boo.so`` (include/mw_boo.h): q4, q6, the neighbour-averaged
qbar4, qbar6 (Lechner & Dellago 2008), the ten Wolde-Frenkel solid-like connection count of every molecule, and the global
Q4, Q6 of every box -- the continuous companions of the CHILL+ classes.

A cell ``h`` is a [3, 3] array whose ROW k is the lattice vector h_(k+1) (``EnergyModule.hmatrix[b]``, the layout of
``mw_set_cell``), lengths in bohr; the cutoff is given in Angstrom and must not exceed the narrowest perpendicular width
of any cell.  The library needs positions and cells only: it works on any configuration, with or without an engine in the
process.  There is no CPU path: without the library or a device the calls raise.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from ._devlib import DevLib, MwError, check_boxes, check_device_tensors, host_boxes

PKG = os.path.dirname(os.path.abspath(__file__))
BOO_LIB_PATH = os.path.join(PKG, "libmw_boo.so")
BOHR_TO_ANG = 0.5291772108                      # constants.f90:42-43, as energy.py converts

#: every symbol include/mw_boo.h declares
BOO_ABI_SYMBOLS = ("mw_boo_init", "mw_boo_finalize", "mw_boo_is_initialised", "mw_boo_last_error", "mw_boo_compute",
                   "mw_boo_compute_device", "mw_boo_plan", "mw_boo_last", "mw_boo_elapsed_ms")
#: the fields of mw_boo_plan / mw_boo_last, in order
PLAN_FIELDS = ("boxes_per_chunk", "chunks", "small", "g1", "g2", "g3", "lds_bytes", "scratch_bytes_per_box", "boxes_per_workgroup")


def _argtypes(L):
    for f in (L.mw_boo_compute, L.mw_boo_compute_device):
        f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_double,
                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.mw_boo_plan.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int]


_dev = DevLib("boo", BOO_LIB_PATH, "bond order", PLAN_FIELDS, setup=_argtypes)

load_boo_library = _dev.load                     # (path=BOO_LIB_PATH): dlopen libmw_boo.so; raises if it has not been built
boo_finalize = _dev.finalize
boo_last = _dev.last                             # the fields of boo_plan for the last call that launched (the grid is that of its first box)


def boo_init(device=0):
    """Initialise the library on ``device`` (the compute functions do it on device 0 when nobody has)."""
    return _dev.live(device)


def boo_plan(nwater, cell, rc_ang=3.5, nboxes=1):
    """{field: value} of PLAN_FIELDS: the launch rules of ``nboxes`` boxes of ``nwater`` molecules with the cell ``cell``
    [3, 3] (bohr) and the cutoff ``rc_ang`` (mw_boo_plan), no device needed."""
    L = _dev.load()
    out = _dev.plan_out()
    cell = np.ascontiguousarray(cell, dtype=np.float64)
    if cell.shape != (3, 3):
        raise MwError(f"cell {cell.shape}: expected [3, 3]")
    _dev.chk(L.mw_boo_plan(int(nwater), cell.ctypes.data, float(rc_ang) / BOHR_TO_ANG, int(nboxes), out, len(out)))
    return _dev.fields(out)


def boo_elapsed_ms():
    """(binning, pass 1, pass 2, summary) of the last call in milliseconds, from the library's event timers; the small
    geometry is one kernel, reported as pass 1."""
    L = _dev.load()
    t = [ctypes.c_float(0.0) for _ in range(4)]
    _dev.chk(L.mw_boo_elapsed_ms(*[ctypes.byref(v) for v in t]))
    return tuple(v.value for v in t)


def bond_order(cells, pos, rc_ang=3.5, threshold=0.5):
    """(q [nboxes, nwater, 4], nn [nboxes, nwater, 2], summary [nboxes, 4]) of the boxes ``cells`` [nboxes, 3, 3] / ``pos``
    [nboxes, nwater, 3] in bohr: q = (q4, q6, qbar4, qbar6), nn = (neighbours within ``rc_ang``, connections with
    s_ij > ``threshold``), summary = (Q4, Q6, <qbar4>, <qbar6>).  One box may come without the leading axis, and then so
    do the results."""
    cells, pos, single = host_boxes(cells, pos)
    L = _dev.live()
    nb, n = pos.shape[0], pos.shape[1]
    q = np.zeros((nb, n, 4))
    nn = np.zeros((nb, n, 2), dtype=np.int32)
    summary = np.zeros((nb, 4))
    _dev.chk(L.mw_boo_compute(nb, n, cells.ctypes.data, pos.ctypes.data, float(rc_ang) / BOHR_TO_ANG, float(threshold),
                              q.ctypes.data, nn.ctypes.data, summary.ctypes.data))
    return (q[0], nn[0], summary[0]) if single else (q, nn, summary)


def bond_order_torch(cells_t, pos_t, rc_ang=3.5, threshold=0.5):
    """(q [nboxes, nwater, 4] float64, nn [nboxes, nwater, 2] int32, summary [nboxes, 4] float64) as tensors on the device
    of the inputs: ``cells_t`` [nboxes, 3, 3] and ``pos_t`` [nboxes, nwater, 3], contiguous float64 device tensors on the
    device the library lives on (mw_boo_compute_device)."""
    import torch
    dev = check_device_tensors((cells_t, torch.float64, "cells_t"), (pos_t, torch.float64, "pos_t"))
    check_boxes(cells_t, pos_t)
    L = _dev.live(dev.index or 0)                  # raises if the library lives on another device
    nb, n = pos_t.shape[0], pos_t.shape[1]
    q = torch.zeros((nb, n, 4), dtype=torch.float64, device=dev)
    nn = torch.zeros((nb, n, 2), dtype=torch.int32, device=dev)
    summary = torch.zeros((nb, 4), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    _dev.chk(L.mw_boo_compute_device(nb, n, cells_t.data_ptr(), pos_t.data_ptr(), float(rc_ang) / BOHR_TO_ANG, float(threshold),
                                     q.data_ptr(), nn.data_ptr(), summary.data_ptr()))
    return q, nn, summary
