"""Tetrahedral order, fifth-neighbour distance and local structure index over the C ABI of ``libmw_tet.so``
(include/mw_tet.h): per molecule the Errington-Debenedetti q, the Chau-Hardwick S_k, d5 and the LSI, the indices of its four
nearest neighbours and the entry counts within the two radii; per box the means over the molecules where each is defined.

A cell ``h`` is a [3, 3] array whose ROW k is the lattice vector h_(k+1) (``EnergyModule.hmatrix[b]``, the layout of
``mw_set_cell``), lengths in bohr.  The two radii are given in Angstrom; the search radius must not exceed the narrowest
perpendicular width of any cell.  The results are the library's own numbers -- d5 in bohr, the LSI in bohr^2
(``BOHR_TO_ANG`` converts) -- so that the host and the device entry stay comparable bit for bit.  A value that is not
defined (fewer than four, five or n_lsi + 1 entries) is NaN.  There is no CPU path: without the library or a device the
calls raise.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from ._devlib import DevLib, MwError, check_boxes, check_device_tensors, host_boxes

PKG = os.path.dirname(os.path.abspath(__file__))
TET_LIB_PATH = os.path.join(PKG, "libmw_tet.so")
BOHR_TO_ANG = 0.5291772108                      # constants.f90:42-43, as energy.py converts

#: every symbol include/mw_tet.h declares
TET_ABI_SYMBOLS = ("mw_tet_init", "mw_tet_finalize", "mw_tet_is_initialised", "mw_tet_last_error", "mw_tet_compute",
                   "mw_tet_compute_device", "mw_tet_plan", "mw_tet_last", "mw_tet_elapsed_ms")
#: the fields of mw_tet_plan / mw_tet_last, in order
PLAN_FIELDS = ("boxes_per_chunk", "chunks", "small", "g1", "g2", "g3", "lds_bytes", "scratch_bytes_per_box", "boxes_per_workgroup")


def _argtypes(L):
    for f in (L.mw_tet_compute, L.mw_tet_compute_device):
        f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_double,
                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.mw_tet_plan.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int]


_dev = DevLib("tet", TET_LIB_PATH, "tetrahedral order", PLAN_FIELDS, setup=_argtypes)

load_tet_library = _dev.load                     # (path=TET_LIB_PATH): dlopen libmw_tet.so; raises if it has not been built
tet_finalize = _dev.finalize
tet_last = _dev.last                             # the fields of tet_plan for the last call that launched (the grid is that of its first box)


def tet_init(device=0):
    """Initialise the library on ``device`` (the compute functions do it on device 0 when nobody has)."""
    return _dev.live(device)


def tet_plan(nwater, cell, r_search_ang=5.5, nboxes=1):
    """{field: value} of PLAN_FIELDS: the launch rules of ``nboxes`` boxes of ``nwater`` molecules with the cell ``cell``
    [3, 3] (bohr) and the search radius ``r_search_ang`` (mw_tet_plan), no device needed."""
    L = _dev.load()
    out = _dev.plan_out()
    cell = np.ascontiguousarray(cell, dtype=np.float64)
    if cell.shape != (3, 3):
        raise MwError(f"cell {cell.shape}: expected [3, 3]")
    _dev.chk(L.mw_tet_plan(int(nwater), cell.ctypes.data, float(r_search_ang) / BOHR_TO_ANG, int(nboxes), out, len(out)))
    return _dev.fields(out)


def tet_elapsed_ms():
    """(binning, selection, summary) of the last call in milliseconds, from the library's event timers; the small geometry
    is one kernel, reported as the selection."""
    L = _dev.load()
    t = [ctypes.c_float(0.0) for _ in range(3)]
    _dev.chk(L.mw_tet_elapsed_ms(*[ctypes.byref(v) for v in t]))
    return tuple(v.value for v in t)


def tetrahedral_order(cells, pos, r_search_ang=5.5, r_lsi_ang=3.7):
    """(order [nboxes, nwater, 4], near [nboxes, nwater, 4], counts [nboxes, nwater, 2], summary [nboxes, 8]) of the boxes
    ``cells`` [nboxes, 3, 3] / ``pos`` [nboxes, nwater, 3] in bohr: order = (q, s_k, d5 in bohr, lsi in bohr^2), near = the
    indices of the four nearest neighbours (-1 where there are fewer), counts = (entries within ``r_search_ang``, within
    ``r_lsi_ang``), summary = the means of the four over the molecules where each is defined, then how many those are.  One
    box may come without the leading axis, and then so do the results."""
    cells, pos, single = host_boxes(cells, pos)
    L = _dev.live()
    nb, n = pos.shape[0], pos.shape[1]
    order = np.zeros((nb, n, 4))
    near = np.zeros((nb, n, 4), dtype=np.int32)
    counts = np.zeros((nb, n, 2), dtype=np.int32)
    summary = np.zeros((nb, 8))
    _dev.chk(L.mw_tet_compute(nb, n, cells.ctypes.data, pos.ctypes.data, float(r_search_ang) / BOHR_TO_ANG, float(r_lsi_ang) / BOHR_TO_ANG,
                              order.ctypes.data, near.ctypes.data, counts.ctypes.data, summary.ctypes.data))
    return (order[0], near[0], counts[0], summary[0]) if single else (order, near, counts, summary)


def tetrahedral_order_torch(cells_t, pos_t, r_search_ang=5.5, r_lsi_ang=3.7):
    """(order [nboxes, nwater, 4] float64, near [nboxes, nwater, 4] int32, counts [nboxes, nwater, 2] int32, summary
    [nboxes, 8] float64) as tensors on the device of the inputs: ``cells_t`` [nboxes, 3, 3] and ``pos_t`` [nboxes, nwater, 3],
    contiguous float64 device tensors on the device the library lives on (mw_tet_compute_device)."""
    import torch
    dev = check_device_tensors((cells_t, torch.float64, "cells_t"), (pos_t, torch.float64, "pos_t"))
    check_boxes(cells_t, pos_t)
    L = _dev.live(dev.index or 0)                  # raises if the library lives on another device
    nb, n = pos_t.shape[0], pos_t.shape[1]
    order = torch.zeros((nb, n, 4), dtype=torch.float64, device=dev)
    near = torch.zeros((nb, n, 4), dtype=torch.int32, device=dev)
    counts = torch.zeros((nb, n, 2), dtype=torch.int32, device=dev)
    summary = torch.zeros((nb, 8), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    _dev.chk(L.mw_tet_compute_device(nb, n, cells_t.data_ptr(), pos_t.data_ptr(), float(r_search_ang) / BOHR_TO_ANG,
                                     float(r_lsi_ang) / BOHR_TO_ANG, order.data_ptr(), near.data_ptr(), counts.data_ptr(), summary.data_ptr()))
    return order, near, counts, summary
