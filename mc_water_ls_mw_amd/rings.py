"""Primitive ring statistics of the bond network over the C ABI of ``libmw_rings.so`` (include/mw_rings.h): per box the
primitive (shortest-path) rings of 3 to 7 members, the closed paths they were chosen from, the rings every molecule sits in,
the entry count of every molecule, four totals and, on request, the list of the rings.

A cell ``h`` is a [3, 3] array whose ROW k is the lattice vector h_(k+1) (``EnergyModule.hmatrix[b]``, the layout of
``mw_set_cell``), lengths in bohr.  The radius is given in Angstrom and must not exceed the narrowest perpendicular width of
any cell.  Every result is one of the library's own integers.  There is no CPU path: without the library or a device the
calls raise.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from ._devlib import DevLib, MwError, check_boxes, check_device_tensors, host_boxes

PKG = os.path.dirname(os.path.abspath(__file__))
RINGS_LIB_PATH = os.path.join(PKG, "libmw_rings.so")
BOHR_TO_ANG = 0.5291772108                      # constants.f90:42-43, as energy.py converts
RINGS_DEG = 8                                   # MW_RINGS_DEG: a molecule with more entries has no edges
RING_SIZES = (3, 4, 5, 6, 7)                    # what index 0..4 of hist, closed and member stands for

#: every symbol include/mw_rings.h declares
RINGS_ABI_SYMBOLS = ("mw_rings_init", "mw_rings_finalize", "mw_rings_is_initialised", "mw_rings_last_error", "mw_rings_compute",
                     "mw_rings_compute_device", "mw_rings_plan", "mw_rings_last", "mw_rings_elapsed_ms")
#: the fields of mw_rings_plan / mw_rings_last, in order (those of tetrahedral.PLAN_FIELDS)
PLAN_FIELDS = ("boxes_per_chunk", "chunks", "small", "g1", "g2", "g3", "lds_bytes", "scratch_bytes_per_box", "boxes_per_workgroup")


def _argtypes(L):
    for f in (L.mw_rings_compute, L.mw_rings_compute_device):
        f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_int, ctypes.c_void_p,
                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.mw_rings_plan.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int]


_dev = DevLib("rings", RINGS_LIB_PATH, "the ring statistics", PLAN_FIELDS, setup=_argtypes)

load_rings_library = _dev.load                   # (path=RINGS_LIB_PATH): dlopen libmw_rings.so; raises if it has not been built
rings_finalize = _dev.finalize
rings_last = _dev.last                           # the fields of rings_plan for the last call that launched (the grid is that of its first box)


def rings_init(device=0):
    """Initialise the library on ``device`` (the compute functions do it on device 0 when nobody has)."""
    return _dev.live(device)


def rings_plan(nwater, cell, r_cut_ang=3.5, nboxes=1):
    """{field: value} of PLAN_FIELDS: the launch rules of ``nboxes`` boxes of ``nwater`` molecules with the cell ``cell``
    [3, 3] (bohr) and the radius ``r_cut_ang`` (mw_rings_plan), no device needed."""
    L = _dev.load()
    out = _dev.plan_out()
    cell = np.ascontiguousarray(cell, dtype=np.float64)
    if cell.shape != (3, 3):
        raise MwError(f"cell {cell.shape}: expected [3, 3]")
    _dev.chk(L.mw_rings_plan(int(nwater), cell.ctypes.data, float(r_cut_ang) / BOHR_TO_ANG, int(nboxes), out, len(out)))
    return _dev.fields(out)


def rings_elapsed_ms():
    """(binning, adjacency, walk) of the last call in milliseconds, from the library's event timers: the counting sort (0 in
    the small geometry), the entries and the sorted rows, and the walk with the zeroing of its results (and, where a list
    was asked for, the scan and the second walk)."""
    L = _dev.load()
    t = [ctypes.c_float(0.0) for _ in range(3)]
    _dev.chk(L.mw_rings_elapsed_ms(*[ctypes.byref(v) for v in t]))
    return tuple(v.value for v in t)


def _list_cap(list_cap):
    list_cap = int(list_cap)
    if list_cap < 0:
        raise MwError(f"list_cap = {list_cap} is negative")
    return list_cap


def ring_statistics(cells, pos, r_cut_ang=3.5, list_cap=0):
    """(hist [nboxes, 5] int64, closed [nboxes, 5] int64, member [nboxes, nwater, 5] int32, counts [nboxes, nwater] int32,
    summary [nboxes, 4] int64, list [nboxes, list_cap, 8] int32) of the boxes ``cells`` [nboxes, 3, 3] / ``pos``
    [nboxes, nwater, 3] in bohr: hist = the primitive rings of 3 ... 7 members (RING_SIZES) of the network of the bonds shorter
    than ``r_cut_ang`` between molecules of at most 8 such bonds, closed = the closed paths before the shortest-path test,
    member = the ring nodes of each size that are images of the molecule, counts = the entries of every molecule, summary =
    (molecules over the cap, undirected edges per cell, primitive rings that took the comparison of all readings, primitive
    rings of all sizes), list = one row (L, m_0 ... m_6) per primitive ring up to ``list_cap`` rows, -1 elsewhere.  One box
    may come without the leading axis, and then so do the results."""
    cells, pos, single = host_boxes(cells, pos)
    list_cap = _list_cap(list_cap)
    nb, n = pos.shape[0], pos.shape[1]
    L = _dev.live()
    hist, closed = np.zeros((nb, 5), dtype=np.int64), np.zeros((nb, 5), dtype=np.int64)
    member, counts = np.zeros((nb, n, 5), dtype=np.int32), np.zeros((nb, n), dtype=np.int32)
    summary, rings = np.zeros((nb, 4), dtype=np.int64), np.full((nb, list_cap, 8), -1, dtype=np.int32)
    _dev.chk(L.mw_rings_compute(nb, n, cells.ctypes.data, pos.ctypes.data, float(r_cut_ang) / BOHR_TO_ANG, list_cap, hist.ctypes.data,
                                closed.ctypes.data, member.ctypes.data, counts.ctypes.data, summary.ctypes.data,
                                rings.ctypes.data if list_cap else None))
    out = (hist, closed, member, counts, summary, rings)
    return tuple(o[0] for o in out) if single else out


def ring_statistics_torch(cells_t, pos_t, r_cut_ang=3.5, list_cap=0):
    """The six results of ``ring_statistics`` as tensors on the device of the inputs: ``cells_t`` [nboxes, 3, 3] and ``pos_t``
    [nboxes, nwater, 3] contiguous float64 device tensors on the device the library lives on (mw_rings_compute_device)."""
    import torch
    dev = check_device_tensors((cells_t, torch.float64, "cells_t"), (pos_t, torch.float64, "pos_t"))
    check_boxes(cells_t, pos_t)
    list_cap = _list_cap(list_cap)
    nb, n = pos_t.shape[0], pos_t.shape[1]
    L = _dev.live(dev.index or 0)                  # raises if the library lives on another device
    hist, closed = torch.zeros((nb, 5), dtype=torch.int64, device=dev), torch.zeros((nb, 5), dtype=torch.int64, device=dev)
    member, counts = torch.zeros((nb, n, 5), dtype=torch.int32, device=dev), torch.zeros((nb, n), dtype=torch.int32, device=dev)
    summary = torch.zeros((nb, 4), dtype=torch.int64, device=dev)
    rings = torch.full((nb, list_cap, 8), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    _dev.chk(L.mw_rings_compute_device(nb, n, cells_t.data_ptr(), pos_t.data_ptr(), float(r_cut_ang) / BOHR_TO_ANG, list_cap, hist.data_ptr(),
                                       closed.data_ptr(), member.data_ptr(), counts.data_ptr(), summary.data_ptr(),
                                       rings.data_ptr() if list_cap else None))
    return hist, closed, member, counts, summary, rings
