"""The O-O-O angle distribution P(theta) over the C ABI of ``libmw_adf.so`` (include/mw_adf.h): per box and group of centre
molecules the integer histogram of cos(theta) between every two of a centre's neighbour entries, the entry count of every
molecule and four totals per box and group.

A cell ``h`` is a [3, 3] array whose ROW k is the lattice vector h_(k+1) (``EnergyModule.hmatrix[b]``, the layout of
``mw_set_cell``), lengths in bohr.  The radius is given in Angstrom and must not exceed the narrowest perpendicular width of
any cell.  The bins are edges in cos(theta), ascending (``adf_edges``); the results are the library's own integers, and
``adf_from_counts`` turns a histogram into densities on the host.  There is no CPU path: without the library or a device the
calls raise.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from ._devlib import DevLib, MwError, check_boxes, check_device_tensors, host_boxes

PKG = os.path.dirname(os.path.abspath(__file__))
ADF_LIB_PATH = os.path.join(PKG, "libmw_adf.so")
BOHR_TO_ANG = 0.5291772108                      # constants.f90:42-43, as energy.py converts
ADF_KEEP = 32                                   # MW_ADF_KEEP: the entries of a centre that take part in its pairs

#: every symbol include/mw_adf.h declares
ADF_ABI_SYMBOLS = ("mw_adf_init", "mw_adf_finalize", "mw_adf_is_initialised", "mw_adf_last_error", "mw_adf_compute",
                   "mw_adf_compute_device", "mw_adf_plan", "mw_adf_last", "mw_adf_elapsed_ms")
#: the fields of mw_adf_plan / mw_adf_last, in order (those of tetrahedral.PLAN_FIELDS)
PLAN_FIELDS = ("boxes_per_chunk", "chunks", "small", "g1", "g2", "g3", "lds_bytes", "scratch_bytes_per_box", "boxes_per_workgroup")


def _argtypes(L):
    for f in (L.mw_adf_compute, L.mw_adf_compute_device):
        f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_int, ctypes.c_void_p,
                      ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.mw_adf_plan.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                              ctypes.POINTER(ctypes.c_int), ctypes.c_int]


_dev = DevLib("adf", ADF_LIB_PATH, "the angle distribution", PLAN_FIELDS, setup=_argtypes)

load_adf_library = _dev.load                     # (path=ADF_LIB_PATH): dlopen libmw_adf.so; raises if it has not been built
adf_finalize = _dev.finalize
adf_last = _dev.last                             # the fields of adf_plan for the last call that launched (the grid is that of its first box)


def adf_init(device=0):
    """Initialise the library on ``device`` (the compute functions do it on device 0 when nobody has)."""
    return _dev.live(device)


def adf_plan(nwater, cell, r_cut_ang=3.5, nbins=90, ngroups=1, nboxes=1):
    """{field: value} of PLAN_FIELDS: the launch rules of ``nboxes`` boxes of ``nwater`` molecules with the cell ``cell``
    [3, 3] (bohr), the radius ``r_cut_ang`` and ``ngroups`` histograms of ``nbins`` bins per box (mw_adf_plan), no device
    needed."""
    L = _dev.load()
    out = _dev.plan_out()
    cell = np.ascontiguousarray(cell, dtype=np.float64)
    if cell.shape != (3, 3):
        raise MwError(f"cell {cell.shape}: expected [3, 3]")
    _dev.chk(L.mw_adf_plan(int(nwater), cell.ctypes.data, float(r_cut_ang) / BOHR_TO_ANG, int(nbins), int(ngroups), int(nboxes), out, len(out)))
    return _dev.fields(out)


def adf_elapsed_ms():
    """(binning, angles, reduce) of the last call in milliseconds, from the library's event timers: the counting sort (0 in the
    small geometry), the angle pass, and the zeroing of the results the angle pass adds into."""
    L = _dev.load()
    t = [ctypes.c_float(0.0) for _ in range(3)]
    _dev.chk(L.mw_adf_elapsed_ms(*[ctypes.byref(v) for v in t]))
    return tuple(v.value for v in t)


def adf_edges(nbins, kind="theta"):
    """[nbins + 1] ascending bin edges in cos(theta).  ``"theta"``: bins uniform in theta over [0, 180] degrees -- edge m is
    cos((nbins - m) 180 / nbins degrees), so bin m holds the angles from 180 (nbins - m) / nbins down to 180 (nbins - m - 1) /
    nbins degrees; ``"cos"``: bins uniform in cos(theta), edge m = -1 + 2 m / nbins.  The end points are exactly -1 and 1."""
    nbins = int(nbins)
    if nbins < 1:
        raise MwError(f"adf_edges: nbins = {nbins} < 1")
    m = np.arange(nbins + 1, dtype=np.float64)
    if kind == "theta":
        e = np.cos((nbins - m) * (np.pi / nbins))
    elif kind == "cos":
        e = -1.0 + 2.0 * m / nbins
    else:
        raise MwError(f"adf_edges: kind = {kind!r} is neither 'theta' nor 'cos'")
    e[0], e[-1] = -1.0, 1.0
    return e


def _edges(edges):
    e = adf_edges(90, "theta") if edges is None else np.ascontiguousarray(edges, dtype=np.float64)
    if e.ndim != 1 or len(e) < 2:
        raise MwError(f"edges {e.shape}: expected [nbins + 1] with nbins >= 1")
    return e


def angle_counts(cells, pos, r_cut_ang=3.5, edges=None, group=None, ngroups=1):
    """(hist [nboxes, ngroups, nbins] int64, counts [nboxes, nwater] int32, summary [nboxes, ngroups, 4] int64) of the boxes
    ``cells`` [nboxes, 3, 3] / ``pos`` [nboxes, nwater, 3] in bohr: hist = the pairs of neighbour entries of the centres of each
    group per bin of cos(theta) (``edges``, default ``adf_edges(90, "theta")``), counts = the entries of every molecule within
    ``r_cut_ang``, summary = (centres, pairs enumerated, pairs binned, centres with more than 32 entries, whose pairs are
    incomplete).  ``group`` [nboxes, nwater] ints: the group of every molecule, -1 for a molecule that is no centre; None:
    every molecule is a centre of group 0.  One box may come without the leading axis, and then so do the results."""
    cells, pos, single = host_boxes(cells, pos)
    e = _edges(edges)
    nb, n, nbins, ngroups = pos.shape[0], pos.shape[1], len(e) - 1, int(ngroups)
    gp = None
    if group is not None:
        group = np.ascontiguousarray(group, dtype=np.int32)
        group = group[None] if single and group.ndim == 1 else group
        if group.shape != (nb, n):
            raise MwError(f"group {group.shape}: expected {(nb, n)}")
        gp = group.ctypes.data
    L = _dev.live()
    hist = np.zeros((nb, max(ngroups, 1), nbins), dtype=np.int64)
    counts = np.zeros((nb, n), dtype=np.int32)
    summary = np.zeros((nb, max(ngroups, 1), 4), dtype=np.int64)
    _dev.chk(L.mw_adf_compute(nb, n, cells.ctypes.data, pos.ctypes.data, float(r_cut_ang) / BOHR_TO_ANG, nbins, e.ctypes.data, ngroups, gp,
                              hist.ctypes.data, counts.ctypes.data, summary.ctypes.data))
    return (hist[0], counts[0], summary[0]) if single else (hist, counts, summary)


def angle_counts_torch(cells_t, pos_t, r_cut_ang=3.5, edges=None, group_t=None, ngroups=1):
    """(hist [nboxes, ngroups, nbins] int64, counts [nboxes, nwater] int32, summary [nboxes, ngroups, 4] int64) as tensors on the
    device of the inputs: ``cells_t`` [nboxes, 3, 3] and ``pos_t`` [nboxes, nwater, 3] contiguous float64 device tensors and
    ``group_t`` None or a contiguous int32 device tensor [nboxes, nwater], on the device the library lives on
    (mw_adf_compute_device).  ``edges`` stays a host array."""
    import torch
    named = [(cells_t, torch.float64, "cells_t"), (pos_t, torch.float64, "pos_t")]
    if group_t is not None:
        named.append((group_t, torch.int32, "group_t"))
    dev = check_device_tensors(*named)
    check_boxes(cells_t, pos_t)
    e = _edges(edges)
    nb, n, nbins, ngroups = pos_t.shape[0], pos_t.shape[1], len(e) - 1, int(ngroups)
    if group_t is not None and tuple(group_t.shape) != (nb, n):
        raise MwError(f"group_t {tuple(group_t.shape)}: expected {(nb, n)}")
    L = _dev.live(dev.index or 0)                  # raises if the library lives on another device
    hist = torch.zeros((nb, max(ngroups, 1), nbins), dtype=torch.int64, device=dev)
    counts = torch.zeros((nb, n), dtype=torch.int32, device=dev)
    summary = torch.zeros((nb, max(ngroups, 1), 4), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    _dev.chk(L.mw_adf_compute_device(nb, n, cells_t.data_ptr(), pos_t.data_ptr(), float(r_cut_ang) / BOHR_TO_ANG, nbins, e.ctypes.data, ngroups,
                                     None if group_t is None else group_t.data_ptr(), hist.data_ptr(), counts.data_ptr(), summary.data_ptr()))
    return hist, counts, summary


def adf_from_counts(hist, edges):
    """(theta_deg [nbins], p_theta [..., nbins], cos_mid [nbins], p_cos [..., nbins]) of histograms ``hist`` [..., nbins] over
    the edges ``edges`` [nbins + 1] in cos(theta): the bin centres in degrees and in cos(theta), and the densities per degree
    and per unit of cos(theta), each normalised to 1 over the binned pairs of its histogram (sum of p_theta x bin width in
    degrees = 1, likewise p_cos); a histogram without pairs gives zeros.  Host arithmetic."""
    hist = np.asarray(hist)
    e = np.asarray(edges, dtype=np.float64)
    if e.ndim != 1 or hist.shape[-1] != len(e) - 1:
        raise MwError(f"hist {hist.shape} / edges {e.shape}: expected [..., nbins] and [nbins + 1]")
    th = np.degrees(np.arccos(np.clip(e, -1.0, 1.0)))                      # descending
    theta_deg, cos_mid = 0.5 * (th[:-1] + th[1:]), 0.5 * (e[:-1] + e[1:])
    dth, dcos = th[:-1] - th[1:], e[1:] - e[:-1]
    total = hist.sum(axis=-1, keepdims=True).astype(np.float64)
    frac = np.divide(hist, total, out=np.zeros(hist.shape, dtype=np.float64), where=total > 0)
    return theta_deg, frac / dth, cos_mid, frac / dcos
