"""Inherent structures over the C ABI of ``libmw_quench.so`` (include/mw_quench.h): every box is moved downhill on the
full-box mW energy at fixed cell by FIRE, from the given positions to the local minimum below them, all boxes of a call at
once on the device and each on its own trajectory.

A cell ``h`` is a [3, 3] array whose ROW k is the lattice vector h_(k+1) (``EnergyModule.hmatrix[b]``, the layout of
``mw_set_cell``).  Everything is in the units of the libraries' arrays: positions and displacements in bohr, energies in
Hartree, forces and ``ftol`` in Hartree / bohr.  The quenched positions are plain positions again (never wrapped: the input
plus the accumulated steps), so they go straight into the other libraries' functions -- ``tetrahedral.tetrahedral_order``
for the LSI of the inherent structure, ``rings.ring_statistics``, ``bondorder.bond_order``.  There is no CPU path: without
the library or a device the calls raise.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from ._devlib import DevLib, MwError, check_boxes, check_device_tensors, host_boxes

PKG = os.path.dirname(os.path.abspath(__file__))
QUENCH_LIB_PATH = os.path.join(PKG, "libmw_quench.so")

#: every symbol include/mw_quench.h declares
QUENCH_ABI_SYMBOLS = ("mw_quench_init", "mw_quench_finalize", "mw_quench_is_initialised", "mw_quench_last_error", "mw_quench_compute",
                      "mw_quench_compute_device", "mw_quench_plan", "mw_quench_last", "mw_quench_elapsed_ms")
#: the fields of mw_quench_plan / mw_quench_last, in order
PLAN_FIELDS = ("boxes_per_chunk", "chunks", "small", "g1", "g2", "g3", "lds_bytes", "scratch_bytes_per_box", "boxes_per_workgroup")
#: FIRE's parameters, in the order of ``fire``, and their defaults (MW_QUENCH_FIRE_DEFAULTS)
FIRE_FIELDS = ("dt0", "dtmax", "maxstep", "alpha0", "f_alpha", "f_inc", "f_dec", "n_min")
FIRE_DEFAULTS = (20.0, 200.0, 0.2, 0.1, 0.99, 1.1, 0.5, 5.0)
#: the columns of ``stats``
STATS_FIELDS = ("e_start", "e_end", "fmax_start", "fmax_end", "max_displacement", "rms_displacement")
MAX_ITER = 1000000


def _argtypes(L):
    for f in (L.mw_quench_compute, L.mw_quench_compute_device):
        f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_int, ctypes.c_void_p,
                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.mw_quench_plan.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int]


_dev = DevLib("quench", QUENCH_LIB_PATH, "the inherent-structure quench", PLAN_FIELDS, setup=_argtypes)

load_quench_library = _dev.load                  # (path=QUENCH_LIB_PATH): dlopen libmw_quench.so; raises if it has not been built
quench_finalize = _dev.finalize
quench_last = _dev.last                          # the fields of quench_plan for the last call that launched (the grid is that of its first box)


def quench_init(device=0):
    """Initialise the library on ``device`` (the compute functions do it on device 0 when nobody has)."""
    return _dev.live(device)


def quench_plan(nwater, cell, nboxes=1):
    """{field: value} of PLAN_FIELDS: the launch rules of ``nboxes`` boxes of ``nwater`` molecules with the cell ``cell``
    [3, 3] (bohr) (mw_quench_plan), no device needed."""
    L = _dev.load()
    out = _dev.plan_out()
    cell = np.ascontiguousarray(cell, dtype=np.float64)
    if cell.shape != (3, 3):
        raise MwError(f"cell {cell.shape}: expected [3, 3]")
    _dev.chk(L.mw_quench_plan(int(nwater), cell.ctypes.data, int(nboxes), out, len(out)))
    return _dev.fields(out)


def quench_elapsed_ms():
    """(sort, moment pass, force pass, step) of the last call in milliseconds, summed over its iterations and chunks, from
    the library's event timers; the small geometry is one kernel, reported as the force pass."""
    L = _dev.load()
    t = [ctypes.c_float(0.0) for _ in range(4)]
    _dev.chk(L.mw_quench_elapsed_ms(*[ctypes.byref(v) for v in t]))
    return tuple(v.value for v in t)


def _fire(fire):
    """None, or the 8 doubles of ``fire``: a sequence in the order of FIRE_FIELDS or a dict over the defaults."""
    if fire is None:
        return None
    if isinstance(fire, dict):
        unknown = set(fire) - set(FIRE_FIELDS)
        if unknown:
            raise MwError(f"fire: unknown parameters {sorted(unknown)} (the parameters are {FIRE_FIELDS})")
        fire = [fire.get(k, d) for k, d in zip(FIRE_FIELDS, FIRE_DEFAULTS)]
    fire = np.ascontiguousarray(fire, dtype=np.float64)
    if fire.shape != (8,):
        raise MwError(f"fire {fire.shape}: expected the 8 numbers {FIRE_FIELDS}")
    return fire


def inherent_structures(cells, pos, ftol=1e-8, max_iter=10000, fire=None):
    """(pos_out [nboxes, nwater, 3], forces [nboxes, nwater, 3], stats [nboxes, 6], iters [nboxes, 2]) of the boxes ``cells``
    [nboxes, 3, 3] / ``pos`` [nboxes, nwater, 3] in bohr: the positions after the quench and the forces there, stats = the
    columns STATS_FIELDS (E at the start and at the end in Hartree, the largest |F| component at the start and at the end,
    the largest and the rms displacement in bohr), iters = (iterations, converged 0 / 1).  A box is converged when its
    largest |F| component is at most ``ftol`` (Hartree / bohr); it stops unconverged after ``max_iter`` iterations, and
    ``max_iter=0`` evaluates E and F at ``pos``.  ``fire``: None for the defaults, or FIRE_FIELDS as a sequence or a dict.
    One box may come without the leading axis, and then so do the results."""
    cells, pos, single = host_boxes(cells, pos)
    fire = _fire(fire)
    L = _dev.live()
    nb, n = pos.shape[0], pos.shape[1]
    pos_out = np.zeros((nb, n, 3))
    forces = np.zeros((nb, n, 3))
    stats = np.zeros((nb, 6))
    iters = np.zeros((nb, 2), dtype=np.int32)
    _dev.chk(L.mw_quench_compute(nb, n, cells.ctypes.data, pos.ctypes.data, float(ftol), int(max_iter), None if fire is None else fire.ctypes.data,
                                 pos_out.ctypes.data, forces.ctypes.data, stats.ctypes.data, iters.ctypes.data))
    return (pos_out[0], forces[0], stats[0], iters[0]) if single else (pos_out, forces, stats, iters)


def inherent_structures_torch(cells_t, pos_t, ftol=1e-8, max_iter=10000, fire=None):
    """(pos_out, forces [nboxes, nwater, 3] float64, stats [nboxes, 6] float64, iters [nboxes, 2] int32) as tensors on the
    device of the inputs: ``cells_t`` [nboxes, 3, 3] and ``pos_t`` [nboxes, nwater, 3], contiguous float64 device tensors on
    the device the library lives on (mw_quench_compute_device); ``fire`` stays on the host."""
    import torch
    dev = check_device_tensors((cells_t, torch.float64, "cells_t"), (pos_t, torch.float64, "pos_t"))
    check_boxes(cells_t, pos_t)
    fire = _fire(fire)
    L = _dev.live(dev.index or 0)                  # raises if the library lives on another device
    nb, n = pos_t.shape[0], pos_t.shape[1]
    pos_out = torch.zeros((nb, n, 3), dtype=torch.float64, device=dev)
    forces = torch.zeros((nb, n, 3), dtype=torch.float64, device=dev)
    stats = torch.zeros((nb, 6), dtype=torch.float64, device=dev)
    iters = torch.zeros((nb, 2), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    _dev.chk(L.mw_quench_compute_device(nb, n, cells_t.data_ptr(), pos_t.data_ptr(), float(ftol), int(max_iter),
                                        None if fire is None else fire.ctypes.data, pos_out.data_ptr(), forces.data_ptr(), stats.data_ptr(),
                                        iters.data_ptr()))
    return pos_out, forces, stats, iters
