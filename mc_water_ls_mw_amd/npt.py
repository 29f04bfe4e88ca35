"""Molecular dynamics at constant pressure over the C ABI of ``libmw_npt.so`` (include/mw_npt.h): the BAOAB step of
``dynamics`` with the cell of every box as part of its state -- an isotropic stochastic-cell-rescaling barostat in ln V scales
cell, positions and velocities every ``baro_every`` steps --, all boxes of a call at once on the device and each on its own
trajectory, cell and noise stream.

Layouts and units are those of ``dynamics``: a cell ``h`` is a [3, 3] array whose ROW k is the lattice vector h_(k+1); bohr,
Hartree, atomic time units, electron masses.  ``pressure`` is in Hartree / bohr^3 (``ATM`` is one atmosphere, ``PASCAL`` one
pascal), ``tau_p`` in atomic time units (``TAU_P_DEFAULT``, one picosecond), ``beta_T`` in bohr^3 / Hartree
(``BETA_T_DEFAULT``, the 4.5e-10 / Pa of liquid water near 300 K; the barostat's stationary state does not depend on it, only
its speed).  The results go straight back in: ``cells_out`` as ``cells``, ``pos_out`` as ``pos``, ``vel_out`` as ``vel``,
``ref_out`` as ``pos_ref`` and ``step0`` advanced by the steps done continue a run byte for byte.  There is no CPU path:
without the library or a device the calls raise.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from ._devlib import DevLib, MwError, check_boxes, check_device_tensors, host_boxes
from .dynamics import FS, KELVIN, MASS_WATER, PLAN_FIELDS, _like_pos, _nrows, _streams

PKG = os.path.dirname(os.path.abspath(__file__))
NPT_LIB_PATH = os.path.join(PKG, "libmw_npt.so")

#: every symbol include/mw_npt.h declares
NPT_ABI_SYMBOLS = ("mw_npt_init", "mw_npt_finalize", "mw_npt_is_initialised", "mw_npt_last_error", "mw_npt_run", "mw_npt_run_device", "mw_npt_plan",
                   "mw_npt_last", "mw_npt_elapsed_ms")
#: the columns of ``trace``
TRACE_FIELDS = ("potential_energy", "kinetic_energy", "mean_squared_displacement", "fmax", "volume", "pressure")
#: Hartree / bohr^3 per pascal (one Hartree / bohr^3 is 2.9421015697e13 Pa)
PASCAL = 1.0 / 2.9421015697e13
#: Hartree / bohr^3 per standard atmosphere
ATM = 101325.0 * PASCAL
#: the barostat's time constant: one picosecond
TAU_P_DEFAULT = 1000.0 * FS
#: the isothermal compressibility the barostat assumes: 4.5e-10 / Pa, liquid water near 300 K, in bohr^3 / Hartree
BETA_T_DEFAULT = 4.5e-10 / PASCAL
MAX_STEPS = 100000000
#: the largest |change of ln V| of one application (MW_NPT_MAX_DLNV)
MAX_DLNV = 0.3

_u64 = ctypes.c_ulonglong


def _argtypes(L):
    for f in (L.mw_npt_run, L.mw_npt_run_device):
        f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _u64, _u64,
                      ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                      ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.mw_npt_plan.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int]


_dev = DevLib("npt", NPT_LIB_PATH, "molecular dynamics at constant pressure", PLAN_FIELDS, setup=_argtypes)

load_npt_library = _dev.load                     # (path=NPT_LIB_PATH): dlopen libmw_npt.so; raises if it has not been built
npt_finalize = _dev.finalize
npt_last = _dev.last                             # the fields of npt_plan for the last call that launched (the grid is that of its first box's input cell)


def npt_init(device=0):
    """Initialise the library on ``device`` (the run functions do it on device 0 when nobody has)."""
    return _dev.live(device)


def npt_plan(nwater, cell, nboxes=1):
    """{field: value} of dynamics.PLAN_FIELDS: the launch rules of ``nboxes`` boxes of ``nwater`` molecules with the cell ``cell``
    [3, 3] (bohr) (mw_npt_plan), no device needed."""
    L = _dev.load()
    out = _dev.plan_out()
    cell = np.ascontiguousarray(cell, dtype=np.float64)
    if cell.shape != (3, 3):
        raise MwError(f"cell {cell.shape}: expected [3, 3]")
    _dev.chk(L.mw_npt_plan(int(nwater), cell.ctypes.data, int(nboxes), out, len(out)))
    return _dev.fields(out)


def npt_elapsed_ms():
    """(sort, moment pass, force pass, drift, barostat) of the last call in milliseconds, summed over its steps and chunks, from
    the library's event timers; the small geometry's step kernel is reported as the force pass."""
    L = _dev.load()
    t = [ctypes.c_float(0.0) for _ in range(5)]
    _dev.chk(L.mw_npt_elapsed_ms(*[ctypes.byref(v) for v in t]))
    return tuple(v.value for v in t)


def molecular_dynamics_npt(cells, pos, nsteps, dt, pressure=ATM, kT=0.0, gamma=0.0, tau_p=TAU_P_DEFAULT, beta_T=BETA_T_DEFAULT, baro_every=10,
                           vel=None, mass=MASS_WATER, seed=0, streams=None, step0=0, sample_every=1, pos_ref=None):
    """(pos_out, vel_out, forces [nboxes, nwater, 3], cells_out [nboxes, 3, 3], ref_out [nboxes, nwater, 3], trace [nboxes,
    nsteps // sample_every + 1, 6], status [nboxes, 2]) of the boxes ``cells`` [nboxes, 3, 3] / ``pos`` [nboxes, nwater, 3]
    after ``nsteps`` BAOAB steps of ``dt`` with the barostat at ``pressure`` applied after every ``baro_every``-th step (0:
    never; the results are then those of dynamics.molecular_dynamics byte for byte).  trace = the columns TRACE_FIELDS: those
    of dynamics, then the volume (bohr^3) and the pressure (2 K + W) / (3 V) (Hartree / bohr^3); status = (steps completed,
    0 / 1: frozen by the drift guard / 2: frozen by the barostat guard -- a change of ln V beyond MAX_DLNV, or a cell narrower
    than the cutoff -- at the state before that application): results, not errors.  ``ref_out`` is ``pos_ref`` (None: ``pos``)
    scaled as the cell was.  The other keywords are those of dynamics.molecular_dynamics; the barostat's noise comes from the
    box's stream too, and with ``kT=0`` there is none.  One box may come without the leading axis, and then so do the
    results."""
    cells, pos, single = host_boxes(cells, pos)
    vel = _like_pos(vel, pos, single, "vel")
    pos_ref = _like_pos(pos_ref, pos, single, "pos_ref")
    nb, n = pos.shape[0], pos.shape[1]
    streams = _streams(streams, nb)
    L = _dev.live()
    pos_out, vel_out, forces, ref_out = (np.zeros((nb, n, 3)) for _ in range(4))
    cells_out = np.zeros((nb, 3, 3))
    trace = np.zeros((nb, _nrows(nsteps, sample_every), len(TRACE_FIELDS)))
    status = np.zeros((nb, 2), dtype=np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data                   # noqa: E731
    _dev.chk(L.mw_npt_run(nb, n, cells.ctypes.data, pos.ctypes.data, ptr(vel), ptr(pos_ref), ptr(streams), int(seed), int(step0), int(nsteps),
                          int(sample_every), float(dt), float(mass), float(kT), float(gamma), float(pressure), float(tau_p), float(beta_T),
                          int(baro_every), pos_out.ctypes.data, vel_out.ctypes.data, forces.ctypes.data, cells_out.ctypes.data, ref_out.ctypes.data,
                          trace.ctypes.data, status.ctypes.data))
    out = (pos_out, vel_out, forces, cells_out, ref_out, trace, status)
    return tuple(o[0] for o in out) if single else out


def molecular_dynamics_npt_torch(cells_t, pos_t, nsteps, dt, pressure=ATM, kT=0.0, gamma=0.0, tau_p=TAU_P_DEFAULT, beta_T=BETA_T_DEFAULT,
                                 baro_every=10, vel_t=None, mass=MASS_WATER, seed=0, streams_t=None, step0=0, sample_every=1, pos_ref_t=None):
    """The same seven results as tensors on the device of the inputs: ``cells_t`` [nboxes, 3, 3], ``pos_t`` and the optional
    ``vel_t`` and ``pos_ref_t`` [nboxes, nwater, 3] are contiguous float64 device tensors on the device the library lives on,
    ``streams_t`` [nboxes] an int64 device tensor holding the 64-bit stream identities (mw_npt_run_device)."""
    import torch
    named = [(cells_t, torch.float64, "cells_t"), (pos_t, torch.float64, "pos_t")]
    named += [(t, torch.float64, name) for t, name in ((vel_t, "vel_t"), (pos_ref_t, "pos_ref_t")) if t is not None]
    if streams_t is not None:
        named.append((streams_t, torch.int64, "streams_t"))
    dev = check_device_tensors(*named)
    check_boxes(cells_t, pos_t)
    nb, n = pos_t.shape[0], pos_t.shape[1]
    for t, name in ((vel_t, "vel_t"), (pos_ref_t, "pos_ref_t")):
        if t is not None and tuple(t.shape) != tuple(pos_t.shape):
            raise MwError(f"{name} {tuple(t.shape)}: expected the shape of pos_t, {tuple(pos_t.shape)}")
    if streams_t is not None and tuple(streams_t.shape) != (nb,):
        raise MwError(f"streams_t {tuple(streams_t.shape)}: expected one 64-bit stream identity per box, [{nb}]")
    L = _dev.live(dev.index or 0)                  # raises if the library lives on another device
    f64 = dict(dtype=torch.float64, device=dev)
    pos_out, vel_out, forces, ref_out = (torch.zeros((nb, n, 3), **f64) for _ in range(4))
    cells_out = torch.zeros((nb, 3, 3), **f64)
    trace = torch.zeros((nb, _nrows(nsteps, sample_every), len(TRACE_FIELDS)), **f64)
    status = torch.zeros((nb, 2), dtype=torch.int32, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()                    # noqa: E731
    torch.cuda.synchronize(dev)
    _dev.chk(L.mw_npt_run_device(nb, n, cells_t.data_ptr(), pos_t.data_ptr(), ptr(vel_t), ptr(pos_ref_t), ptr(streams_t), int(seed), int(step0),
                                 int(nsteps), int(sample_every), float(dt), float(mass), float(kT), float(gamma), float(pressure), float(tau_p),
                                 float(beta_T), int(baro_every), pos_out.data_ptr(), vel_out.data_ptr(), forces.data_ptr(), cells_out.data_ptr(),
                                 ref_out.data_ptr(), trace.data_ptr(), status.data_ptr()))
    return pos_out, vel_out, forces, cells_out, ref_out, trace, status
