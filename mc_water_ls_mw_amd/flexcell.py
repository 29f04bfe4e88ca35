"""Molecular dynamics at constant pressure with a cell whose Cartesian axes move on their own, over the C ABI of
``libmw_flex.so`` (include/mw_flex.h): the BAOAB step of ``dynamics`` with the cell of every box as part of its state, a per-axis
stochastic-cell-rescaling barostat every ``baro_every`` steps, and the pressure tensor in every trace row -- all boxes of a call
at once on the device and each on its own trajectory, cell and noise stream.

Layouts, units and defaults are those of ``npt``: a cell ``h`` is a [3, 3] array whose ROW k is the lattice vector h_(k+1), so
the barostat scales its COLUMNS; bohr, Hartree, atomic time units, electron masses; ``pressure`` in Hartree / bohr^3.
``coupling`` names the groups of axes that share a scale factor (``COUPLINGS``): "iso" (the stage of ``npt``, byte for byte),
"aniso" (x, y and z each on its own: the shape of a crystal), "semi" (the two axes other than ``axis`` together, ``axis`` on its
own: slabs) and "uniaxial" (``axis`` alone, the other two fixed: direct coexistence).  The results go straight back in as in
``npt``.  There is no CPU path: without the library or a device the calls raise.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from ._devlib import DevLib, MwError, check_boxes, check_device_tensors, host_boxes
from .dynamics import MASS_WATER, PLAN_FIELDS, _like_pos, _nrows, _streams
from .npt import ATM, BETA_T_DEFAULT, TAU_P_DEFAULT

PKG = os.path.dirname(os.path.abspath(__file__))
FLEX_LIB_PATH = os.path.join(PKG, "libmw_flex.so")

#: every symbol include/mw_flex.h declares
FLEX_ABI_SYMBOLS = ("mw_flex_init", "mw_flex_finalize", "mw_flex_is_initialised", "mw_flex_last_error", "mw_flex_run", "mw_flex_run_device",
                    "mw_flex_plan", "mw_flex_last", "mw_flex_elapsed_ms")
#: the columns of ``trace``
TRACE_FIELDS = ("potential_energy", "kinetic_energy", "mean_squared_displacement", "fmax", "volume", "pressure", "p_xx", "p_yy", "p_zz", "p_xy",
                "p_xz", "p_yz", "length_1", "length_2", "length_3")
#: the values of ``coupling`` (MW_FLEX_ISO, MW_FLEX_ANISO, MW_FLEX_SEMI, MW_FLEX_UNIAXIAL)
COUPLINGS = {"iso": 0, "aniso": 1, "semi": 2, "uniaxial": 3}
MAX_STEPS = 100000000
#: the largest |change of ln V| of one application in coupling "iso" (MW_FLEX_MAX_DLNV)
MAX_DLNV = 0.3
#: the largest |change of the logarithm of a length| of one application in the other couplings (MW_FLEX_MAX_DLNL)
MAX_DLNL = 0.1

_u64 = ctypes.c_ulonglong


def _argtypes(L):
    for f in (L.mw_flex_run, L.mw_flex_run_device):
        f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _u64, _u64,
                      ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                      ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.mw_flex_plan.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int]


_dev = DevLib("flex", FLEX_LIB_PATH, "molecular dynamics at constant pressure with a per-axis cell", PLAN_FIELDS, setup=_argtypes)

load_flex_library = _dev.load                    # (path=FLEX_LIB_PATH): dlopen libmw_flex.so; raises if it has not been built
flex_finalize = _dev.finalize
flex_last = _dev.last                            # the fields of flex_plan for the last call that launched (the grid is that of its first box's input cell)


def flex_init(device=0):
    """Initialise the library on ``device`` (the run functions do it on device 0 when nobody has)."""
    return _dev.live(device)


def flex_plan(nwater, cell, nboxes=1):
    """{field: value} of dynamics.PLAN_FIELDS: the launch rules of ``nboxes`` boxes of ``nwater`` molecules with the cell ``cell``
    [3, 3] (bohr) (mw_flex_plan), no device needed."""
    L = _dev.load()
    out = _dev.plan_out()
    cell = np.ascontiguousarray(cell, dtype=np.float64)
    if cell.shape != (3, 3):
        raise MwError(f"cell {cell.shape}: expected [3, 3]")
    _dev.chk(L.mw_flex_plan(int(nwater), cell.ctypes.data, int(nboxes), out, len(out)))
    return _dev.fields(out)


def flex_elapsed_ms():
    """(sort, moment pass, force pass, drift, barostat) of the last call in milliseconds, summed over its steps and chunks, from
    the library's event timers; the small geometry's step kernel is reported as the force pass."""
    L = _dev.load()
    t = [ctypes.c_float(0.0) for _ in range(5)]
    _dev.chk(L.mw_flex_elapsed_ms(*[ctypes.byref(v) for v in t]))
    return tuple(v.value for v in t)


def _coupling(coupling):
    if isinstance(coupling, str):
        if coupling not in COUPLINGS:
            raise MwError(f"coupling {coupling!r}: expected one of {sorted(COUPLINGS)} or 0..3")
        return COUPLINGS[coupling]
    return int(coupling)


def molecular_dynamics_flex(cells, pos, nsteps, dt, pressure=ATM, kT=0.0, gamma=0.0, tau_p=TAU_P_DEFAULT, beta_T=BETA_T_DEFAULT, baro_every=10,
                            coupling="aniso", axis=2, vel=None, mass=MASS_WATER, seed=0, streams=None, step0=0, sample_every=1, pos_ref=None):
    """(pos_out, vel_out, forces [nboxes, nwater, 3], cells_out [nboxes, 3, 3], ref_out [nboxes, nwater, 3], trace [nboxes,
    nsteps // sample_every + 1, 15], status [nboxes, 2]) of the boxes ``cells`` [nboxes, 3, 3] / ``pos`` [nboxes, nwater, 3]
    after ``nsteps`` BAOAB steps of ``dt`` with the per-axis barostat at ``pressure`` applied after every ``baro_every``-th step
    (0: never).  ``coupling`` is a key of COUPLINGS or its number, ``axis`` 0, 1 or 2 the Cartesian axis that "semi" and
    "uniaxial" single out.  trace = the columns TRACE_FIELDS: those of ``npt``, the pressure tensor P_xx, P_yy, P_zz, P_xy, P_xz,
    P_yz (Hartree / bohr^3; see :func:`pressure_tensor`) and the lengths of the three cell vectors (bohr); status = (steps
    completed, 0 / 1: frozen by the drift guard / 2: frozen by the barostat guard -- a change of the logarithm of a length beyond
    MAX_DLNL, of ln V beyond MAX_DLNV in coupling "iso", or a cell narrower than the cutoff -- at the state before that
    application): results, not errors.  The other keywords are those of npt.molecular_dynamics_npt.  One box may come without
    the leading axis, and then so do the results."""
    cells, pos, single = host_boxes(cells, pos)
    vel = _like_pos(vel, pos, single, "vel")
    pos_ref = _like_pos(pos_ref, pos, single, "pos_ref")
    nb, n = pos.shape[0], pos.shape[1]
    streams = _streams(streams, nb)
    coupling = _coupling(coupling)
    L = _dev.live()
    pos_out, vel_out, forces, ref_out = (np.zeros((nb, n, 3)) for _ in range(4))
    cells_out = np.zeros((nb, 3, 3))
    trace = np.zeros((nb, _nrows(nsteps, sample_every), len(TRACE_FIELDS)))
    status = np.zeros((nb, 2), dtype=np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data                   # noqa: E731
    _dev.chk(L.mw_flex_run(nb, n, cells.ctypes.data, pos.ctypes.data, ptr(vel), ptr(pos_ref), ptr(streams), int(seed), int(step0), int(nsteps),
                           int(sample_every), float(dt), float(mass), float(kT), float(gamma), float(pressure), float(tau_p), float(beta_T),
                           int(baro_every), coupling, int(axis), pos_out.ctypes.data, vel_out.ctypes.data, forces.ctypes.data, cells_out.ctypes.data,
                           ref_out.ctypes.data, trace.ctypes.data, status.ctypes.data))
    out = (pos_out, vel_out, forces, cells_out, ref_out, trace, status)
    return tuple(o[0] for o in out) if single else out


def molecular_dynamics_flex_torch(cells_t, pos_t, nsteps, dt, pressure=ATM, kT=0.0, gamma=0.0, tau_p=TAU_P_DEFAULT, beta_T=BETA_T_DEFAULT,
                                  baro_every=10, coupling="aniso", axis=2, vel_t=None, mass=MASS_WATER, seed=0, streams_t=None, step0=0,
                                  sample_every=1, pos_ref_t=None):
    """The same seven results as tensors on the device of the inputs: ``cells_t`` [nboxes, 3, 3], ``pos_t`` and the optional
    ``vel_t`` and ``pos_ref_t`` [nboxes, nwater, 3] are contiguous float64 device tensors on the device the library lives on,
    ``streams_t`` [nboxes] an int64 device tensor holding the 64-bit stream identities (mw_flex_run_device)."""
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
    coupling = _coupling(coupling)
    L = _dev.live(dev.index or 0)                  # raises if the library lives on another device
    f64 = dict(dtype=torch.float64, device=dev)
    pos_out, vel_out, forces, ref_out = (torch.zeros((nb, n, 3), **f64) for _ in range(4))
    cells_out = torch.zeros((nb, 3, 3), **f64)
    trace = torch.zeros((nb, _nrows(nsteps, sample_every), len(TRACE_FIELDS)), **f64)
    status = torch.zeros((nb, 2), dtype=torch.int32, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()                    # noqa: E731
    torch.cuda.synchronize(dev)
    _dev.chk(L.mw_flex_run_device(nb, n, cells_t.data_ptr(), pos_t.data_ptr(), ptr(vel_t), ptr(pos_ref_t), ptr(streams_t), int(seed), int(step0),
                                  int(nsteps), int(sample_every), float(dt), float(mass), float(kT), float(gamma), float(pressure), float(tau_p),
                                  float(beta_T), int(baro_every), coupling, int(axis), pos_out.data_ptr(), vel_out.data_ptr(), forces.data_ptr(),
                                  cells_out.data_ptr(), ref_out.data_ptr(), trace.data_ptr(), status.data_ptr()))
    return pos_out, vel_out, forces, cells_out, ref_out, trace, status


# ---- host read-outs of a trace --------------------------------------------------------------------------------------------
def pressure_tensor(trace):
    """[..., 3, 3]: the symmetric pressure tensor of every row of ``trace`` [..., 15] (Hartree / bohr^3)."""
    t = np.asarray(trace, dtype=np.float64)
    if t.shape[-1] != len(TRACE_FIELDS):
        raise MwError(f"trace {t.shape}: expected {len(TRACE_FIELDS)} columns")
    xx, yy, zz, xy, xz, yz = (t[..., 6 + k] for k in range(6))
    return np.stack([np.stack([xx, xy, xz], axis=-1), np.stack([xy, yy, yz], axis=-1), np.stack([xz, yz, zz], axis=-1)], axis=-2)


def surface_tension(trace, axis=2, interfaces=2):
    """[...]: L_c (P_cc - (P_aa + P_bb) / 2) / ``interfaces`` of every row of ``trace`` [..., 15], for a cell whose vector c =
    ``axis`` lies along the Cartesian axis ``axis`` and a slab with ``interfaces`` faces normal to it (Hartree / bohr^2).  As
    the rows define it, P_cc is the normal pressure; the sign is that of this formula."""
    t = np.asarray(trace, dtype=np.float64)
    if t.shape[-1] != len(TRACE_FIELDS):
        raise MwError(f"trace {t.shape}: expected {len(TRACE_FIELDS)} columns")
    c = int(axis)
    if c not in (0, 1, 2):
        raise MwError(f"axis = {axis}: expected 0, 1 or 2")
    a, b = (c + 1) % 3, (c + 2) % 3
    return t[..., 12 + c] * (t[..., 6 + c] - 0.5 * (t[..., 6 + a] + t[..., 6 + b])) / float(interfaces)
