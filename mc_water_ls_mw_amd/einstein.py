"""Einstein-crystal thermodynamic integration (Frenkel-Ladd) over the C ABI of ``libmw_ti.so`` (include/mw_ti.h): every box is
moved by the BAOAB step of ``dynamics`` on the mixed energy

    U_lambda(x) = (1 - lambda) E_mW(x) + lambda 1/2 k sum_i |x_i - s_i|^2

with a ``lambda``, a spring ``k`` (Hartree / bohr^2) and Einstein sites ``s`` of its own, and the block averages of the five trace
columns are taken on the device at every step.  A lambda-integration is 10 - 20 independent boxes per lattice: one call
integrates them all.  The host arithmetic of the integration (:func:`gauss_legendre`, :func:`integrand`,
:func:`einstein_free_energy`, :func:`frenkel_ladd`, :func:`spring_from_msd`) is numpy and needs neither the library nor a
device; the runs have no CPU path: without the library or a device they raise.

Units and the layout of cells are those of ``dynamics``.  The free energy of the mW crystal at lambda = 0 is

    F = F_E - integral_0^1 <U_E' - E_mW>_lambda d lambda,

with U_E' = 1/2 k N (f2 - f4) the spring energy without the centre of mass (trace columns 2 and 4) and F_E the classical free
energy of 3 (N - 1) oscillators: the centre of mass factorises exactly (E_mW is translation invariant, the springs are equal)
and is the same for two lattices of equal N, so it is left out on both sides -- the convention of
``phonons.harmonic_free_energy`` with its three translations dropped, to which F - E_min is directly comparable.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from ._devlib import DevLib, MwError, check_boxes, check_device_tensors, host_boxes
from .dynamics import MASS_WATER, PLAN_FIELDS, _like_pos, _nrows, _streams

PKG = os.path.dirname(os.path.abspath(__file__))
TI_LIB_PATH = os.path.join(PKG, "libmw_ti.so")

#: every symbol include/mw_ti.h declares
TI_ABI_SYMBOLS = ("mw_ti_init", "mw_ti_finalize", "mw_ti_is_initialised", "mw_ti_last_error", "mw_ti_run", "mw_ti_run_device", "mw_ti_plan",
                  "mw_ti_last", "mw_ti_elapsed_ms")
#: the columns of ``trace`` and of ``blocks``
TRACE_FIELDS = ("mw_energy", "kinetic_energy", "mean_squared_displacement", "fmax", "com_squared_displacement")
MAX_STEPS = 100000000

_u64 = ctypes.c_ulonglong


def _argtypes(L):
    p, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    for f in (L.mw_ti_run, L.mw_ti_run_device):
        f.argtypes = [i, i, p, p, p, p, p, p, p, _u64, _u64, i, i, i, i, d, d, d, d, p, p, p, p, p, p]
    L.mw_ti_plan.argtypes = [i, p, i, ctypes.POINTER(i), i]


_dev = DevLib("ti", TI_LIB_PATH, "thermodynamic integration", PLAN_FIELDS, setup=_argtypes)

load_ti_library = _dev.load                      # (path=TI_LIB_PATH): dlopen libmw_ti.so; raises if it has not been built
ti_finalize = _dev.finalize
ti_last = _dev.last                              # the fields of ti_plan for the last call that launched


def ti_init(device=0):
    """Initialise the library on ``device`` (the run functions do it on device 0 when nobody has)."""
    return _dev.live(device)


def ti_plan(nwater, cell, nboxes=1):
    """{field: value} of dynamics.PLAN_FIELDS: the launch rules of ``nboxes`` boxes of ``nwater`` molecules with the cell
    ``cell`` [3, 3] (bohr) (mw_ti_plan), no device needed."""
    L = _dev.load()
    out = _dev.plan_out()
    cell = np.ascontiguousarray(cell, dtype=np.float64)
    if cell.shape != (3, 3):
        raise MwError(f"cell {cell.shape}: expected [3, 3]")
    _dev.chk(L.mw_ti_plan(int(nwater), cell.ctypes.data, int(nboxes), out, len(out)))
    return _dev.fields(out)


def ti_elapsed_ms():
    """(sort, moment pass, force pass, drift) of the last call in milliseconds, as dynamics.md_elapsed_ms."""
    L = _dev.load()
    t = [ctypes.c_float(0.0) for _ in range(4)]
    _dev.chk(L.mw_ti_elapsed_ms(*[ctypes.byref(v) for v in t]))
    return tuple(v.value for v in t)


def nblocks_of(nsteps, equil_steps, block_steps):
    """The number of blocks of a call (include/mw_ti.h)."""
    nsteps, equil_steps, block_steps = int(nsteps), int(equil_steps), int(block_steps)
    return (nsteps - equil_steps) // block_steps if block_steps > 0 and nsteps >= equil_steps >= 0 else 0


def _per_box(a, nb, name):
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (nb,)) if np.ndim(a) == 0 else a, dtype=np.float64)
    if a.shape != (nb,):
        raise MwError(f"{name} {a.shape}: expected one value per box, [{nb}]")
    return a


def einstein_md(cells, sites, lambdas, springs, nsteps, dt, kT=0.0, gamma=0.0, pos=None, vel=None, mass=MASS_WATER, seed=0, streams=None, step0=0,
                sample_every=1, equil_steps=0, block_steps=0):
    """(pos_out, vel_out, forces [nboxes, nwater, 3], trace [nboxes, nsteps // sample_every + 1, 5], blocks [nboxes, nblocks, 5],
    status [nboxes, 2]) of the boxes ``cells`` [nboxes, 3, 3] with the Einstein sites ``sites`` [nboxes, nwater, 3] after
    ``nsteps`` BAOAB steps of ``dt`` on U_lambda with ``lambdas`` and ``springs`` (one per box, or one number for all).  ``pos``:
    None to start on the sites; ``vel``: None for zero velocities.  trace = the columns TRACE_FIELDS (E_mW unscaled, the kinetic
    energy, sum |u|^2 / nwater, the largest |F_tot| component, |sum u / nwater|^2) before the first step and after every
    ``sample_every``-th; blocks = the means of the same columns over the steps ``equil_steps`` + j ``block_steps`` ... of the
    call, accumulated on the device at every step (nblocks = (nsteps - equil_steps) // block_steps; none if ``block_steps`` is
    0); forces = F_tot at pos_out; status = (steps completed, frozen 0 / 1).  The noise and everything else are those of
    dynamics.molecular_dynamics, to which a call with every lambda = 0 is equal byte for byte.  One box may come without the
    leading axis, and then so do the results."""
    cells, sites, single = host_boxes(cells, sites)
    pos = _like_pos(pos, sites, single, "pos")
    vel = _like_pos(vel, sites, single, "vel")
    nb, n = sites.shape[0], sites.shape[1]
    streams = _streams(streams, nb)
    lambdas, springs = _per_box(lambdas, nb, "lambdas"), _per_box(springs, nb, "springs")
    L = _dev.live()
    pos_out, vel_out, forces = np.zeros((nb, n, 3)), np.zeros((nb, n, 3)), np.zeros((nb, n, 3))
    trace = np.zeros((nb, _nrows(nsteps, sample_every), 5))
    blocks = np.zeros((nb, nblocks_of(nsteps, equil_steps, block_steps), 5))
    status = np.zeros((nb, 2), dtype=np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data                   # noqa: E731
    _dev.chk(L.mw_ti_run(nb, n, cells.ctypes.data, ptr(pos), ptr(vel), sites.ctypes.data, lambdas.ctypes.data, springs.ctypes.data, ptr(streams),
                         int(seed), int(step0), int(nsteps), int(sample_every), int(equil_steps), int(block_steps), float(dt), float(mass),
                         float(kT), float(gamma), pos_out.ctypes.data, vel_out.ctypes.data, forces.ctypes.data, trace.ctypes.data,
                         blocks.ctypes.data if blocks.size else None, status.ctypes.data))
    out = (pos_out, vel_out, forces, trace, blocks, status)
    return tuple(a[0] for a in out) if single else out


def einstein_md_torch(cells_t, sites_t, lambdas_t, springs_t, nsteps, dt, kT=0.0, gamma=0.0, pos_t=None, vel_t=None, mass=MASS_WATER, seed=0,
                      streams_t=None, step0=0, sample_every=1, equil_steps=0, block_steps=0):
    """The same six results as tensors on the device of the inputs: ``cells_t`` [nboxes, 3, 3], ``sites_t`` and the optional
    ``pos_t`` and ``vel_t`` [nboxes, nwater, 3], ``lambdas_t`` and ``springs_t`` [nboxes] are contiguous float64 device tensors
    on the device the library lives on, ``streams_t`` [nboxes] an int64 device tensor (mw_ti_run_device)."""
    import torch
    named = [(cells_t, torch.float64, "cells_t"), (sites_t, torch.float64, "sites_t"), (lambdas_t, torch.float64, "lambdas_t"),
             (springs_t, torch.float64, "springs_t")]
    named += [(t, torch.float64, name) for t, name in ((pos_t, "pos_t"), (vel_t, "vel_t")) if t is not None]
    if streams_t is not None:
        named.append((streams_t, torch.int64, "streams_t"))
    dev = check_device_tensors(*named)
    check_boxes(cells_t, sites_t)
    nb, n = sites_t.shape[0], sites_t.shape[1]
    for t, name in ((pos_t, "pos_t"), (vel_t, "vel_t")):
        if t is not None and tuple(t.shape) != tuple(sites_t.shape):
            raise MwError(f"{name} {tuple(t.shape)}: expected the shape of sites_t, {tuple(sites_t.shape)}")
    for t, name in ((lambdas_t, "lambdas_t"), (springs_t, "springs_t"), (streams_t, "streams_t")):
        if t is not None and tuple(t.shape) != (nb,):
            raise MwError(f"{name} {tuple(t.shape)}: expected one value per box, [{nb}]")
    L = _dev.live(dev.index or 0)                  # raises if the library lives on another device
    new = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)     # noqa: E731
    pos_out, vel_out, forces = new(nb, n, 3), new(nb, n, 3), new(nb, n, 3)
    trace = new(nb, _nrows(nsteps, sample_every), 5)
    blocks = new(nb, nblocks_of(nsteps, equil_steps, block_steps), 5)
    status = new(nb, 2, dtype=torch.int32)
    ptr = lambda t: None if t is None else t.data_ptr()                    # noqa: E731
    torch.cuda.synchronize(dev)
    _dev.chk(L.mw_ti_run_device(nb, n, cells_t.data_ptr(), ptr(pos_t), ptr(vel_t), sites_t.data_ptr(), lambdas_t.data_ptr(), springs_t.data_ptr(),
                                ptr(streams_t), int(seed), int(step0), int(nsteps), int(sample_every), int(equil_steps), int(block_steps),
                                float(dt), float(mass), float(kT), float(gamma), pos_out.data_ptr(), vel_out.data_ptr(), forces.data_ptr(),
                                trace.data_ptr(), blocks.data_ptr() if blocks.numel() else None, status.data_ptr()))
    return pos_out, vel_out, forces, trace, blocks, status


# -- the host arithmetic of the integration (numpy; no library, no device) -----------------------------------------------------
def gauss_legendre(n):
    """(nodes [n], weights [n]) of the n-point Gauss-Legendre rule on (0, 1): exact for polynomials of degree 2 n - 1."""
    n = int(n)
    if n < 1:
        raise MwError(f"gauss_legendre: n = {n} is not at least 1")
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (x + 1.0), 0.5 * w


def integrand(blocks, springs, nwater, com_free=True):
    """[nboxes, nblocks]: per box and block <U_E' - E_mW> from ``blocks`` [nboxes, nblocks, 5] (the block means of
    TRACE_FIELDS) and the boxes' ``springs`` (one number or [nboxes]): U_E' = 1/2 k N (f2 - f4), or with ``com_free=False``
    U_E = 1/2 k N f2."""
    blocks = np.asarray(blocks, dtype=np.float64)
    if blocks.ndim != 3 or blocks.shape[2] != 5:
        raise MwError(f"blocks {blocks.shape}: expected [nboxes, nblocks, 5]")
    if int(nwater) < 1:
        raise MwError(f"nwater = {nwater} is not at least 1")
    k = _per_box(springs, blocks.shape[0], "springs")
    if not np.all(k > 0.0):
        raise MwError("springs: every spring constant must be > 0")
    u2 = blocks[:, :, 2] - blocks[:, :, 4] if com_free else blocks[:, :, 2]
    return 0.5 * k[:, None] * float(int(nwater)) * u2 - blocks[:, :, 0]


def einstein_free_energy(nwater, spring, mass, kT, com_free=True):
    """The classical free energy of the Einstein crystal, 3 (N - 1) kT ln(sqrt(k / m) / kT) (hbar = 1; 3 N without ``com_free``):
    phonons.harmonic_free_energy of 3 N equal frequencies sqrt(k / m), which drops three of them as translations."""
    if not (kT > 0.0 and spring > 0.0 and mass > 0.0) or int(nwater) < 1:
        raise MwError(f"einstein_free_energy: nwater = {nwater}, spring = {spring}, mass = {mass}, kT = {kT}: expected all positive")
    modes = 3 * (int(nwater) - 1) if com_free else 3 * int(nwater)
    return float(modes * kT * np.log(np.sqrt(spring / mass) / kT))


def frenkel_ladd(nodes, weights, block_integrands, f_einstein):
    """(F, its standard error): F = ``f_einstein`` - sum_w w <U_E' - E_mW>_lambda from ``block_integrands`` [nnodes, nblocks]
    (:func:`integrand` of the boxes at the ``nodes`` of a quadrature with the ``weights``); the error is that of the block
    means, sqrt(sum_w w^2 s_w^2 / nblocks) with s_w the sample standard deviation of node w's blocks (NaN with one block)."""
    nodes, weights = np.asarray(nodes, dtype=np.float64), np.asarray(weights, dtype=np.float64)
    y = np.asarray(block_integrands, dtype=np.float64)
    if nodes.ndim != 1 or weights.shape != nodes.shape or y.ndim != 2 or y.shape[0] != nodes.size:
        raise MwError(f"frenkel_ladd: nodes {nodes.shape}, weights {weights.shape}, block_integrands {y.shape}: expected [n], [n], [n, nblocks]")
    if y.shape[1] < 1:
        raise MwError("frenkel_ladd: no blocks")
    if np.any(nodes < 0.0) or np.any(nodes > 1.0):
        raise MwError("frenkel_ladd: a node lies outside [0, 1]")
    mean = y.mean(axis=1)
    var = y.var(axis=1, ddof=1) / y.shape[1] if y.shape[1] > 1 else np.full(nodes.size, np.nan)
    return float(f_einstein - np.dot(weights, mean)), float(np.sqrt(np.dot(weights * weights, var)))


def spring_from_msd(msd, kT):
    """3 kT / msd: the spring whose Einstein crystal has the mean squared displacement ``msd`` (bohr^2) at ``kT``."""
    if not (msd > 0.0 and kT > 0.0):
        raise MwError(f"spring_from_msd: msd = {msd}, kT = {kT}: expected both positive")
    return 3.0 * float(kT) / float(msd)
