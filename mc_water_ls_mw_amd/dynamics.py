"""Molecular dynamics over the C ABI of ``libmw_md.so`` (include/mw_md.h): every box is moved in time on the full-box mW
energy at fixed cell by BAOAB -- at constant energy (``gamma=0``) or in contact with a Langevin thermostat at ``kT`` --, all
boxes of a call at once on the device and each on its own trajectory with its own noise stream.

A cell ``h`` is a [3, 3] array whose ROW k is the lattice vector h_(k+1) (``EnergyModule.hmatrix[b]``, the layout of
``mw_set_cell``).  Everything is in atomic units: positions in bohr, energies and ``kT`` in Hartree, forces in Hartree / bohr,
``dt`` in atomic time units (``5 * FS`` is five femtoseconds), ``mass`` in electron masses (``MASS_WATER``), ``gamma`` in
inverse atomic time units, velocities in bohr per atomic time unit; ``250 * KELVIN`` is the kT of 250 K.  Positions are never
wrapped, so ``pos_out`` goes straight back in (with ``vel_out``, ``pos_ref`` = the first positions and ``step0`` advanced by
the steps done, a run continues byte for byte) and into the other libraries' functions -- ``quench.inherent_structures``,
``tetrahedral.tetrahedral_order``, ``rings.ring_statistics``.  There is no CPU path: without the library or a device the
calls raise.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from ._devlib import DevLib, MwError, check_boxes, check_device_tensors, host_boxes

PKG = os.path.dirname(os.path.abspath(__file__))
MD_LIB_PATH = os.path.join(PKG, "libmw_md.so")

#: every symbol include/mw_md.h declares
MD_ABI_SYMBOLS = ("mw_md_init", "mw_md_finalize", "mw_md_is_initialised", "mw_md_last_error", "mw_md_run", "mw_md_run_device", "mw_md_plan",
                  "mw_md_last", "mw_md_elapsed_ms")
#: the fields of mw_md_plan / mw_md_last, in order
PLAN_FIELDS = ("boxes_per_chunk", "chunks", "small", "g1", "g2", "g3", "lds_bytes", "scratch_bytes_per_box", "boxes_per_workgroup",
               "steps_per_launch")
#: the columns of ``trace``
TRACE_FIELDS = ("potential_energy", "kinetic_energy", "mean_squared_displacement", "fmax")
#: the mass of a water molecule in electron masses (MW_MD_MASS_WATER): 18.01528 amu x 1822.888486209 electron masses per amu
MASS_WATER = 18.01528 * 1822.888486209
#: atomic time units per femtosecond (the atomic unit of time is 2.4188843265857e-17 s)
FS = 1.0e-15 / 2.4188843265857e-17
#: Hartree per kelvin (the Boltzmann constant in atomic units)
KELVIN = 3.1668115634556e-6
MAX_STEPS = 100000000

_u64 = ctypes.c_ulonglong


def _argtypes(L):
    for f in (L.mw_md_run, L.mw_md_run_device):
        f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _u64, _u64,
                      ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_void_p,
                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.mw_md_plan.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int]


_dev = DevLib("md", MD_LIB_PATH, "molecular dynamics", PLAN_FIELDS, setup=_argtypes)

load_md_library = _dev.load                      # (path=MD_LIB_PATH): dlopen libmw_md.so; raises if it has not been built
md_finalize = _dev.finalize
md_last = _dev.last                              # the fields of md_plan for the last call that launched (the grid is that of its first box)


def md_init(device=0):
    """Initialise the library on ``device`` (the run functions do it on device 0 when nobody has)."""
    return _dev.live(device)


def md_plan(nwater, cell, nboxes=1):
    """{field: value} of PLAN_FIELDS: the launch rules of ``nboxes`` boxes of ``nwater`` molecules with the cell ``cell``
    [3, 3] (bohr) (mw_md_plan), no device needed."""
    L = _dev.load()
    out = _dev.plan_out()
    cell = np.ascontiguousarray(cell, dtype=np.float64)
    if cell.shape != (3, 3):
        raise MwError(f"cell {cell.shape}: expected [3, 3]")
    _dev.chk(L.mw_md_plan(int(nwater), cell.ctypes.data, int(nboxes), out, len(out)))
    return _dev.fields(out)


def md_elapsed_ms():
    """(sort, moment pass, force pass, drift) of the last call in milliseconds, summed over its steps and chunks, from the
    library's event timers; the small geometry is one kernel, reported as the force pass."""
    L = _dev.load()
    t = [ctypes.c_float(0.0) for _ in range(4)]
    _dev.chk(L.mw_md_elapsed_ms(*[ctypes.byref(v) for v in t]))
    return tuple(v.value for v in t)


def maxwell_boltzmann(nboxes, nwater, kT, mass=MASS_WATER, seed=0):
    """[nboxes, nwater, 3] velocities (bohr per atomic time unit) drawn on the host from the Maxwell-Boltzmann distribution at
    ``kT`` (Hartree) for molecules of ``mass`` (electron masses), the centre-of-mass velocity of every box removed."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((int(nboxes), int(nwater), 3)) * np.sqrt(float(kT) / float(mass))
    return np.ascontiguousarray(v - v.mean(axis=1, keepdims=True))


def _like_pos(a, pos, single, name):
    """None, or ``a`` as a contiguous float64 array of the shape of ``pos`` (the leading axis added where ``pos`` got one)."""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float64)
    if single and a.ndim == 2:
        a = a[None]
    if a.shape != pos.shape:
        raise MwError(f"{name} {a.shape}: expected the shape of pos, {pos.shape}")
    return a


def _streams(streams, nb):
    if streams is None:
        return None
    s = np.ascontiguousarray(np.atleast_1d(streams), dtype=np.uint64)
    if s.shape != (nb,):
        raise MwError(f"streams {s.shape}: expected one 64-bit stream identity per box, [{nb}]")
    return s


def _nrows(nsteps, sample_every):
    return int(nsteps) // int(sample_every) + 1 if int(sample_every) >= 1 and int(nsteps) >= 0 else 1


def molecular_dynamics(cells, pos, nsteps, dt, kT=0.0, gamma=0.0, vel=None, mass=MASS_WATER, seed=0, streams=None, step0=0, sample_every=1,
                       pos_ref=None):
    """(pos_out [nboxes, nwater, 3], vel_out [nboxes, nwater, 3], forces [nboxes, nwater, 3], trace [nboxes, nsteps //
    sample_every + 1, 4], status [nboxes, 2]) of the boxes ``cells`` [nboxes, 3, 3] / ``pos`` [nboxes, nwater, 3] after
    ``nsteps`` BAOAB steps of ``dt``: positions, velocities and the forces there; trace = the columns TRACE_FIELDS (potential
    and kinetic energy in Hartree, the mean squared displacement from ``pos_ref`` -- None: ``pos`` -- in bohr^2, the largest
    |F| component) before the first step and after every ``sample_every``-th; status = (steps completed, frozen 0 / 1): a
    box whose half drift would exceed a quarter of the cutoff is frozen where it is, a result and not an error.  ``vel``:
    None for zero velocities.  ``gamma=0`` is NVE and draws no random number; otherwise box b's noise is a function of
    (``seed``, ``streams[b]`` -- None: b --, the step index ``step0`` + s, the molecule) alone.  One box may come without the
    leading axis, and then so do the results."""
    cells, pos, single = host_boxes(cells, pos)
    vel = _like_pos(vel, pos, single, "vel")
    pos_ref = _like_pos(pos_ref, pos, single, "pos_ref")
    nb, n = pos.shape[0], pos.shape[1]
    streams = _streams(streams, nb)
    L = _dev.live()
    pos_out, vel_out, forces = np.zeros((nb, n, 3)), np.zeros((nb, n, 3)), np.zeros((nb, n, 3))
    trace = np.zeros((nb, _nrows(nsteps, sample_every), 4))
    status = np.zeros((nb, 2), dtype=np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data                   # noqa: E731
    _dev.chk(L.mw_md_run(nb, n, cells.ctypes.data, pos.ctypes.data, ptr(vel), ptr(pos_ref), ptr(streams), int(seed), int(step0), int(nsteps),
                         int(sample_every), float(dt), float(mass), float(kT), float(gamma), pos_out.ctypes.data, vel_out.ctypes.data,
                         forces.ctypes.data, trace.ctypes.data, status.ctypes.data))
    return (pos_out[0], vel_out[0], forces[0], trace[0], status[0]) if single else (pos_out, vel_out, forces, trace, status)


def molecular_dynamics_torch(cells_t, pos_t, nsteps, dt, kT=0.0, gamma=0.0, vel_t=None, mass=MASS_WATER, seed=0, streams_t=None, step0=0,
                             sample_every=1, pos_ref_t=None):
    """The same five results as tensors on the device of the inputs: ``cells_t`` [nboxes, 3, 3], ``pos_t`` and the optional
    ``vel_t`` and ``pos_ref_t`` [nboxes, nwater, 3] are contiguous float64 device tensors on the device the library lives on,
    ``streams_t`` [nboxes] an int64 device tensor holding the 64-bit stream identities (mw_md_run_device)."""
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
    pos_out = torch.zeros((nb, n, 3), dtype=torch.float64, device=dev)
    vel_out = torch.zeros((nb, n, 3), dtype=torch.float64, device=dev)
    forces = torch.zeros((nb, n, 3), dtype=torch.float64, device=dev)
    trace = torch.zeros((nb, _nrows(nsteps, sample_every), 4), dtype=torch.float64, device=dev)
    status = torch.zeros((nb, 2), dtype=torch.int32, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()                    # noqa: E731
    torch.cuda.synchronize(dev)
    _dev.chk(L.mw_md_run_device(nb, n, cells_t.data_ptr(), pos_t.data_ptr(), ptr(vel_t), ptr(pos_ref_t), ptr(streams_t), int(seed), int(step0),
                                int(nsteps), int(sample_every), float(dt), float(mass), float(kT), float(gamma), pos_out.data_ptr(),
                                vel_out.data_ptr(), forces.data_ptr(), trace.data_ptr(), status.data_ptr()))
    return pos_out, vel_out, forces, trace, status


def trajectory(cells_t, pos_t, nframes, steps_per_frame, dt, sample_every=1, **md_keywords):
    """(frames [nframes, nboxes, nwater, 3], vel_frames [nframes, nboxes, nwater, 3], trace [nboxes, (nframes - 1) *
    steps_per_frame // sample_every + 1, 4], status [nboxes, 2]) as device tensors: a recorded run of (``nframes`` - 1) *
    ``steps_per_frame`` steps of ``dt`` from ``pos_t``, one frame every ``steps_per_frame`` steps, frame 0 being the input
    (``vel_t``: None for zero velocities).  The frames are what ``timecorr.time_correlations_torch`` takes.

    The run is ``nframes`` - 1 chained :func:`molecular_dynamics_torch` calls -- ``pos_ref_t`` the first positions (or the one
    given), ``step0`` advanced by the steps done -- so by the contract of include/mw_md.h every frame is byte for byte what one
    uninterrupted run holds at that step, the last frame that run's ``pos_out``, and the trace its trace.  The keywords are
    those of molecular_dynamics_torch (kT, gamma, vel_t, mass, seed, streams_t, step0, pos_ref_t); ``sample_every`` must divide
    ``steps_per_frame``.  A box that freezes (status [b, 1] = 1, status [b, 0] = the steps it completed) repeats its frozen
    state in every later frame and its last trace row in every later row."""
    import torch
    nframes, spf, sample_every = int(nframes), int(steps_per_frame), int(sample_every)
    if nframes < 1 or spf < 1 or sample_every < 1 or spf % sample_every:
        raise MwError(f"trajectory: nframes = {nframes}, steps_per_frame = {spf}, sample_every = {sample_every}: expected nframes >= 1 and "
                      f"sample_every >= 1 dividing steps_per_frame >= 1")
    kw = dict(md_keywords)
    for name in ("nsteps",):
        if name in kw:
            raise MwError(f"trajectory: {name} is set by nframes and steps_per_frame")
    vel_t, step0 = kw.pop("vel_t", None), int(kw.pop("step0", 0))
    pos_ref_t = kw.pop("pos_ref_t", None)
    check_device_tensors((cells_t, torch.float64, "cells_t"), (pos_t, torch.float64, "pos_t"))
    check_boxes(cells_t, pos_t)
    nb, n = pos_t.shape[0], pos_t.shape[1]
    frames = torch.zeros((nframes, nb, n, 3), dtype=torch.float64, device=pos_t.device)
    vel_frames = torch.zeros_like(frames)
    frames[0] = pos_t
    if vel_t is not None:
        vel_frames[0] = vel_t
    pos_ref_t = frames[0].clone() if pos_ref_t is None else pos_ref_t
    rows = spf // sample_every
    trace = torch.zeros((nb, (nframes - 1) * rows + 1, 4), dtype=torch.float64, device=pos_t.device)
    status = torch.zeros((nb, 2), dtype=torch.int32, device=pos_t.device)
    for f in range(1, nframes):
        p, v, _, tr, st = molecular_dynamics_torch(cells_t, frames[f - 1], spf, dt, vel_t=vel_frames[f - 1], step0=step0 + (f - 1) * spf,
                                                   sample_every=sample_every, pos_ref_t=pos_ref_t, **kw)
        was = status[:, 1] != 0                                              # frozen in an earlier call: its state and its row repeat
        frames[f] = torch.where(was[:, None, None], frames[f - 1], p)
        vel_frames[f] = torch.where(was[:, None, None], vel_frames[f - 1], v)
        r0 = (f - 1) * rows
        if f == 1:
            trace[:, 0] = tr[:, 0]
        trace[:, r0 + 1:r0 + rows + 1] = torch.where(was[:, None, None], trace[:, r0:r0 + 1].expand(-1, rows, -1), tr[:, 1:])
        status[:, 0] += torch.where(was, torch.zeros_like(st[:, 0]), st[:, 0])
        status[:, 1] = torch.where(was, status[:, 1], st[:, 1])
    if nframes == 1:
        _, _, _, tr, st = molecular_dynamics_torch(cells_t, frames[0], 0, dt, vel_t=vel_frames[0], step0=step0, sample_every=sample_every,
                                                   pos_ref_t=pos_ref_t, **kw)
        trace[:, 0], status = tr[:, 0], st
    return frames, vel_frames, trace, status
