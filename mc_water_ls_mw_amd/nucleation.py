"""Nucleus-size molecular dynamics over the C ABI of ``libmw_nuc.so`` (include/mw_nuc.h): the molecular dynamics of ``flexcell``
-- BAOAB, NVE or Langevin, the per-axis barostat in all four couplings -- with the size lambda of the largest cluster of
solid-like molecules of every box evaluated on the device every ``check_every`` steps, and every box stopped on its own, on the
device, when lambda reaches ``lam_hi`` (status code 3) or falls to ``lam_lo`` (code 4).  That is the primitive of seeding,
committor runs and forward-flux sampling; :func:`seeded_box`, :func:`shoot`, :func:`basin_crossings` and
:func:`rate_from_stages` are thin host helpers over it.

The order parameter is that of ``bondorder`` restricted to l = 6: the entries of a molecule are its neighbours within ``rc_ang``,
a connection is an entry with s_ij > ``threshold``, a molecule is solid-like with at least ``min_conn`` connections, solid-like
molecules that are entries of one another are bonded, and lambda is the size of the largest connected cluster.  The defaults
RC_ANG_DEFAULT = 3.5 Angstrom, THRESHOLD_DEFAULT = 0.5 and MIN_CONN_DEFAULT = 3 are a choice of this module -- the cutoff and
threshold that ``bondorder`` defaults to, and three of the four neighbours of an ice molecule -- and are not taken from any
published parametrisation; a study has to pick and validate its own.

Layouts, units and the other defaults are those of ``flexcell``.  The library serves boxes of at least 65 molecules.  There is
no CPU path: without the library or a device the calls raise.
"""
from __future__ import annotations

import ctypes
import math
import os

import numpy as np

from ._devlib import DevLib, MwError, check_boxes, check_device_tensors, host_boxes
from .dynamics import MASS_WATER, PLAN_FIELDS, _like_pos, _nrows, _streams
from .flexcell import COUPLINGS, TRACE_FIELDS as FLEX_TRACE_FIELDS, _coupling    # noqa: F401  (COUPLINGS: the values of ``coupling``)
from .lattice import ANG_TO_BOHR
from .npt import ATM, BETA_T_DEFAULT, TAU_P_DEFAULT

PKG = os.path.dirname(os.path.abspath(__file__))
NUC_LIB_PATH = os.path.join(PKG, "libmw_nuc.so")

#: every symbol include/mw_nuc.h declares
NUC_ABI_SYMBOLS = ("mw_nuc_init", "mw_nuc_finalize", "mw_nuc_is_initialised", "mw_nuc_last_error", "mw_nuc_run", "mw_nuc_run_device",
                   "mw_nuc_plan", "mw_nuc_last", "mw_nuc_elapsed_ms")
#: the columns of ``trace``: those of flexcell.TRACE_FIELDS, then the latest evaluation of the order parameter
TRACE_FIELDS = FLEX_TRACE_FIELDS + ("largest_cluster", "solid_like", "clusters")
#: the columns of ``op``
OP_FIELDS = ("solid_like", "clusters", "largest_cluster", "largest_label")
#: the fields of nuc_plan and nuc_last
NUC_PLAN_FIELDS = PLAN_FIELDS + ("labels_in_lds", "cluster_rounds")
#: the status codes of the stopping rule (MW_NUC_REACHED_HI, MW_NUC_REACHED_LO), beside 0 and the guards' 1 and 2
REACHED_HI, REACHED_LO = 3, 4
MIN_WATER = 65
MAX_CONN = 64
MAX_STEPS = 100000000
#: the defaults of the order parameter: a choice of this module (module docstring)
RC_ANG_DEFAULT = 3.5
THRESHOLD_DEFAULT = 0.5
MIN_CONN_DEFAULT = 3

_u64 = ctypes.c_ulonglong


def _argtypes(L):
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    for f in (L.mw_nuc_run, L.mw_nuc_run_device):
        f.argtypes = [i, i, vp, vp, vp, vp, vp, _u64, _u64, i, i, d, d, d, d, d, d, d, i, i, i, d, d, i, i, vp, vp,
                      vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mw_nuc_plan.argtypes = [i, vp, i, ctypes.POINTER(i), i]


_dev = DevLib("nuc", NUC_LIB_PATH, "nucleus-size molecular dynamics with on-device stopping rules", NUC_PLAN_FIELDS, setup=_argtypes)

load_nuc_library = _dev.load                     # (path=NUC_LIB_PATH): dlopen libmw_nuc.so; raises if it has not been built
nuc_finalize = _dev.finalize
nuc_last = _dev.last                             # the fields of nuc_plan for the last call that launched; cluster_rounds: of its first box


def nuc_init(device=0):
    """Initialise the library on ``device`` (the run functions do it on device 0 when nobody has)."""
    return _dev.live(device)


def nuc_plan(nwater, cell, nboxes=1):
    """{field: value} of NUC_PLAN_FIELDS: the launch rules of ``nboxes`` boxes of ``nwater`` molecules with the cell ``cell``
    [3, 3] (bohr) (mw_nuc_plan), no device needed."""
    L = _dev.load()
    out = _dev.plan_out()
    cell = np.ascontiguousarray(cell, dtype=np.float64)
    if cell.shape != (3, 3):
        raise MwError(f"cell {cell.shape}: expected [3, 3]")
    _dev.chk(L.mw_nuc_plan(int(nwater), cell.ctypes.data, int(nboxes), out, len(out)))
    return _dev.fields(out)


def nuc_elapsed_ms():
    """(sort, moment pass, force pass, drift, barostat, order, clusters) of the last call in milliseconds, summed over its steps
    and chunks, from the library's event timers: the five of flexcell.flex_elapsed_ms, the two order-parameter passes and the
    cluster pass."""
    L = _dev.load()
    t = [ctypes.c_float(0.0) for _ in range(7)]
    _dev.chk(L.mw_nuc_elapsed_ms(*[ctypes.byref(v) for v in t]))
    return tuple(v.value for v in t)


def _bounds(lam_lo, lam_hi, nb, n):
    """(lam_lo, lam_hi) int32 [nb], contiguous, from per-box arrays or one value for every box; None disables a test."""
    out = []
    for v, name, off in ((lam_lo, "lam_lo", -1), (lam_hi, "lam_hi", n + 1)):
        a = np.asarray(off if v is None else v)
        if a.dtype.kind not in "iu":
            raise MwError(f"{name} of dtype {a.dtype}: expected integers")
        if a.shape == ():
            a = np.broadcast_to(a, (nb,))
        if a.shape != (nb,):
            raise MwError(f"{name} {a.shape}: expected an integer or [{nb}]")
        out.append(np.ascontiguousarray(a, dtype=np.int32))
    return out


def nucleus_md(cells, pos, nsteps, dt, lam_lo=None, lam_hi=None, check_every=1, rc_ang=RC_ANG_DEFAULT, threshold=THRESHOLD_DEFAULT,
               min_conn=MIN_CONN_DEFAULT, pressure=ATM, kT=0.0, gamma=0.0, tau_p=TAU_P_DEFAULT, beta_T=BETA_T_DEFAULT, baro_every=10,
               coupling="aniso", axis=2, vel=None, mass=MASS_WATER, seed=0, streams=None, step0=0, sample_every=1, pos_ref=None):
    """(pos_out, vel_out, forces [nboxes, nwater, 3], cells_out [nboxes, 3, 3], ref_out [nboxes, nwater, 3], trace [nboxes,
    nsteps // sample_every + 1, 18], status [nboxes, 2], nn [nboxes, nwater, 2], label [nboxes, nwater], op [nboxes, 4]) of the
    boxes ``cells`` [nboxes, 3, 3] / ``pos`` [nboxes, nwater, 3] after up to ``nsteps`` steps of
    flexcell.molecular_dynamics_flex, the order parameter evaluated at entry and after every ``check_every``-th step (which must
    divide ``nsteps``).  ``lam_lo`` / ``lam_hi``: an integer or one per box, None to disable the test; a box whose lambda
    reaches ``lam_hi`` is frozen with status (steps completed, 3), one whose lambda falls to ``lam_lo`` with (steps completed,
    4); 1 and 2 are the guards of ``flexcell``: results, not errors.  trace = the columns TRACE_FIELDS; nn = (neighbours within
    ``rc_ang``, connections), label = 0 or the 1-based index of the smallest molecule of the molecule's cluster, op = the
    columns OP_FIELDS, all of the box's final state.  The defaults of ``rc_ang``, ``threshold`` and ``min_conn`` are a choice
    (module docstring).  One box may come without the leading axis, and then so do the results."""
    cells, pos, single = host_boxes(cells, pos)
    vel = _like_pos(vel, pos, single, "vel")
    pos_ref = _like_pos(pos_ref, pos, single, "pos_ref")
    nb, n = pos.shape[0], pos.shape[1]
    streams = _streams(streams, nb)
    lo, hi = _bounds(lam_lo, lam_hi, nb, n)
    coupling = _coupling(coupling)
    L = _dev.live()
    pos_out, vel_out, forces, ref_out = (np.zeros((nb, n, 3)) for _ in range(4))
    cells_out = np.zeros((nb, 3, 3))
    trace = np.zeros((nb, _nrows(nsteps, sample_every), len(TRACE_FIELDS)))
    status = np.zeros((nb, 2), dtype=np.int32)
    nn = np.zeros((nb, n, 2), dtype=np.int32)
    label = np.zeros((nb, n), dtype=np.int32)
    op = np.zeros((nb, 4), dtype=np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data                   # noqa: E731
    _dev.chk(L.mw_nuc_run(nb, n, cells.ctypes.data, pos.ctypes.data, ptr(vel), ptr(pos_ref), ptr(streams), int(seed), int(step0), int(nsteps),
                          int(sample_every), float(dt), float(mass), float(kT), float(gamma), float(pressure), float(tau_p), float(beta_T),
                          int(baro_every), coupling, int(axis), float(rc_ang) * ANG_TO_BOHR, float(threshold), int(min_conn), int(check_every),
                          lo.ctypes.data, hi.ctypes.data, pos_out.ctypes.data, vel_out.ctypes.data, forces.ctypes.data, cells_out.ctypes.data,
                          ref_out.ctypes.data, trace.ctypes.data, status.ctypes.data, nn.ctypes.data, label.ctypes.data, op.ctypes.data))
    out = (pos_out, vel_out, forces, cells_out, ref_out, trace, status, nn, label, op)
    return tuple(o[0] for o in out) if single else out


def nucleus_md_torch(cells_t, pos_t, nsteps, dt, lam_lo_t, lam_hi_t, check_every=1, rc_ang=RC_ANG_DEFAULT, threshold=THRESHOLD_DEFAULT,
                     min_conn=MIN_CONN_DEFAULT, pressure=ATM, kT=0.0, gamma=0.0, tau_p=TAU_P_DEFAULT, beta_T=BETA_T_DEFAULT, baro_every=10,
                     coupling="aniso", axis=2, vel_t=None, mass=MASS_WATER, seed=0, streams_t=None, step0=0, sample_every=1, pos_ref_t=None):
    """The same ten results as tensors on the device of the inputs: ``cells_t`` [nboxes, 3, 3], ``pos_t`` and the optional
    ``vel_t`` and ``pos_ref_t`` [nboxes, nwater, 3] contiguous float64 device tensors, ``lam_lo_t`` and ``lam_hi_t`` [nboxes] int32
    (-1 and nwater + 1 disable a test), ``streams_t`` [nboxes] int64, all on the device the library lives on (mw_nuc_run_device)."""
    import torch
    named = [(cells_t, torch.float64, "cells_t"), (pos_t, torch.float64, "pos_t"), (lam_lo_t, torch.int32, "lam_lo_t"),
             (lam_hi_t, torch.int32, "lam_hi_t")]
    named += [(t, torch.float64, name) for t, name in ((vel_t, "vel_t"), (pos_ref_t, "pos_ref_t")) if t is not None]
    if streams_t is not None:
        named.append((streams_t, torch.int64, "streams_t"))
    dev = check_device_tensors(*named)
    check_boxes(cells_t, pos_t)
    nb, n = pos_t.shape[0], pos_t.shape[1]
    for t, name in ((vel_t, "vel_t"), (pos_ref_t, "pos_ref_t")):
        if t is not None and tuple(t.shape) != tuple(pos_t.shape):
            raise MwError(f"{name} {tuple(t.shape)}: expected the shape of pos_t, {tuple(pos_t.shape)}")
    for t, name in ((lam_lo_t, "lam_lo_t"), (lam_hi_t, "lam_hi_t")):
        if tuple(t.shape) != (nb,):
            raise MwError(f"{name} {tuple(t.shape)}: expected [{nb}]")
    if streams_t is not None and tuple(streams_t.shape) != (nb,):
        raise MwError(f"streams_t {tuple(streams_t.shape)}: expected one 64-bit stream identity per box, [{nb}]")
    coupling = _coupling(coupling)
    L = _dev.live(dev.index or 0)                  # raises if the library lives on another device
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    pos_out, vel_out, forces, ref_out = (torch.zeros((nb, n, 3), **f64) for _ in range(4))
    cells_out = torch.zeros((nb, 3, 3), **f64)
    trace = torch.zeros((nb, _nrows(nsteps, sample_every), len(TRACE_FIELDS)), **f64)
    status = torch.zeros((nb, 2), **i32)
    nn = torch.zeros((nb, n, 2), **i32)
    label = torch.zeros((nb, n), **i32)
    op = torch.zeros((nb, 4), **i32)
    ptr = lambda t: None if t is None else t.data_ptr()                    # noqa: E731
    torch.cuda.synchronize(dev)
    _dev.chk(L.mw_nuc_run_device(nb, n, cells_t.data_ptr(), pos_t.data_ptr(), ptr(vel_t), ptr(pos_ref_t), ptr(streams_t), int(seed), int(step0),
                                 int(nsteps), int(sample_every), float(dt), float(mass), float(kT), float(gamma), float(pressure), float(tau_p),
                                 float(beta_T), int(baro_every), coupling, int(axis), float(rc_ang) * ANG_TO_BOHR, float(threshold), int(min_conn),
                                 int(check_every), lam_lo_t.data_ptr(), lam_hi_t.data_ptr(), pos_out.data_ptr(), vel_out.data_ptr(),
                                 forces.data_ptr(), cells_out.data_ptr(), ref_out.data_ptr(), trace.data_ptr(), status.data_ptr(), nn.data_ptr(),
                                 label.data_ptr(), op.data_ptr()))
    return pos_out, vel_out, forces, cells_out, ref_out, trace, status, nn, label, op


def largest_cluster(cells, pos, rc_ang=RC_ANG_DEFAULT, threshold=THRESHOLD_DEFAULT, min_conn=MIN_CONN_DEFAULT):
    """(nn [nboxes, nwater, 2], label [nboxes, nwater], op [nboxes, 4]) of the boxes as they stand: the single point of
    :func:`nucleus_md` (no step, both tests disabled).  One box may come without the leading axis."""
    out = nucleus_md(cells, pos, 0, 1.0, rc_ang=rc_ang, threshold=threshold, min_conn=min_conn, baro_every=0)
    return out[7], out[8], out[9]


# ---- host helpers (host arithmetic only) ------------------------------------------------------------------------------------
def _widths(h):
    vol = abs(np.linalg.det(h))
    return np.array([vol / np.linalg.norm(np.cross(h[(k + 1) % 3], h[(k + 2) % 3])) for k in range(3)])


def _min_image(h, d):
    """The shortest periodic image of every row of ``d`` [M, 3] (valid for |d| below half the narrowest width)."""
    s = d @ np.linalg.inv(h)
    return (s - np.round(s)) @ h


def seeded_box(h, xyz, kind, radius_ang, centre=None, d_min_ang=2.4):
    """(h, xyz_new [N', 3], nseed): the configuration ``h`` [3, 3] / ``xyz`` [N, 3] (bohr) with a spherical seed of ice ``kind``
    ("ih" or "ic") of radius ``radius_ang`` put in at ``centre`` (bohr; None: the middle of the cell).  The seed is made of the
    sites of a lattice.ice_box of ``kind`` that lie inside the sphere around that lattice's own middle, in the lattice's own
    orientation; every molecule of ``xyz`` inside the sphere, or closer than ``d_min_ang`` to an inserted site, is removed.  The
    seed's ``nseed`` molecules come first in ``xyz_new``; N changes.  The sphere must fit the cell: 2 (radius + d_min) below its
    narrowest width."""
    from . import lattice as lat
    h = np.asarray(h, dtype=np.float64).reshape(3, 3)
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    radius, d_min = float(radius_ang) * ANG_TO_BOHR, float(d_min_ang) * ANG_TO_BOHR
    if not radius > 0.0 or not d_min >= 0.0:
        raise MwError(f"radius_ang = {radius_ang}, d_min_ang = {d_min_ang}: expected a radius > 0 and a distance >= 0")
    if not 2.0 * (radius + d_min) < _widths(h).min():
        raise MwError(f"a seed of radius {radius_ang} A does not fit the cell: 2 (radius + d_min) must stay below its narrowest width")
    centre = 0.5 * h.sum(axis=0) if centre is None else np.asarray(centre, dtype=np.float64).reshape(3)
    hc, _ = {"ih": lat.ice_ih_cell, "ic": lat.ice_ic_cell}[kind]()
    reps = tuple(int(math.ceil(2.0 * radius / hc[k, k])) + 1 for k in range(3))
    hl, xl = lat.ice_box(kind, reps)
    rel = xl - 0.5 * hl.sum(axis=0)
    seed = rel[(rel * rel).sum(axis=1) < radius * radius] + centre
    d = _min_image(h, xyz - centre)
    keep = (d * d).sum(axis=1) >= radius * radius
    if len(seed) and d_min > 0.0:
        for k0 in range(0, len(xyz), 4096):
            dd = _min_image(h, (xyz[k0:k0 + 4096, None, :] - seed[None, :, :]).reshape(-1, 3)).reshape(-1, len(seed), 3)
            keep[k0:k0 + 4096] &= ((dd * dd).sum(axis=2) >= d_min * d_min).all(axis=1)
    return h.copy(), np.ascontiguousarray(np.concatenate([seed, xyz[keep]], axis=0)), len(seed)


def binomial_error(successes, trials):
    """The standard error sqrt(p (1 - p) / trials) of the fraction p = successes / trials (0 for no trials)."""
    if trials <= 0:
        return 0.0
    p = successes / trials
    return math.sqrt(p * (1.0 - p) / trials)


def shoot(cells, pos, vel, nsteps, dt, lam_lo, lam_hi, trials, seed, stream0=0, step0=0, **kwargs):
    """One forward-flux stage from the configurations ``cells`` [M, 3, 3] / ``pos`` / ``vel`` [M, nwater, 3] (``vel`` None:
    zero): every (configuration, trial) pair is one box of ONE :func:`nucleus_md` call of up to ``nsteps`` steps, with the noise
    stream stream0 + configuration * trials + trial of its own (``gamma`` > 0 is what makes the trials differ), stopped at
    ``lam_hi`` or ``lam_lo``.  Returns a dict: ``cells``, ``pos``, ``vel`` of the boxes that reached ``lam_hi``, ``parent``
    their configurations' indices, ``reached_hi``, ``reached_lo``, ``undecided`` (neither within ``nsteps``), ``frozen`` (a
    guard), ``total``, ``fraction`` = reached_hi / total with its binomial standard error ``error``, and ``steps``, the steps
    completed by all boxes.  The other keywords are those of nucleus_md."""
    cells, pos, single = host_boxes(cells, pos)
    vel = _like_pos(vel, pos, single, "vel")
    m, trials = pos.shape[0], int(trials)
    if trials < 1:
        raise MwError(f"trials = {trials}: expected at least 1")
    if "streams" in kwargs:
        raise MwError("shoot names the noise streams itself: stream0 + configuration * trials + trial")
    rep = lambda a: None if a is None else np.repeat(a, trials, axis=0)    # noqa: E731
    streams = np.uint64(int(stream0)) + np.arange(m * trials, dtype=np.uint64)
    out = nucleus_md(rep(cells), rep(pos), nsteps, dt, lam_lo=lam_lo, lam_hi=lam_hi, vel=rep(vel), seed=seed, streams=streams, step0=step0, **kwargs)
    code = out[6][:, 1]
    hit = np.nonzero(code == REACHED_HI)[0]
    total = m * trials
    n_hi, n_lo = int(len(hit)), int((code == REACHED_LO).sum())
    return dict(cells=out[3][hit], pos=out[0][hit], vel=out[1][hit], parent=hit // trials, reached_hi=n_hi, reached_lo=n_lo,
                undecided=int((code == 0).sum()), frozen=int(((code == 1) | (code == 2)).sum()), total=total, fraction=n_hi / total,
                error=binomial_error(n_hi, total), steps=int(out[6][:, 0].sum()))


def basin_crossings(cells, pos, vel, lam_a, lam_0, nsteps, dt, calls, seed, stream0=0, **kwargs):
    """The flux out of the basin lambda <= ``lam_a`` through the first interface ``lam_0`` > ``lam_a``, from ``calls``
    :func:`nucleus_md` calls of up to ``nsteps`` steps each over the boxes ``cells`` / ``pos`` / ``vel``, chained box by box.  A
    box alternates between two kinds of run: one that stops at lambda >= ``lam_0`` (a crossing: its configuration is kept),
    then one with the upper test disabled that stops at lambda <= ``lam_a`` (back in the basin); a box that ends a call without
    stopping goes on in the same kind.  Call k draws its noise at the step indices from k * nsteps on, so no draw is used twice.
    Returns a dict: ``cells``, ``pos``, ``vel`` of the crossing configurations, ``crossings``, ``steps`` (the steps completed by
    all boxes in all calls), ``time`` = steps * dt, ``flux`` = crossings / time (per box and atomic time unit), ``frozen`` (boxes
    a guard froze; they take no further part)."""
    cells, pos, single = host_boxes(cells, pos)
    vel = _like_pos(vel, pos, single, "vel")
    nb, n = pos.shape[0], pos.shape[1]
    if not -1 <= int(lam_a) < int(lam_0):
        raise MwError(f"lam_a = {lam_a}, lam_0 = {lam_0}: expected -1 <= lam_a < lam_0")
    if "streams" in kwargs:
        raise MwError("basin_crossings names the noise streams itself: stream0 + box")
    streams = np.uint64(int(stream0)) + np.arange(nb, dtype=np.uint64)
    cells, pos = cells.copy(), pos.copy()
    vel = np.zeros_like(pos) if vel is None else vel.copy()
    ref = pos.copy()
    outward = np.ones(nb, dtype=bool)                   # looking for lam_0; otherwise on the way back to lam_a
    alive = np.ones(nb, dtype=bool)
    got = dict(cells=[], pos=[], vel=[])
    steps = 0
    for k in range(int(calls)):
        act = np.nonzero(alive)[0]
        if len(act) == 0:
            break
        lo = np.where(outward[act], -1, int(lam_a)).astype(np.int32)
        hi = np.where(outward[act], int(lam_0), n + 1).astype(np.int32)
        out = nucleus_md(cells[act], pos[act], nsteps, dt, lam_lo=lo, lam_hi=hi, vel=vel[act], pos_ref=ref[act], seed=seed, streams=streams[act],
                         step0=k * int(nsteps), **kwargs)
        pos[act], vel[act], cells[act], ref[act] = out[0], out[1], out[3], out[4]
        done, code = out[6][:, 0], out[6][:, 1]
        steps += int(done.sum())
        crossed = act[code == REACHED_HI]
        got["cells"].append(cells[crossed]), got["pos"].append(pos[crossed]), got["vel"].append(vel[crossed])
        outward[crossed] = False
        outward[act[code == REACHED_LO]] = True
        alive[act[(code == 1) | (code == 2)]] = False
    res = {key: np.concatenate(v, axis=0) if v else np.zeros((0,) + pos.shape[1:]) for key, v in got.items()}
    if not got["cells"]:
        res["cells"] = np.zeros((0, 3, 3))
    crossings = int(len(res["pos"]))
    time = steps * float(dt)
    res.update(crossings=crossings, steps=steps, time=time, flux=crossings / time if time > 0.0 else 0.0, frozen=int((~alive).sum()))
    return res


def rate_from_stages(flux, fractions):
    """The forward-flux rate: ``flux`` through the first interface times the product of the stages' fractions."""
    rate = float(flux)
    for p in fractions:
        rate *= float(p)
    return rate
