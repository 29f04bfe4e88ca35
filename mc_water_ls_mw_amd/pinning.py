"""Interface pinning over the C ABI of ``libmw_pin.so`` (include/mw_pin.h): the molecular dynamics of ``flexcell`` -- BAOAB, NVE
or Langevin, the per-axis barostat in all four couplings -- on E_mW + 1/2 kappa (Q - a)^2, a harmonic bias on the modulus
Q = |rho(n)| / sqrt(N) of one collective density mode of every box (Pedersen et al., Phys. Rev. B 88, 094101 (2013); Pedersen,
J. Chem. Phys. 139, 104102 (2013)).  A two-phase box held at a chosen amount of crystal reports mu_solid - mu_liquid as the mean
force of the bias (:func:`delta_mu`); the melting point is where it vanishes.

Layouts, units and defaults are those of ``flexcell``.  Per box: ``nvec`` an integer triple, ``kappa`` (Hartree) and ``anchor``
(a pure number; Q is about 1 in a liquid and of the order sqrt(N) in a crystal at one of its Bragg vectors); a scalar or one
triple serves every box.  A box with kappa = 0 gets the bits of ``flexcell.molecular_dynamics_flex``.  There is no two-phase box
builder: a crystal started with the anchor at half its own Q melts half of itself under the bias.  There is no CPU path: without
the library or a device the calls raise.
"""
from __future__ import annotations

import ctypes
import math
import os

import numpy as np

from ._devlib import DevLib, MwError, check_boxes, check_device_tensors, host_boxes
from .dynamics import MASS_WATER, PLAN_FIELDS, _like_pos, _nrows, _streams
from .flexcell import COUPLINGS, _coupling
from .npt import ATM, BETA_T_DEFAULT, TAU_P_DEFAULT

PKG = os.path.dirname(os.path.abspath(__file__))
PIN_LIB_PATH = os.path.join(PKG, "libmw_pin.so")

#: every symbol include/mw_pin.h declares
PIN_ABI_SYMBOLS = ("mw_pin_init", "mw_pin_finalize", "mw_pin_is_initialised", "mw_pin_last_error", "mw_pin_run", "mw_pin_run_device",
                   "mw_pin_plan", "mw_pin_last", "mw_pin_elapsed_ms")
#: the columns of ``trace``: those of flexcell.TRACE_FIELDS (fmax is that of the total force), then the mode and the bias energy
TRACE_FIELDS = ("potential_energy", "kinetic_energy", "mean_squared_displacement", "fmax", "volume", "pressure", "p_xx", "p_yy", "p_zz", "p_xy",
                "p_xz", "p_yz", "length_1", "length_2", "length_3", "order_parameter", "bias_energy")
#: the columns of ``blocks``: block averages of Q, Q^2, V and E_mW
BLOCK_FIELDS = ("q", "q_squared", "volume", "potential_energy")
#: the largest |component| of a triple (MW_PIN_MAX_N)
MAX_N = 255
MAX_STEPS = 100000000

_u64 = ctypes.c_ulonglong


def _argtypes(L):
    vp, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    for f in (L.mw_pin_run, L.mw_pin_run_device):
        f.argtypes = [i, i, vp, vp, vp, vp, vp, vp, vp, vp, _u64, _u64, i, i, i, i, d, d, d, d, d, d, d, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mw_pin_plan.argtypes = [i, vp, i, ctypes.POINTER(i), i]


_dev = DevLib("pin", PIN_LIB_PATH, "interface pinning: molecular dynamics with a bias on a collective density mode", PLAN_FIELDS, setup=_argtypes)

load_pin_library = _dev.load                     # (path=PIN_LIB_PATH): dlopen libmw_pin.so; raises if it has not been built
pin_finalize = _dev.finalize
pin_last = _dev.last                             # the fields of pin_plan for the last call that launched


def pin_init(device=0):
    """Initialise the library on ``device`` (the run functions do it on device 0 when nobody has)."""
    return _dev.live(device)


def pin_plan(nwater, cell, nboxes=1):
    """{field: value} of dynamics.PLAN_FIELDS: the launch rules of ``nboxes`` boxes of ``nwater`` molecules with the cell ``cell``
    [3, 3] (bohr) (mw_pin_plan), no device needed."""
    L = _dev.load()
    out = _dev.plan_out()
    cell = np.ascontiguousarray(cell, dtype=np.float64)
    if cell.shape != (3, 3):
        raise MwError(f"cell {cell.shape}: expected [3, 3]")
    _dev.chk(L.mw_pin_plan(int(nwater), cell.ctypes.data, int(nboxes), out, len(out)))
    return _dev.fields(out)


def pin_elapsed_ms():
    """(sort, moment pass, force pass, drift, barostat, rho) of the last call in milliseconds, summed over its steps and chunks,
    from the library's event timers: the five of flexcell.flex_elapsed_ms, and the kernel that sums the mode of every box and forms
    its bias (general geometry; the phasors are formed inside the moment pass and count there)."""
    L = _dev.load()
    t = [ctypes.c_float(0.0) for _ in range(6)]
    _dev.chk(L.mw_pin_elapsed_ms(*[ctypes.byref(v) for v in t]))
    return tuple(v.value for v in t)


def _bias(nvec, kappa, anchor, nb):
    """(nvec int32 [nb, 3], kappas [nb], anchors [nb]), contiguous, from per-box arrays or one value for every box."""
    n = np.asarray(nvec)
    if n.dtype.kind not in "iu":
        raise MwError(f"nvec of dtype {n.dtype}: expected integers")
    if n.shape == (3,):
        n = np.broadcast_to(n, (nb, 3))
    if n.shape != (nb, 3):
        raise MwError(f"nvec {n.shape}: expected [3] or [{nb}, 3]")
    out = [np.ascontiguousarray(n, dtype=np.int32)]
    for v, name in ((kappa, "kappa"), (anchor, "anchor")):
        a = np.asarray(v, dtype=np.float64)
        if a.shape == ():
            a = np.broadcast_to(a, (nb,))
        if a.shape != (nb,):
            raise MwError(f"{name} {a.shape}: expected a number or [{nb}]")
        out.append(np.ascontiguousarray(a, dtype=np.float64))
    return out


def _nblocks(nsteps, equil_steps, block_steps):
    return (nsteps - equil_steps) // block_steps if block_steps > 0 and nsteps >= equil_steps >= 0 else 0


def interface_pinning(cells, pos, nvec, kappa, anchor, nsteps, dt, pressure=ATM, kT=0.0, gamma=0.0, tau_p=TAU_P_DEFAULT, beta_T=BETA_T_DEFAULT,
                      baro_every=10, coupling="uniaxial", axis=2, vel=None, mass=MASS_WATER, seed=0, streams=None, step0=0, sample_every=1,
                      pos_ref=None, equil_steps=0, block_steps=0):
    """(pos_out, vel_out, forces [nboxes, nwater, 3], cells_out [nboxes, 3, 3], ref_out [nboxes, nwater, 3], trace [nboxes,
    nsteps // sample_every + 1, 17], blocks [nboxes, nblocks, 4], status [nboxes, 2]) of the boxes ``cells`` [nboxes, 3, 3] /
    ``pos`` [nboxes, nwater, 3] after ``nsteps`` steps of flexcell.molecular_dynamics_flex under the bias 1/2 ``kappa``
    (Q - ``anchor``)^2 on the mode ``nvec`` of every box.  ``forces`` are the total forces; trace = the columns TRACE_FIELDS;
    blocks = the averages BLOCK_FIELDS over the nblocks = (nsteps - equil_steps) // block_steps blocks of ``block_steps`` steps
    after ``equil_steps``, accumulated on the device at every step; status as in ``flexcell`` (1: the drift guard, which a huge
    kappa trips; 2: the barostat guard): results, not errors.  The default ensemble is NP_zT along ``axis``.  One box may come
    without the leading axis, and then so do the results."""
    cells, pos, single = host_boxes(cells, pos)
    vel = _like_pos(vel, pos, single, "vel")
    pos_ref = _like_pos(pos_ref, pos, single, "pos_ref")
    nb, n = pos.shape[0], pos.shape[1]
    streams = _streams(streams, nb)
    nvec, kappas, anchors = _bias(nvec, kappa, anchor, nb)
    coupling = _coupling(coupling)
    L = _dev.live()
    pos_out, vel_out, forces, ref_out = (np.zeros((nb, n, 3)) for _ in range(4))
    cells_out = np.zeros((nb, 3, 3))
    trace = np.zeros((nb, _nrows(nsteps, sample_every), len(TRACE_FIELDS)))
    blocks = np.zeros((nb, _nblocks(int(nsteps), int(equil_steps), int(block_steps)), len(BLOCK_FIELDS)))
    status = np.zeros((nb, 2), dtype=np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data                   # noqa: E731
    _dev.chk(L.mw_pin_run(nb, n, cells.ctypes.data, pos.ctypes.data, ptr(vel), ptr(pos_ref), nvec.ctypes.data, kappas.ctypes.data,
                          anchors.ctypes.data, ptr(streams), int(seed), int(step0), int(nsteps), int(sample_every), int(equil_steps),
                          int(block_steps), float(dt), float(mass), float(kT), float(gamma), float(pressure), float(tau_p), float(beta_T),
                          int(baro_every), coupling, int(axis), pos_out.ctypes.data, vel_out.ctypes.data, forces.ctypes.data,
                          cells_out.ctypes.data, ref_out.ctypes.data, trace.ctypes.data, blocks.ctypes.data if blocks.size else None,
                          status.ctypes.data))
    out = (pos_out, vel_out, forces, cells_out, ref_out, trace, blocks, status)
    return tuple(o[0] for o in out) if single else out


def interface_pinning_torch(cells_t, pos_t, nvec_t, kappa_t, anchor_t, nsteps, dt, pressure=ATM, kT=0.0, gamma=0.0, tau_p=TAU_P_DEFAULT,
                            beta_T=BETA_T_DEFAULT, baro_every=10, coupling="uniaxial", axis=2, vel_t=None, mass=MASS_WATER, seed=0, streams_t=None,
                            step0=0, sample_every=1, pos_ref_t=None, equil_steps=0, block_steps=0):
    """The same eight results as tensors on the device of the inputs: ``cells_t`` [nboxes, 3, 3], ``pos_t`` and the optional
    ``vel_t`` and ``pos_ref_t`` [nboxes, nwater, 3] contiguous float64 device tensors, ``nvec_t`` [nboxes, 3] int32, ``kappa_t`` and
    ``anchor_t`` [nboxes] float64, ``streams_t`` [nboxes] int64, all on the device the library lives on (mw_pin_run_device)."""
    import torch
    named = [(cells_t, torch.float64, "cells_t"), (pos_t, torch.float64, "pos_t"), (nvec_t, torch.int32, "nvec_t"),
             (kappa_t, torch.float64, "kappa_t"), (anchor_t, torch.float64, "anchor_t")]
    named += [(t, torch.float64, name) for t, name in ((vel_t, "vel_t"), (pos_ref_t, "pos_ref_t")) if t is not None]
    if streams_t is not None:
        named.append((streams_t, torch.int64, "streams_t"))
    dev = check_device_tensors(*named)
    check_boxes(cells_t, pos_t)
    nb, n = pos_t.shape[0], pos_t.shape[1]
    for t, name in ((vel_t, "vel_t"), (pos_ref_t, "pos_ref_t")):
        if t is not None and tuple(t.shape) != tuple(pos_t.shape):
            raise MwError(f"{name} {tuple(t.shape)}: expected the shape of pos_t, {tuple(pos_t.shape)}")
    for t, name, shape in ((nvec_t, "nvec_t", (nb, 3)), (kappa_t, "kappa_t", (nb,)), (anchor_t, "anchor_t", (nb,))):
        if tuple(t.shape) != shape:
            raise MwError(f"{name} {tuple(t.shape)}: expected {list(shape)}")
    if streams_t is not None and tuple(streams_t.shape) != (nb,):
        raise MwError(f"streams_t {tuple(streams_t.shape)}: expected one 64-bit stream identity per box, [{nb}]")
    coupling = _coupling(coupling)
    L = _dev.live(dev.index or 0)                  # raises if the library lives on another device
    f64 = dict(dtype=torch.float64, device=dev)
    pos_out, vel_out, forces, ref_out = (torch.zeros((nb, n, 3), **f64) for _ in range(4))
    cells_out = torch.zeros((nb, 3, 3), **f64)
    trace = torch.zeros((nb, _nrows(nsteps, sample_every), len(TRACE_FIELDS)), **f64)
    blocks = torch.zeros((nb, _nblocks(int(nsteps), int(equil_steps), int(block_steps)), len(BLOCK_FIELDS)), **f64)
    status = torch.zeros((nb, 2), dtype=torch.int32, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()                    # noqa: E731
    torch.cuda.synchronize(dev)
    _dev.chk(L.mw_pin_run_device(nb, n, cells_t.data_ptr(), pos_t.data_ptr(), ptr(vel_t), ptr(pos_ref_t), nvec_t.data_ptr(), kappa_t.data_ptr(),
                                 anchor_t.data_ptr(), ptr(streams_t), int(seed), int(step0), int(nsteps), int(sample_every), int(equil_steps),
                                 int(block_steps), float(dt), float(mass), float(kT), float(gamma), float(pressure), float(tau_p), float(beta_T),
                                 int(baro_every), coupling, int(axis), pos_out.data_ptr(), vel_out.data_ptr(), forces.data_ptr(),
                                 cells_out.data_ptr(), ref_out.data_ptr(), trace.data_ptr(), blocks.data_ptr() if blocks.numel() else None,
                                 status.data_ptr()))
    return pos_out, vel_out, forces, cells_out, ref_out, trace, blocks, status


# ---- host helpers -------------------------------------------------------------------------------------------------------
def _half_space(nmax, axis):
    """int32 [M, 3]: one of every pair +-n with |n_a| <= nmax, n != 0 (the half space of structure.kvectors); n[axis] = 0 when
    ``axis`` is given."""
    r = np.arange(-int(nmax), int(nmax) + 1)
    n = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    n = n[(n[:, 0] > 0) | ((n[:, 0] == 0) & ((n[:, 1] > 0) | ((n[:, 1] == 0) & (n[:, 2] > 0))))]
    if axis is not None:
        if int(axis) not in (0, 1, 2):
            raise MwError(f"axis = {axis}: expected 0, 1, 2 or None")
        n = n[n[:, int(axis)] == 0]
    return np.ascontiguousarray(n, dtype=np.int32)


def choose_wavevector(cell, pos, axis=None, nmax=8):
    """The integer triple with the largest S(n) of the box ``cell`` [3, 3] / ``pos`` [nwater, 3] among one of every pair +-n
    with |n_a| <= ``nmax``, from structure.structure_factor (the first in lexicographic order of equals).  With ``axis`` given,
    n[axis] = 0: a mode in the plane of an interface normal to that axis, which the interface does not modulate."""
    if not 1 <= int(nmax) <= MAX_N:
        raise MwError(f"nmax = {nmax} outside 1..{MAX_N}")
    from . import structure
    n = _half_space(nmax, axis)
    S = structure.structure_factor(np.asarray(cell, dtype=np.float64).reshape(3, 3), np.asarray(pos, dtype=np.float64), n)
    return n[int(np.argmax(S.reshape(-1)))].copy()


def order_parameter(cells, pos, nvec):
    """Q = sqrt(S(n)) [nboxes] of the boxes ``cells`` / ``pos`` for the one triple ``nvec`` [3], from structure.structure_factor;
    one box without the leading axis gives a float."""
    from . import structure
    single = np.asarray(pos).ndim == 2
    S = structure.structure_factor(cells, pos, np.asarray(nvec, dtype=np.int32).reshape(1, 3))
    q = np.sqrt(np.asarray(S, dtype=np.float64).reshape(-1))
    return float(q[0]) if single else q


def delta_mu(blocks, kappa, anchor, q_solid, q_liquid, nwater):
    """(mu_solid - mu_liquid, its standard error) in Hartree per molecule from the ``blocks`` [nblocks, 4] of one box:
    -kappa (<Q> - anchor) (q_solid - q_liquid) / nwater, with <Q> the mean of the block means and the error from their spread
    (at least two blocks).  ``q_solid`` and ``q_liquid`` are Q of the box all solid and all liquid."""
    b = np.asarray(blocks, dtype=np.float64)
    if b.ndim != 2 or b.shape[1] != len(BLOCK_FIELDS) or b.shape[0] < 2:
        raise MwError(f"blocks {b.shape}: expected [nblocks >= 2, {len(BLOCK_FIELDS)}] of one box")
    slope = -float(kappa) * (float(q_solid) - float(q_liquid)) / float(nwater)
    q = b[:, 0]
    return slope * (q.mean() - float(anchor)), abs(slope) * q.std(ddof=1) / math.sqrt(len(q))


def anchor_for_fraction(q_solid, q_liquid, fraction):
    """The anchor at which the fraction ``fraction`` of the box is crystal: Q is linear in the amount of crystal between
    ``q_liquid`` (0) and ``q_solid`` (1)."""
    if not 0.0 <= float(fraction) <= 1.0:
        raise MwError(f"fraction = {fraction} outside 0..1")
    return float(q_liquid) + float(fraction) * (float(q_solid) - float(q_liquid))
