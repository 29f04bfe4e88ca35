"""The Hessian of the full-box mW energy over the C ABI of ``libmw_hess.so`` (include/mw_hess.h) and the harmonic analysis on
top of it: the dense Gamma-point Hessian of every box, its products with given vectors, normal modes, the harmonic free
energy, the density of modes and their participation ratios.

A cell ``h`` is a [3, 3] array whose ROW k is the lattice vector h_(k+1) (``EnergyModule.hmatrix[b]``, the layout of
``mw_set_cell``).  Positions are in bohr, energies in Hartree, the Hessian in Hartree / bohr^2; with the mass in electron
masses the frequencies come out in atomic units (Hartree / hbar), and ``kT`` is in Hartree.  The device does the second
derivatives; the eigenproblem and what follows from it are host arithmetic in numpy.  There is no CPU path for the Hessian:
without the library or a device those calls raise.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from ._devlib import DevLib, MwError, check_boxes, check_device_tensors, host_boxes

PKG = os.path.dirname(os.path.abspath(__file__))
HESS_LIB_PATH = os.path.join(PKG, "libmw_hess.so")

#: every symbol include/mw_hess.h declares
HESS_ABI_SYMBOLS = ("mw_hess_init", "mw_hess_finalize", "mw_hess_is_initialised", "mw_hess_last_error", "mw_hess_matvec",
                    "mw_hess_matvec_device", "mw_hess_dense", "mw_hess_dense_device", "mw_hess_plan", "mw_hess_last", "mw_hess_elapsed_ms")
#: the fields of mw_hess_plan / mw_hess_last, in order
PLAN_FIELDS = ("boxes_per_chunk", "chunks", "g1", "g2", "g3", "lds_bytes", "scratch_bytes_per_box", "vectors_per_group")
MAX_VEC = 1024
VEC_GROUP = 32
MAX_DENSE_WATER = 8192
#: the mass of a water molecule in electron masses (18.01528 u)
MASS_WATER = 18.01528 * 1822.888486209
#: Boltzmann's constant in Hartree / K
KB_HARTREE = 1.0 / 3.1577465e5


def _argtypes(L):
    for f in (L.mw_hess_matvec, L.mw_hess_matvec_device):
        f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    for f in (L.mw_hess_dense, L.mw_hess_dense_device):
        f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.mw_hess_plan.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int]


class _HessLib(DevLib):
    def fields(self, out):                         # (this library has one geometry: no `small` field)
        return dict(zip(self.plan_fields, (int(v) for v in out)))


_dev = _HessLib("hess", HESS_LIB_PATH, "the Hessian", PLAN_FIELDS, setup=_argtypes)

load_hess_library = _dev.load                    # (path=HESS_LIB_PATH): dlopen libmw_hess.so; raises if it has not been built
hess_finalize = _dev.finalize
hess_last = _dev.last                            # the fields of hess_plan for the last call that launched (the grid is that of its first box)


def hess_init(device=0):
    """Initialise the library on ``device`` (the compute functions do it on device 0 when nobody has)."""
    return _dev.live(device)


def hess_plan(nwater, cell, nboxes=1, nvec=1, dense=False):
    """{field: value} of PLAN_FIELDS: the launch rules of ``nboxes`` boxes of ``nwater`` molecules with the cell ``cell``
    [3, 3] (bohr) for products with ``nvec`` vectors, or with ``dense`` for the dense matrix through host arrays
    (mw_hess_plan), no device needed."""
    L = _dev.load()
    out = _dev.plan_out()
    cell = np.ascontiguousarray(cell, dtype=np.float64)
    if cell.shape != (3, 3):
        raise MwError(f"cell {cell.shape}: expected [3, 3]")
    _dev.chk(L.mw_hess_plan(int(nwater), cell.ctypes.data, int(nboxes), int(nvec), 1 if dense else 0, out, len(out)))
    return _dev.fields(out)


def hess_elapsed_ms():
    """(sort, moment pass with the forces, products, dense assembly) of the last call in milliseconds, summed over its
    chunks and vector groups, from the library's event timers."""
    L = _dev.load()
    t = [ctypes.c_float(0.0) for _ in range(4)]
    _dev.chk(L.mw_hess_elapsed_ms(*[ctypes.byref(v) for v in t]))
    return tuple(v.value for v in t)


def hessian(cells, pos):
    """(H [nboxes, 3 nwater, 3 nwater], ef [nboxes, 2]) of the boxes ``cells`` [nboxes, 3, 3] / ``pos`` [nboxes, nwater, 3]
    in bohr: the Gamma-point Hessian in Hartree / bohr^2, row 3 i + a and column 3 j + b, and beside it the energy and the
    largest |F| component of every box (at a minimum the latter is the quench's ``ftol`` or less).  One box may come without
    the leading axis, and then so do the results."""
    cells, pos, single = host_boxes(cells, pos)
    L = _dev.live()
    nb, n = pos.shape[0], pos.shape[1]
    H = np.zeros((nb, 3 * n, 3 * n))
    ef = np.zeros((nb, 2))
    _dev.chk(L.mw_hess_dense(nb, n, cells.ctypes.data, pos.ctypes.data, H.ctypes.data, ef.ctypes.data))
    return (H[0], ef[0]) if single else (H, ef)


def hessian_torch(cells_t, pos_t):
    """(H [nboxes, 3 nwater, 3 nwater], ef [nboxes, 2]) as float64 tensors on the device of the inputs: ``cells_t``
    [nboxes, 3, 3] and ``pos_t`` [nboxes, nwater, 3], contiguous float64 device tensors on the device the library lives on
    (mw_hess_dense_device: the matrices are written where they stay, not staged)."""
    import torch
    dev = check_device_tensors((cells_t, torch.float64, "cells_t"), (pos_t, torch.float64, "pos_t"))
    check_boxes(cells_t, pos_t)
    L = _dev.live(dev.index or 0)                  # raises if the library lives on another device
    nb, n = pos_t.shape[0], pos_t.shape[1]
    H = torch.empty((nb, 3 * n, 3 * n), dtype=torch.float64, device=dev)
    ef = torch.zeros((nb, 2), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    _dev.chk(L.mw_hess_dense_device(nb, n, cells_t.data_ptr(), pos_t.data_ptr(), H.data_ptr(), ef.data_ptr()))
    return H, ef


def _host_vecs(vecs, pos, single):
    vecs = np.ascontiguousarray(vecs, dtype=np.float64)
    if single:
        vecs = vecs[None]
    if vecs.ndim == 3:                             # one vector per box
        vecs = vecs[:, None]
        one = True
    else:
        one = False
    if vecs.ndim != 4 or vecs.shape[0] != pos.shape[0] or tuple(vecs.shape[2:]) != tuple(pos.shape[1:]):
        raise MwError(f"vecs {tuple(vecs.shape)}: expected [nboxes, nvec, nwater, 3] for pos {tuple(pos.shape)}")
    return np.ascontiguousarray(vecs), one


def hessian_matvec(cells, pos, vecs):
    """(out, ef [nboxes, 2]): out[b, v] = H_b vecs[b, v] for ``vecs`` [nboxes, nvec, nwater, 3] (at most MAX_VEC vectors per
    box), never forming H, and the energy and the largest |F| component of every box.  One box may come without the leading
    axis (``vecs`` [nvec, nwater, 3]), and then so do the results."""
    cells, pos, single = host_boxes(cells, pos)
    if single and np.ndim(vecs) == 2:
        raise MwError("vecs: expected [nvec, nwater, 3] for a single box")
    vecs, _ = _host_vecs(vecs, pos, single)
    L = _dev.live()
    nb, n, nvec = pos.shape[0], pos.shape[1], vecs.shape[1]
    out = np.zeros_like(vecs)
    ef = np.zeros((nb, 2))
    _dev.chk(L.mw_hess_matvec(nb, n, cells.ctypes.data, pos.ctypes.data, nvec, vecs.ctypes.data, out.ctypes.data, ef.ctypes.data))
    return (out[0], ef[0]) if single else (out, ef)


def hessian_matvec_torch(cells_t, pos_t, vecs_t):
    """(out [nboxes, nvec, nwater, 3], ef [nboxes, 2]) as float64 tensors on the device of the inputs, all of them contiguous
    float64 device tensors on the device the library lives on (mw_hess_matvec_device)."""
    import torch
    dev = check_device_tensors((cells_t, torch.float64, "cells_t"), (pos_t, torch.float64, "pos_t"), (vecs_t, torch.float64, "vecs_t"))
    check_boxes(cells_t, pos_t)
    if vecs_t.ndim != 4 or vecs_t.shape[0] != pos_t.shape[0] or tuple(vecs_t.shape[2:]) != tuple(pos_t.shape[1:]):
        raise MwError(f"vecs_t {tuple(vecs_t.shape)}: expected [nboxes, nvec, nwater, 3] for pos_t {tuple(pos_t.shape)}")
    L = _dev.live(dev.index or 0)
    nb, n, nvec = pos_t.shape[0], pos_t.shape[1], vecs_t.shape[1]
    out = torch.zeros_like(vecs_t)
    ef = torch.zeros((nb, 2), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    _dev.chk(L.mw_hess_matvec_device(nb, n, cells_t.data_ptr(), pos_t.data_ptr(), nvec, vecs_t.data_ptr(), out.data_ptr(), ef.data_ptr()))
    return out, ef


# ---- host arithmetic -----------------------------------------------------------------------------------------------------

def normal_modes(H, mass=MASS_WATER, vectors=False):
    """The signed frequencies omega = sign(lambda) sqrt(|lambda| / mass) of the eigenvalues lambda of (H + H^T) / 2 in ascending
    order (a negative one stands for an imaginary frequency: an unstable direction), and with ``vectors`` the eigenvectors
    [3 n, 3 n] as columns in the same order."""
    H = np.asarray(H, dtype=np.float64)
    if H.ndim != 2 or H.shape[0] != H.shape[1]:
        raise MwError(f"H {H.shape}: expected a square matrix")
    if not mass > 0.0:
        raise MwError(f"mass = {mass} is not positive")
    sym = 0.5 * (H + H.T)
    if vectors:
        lam, vec = np.linalg.eigh(sym)
    else:
        lam, vec = np.linalg.eigvalsh(sym), None
    omega = np.sign(lam) * np.sqrt(np.abs(lam) / mass)
    return (omega, vec) if vectors else omega


def harmonic_free_energy(omega, kT, quantum=False, nzero=3):
    """The vibrational free energy of the modes ``omega`` (atomic units, hbar = 1) at ``kT`` (Hartree) without the ``nzero``
    modes of smallest |omega| (the translations of a periodic box): classically kT sum ln(omega / kT), with ``quantum``
    sum [omega / 2 + kT ln(1 - exp(-omega / kT))].  A kept mode with omega <= 0 raises: the configuration is not a minimum."""
    omega = np.asarray(omega, dtype=np.float64).ravel()
    if not kT > 0.0:
        raise MwError(f"kT = {kT} is not positive")
    if nzero < 0 or nzero > omega.size:
        raise MwError(f"nzero = {nzero} outside 0..{omega.size}")
    keep = omega[np.argsort(np.abs(omega), kind="stable")[nzero:]]
    if keep.size and keep.min() <= 0.0:
        raise MwError(f"harmonic_free_energy: {int((keep <= 0.0).sum())} of the kept modes are not positive (the lowest is {keep.min():.6g}): "
                      "not a minimum")
    if quantum:
        return float(np.sum(0.5 * keep + kT * np.log1p(-np.exp(-keep / kT))))
    return float(kT * np.sum(np.log(keep / kT)))


def mode_dos(omega, edges):
    """The number of modes in each bin [edges[k], edges[k + 1]) (the last bin closed), as numpy.histogram counts them."""
    return np.histogram(np.asarray(omega, dtype=np.float64).ravel(), bins=np.asarray(edges, dtype=np.float64))[0]


def participation_ratio(vectors):
    """p_m = (sum_i |e_im|^2)^2 / (N sum_i |e_im|^4) of the eigenvectors ``vectors`` [3 N, modes] (columns): 1 for a mode every
    molecule shares equally, 1 / N for one that moves a single molecule."""
    v = np.asarray(vectors, dtype=np.float64)
    if v.ndim == 1:
        v = v[:, None]
    if v.shape[0] % 3:
        raise MwError(f"vectors {v.shape}: expected [3 N, modes]")
    n = v.shape[0] // 3
    w = (v.reshape(n, 3, -1) ** 2).sum(axis=1)
    return w.sum(axis=0) ** 2 / (n * (w * w).sum(axis=0))
