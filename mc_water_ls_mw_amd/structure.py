"""The static structure factor S(k) over the C ABI of ``libmw_sk.so`` (include/mw_sk.h), the reciprocal-space companion of
``energy.rdf_from_counts``.

A cell ``h`` is a [3, 3] array whose ROW k is the lattice vector h_(k+1) (``EnergyModule.hmatrix[b]``, the layout of
``mw_set_cell``), lengths in bohr.  For an integer triple n the wave vector is k_n = 2 pi H^-T n, i.e. ``2 pi inv(h) @ n``;
rho(n) = sum_j exp(-i k_n . r_j) and S(n) = |rho(n)|^2 / N.  The library needs positions and cells only: it works on any
configuration, with or without an engine in the process.  There is no CPU path: without the library or a device the calls
raise.  Shell averages over |k| are host arithmetic (:func:`sq_from_sk`).
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from ._devlib import DevLib, MwError, check_boxes, check_device_tensors, host_boxes

PKG = os.path.dirname(os.path.abspath(__file__))
SK_LIB_PATH = os.path.join(PKG, "libmw_sk.so")
BOHR_TO_ANG = 0.5291772108                      # constants.f90:42-43, as energy.py converts
MAX_VECTORS = 1 << 20
MAX_COMPONENT = 255

#: every symbol include/mw_sk.h declares
SK_ABI_SYMBOLS = ("mw_sk_init", "mw_sk_finalize", "mw_sk_is_initialised", "mw_sk_last_error", "mw_sk_compute",
                  "mw_sk_compute_device", "mw_sk_mean", "mw_sk_plan", "mw_sk_last", "mw_sk_elapsed_ms")
#: the fields of mw_sk_plan / mw_sk_last, in order
PLAN_FIELDS = ("boxes_per_chunk", "chunks", "kvec_per_lane", "segments", "lds_bytes", "small", "tile", "segment_length",
               "kvec_per_workgroup")

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)
_dev = DevLib("sk", SK_LIB_PATH, "S(k)", PLAN_FIELDS)

load_sk_library = _dev.load                     # (path=SK_LIB_PATH): dlopen libmw_sk.so; raises if it has not been built
sk_finalize = _dev.finalize
sk_last = _dev.last                             # the fields of sk_plan for the last call that launched


def sk_init(device=0):
    """Initialise the library on ``device`` (the compute functions do it on device 0 when nobody has)."""
    return _dev.live(device)


def sk_plan(nwater, nmax, M, nboxes=1):
    """{field: value} of PLAN_FIELDS: the launch rules of a call (mw_sk_plan), no device needed."""
    L = _dev.load()
    out = _dev.plan_out()
    nm = (ctypes.c_int * 3)(*[int(v) for v in nmax])
    _dev.chk(L.mw_sk_plan(int(nwater), nm, int(M), int(nboxes), out, len(out)))
    return _dev.fields(out)


def sk_elapsed_ms():
    """(table pass, sums) of the last call in milliseconds, from the library's event timers."""
    L = _dev.load()
    a, b = ctypes.c_float(0.0), ctypes.c_float(0.0)
    _dev.chk(L.mw_sk_elapsed_ms(ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


# -- wave vectors (host arithmetic) ---------------------------------------------------------
def _kvec_bohr(h, nvec):
    """k_n in 1 / bohr, [M, 3]."""
    g = 2.0 * np.pi * np.linalg.inv(np.asarray(h, dtype=np.float64))       # column a = b_(a+1): k = sum_a n_a b_a
    return np.asarray(nvec, dtype=np.float64) @ g.T


def k_lengths(h, nvec):
    """|k_n| in 1 / Angstrom for the triples ``nvec`` [M, 3] of the cell ``h`` (bohr)."""
    return np.linalg.norm(_kvec_bohr(h, nvec), axis=1) / BOHR_TO_ANG


def kvectors(h, k_max_ang, half=True):
    """int32 [M, 3]: every integer triple n with 0 < |k_n| <= ``k_max_ang`` (1 / Angstrom) for the cell ``h`` (bohr), sorted
    by |k| and then lexicographically.  ``half``: only the half space n1 > 0, or n1 = 0 and n2 > 0, or n1 = n2 = 0 and
    n3 > 0 -- S(-n) = S(n), so the other half carries nothing new."""
    h = np.asarray(h, dtype=np.float64)
    kmax = float(k_max_ang) * BOHR_TO_ANG                                   # 1 / bohr
    # |n_a| = |h_a . k| / (2 pi) <= |h_a| |k| / (2 pi)
    lim = np.floor(np.linalg.norm(h, axis=1) * kmax / (2.0 * np.pi) + 1e-9).astype(np.int64)
    if lim.max(initial=0) > MAX_COMPONENT:
        raise MwError(f"k_max = {k_max_ang} / Angstrom needs components up to {int(lim.max())}, beyond {MAX_COMPONENT}")
    axes = [np.arange(0 if (half and a == 0) else -lim[a], lim[a] + 1) for a in range(3)]
    n = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
    if half:
        n = n[(n[:, 0] > 0) | ((n[:, 0] == 0) & ((n[:, 1] > 0) | ((n[:, 1] == 0) & (n[:, 2] > 0))))]
    else:
        n = n[np.any(n != 0, axis=1)]
    k = np.linalg.norm(_kvec_bohr(h, n), axis=1)
    keep = k <= kmax
    n, k = n[keep], k[keep]
    order = np.lexsort((n[:, 2], n[:, 1], n[:, 0], k))
    return np.ascontiguousarray(n[order], dtype=np.int32)


def sq_from_sk(S, klen, q_max_ang, nbins):
    """(q [nbins], Sq [..., nbins], count [nbins]): the shell average of ``S`` [..., M] over ``nbins`` equal bins of |k| on
    (0, q_max_ang], bin b holding b dq < |k| <= (b + 1) dq with dq = q_max_ang / nbins; q are the bin centres, count the
    vectors per bin, and Sq is NaN where a bin is empty.  Host arithmetic only."""
    S = np.asarray(S, dtype=np.float64)
    klen = np.asarray(klen, dtype=np.float64)
    nbins = int(nbins)
    dq = float(q_max_ang) / nbins
    b = np.ceil(klen / dq).astype(np.int64) - 1
    ok = (klen > 0.0) & (b >= 0) & (b < nbins)
    count = np.bincount(b[ok], minlength=nbins).astype(np.int64)
    flat = S.reshape(-1, S.shape[-1])
    tot = np.stack([np.bincount(b[ok], weights=row[ok], minlength=nbins) for row in flat])
    with np.errstate(invalid="ignore", divide="ignore"):
        sq = np.where(count > 0, tot / count, np.nan)
    return (np.arange(nbins) + 0.5) * dq, sq.reshape(S.shape[:-1] + (nbins,)), count


# -- the device calls -------------------------------------------------------------------------
def _arrays(cells, pos, nvec):
    cells, pos, _ = host_boxes(cells, pos)
    nvec = np.ascontiguousarray(nvec, dtype=np.int32)
    if nvec.ndim != 2 or nvec.shape[1] != 3:
        raise MwError(f"nvec {nvec.shape}: expected [M, 3]")
    return cells, pos, nvec


def structure_factor(cells, pos, nvec, want_rho=False):
    """S [nboxes, M] of the boxes ``cells`` [nboxes, 3, 3] / ``pos`` [nboxes, nwater, 3] (bohr; one box may come without the
    leading axis) for the triples ``nvec`` [M, 3]; with ``want_rho`` also rho as a complex array [nboxes, M]."""
    cells, pos, nvec = _arrays(cells, pos, nvec)
    L = _dev.live()
    nb, n, M = pos.shape[0], pos.shape[1], nvec.shape[0]
    S = np.zeros((nb, M))
    rho = np.zeros((nb, M, 2)) if want_rho else None
    _dev.chk(L.mw_sk_compute(nb, n, cells.ctypes.data_as(_dp), pos.ctypes.data_as(_dp), M, nvec.ctypes.data_as(_ip),
                             None if rho is None else rho.ctypes.data_as(_dp), S.ctypes.data_as(_dp)))
    if want_rho:
        return S, rho[..., 0] + 1j * rho[..., 1]
    return S


def structure_factor_mean(cells, pos, nvec, ngroups):
    """S_mean [ngroups, M]: box w * ngroups + g is walker w's box of group g; the mean over the walkers, taken on the device
    in walker order (mw_sk_mean)."""
    cells, pos, nvec = _arrays(cells, pos, nvec)
    L = _dev.live()
    nb, n, M = pos.shape[0], pos.shape[1], nvec.shape[0]
    out = np.zeros((max(int(ngroups), 0), M))
    _dev.chk(L.mw_sk_mean(nb, n, cells.ctypes.data_as(_dp), pos.ctypes.data_as(_dp), M, nvec.ctypes.data_as(_ip), int(ngroups),
                          out.ctypes.data_as(_dp)))
    return out


def structure_factor_torch(cells_t, pos_t, nvec_t):
    """(S [nboxes, M], rho [nboxes, M, 2]) as float64 tensors on the device of the inputs: ``cells_t`` [nboxes, 3, 3] and
    ``pos_t`` [nboxes, nwater, 3] float64, ``nvec_t`` [M, 3] int32, contiguous device tensors on the device the library
    lives on (mw_sk_compute_device)."""
    import torch
    dev = check_device_tensors((cells_t, torch.float64, "cells_t"), (pos_t, torch.float64, "pos_t"), (nvec_t, torch.int32, "nvec_t"))
    check_boxes(cells_t, pos_t)
    if nvec_t.dim() != 2 or nvec_t.shape[1] != 3:
        raise MwError(f"nvec_t {tuple(nvec_t.shape)}: expected [M, 3]")
    L = _dev.live(dev.index or 0)                  # raises if the library lives on another device
    nb, n, M = pos_t.shape[0], pos_t.shape[1], nvec_t.shape[0]
    S = torch.zeros((nb, M), dtype=torch.float64, device=dev)
    rho = torch.zeros((nb, M, 2), dtype=torch.float64, device=dev)
    torch.cuda.synchronize(dev)
    _dev.chk(L.mw_sk_compute_device(nb, n, ctypes.c_void_p(cells_t.data_ptr()), ctypes.c_void_p(pos_t.data_ptr()), M,
                                    ctypes.c_void_p(nvec_t.data_ptr()), ctypes.c_void_p(rho.data_ptr()),
                                    ctypes.c_void_p(S.data_ptr())))
    return S, rho
