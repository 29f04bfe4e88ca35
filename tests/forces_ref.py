"""Vectorised numpy reference for the gradient of the mW full-box energy: energy, forces and virial of one box from
(xyz, ivect, nn, jn, vn) -- the reference's list layout, 1-based -- and the engine's constants (tests/golden/constants.npz).

It is written independently of the engine's moment formulation (mw_forces.hip.h): the three-body term is differentiated
triplet by triplet, and every derivative is scattered onto both molecules it moves, so

  E = 1/2 sum_i sum_k phi(r_ik) + lambda eps sum_i sum_{k<l} g_k g_l (cos theta_kl - cos0)^2     (molint.F90:407-499)
  F = -dE/dr,  W_ab = -sum_i sum_k (dE/dd_ik)_a (d_ik)_b                                     (homogeneous strain)

with d_ik = r_j + ivect - r_i over in-range list entries (|d|^2 < (a sigma)^2).  An entry of a molecule's own image has a
constant d: it moves nothing, but it is part of the energy and of the virial.  tests/test_forces_ref.py checks this module
against central differences of the C oracle's energy.
"""
from __future__ import annotations

import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def constants():
    """sigma, epsilon, lambda, A, B, gamma, a, cos0 as the engine holds them (cos0 is the float32-widened value)."""
    return np.load(os.path.join(GOLDEN, "constants.npz"))["constants"]


def model_forces(xyz, ivect, nn, jn, vn, chunk=4096):
    """(energy, forces [N, 3], virial [3, 3]) of one box.  ``chunk`` molecules are expanded at a time."""
    sigma, eps, lam, big_a, big_b, gamma, small_a, cos0 = (float(c) for c in constants())
    xyz = np.asarray(xyz, dtype=np.float64)
    ivect = np.asarray(ivect, dtype=np.float64)
    n = len(xyz)
    rcsq = sigma * small_a * sigma * small_a
    sig_a = sigma * small_a
    aeps, lam_eps, gam_sig = big_a * eps, lam * eps, gamma * sigma

    e_pair = 0.0
    e_trip = 0.0
    force = np.zeros((n, 3))
    virial = np.zeros((3, 3))
    slots = np.arange(jn.shape[1])
    for i0 in range(0, n, chunk):
        i1 = min(n, i0 + chunk)
        ii = np.arange(i0, i1)
        live = slots[None, :] < nn[i0:i1, None]
        j = np.where(live, jn[i0:i1] - 1, 0)
        v = np.where(live, vn[i0:i1] - 1, 0)
        d = (xyz[j] + ivect[v]) - xyz[ii][:, None, :]                     # molint.F90:447,450
        r2 = np.einsum("nsc,nsc->ns", d, d)
        inr = live & (r2 < rcsq)                                          # :454
        # in-range entries first (list order kept), then only as many columns as the fullest molecule needs
        perm = np.argsort(~inr, axis=1, kind="stable")
        kmax = max(1, int(inr.sum(axis=1).max()))
        perm = perm[:, :kmax]
        inr = np.take_along_axis(inr, perm, 1)
        j = np.take_along_axis(j, perm, 1)
        d = np.take_along_axis(d, perm[:, :, None], 1)
        r2 = np.where(inr, np.take_along_axis(r2, perm, 1), 1.0)

        r = np.sqrt(r2)
        den = np.where(inr, r - sig_a, -1.0)
        with np.errstate(over="ignore", under="ignore"):
            e1 = np.where(inr, np.exp(sigma / den), 0.0)
            g = np.where(inr, np.exp(gam_sig / den), 0.0)
        q = sigma * sigma / r2
        phi = aeps * (big_b * q * q - 1.0) * e1
        dphi = -e1 * (4.0 * aeps * big_b * q * q / r + aeps * (big_b * q * q - 1.0) * sigma / (den * den))
        dg = -gam_sig * g / (den * den)
        u = d / r[:, :, None]

        # triplets (k, l), k != l, of the same centre: T = 1/2 sum_{k != l} g_k g_l (c_kl - cos0)^2
        c = np.einsum("nkc,nlc->nkl", u, u)
        off = inr[:, :, None] & inr[:, None, :] & ~np.eye(kmax, dtype=bool)[None]
        x = np.where(off, c - cos0, 0.0)
        gg = g[:, :, None] * g[:, None, :]
        e_pair += 0.5 * phi[inr].sum()
        e_trip += 0.5 * (gg * x * x).sum()
        # dT/dd_k = sum_{l != k} [ g'_k g_l x^2 u_k + g_k g_l 2 x (u_l - c_kl u_k) / r_k ]
        a1 = (dg[:, :, None] * g[:, None, :] * x * x).sum(axis=2)                        # coefficient of u_k
        b = 2.0 * gg * x / r[:, :, None]
        t = a1[:, :, None] * u + np.einsum("nkl,nlc->nkc", b, u) - (b * c).sum(axis=2)[:, :, None] * u
        grad = 0.5 * dphi[:, :, None] * u + lam_eps * t                                   # dE/dd_k, entry by entry
        grad = np.where(inr[:, :, None], grad, 0.0)

        virial -= np.einsum("nka,nkb->ab", grad, d)
        moves = inr & (j != ii[:, None])                                  # d_k = r_j + ivect - r_i: dd/dr_j = I, dd/dr_i = -I
        gm = np.where(moves[:, :, None], grad, 0.0)
        force[i0:i1] += gm.sum(axis=1)
        np.add.at(force, j[moves], -gm[moves])
    return e_pair + lam_eps * e_trip, force, virial


def strained(h, xyz, strain):
    """Cell and positions under the homogeneous deformation x -> (I + strain) x (rows of h are the cell vectors)."""
    m = np.eye(3) + strain
    return np.asarray(h) @ m.T, np.asarray(xyz) @ m.T


def virial_pressure(virial, volume, nmol, temperature_k, kb=1.0 / 3.1577465e5):
    """Instantaneous pressure (N k_B T + tr W / 3) / V in Hartree / bohr^3."""
    return (nmol * kb * temperature_k + np.trace(virial) / 3.0) / volume
