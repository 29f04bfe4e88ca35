"""The reference of the second derivatives of include/mw_hess.h: the full-box mW energy restated in torch float64 on the CPU
and differentiated by autograd, and the cases tests/test_hess_ref.py (CPU, the preconditions) and tests/test_gpu_hess.py (the
device) share.

It shares no code with the device library and holds no hand-derived second derivative.  The entries of a molecule are found
by brute force over the 27 translations n in {-1, 0, 1}^3, which is every image that can come within a sigma in the supported
range (every perpendicular width of the cell at least a sigma): (j, n) with |r_j + n H - r_i|^2 < (a sigma)^2, a molecule's own
images left out (none is in range there).  The energy is the one of include/mw_quench.h,

  E = 1/2 sum_i sum_k phi(r_k) + lambda eps sum_i sum_{k<l} g_k g_l (u_k . u_l - cos0)^2,

the three-body term written triplet by triplet, not through the moments.  Which entries are in range is decided once at the
given positions (the derivative of a fixed list: phi, g and all their derivatives vanish at the cutoff).

What the reference itself is good for, measured on the CPU over the cases below: |E - forces_ref E| <= 9e-16 Hartree,
|grad E + F of forces_ref| <= 2e-15, the asymmetry of H <= 6e-17 and the acoustic sum rule <= 1e-16 in units where max |H| is
8.7e-3 (dimer), 9.4 (gas20) and 0.016 ... 0.37 (the ice boxes): about 1e-14 of max |H|.

FD_GAP_MEASURED: central differences of forces_ref.model_forces at h = 1e-4 bohr along a seeded unit vector against the
reference's H v, as a fraction of max |H v|, measured on the CPU: 1.2e-10 ... 3.5e-10 on the ice boxes of up to 96 molecules
(ic48_t015 2.7e-10, ic64_sheared 3.5e-10, ic65_interstitial 1.6e-10, ic96 1.2e-10, ih96_disordered 1.9e-10), 1.0e-9 on gas20,
2.3e-9 on ih1536_t012 and 2.6e-9 on narrow6 (the truncation error of the differences, h^2 times the fourth derivative, which
is largest where molecules are close).  FD_GAP_MEASURED is the largest of them; tests/test_hess_ref.py measures them again,
prints them and holds each to ten times that.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from forces_ref import constants
from quench_ref import load_case as _load_quench_case

#: the largest gap of the central-difference check, as a fraction of max |H v| (module docstring)
FD_GAP_MEASURED = 2.6e-9
FD_STEP = 1e-4                                                        # bohr

#: every case with a dense reference (at most 96 molecules)
DENSE_CASES = ("dimer", "single_atom", "gas20", "ic48_t015", "ic64_sheared", "ic65_interstitial", "ic96", "ih96_disordered", "narrow6", "sc80")
#: matvec only: the box that spans several workgroups
LARGE_CASE = "ih1536_t012"
MATVEC_CASES = DENSE_CASES + (LARGE_CASE,)
#: cases the C oracle's lists cover: all of them
ORACLE_CASES = ("dimer", "single_atom", "gas20", "ic48_t015", "ic64_sheared", "ic65_interstitial", "ic96", "ih96_disordered", "ih1536_t012", "narrow6", "sc80")
NARROW_SEED = 3
#: the columns of a row of the dense matrix that the device keeps in its on-chip table (include/mw_hess.h); ``sc80`` has more
TABLE_COLUMNS = 64


def rc():
    sigma, _, _, _, _, _, small_a, _ = (float(c) for c in constants())
    return sigma * small_a


@functools.lru_cache(maxsize=None)
def load_case(name):
    """(h [3, 3], xyz [n, 3]) in bohr, read-only.  ``narrow6``: 6 molecules drawn by a seeded generator in a cubic cell of side
    1.1 a sigma, a draw rejected while it comes within 4 bohr of an earlier molecule (minimum image); the seed is one at which
    some molecule has two images of the same neighbour among its entries (tests/test_hess_ref.py asserts it).  ``sc80``: a
    5 x 4 x 4 simple cubic lattice of spacing 4.5 bohr, every molecule moved by a seeded step of at most 0.3 bohr per axis: 26
    entries per molecule, and every row of H has blocks in more columns than TABLE_COLUMNS."""
    if name == "sc80":
        rng = np.random.default_rng(80)
        grid = np.array([[x, y, z] for x in range(5) for y in range(4) for z in range(4)], dtype=np.float64)
        h = np.diag([5.0, 4.0, 4.0]) * 4.5
        xyz = grid * 4.5 + rng.uniform(-0.3, 0.3, size=grid.shape)
        h.setflags(write=False), xyz.setflags(write=False)
        return h, xyz
    if name != "narrow6":
        return _load_quench_case(name)
    side = 1.1 * rc()
    h = np.eye(3) * side
    rng = np.random.default_rng(NARROW_SEED)
    pts = []
    while len(pts) < 6:
        p = rng.random(3) * side
        ok = True
        for q in pts:
            d = p - q
            d -= side * np.round(d / side)
            ok = ok and float(np.sqrt((d * d).sum())) > 4.0
        if ok:
            pts.append(p)
    xyz = np.array(pts)
    h.setflags(write=False), xyz.setflags(write=False)
    return h, xyz


def entries(h, xyz):
    """(i, j, shift [m, 3] in bohr, n [m, 3] integers) of every entry, ordered by i."""
    h, xyz = np.asarray(h, dtype=np.float64), np.asarray(xyz, dtype=np.float64)
    n = len(xyz)
    rcsq = rc() ** 2
    out = []
    for tz in (-1, 0, 1):
        for ty in (-1, 0, 1):
            for tx in (-1, 0, 1):
                t = np.array([tx, ty, tz], dtype=np.float64)
                d = xyz[None, :, :] + (t @ h)[None, None, :] - xyz[:, None, :]
                r2 = (d * d).sum(axis=2)
                hit = r2 < rcsq
                hit &= ~np.eye(n, dtype=bool)                          # an own image is never in range in the supported range
                i, j = np.nonzero(hit)
                out.append((i, j, np.broadcast_to(t, (len(i), 3))))
    i = np.concatenate([o[0] for o in out])
    j = np.concatenate([o[1] for o in out])
    t = np.concatenate([o[2] for o in out])
    order = np.argsort(i, kind="stable")
    i, j, t = i[order], j[order], t[order]
    return i, j, t @ h, t.astype(np.int64)


def row_columns(h, xyz):
    """The number of distinct columns with a block in each row of H: the molecule, its entries and theirs."""
    i, j, _, _ = entries(h, xyz)
    n = len(xyz)
    near = [set(j[i == c].tolist()) for c in range(n)]
    return np.array([len({c} | near[c] | set().union(*[near[k] for k in near[c]])) if near[c] else 1 for c in range(n)])


def _triplets(i, n):
    """(k, l) over all pairs k < l of entries with the same centre."""
    counts = np.bincount(i, minlength=n)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    ks, ls = [], []
    for c in range(n):
        m = counts[c]
        if m > 1:
            a, b = np.triu_indices(m, 1)
            ks.append(starts[c] + a)
            ls.append(starts[c] + b)
    if not ks:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate(ks), np.concatenate(ls)


class Energy:
    """The energy of one box as a differentiable function of its positions, over the entries found at ``xyz``."""

    def __init__(self, h, xyz):
        self.n = len(xyz)
        i, j, shift, _ = entries(h, xyz)
        k, l = _triplets(i, self.n)
        self.i, self.j, self.k, self.l = (torch.from_numpy(np.ascontiguousarray(a)) for a in (i, j, k, l))
        self.shift = torch.from_numpy(np.ascontiguousarray(shift))
        self.x0 = torch.tensor(np.asarray(xyz, dtype=np.float64))
        self.c = tuple(float(c) for c in constants())

    def __call__(self, x):
        sigma, eps, lam, big_a, big_b, gamma, small_a, cos0 = self.c
        if self.i.numel() == 0:
            return (x * 0.0).sum()
        d = x[self.j] + self.shift - x[self.i]
        r = torch.sqrt((d * d).sum(dim=1))
        den = r - sigma * small_a
        q = (sigma / r) ** 4
        e2 = 0.5 * (big_a * eps * (big_b * q - 1.0) * torch.exp(sigma / den)).sum()
        g = torch.exp(gamma * sigma / den)
        u = d / r[:, None]
        cs = (u[self.k] * u[self.l]).sum(dim=1)
        e3 = lam * eps * (g[self.k] * g[self.l] * (cs - cos0) ** 2).sum()
        return e2 + e3

    def energy_gradient(self):
        x = self.x0.clone().requires_grad_(True)
        e = self(x)
        (g,) = torch.autograd.grad(e, x)
        return float(e.detach()), g.numpy()

    def dense(self):
        """H [3 n, 3 n], row 3 i + a, column 3 j + b."""
        hess = torch.autograd.functional.hessian(self, self.x0.clone(), vectorize=True)
        return hess.reshape(3 * self.n, 3 * self.n).numpy()

    def matvec(self, vecs):
        """H v for every v of vecs [nvec, n, 3], by the double-backward product."""
        x = self.x0.clone().requires_grad_(True)
        (g,) = torch.autograd.grad(self(x), x, create_graph=True)
        out = []
        for v in np.asarray(vecs, dtype=np.float64):
            if not g.requires_grad:                                    # no entries: the energy is constant
                out.append(np.zeros_like(v))
                continue
            (hv,) = torch.autograd.grad((g * torch.from_numpy(np.ascontiguousarray(v))).sum(), x, retain_graph=True)
            out.append(hv.numpy())
        return np.array(out)


@functools.lru_cache(maxsize=None)
def energy(name):
    return Energy(*load_case(name))


@functools.lru_cache(maxsize=None)
def dense_reference(name):
    """The reference H of a case, computed once per process and shared: read-only."""
    H = energy(name).dense()
    H.setflags(write=False)
    return H


def test_vectors(name, nvec=2):
    """vecs [nvec + 1, n, 3]: ``nvec`` seeded vectors of unit length and one uniform translation."""
    n = len(load_case(name)[1])
    rng = np.random.default_rng(1000 + n)
    v = rng.standard_normal((nvec, n, 3))
    v /= np.sqrt((v * v).sum(axis=(1, 2)))[:, None, None]
    t = np.broadcast_to(np.array([0.3, -0.5, 0.8]) / np.sqrt(0.98), (1, n, 3))
    return np.ascontiguousarray(np.concatenate([v, t]))


@functools.lru_cache(maxsize=None)
def matvec_reference(name, nvec=2):
    vecs = test_vectors(name, nvec)
    out = energy(name).matvec(vecs)
    out.setflags(write=False)
    return out
