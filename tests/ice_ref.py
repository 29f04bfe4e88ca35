"""Vectorised numpy reference for the engine's CHILL+ ice structure classes (mw_ice.hip.h, DESIGN.md "Ice structure
classes"), from (xyz, ivect, nn, jn, vn) -- the reference's list layout, 1-based -- and the bond cutoff rc in bohr.

It is written independently of the kernels' real harmonics: by the addition theorem Y3(a).Y3(b) = 7 / (4 pi) P3(a.b), so

  q_i.q_j = 7 / (4 pi) sum_{a in N(i)} sum_{b in N(j)} P3(u_a.u_b),   P3(x) = (5 x^3 - 3 x) / 2,

and c_ij = q_i.q_j / (|q_i| |q_j|), with the neighbours N(i) the list entries with 0 < |d| < rc, d = r_j + ivect - r_i.
A molecule with |q|^2 <= 1e-24 n^2 is degenerate (its bonds are NaN), an image of i itself is a bond with c = 1.
"""
from __future__ import annotations

import numpy as np

STAGGERED = -0.8
ECLIPSED = (-0.35, 0.25)
NOT_A_BOND = 2.0
RC_ANG = 3.5
ANG_TO_BOHR = 1.0 / 0.5291772108


def _p3(x):
    return 0.5 * x * (5.0 * x * x - 3.0)


def classify_counts(n, nst, necl):
    """The class rule on (n_i, staggered bonds, eclipsed bonds), arrays of any shape."""
    cls = np.zeros(np.shape(n), dtype=np.uint8)
    four = np.asarray(n) == 4
    rules = [(nst == 4, 1), ((nst == 3) & (necl == 1), 2), (necl == 4, 4), (necl == 3, 5), (nst >= 2, 3)]
    done = ~four
    for cond, k in rules:
        hit = four & cond & ~done
        cls[hit] = k
        done |= hit
    return cls


def ice_classes(xyz, ivect, nn, jn, vn, rc):
    """(classes uint8 [N], bonds [N, maxneigh], counts [6]).  bonds holds c for every neighbour entry, NaN for a degenerate
    one and exactly 2.0 where the entry is not a bond (unused slot, |d| >= rc, d = 0)."""
    xyz = np.asarray(xyz, dtype=np.float64)
    ivect = np.asarray(ivect, dtype=np.float64)
    nn, jn, vn = np.asarray(nn), np.asarray(jn), np.asarray(vn)
    n, smax = jn.shape
    live = np.arange(smax)[None, :] < nn[:, None]
    j = np.where(live, jn - 1, 0)
    v = np.where(live, vn - 1, 0)
    d = (xyz[j] + ivect[v]) - xyz[:, None, :]                          # as the energy kernels form d
    r2 = d[..., 2] * d[..., 2] + (d[..., 1] * d[..., 1] + d[..., 0] * d[..., 0])
    bond = live & (r2 < rc * rc) & (r2 > 0.0)
    nb = bond.sum(axis=1)

    # the neighbour unit vectors of every molecule, packed to the first kmax columns (list order kept)
    perm = np.argsort(~bond, axis=1, kind="stable")
    kmax = max(1, int(nb.max()))
    perm = perm[:, :kmax]
    mask = np.take_along_axis(bond, perm, 1)
    u = np.take_along_axis(d, perm[:, :, None], 1)
    u = u / np.sqrt(np.where(mask, np.take_along_axis(r2, perm, 1), 1.0))[:, :, None]
    u = np.where(mask[:, :, None], u, 0.0)

    pair = mask[:, :, None] & mask[:, None, :]
    q2 = 7.0 / (4.0 * np.pi) * np.where(pair, _p3(np.einsum("iac,ibc->iab", u, u)), 0.0).sum(axis=(1, 2))
    valid = q2 > 1e-24 * nb.astype(np.float64) ** 2

    c = np.full((n, smax), NOT_A_BOND)
    ii, ss = np.nonzero(bond)
    jj = j[ii, ss]
    for k0 in range(0, len(ii), 1 << 16):
        a, jb = ii[k0:k0 + (1 << 16)], jj[k0:k0 + (1 << 16)]
        m = mask[a][:, :, None] & mask[jb][:, None, :]
        s = 7.0 / (4.0 * np.pi) * np.where(m, _p3(np.einsum("eac,ebc->eab", u[a], u[jb])), 0.0).sum(axis=(1, 2))
        with np.errstate(invalid="ignore", divide="ignore"):
            val = s / (np.sqrt(q2[a]) * np.sqrt(q2[jb]))
        val = np.where(a == jb, 1.0, val)
        c[a, ss[k0:k0 + (1 << 16)]] = np.where(valid[a] & valid[jb], val, np.nan)

    with np.errstate(invalid="ignore"):
        nst = (bond & (c <= STAGGERED)).sum(axis=1)
        necl = (bond & (c >= ECLIPSED[0]) & (c <= ECLIPSED[1])).sum(axis=1)
    cls = classify_counts(nb, nst, necl)
    return cls, c, np.bincount(cls, minlength=6)


def image_vectors(h, rc):
    """Every lattice translation n1 h1 + n2 h2 + n3 h3 that can bring a molecule within rc of another: |n_k| up to the
    number of cell heights along k that rc spans, plus one.  Central image first."""
    h = np.asarray(h, dtype=np.float64)
    vol = abs(np.linalg.det(h))
    reach = []
    for k in range(3):
        other = np.cross(h[(k + 1) % 3], h[(k + 2) % 3])
        reach.append(int(np.ceil(rc / (vol / np.linalg.norm(other)))) + 1)
    ns = [(a, b, c) for a in range(-reach[0], reach[0] + 1) for b in range(-reach[1], reach[1] + 1)
          for c in range(-reach[2], reach[2] + 1)]
    ns.sort(key=lambda t: (t != (0, 0, 0), t))
    return np.array(ns, dtype=np.float64) @ h


def brute_neighbours(h, xyz, rc):
    """(ivect, nn, jn, vn): every (j, image) with 0 < |d| < rc by brute force over images, in the reference's layout."""
    xyz = np.asarray(xyz, dtype=np.float64)
    n = len(xyz)
    iv = image_vectors(h, rc)
    rows = [[] for _ in range(n)]
    for k, t in enumerate(iv):
        d = (xyz[None, :, :] + t) - xyz[:, None, :]
        r2 = (d * d).sum(axis=2)
        for i, jj in zip(*np.nonzero((r2 < rc * rc) & (r2 > 0.0))):
            rows[i].append((jj + 1, k + 1))
    smax = max(1, max(len(r) for r in rows))
    nn = np.array([len(r) for r in rows], dtype=np.int32)
    jn = np.zeros((n, smax), dtype=np.int32)
    vn = np.zeros((n, smax), dtype=np.int32)
    for i, r in enumerate(rows):
        for s, (jj, k) in enumerate(r):
            jn[i, s], vn[i, s] = jj, k
    return iv, nn, jn, vn


def stacking_counts(sequence, reps_xy=(2, 1)):
    """(cubic, hexagonal) molecules of an ideal stacked_ice_box: each junction k owns two sublayers, hexagonal iff
    sequence[k-1] == sequence[k+1]."""
    n = len(sequence)
    per_sublayer = 2 * reps_xy[0] * reps_xy[1]
    hexj = sum(sequence[k - 1] == sequence[(k + 1) % n] for k in range(n))
    return 2 * n * per_sublayer - 2 * hexj * per_sublayer, 2 * hexj * per_sublayer
