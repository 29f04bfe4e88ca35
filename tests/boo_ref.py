"""Numpy references for the Steinhardt bond-order parameters of include/mw_boo.h, written independently of the kernels'
real harmonics.

By the addition theorem sum_m Y_lm(a) Y_lm(b) = (2 l + 1) / (4 pi) P_l(a . b), so with E(i) the neighbour entries of i and
u_a their unit vectors

    q_l(i)^2    = 1 / n_i^2 sum_{a, b in E(i)} P_l(u_a . u_b)
    qbar_l(i)^2 = 1 / (n_i + 1)^2 sum_{k, k' in G(i)} 1 / (n_k n_k') sum_{a in E(k), b in E(k')} P_l(u_a . u_b),  G(i) = i and its entries
    s_ij        = 1 / (n_i n_j) sum_{a in E(i), b in E(j)} P_6(u_a . u_b) / (q_6(i) q_6(j))
    Q_l^2       = 1 / (sum n)^2 sum_{a, b over all entries of the box} P_l(u_a . u_b)

``boo_exact`` evaluates these in np.longdouble: as the double sums themselves (``sums=True``, the default up to 1536
molecules of at most 8 entries each), or with every P_l(a . b) expanded in monomials, (a . b)^k = sum_{p+q+r=k} k!/(p! q! r!) a^pqr b^pqr, which turns
each double sum into a bilinear form of per-molecule moment sums (linear in the number of entries; the only way to the box
sum of a large box).  tests/test_boo_ref.py holds the two to each other.  ``boo_tables`` is a second, plain-double evaluation
through explicit real harmonics (coefficients from numpy's Legendre class), the noise floor of a double evaluation.
"""
from __future__ import annotations

import math

import numpy as np


ANG_TO_BOHR = 1.0 / 0.5291772108
LD = np.longdouble
#: P_l(x) = sum_k PCOEF[l][k] x^k
PCOEF = {4: {4: LD(35) / 8, 2: LD(-30) / 8, 0: LD(3) / 8}, 6: {6: LD(231) / 16, 4: LD(-315) / 16, 2: LD(105) / 16, 0: LD(-5) / 16}}
BRUTE_MAX = 1536
SUMS_MAX = 1536
SUMS_MAX_NEIGHBOURS = 8            # (the double sum of qbar takes ((n + 1) n)^2 terms per molecule)


def _legendre(l, x):
    x2 = x * x
    if l == 4:
        return ((PCOEF[4][4] * x2 + PCOEF[4][2]) * x2) + PCOEF[4][0]
    return (((PCOEF[6][6] * x2 + PCOEF[6][4]) * x2 + PCOEF[6][2]) * x2) + PCOEF[6][0]


def widths(h):
    h = np.asarray(h, dtype=np.float64)
    vol = abs(np.linalg.det(h))
    return np.array([vol / np.linalg.norm(np.cross(h[(k + 1) % 3], h[(k + 2) % 3])) for k in range(3)])


# -- neighbour entries ------------------------------------------------------------------------
def _entries_brute(h, xyz, rc):
    """Brute force over the images of the molecules wrapped into the cell: with s in [0, 1) a pair within rc has
    |n_k| <= ceil(rc / w_k)."""
    s = xyz @ np.linalg.inv(h)
    wrapped = (s - np.floor(s)) @ h
    reach = np.ceil(rc / widths(h)).astype(np.int64)
    out_i, out_j, out_d = [], [], []
    for a in range(-reach[0], reach[0] + 1):
        for b in range(-reach[1], reach[1] + 1):
            for c in range(-reach[2], reach[2] + 1):
                d = (wrapped[None, :, :] + np.array([a, b, c], dtype=np.float64) @ h) - wrapped[:, None, :]
                r2 = (d * d).sum(axis=2)
                i, j = np.nonzero((r2 < rc * rc) & (r2 > 0.0))
                out_i.append(i), out_j.append(j), out_d.append(d[i, j])
    return np.concatenate(out_i), np.concatenate(out_j), np.concatenate(out_d)


def _entries_grid(h, xyz, rc):
    """A numpy cell grid over fractional coordinates, at least three cells per axis (large boxes only)."""
    g = np.floor(widths(h) / rc).astype(np.int64)
    assert np.all(g >= 3), "the grid reference is for boxes of at least three cutoffs per axis"
    s = xyz @ np.linalg.inv(h)
    s = s - np.floor(s)
    wrapped = s @ h
    c = np.minimum((s * g).astype(np.int64), g - 1)
    lin = (c[:, 2] * g[1] + c[:, 1]) * g[0] + c[:, 0]
    order = np.argsort(lin, kind="stable")
    ncell = int(g.prod())
    count = np.bincount(lin, minlength=ncell)
    start = np.concatenate([[0], np.cumsum(count)])
    kmax = int(count.max())
    members = np.full((ncell, kmax), -1, dtype=np.int64)
    rank = np.arange(len(xyz)) - start[lin[order]]
    members[lin[order], rank] = order
    out_i, out_j, out_d = [], [], []
    me = np.arange(len(xyz))
    for oz in (-1, 0, 1):
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                cc = c + np.array([ox, oy, oz])
                shift = np.floor_divide(cc, g)                         # -1, 0 or 1: the image the wrapped cell stands for
                cc = cc - shift * g
                cand = members[(cc[:, 2] * g[1] + cc[:, 1]) * g[0] + cc[:, 0]]            # [N, kmax]
                ok = cand >= 0
                j = np.where(ok, cand, 0)
                d = (wrapped[j] + (shift.astype(np.float64) @ h)[:, None, :]) - wrapped[:, None, :]
                r2 = (d * d).sum(axis=2)
                hit = ok & (r2 < rc * rc) & (r2 > 0.0)
                a, b = np.nonzero(hit)
                out_i.append(me[a]), out_j.append(j[a, b]), out_d.append(d[a, b])
    return np.concatenate(out_i), np.concatenate(out_j), np.concatenate(out_d)


def entries(h, xyz, rc, grid=None):
    """(i, j, d): every neighbour entry (j, image) of every molecule i with 0 < |d| < rc, d = r_j + H n - r_i; sorted by i
    (stable).  Brute force over images up to BRUTE_MAX molecules, a cell grid beyond."""
    h = np.asarray(h, dtype=np.float64)
    xyz = np.asarray(xyz, dtype=np.float64)
    grid = len(xyz) > BRUTE_MAX if grid is None else grid
    i, j, d = (_entries_grid if grid else _entries_brute)(h, xyz, rc)
    order = np.lexsort((j, i))
    return i[order], j[order], d[order]


def nearest_to_cutoff(h, xyz, rc, grid=None):
    """min | |d| - rc | over every pair and image that comes within 1.05 rc (inf if none does)."""
    _, _, d = entries(h, xyz, 1.05 * rc, grid)
    if len(d) == 0:
        return np.inf
    return float(np.abs(np.sqrt((d * d).sum(axis=1)) - rc).min())


# -- the moment route ---------------------------------------------------------------------------
def _monomials():
    out = []
    for k in (0, 2, 4, 6):
        for p in range(k + 1):
            for q in range(k + 1 - p):
                r = k - p - q
                out.append((k, p, q, r, math.factorial(k) // (math.factorial(p) * math.factorial(q) * math.factorial(r))))
    return out


MONO = _monomials()


def _weights(l):
    """w[m]: the weight of monomial m in the bilinear form of P_l."""
    return np.array([PCOEF[l].get(k, LD(0)) * mult for k, _, _, _, mult in MONO], dtype=LD)


def _moments(u):
    """[E, len(MONO)] monomials of the unit vectors u [E, 3]."""
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    pw = [[np.ones_like(v)] for v in (x, y, z)]
    for a, v in enumerate((x, y, z)):
        for _ in range(6):
            pw[a].append(pw[a][-1] * v)
    return np.stack([pw[0][p] * pw[1][q] * pw[2][r] for _, p, q, r, _ in MONO], axis=1)


def _form(l, a, b):
    return (a * b * _weights(l)).sum(axis=-1)


# -- the evaluations ----------------------------------------------------------------------------
def _padded(i, n, nmol):
    """(slot [E], K): entry e is the slot-th entry of its molecule."""
    first = np.concatenate([[0], np.cumsum(n)])[:-1]
    return np.arange(len(i)) - first[i], max(1, int(n.max(initial=0)))


def boo_exact(h, xyz, rc, threshold, sums=None, grid=None):
    """dict: n [N] int, conn [N] int, q2 [N, 4] longdouble = (q4^2, q6^2, qbar4^2, qbar6^2), s [E] longdouble (NaN where a
    side is degenerate), summary [4] longdouble = (Q4^2, Q6^2, <qbar4>, <qbar6>), i, j [E], r [E] the entries' distances.
    ``sums``: the double sums (default up to SUMS_MAX molecules of at most SUMS_MAX_NEIGHBOURS entries) or the moment route;
    ``grid``: as `entries`."""
    h = np.asarray(h, dtype=np.float64)
    xyz = np.asarray(xyz, dtype=np.float64)
    nmol = len(xyz)
    i, j, d = entries(h, xyz, rc, grid)
    n = np.bincount(i, minlength=nmol)
    sums = (nmol <= SUMS_MAX and n.max() <= SUMS_MAX_NEIGHBOURS) if sums is None else sums
    dl = d.astype(LD)
    r = np.sqrt((dl * dl).sum(axis=1))
    u = dl / r[:, None]
    nl = n.astype(LD)
    safe = np.where(n > 0, nl, LD(1))
    q2 = np.zeros((nmol, 4), dtype=LD)
    summary = np.zeros(4, dtype=LD)
    if sums:
        slot, K = _padded(i, n, nmol)
        U = np.zeros((nmol, K, 3), dtype=LD)
        M = np.zeros((nmol, K), dtype=bool)
        U[i, slot], M[i, slot] = u, True
        W = np.where(M, 1.0 / safe[:, None], LD(0))                       # 1 / n_k on k's own vectors
        for c, l in enumerate((4, 6)):
            for k0 in range(0, nmol, 512):
                sl = slice(k0, k0 + 512)
                P = _legendre(l, np.einsum("iac,ibc->iab", U[sl], U[sl]))
                q2[sl, c] = (P * W[sl][:, :, None] * W[sl][:, None, :]).sum(axis=(1, 2))
        # s_ij: E(i) against E(j)
        s = np.zeros(len(i), dtype=LD)
        for k0 in range(0, len(i), 4096):
            a, b = i[k0:k0 + 4096], j[k0:k0 + 4096]
            P = _legendre(6, np.einsum("eac,ebc->eab", U[a], U[b]))
            s[k0:k0 + 4096] = (P * W[a][:, :, None] * W[b][:, None, :]).sum(axis=(1, 2))
        # qbar: all vectors of G(i) = i and its entries, each with 1 / n_k
        J = np.zeros((nmol, K + 1), dtype=np.int64)
        JM = np.zeros((nmol, K + 1), dtype=bool)
        J[:, 0], JM[:, 0] = np.arange(nmol), True
        J[i, slot + 1], JM[i, slot + 1] = j, True
        step = max(1, (1 << 22) // ((K + 1) * K) ** 2)
        for k0 in range(0, nmol, step):
            sl = slice(k0, k0 + step)
            V = U[J[sl]].reshape(-1, (K + 1) * K, 3)
            w = (W[J[sl]] * JM[sl][:, :, None]).reshape(-1, (K + 1) * K)
            dots = np.einsum("iac,ibc->iab", V, V)
            for c, l in enumerate((4, 6)):
                q2[sl, 2 + c] = (_legendre(l, dots) * w[:, :, None] * w[:, None, :]).sum(axis=(1, 2)) / (nl[sl] + 1) ** 2
        if 0 < len(i) <= 2048:
            dots = u @ u.T
            for c, l in enumerate((4, 6)):
                summary[c] = _legendre(l, dots).sum() / LD(len(i)) ** 2
    if not sums or len(i) > 2048:
        mom = _moments(u)
        tot = np.zeros((nmol, mom.shape[1]), dtype=LD)
        np.add.at(tot, i, mom)
        if len(i):
            box = mom.sum(axis=0) / LD(len(i))
            for c, l in enumerate((4, 6)):
                summary[c] = _form(l, box, box)
    if not sums:
        qm = tot / safe[:, None]                                            # "q_lm" in the monomial basis
        bar = qm.copy()
        np.add.at(bar, i, qm[j])
        bar = bar / (nl + 1)[:, None]
        for c, l in enumerate((4, 6)):
            q2[:, c] = _form(l, qm, qm)
            q2[:, 2 + c] = _form(l, bar, bar)
        s = _form(6, qm[i], qm[j])
    q2 = np.where(q2 < 0, LD(0), q2)                                        # (rounding of an exact zero)
    q6 = np.sqrt(q2[:, 1])
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where((q6[i] > 0) & (q6[j] > 0), s / (q6[i] * q6[j]), np.nan)
    conn = np.bincount(i[np.nan_to_num(s.astype(np.float64), nan=-2.0) > threshold], minlength=nmol)
    summary[2], summary[3] = np.sqrt(q2[:, 2]).sum() / nmol, np.sqrt(q2[:, 3]).sum() / nmol
    return dict(n=n, conn=conn, q2=q2, s=s, summary=summary, i=i, j=j, r=r.astype(np.float64))


def real_harmonics(l, u):
    """[E, 2 l + 1] float64: sqrt(4 pi / (2 l + 1)) times an orthonormal real basis of degree l at the unit vectors u."""
    from numpy.polynomial import legendre as L
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    w = x + 1j * y
    cols = []
    for m in range(l + 1):
        c = math.sqrt((1 if m == 0 else 2) * math.factorial(l - m) / math.factorial(l + m))
        pm = L.legval(z, L.legder([0] * l + [1], m)) if m else L.legval(z, [0] * l + [1])
        wm = w ** m
        cols.append(c * pm * wm.real)
        if m:
            cols.append(c * pm * wm.imag)
    return np.stack(cols, axis=1)


def boo_tables(h, xyz, rc, threshold, grid=None):
    """The same dict as boo_exact in plain float64 through explicit real harmonics (q_lm tables as the definition has them)."""
    h = np.asarray(h, dtype=np.float64)
    xyz = np.asarray(xyz, dtype=np.float64)
    nmol = len(xyz)
    i, j, d = entries(h, xyz, rc, grid)
    n = np.bincount(i, minlength=nmol)
    r = np.sqrt((d * d).sum(axis=1))
    u = d / r[:, None]
    safe = np.where(n > 0, n, 1).astype(np.float64)
    q2 = np.zeros((nmol, 4))
    summary = np.zeros(4)
    qv = {}
    for c, l in enumerate((4, 6)):
        Y = real_harmonics(l, u)
        tot = np.zeros((nmol, 2 * l + 1))
        np.add.at(tot, i, Y)
        qlm = tot / safe[:, None]
        bar = qlm.copy()
        np.add.at(bar, i, qlm[j])
        bar = bar / (n + 1.0)[:, None]
        q2[:, c], q2[:, 2 + c] = (qlm * qlm).sum(axis=1), (bar * bar).sum(axis=1)
        if len(i):
            Q = Y.sum(axis=0) / len(i)
            summary[c] = (Q * Q).sum()
        qv[l] = qlm
    q6 = np.sqrt(q2[:, 1])
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where((q6[i] > 0) & (q6[j] > 0), (qv[6][i] * qv[6][j]).sum(axis=1) / (q6[i] * q6[j]), np.nan)
    conn = np.bincount(i[np.nan_to_num(s, nan=-2.0) > threshold], minlength=nmol)
    summary[2], summary[3] = np.sqrt(q2[:, 2]).mean(), np.sqrt(q2[:, 3]).mean()
    return dict(n=n, conn=conn, q2=q2, s=s, summary=summary, i=i, j=j, r=r)


# -- the inputs the GPU tests use (tests/test_gpu_boo.py), and their preconditions (tests/test_boo_ref.py) ---------------
def gas_box(n, seed):
    """A random gas of n molecules in a sheared cell, some of them outside the cell."""
    rng = np.random.default_rng(seed)
    h = np.array([[31.0, 0.0, 0.0], [4.5, 28.0, 0.0], [-3.0, 5.0, 35.0]]) * (max(n, 8) / 256.0) ** (1.0 / 3.0) * (1.6 if n > 65 else 1.0)
    return h, np.ascontiguousarray((rng.random((n, 3)) * 1.6 - 0.3) @ h)


GAS_SIZES = (1, 2, 63, 64, 65, 255, 256, 257)


def gas_rc_ang(n):
    """Up to 65 molecules the gas boxes keep the density of 256 molecules in a 31 x 28 x 35 bohr cell -- two or three cells
    per axis at 3.5 Angstrom, the smallest boxes narrower than that -- and the larger ones a quarter of it."""
    h, _ = gas_box(n, 0)
    return min(3.5, 0.98 * float(widths(h).min()) / ANG_TO_BOHR)


def cases():
    """[(label, golden name or None, gas size or None, rc in Angstrom, threshold)]: every input of tests/test_gpu_boo.py.  The
    cutoffs and thresholds are held to the preconditions (no |d| within 1e-9 rc of rc, no s_ij within 1e-6 of the threshold)
    by tests/test_boo_ref.py, which is what lets the GPU tests compare nn exactly."""
    from conftest import golden_names
    out = [(name, name, None, 3.5, 0.5) for name in golden_names() if not any(t in name for t in ("4096", "32768"))]
    out += [("ic48_t015 second shell", "ic48_t015", None, 5.0, 0.5), ("ih48_t020 second shell", "ih48_t020", None, 5.0, 0.5),
            ("ih8_small at its width", "ih8_small", None, None, 0.5),
            ("ih4096_t015", "ih4096_t015", None, 3.5, 0.5), ("ih32768_t015", "ih32768_t015", None, 3.5, 0.5)]
    out += [(f"gas N = {n}", None, n, gas_rc_ang(n), 0.3) for n in GAS_SIZES]
    # the general geometry with one and two cells per axis: 0.55 of the narrowest width (dozens of neighbours: moment route)
    out += [("gas N = 65 in one cell", None, 65, 0.55 * float(widths(gas_box(65, 0)[0]).min()) / ANG_TO_BOHR, 0.3)]
    return out


def load_case(case):
    """(h, xyz, rc in bohr, threshold, grid) of a case of `cases`: grid says how the reference finds the neighbours."""
    from conftest import load_golden
    label, name, gas, rc_ang, thr = case
    if name is None:
        h, xyz = gas_box(gas, 1000 + gas)
    else:
        z = load_golden(name)
        h, xyz = z["h"], z["xyz"]
    rc = 0.9999 * float(widths(h).min()) if rc_ang is None else rc_ang * ANG_TO_BOHR
    return h, xyz, rc, thr, len(xyz) > 256


#: (golden, boxes) of the batches of tests/test_gpu_boo.py: the LAST box of each is also compared with boo_exact, counts exactly
BATCHES = (("ih48_t020", 9), ("ic96", 4), ("ih1536_t012", 3))


def scaled_set(name, n, sigma, seed):
    """n thermalised, rescaled copies of a golden box: (cells [n, 3, 3], positions [n, N, 3])."""
    from conftest import load_golden
    from mc_water_ls_mw_amd import lattice as lat
    z = load_golden(name)
    hs, xs = [], []
    for k in range(n):
        f = 1.0 + 0.013 * (k % 5 - 2)
        hs.append(z["h"] * f)
        xs.append(lat.thermalise(z["xyz"], sigma, seed + k) * f)
    return np.array(hs), np.array(xs)


def batch_set(name, n):
    return scaled_set(name, n, 0.1, 40)


def gaps(h, xyz, rc, thr, ref, grid=None):
    """(nearest | |d| - rc | / rc, nearest |s_ij - thr|) of a box and its boo_exact dict: the two preconditions of an exact
    comparison of neighbour and connection counts (> 1e-9 and > 1e-6)."""
    s = np.asarray(ref["s"], dtype=np.float64)
    return nearest_to_cutoff(h, xyz, rc, grid) / rc, (float(np.nanmin(np.abs(s - thr))) if np.any(np.isfinite(s)) else np.inf)


def case_exact(case):
    """boo_exact of a case."""
    h, xyz, rc, thr, grid = load_case(case)
    return boo_exact(h, xyz, rc, thr, grid=grid)
