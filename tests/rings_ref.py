"""A plain Python/numpy restatement of include/mw_rings.h: the entries of every molecule with their lattice translations, held
in np.longdouble as tests/adf_ref.py holds them, then a depth-first search over (molecule, image) nodes for the closed paths
of 3 to 7 members, the full comparison of the 2 L readings of every closed path, and the shortest-path test.

Every result is an integer, so the device's are compared with these exactly wherever no r^2 comes within the rounding of the
device's doubles of r_cut^2: ``rings_exact`` returns that gap, and tests/test_rings_ref.py asserts it against MARGIN for
every input of tests/test_gpu_rings.py.
"""
from __future__ import annotations

import itertools

import numpy as np

from adf_ref import _fractional
from boo_ref import gas_box, widths

ANG_TO_BOHR = 1.0 / 0.5291772108
LD = np.longdouble
DEG = 8                            # MW_RINGS_DEG
SIZES = (3, 4, 5, 6, 7)
MARGIN = 1e-9
R_ANG = 3.5
GAS_SIZES = (1, 2, 63, 64, 65, 257)
IMAGES = np.array(list(itertools.product((-1, 0, 1), repeat=3)), dtype=np.int64)


def entries(h, xyz, r_cut):
    """(i, j, n [., 3], gap_r): every entry (j, n) of every molecule i, 0 < |H (s_j - s_i + n)|^2 < r_cut^2 in long double, and
    the smallest |r^2 - r_cut^2| / r_cut^2 over every candidate.  Candidates are picked in double within 1.1 r_cut^2 (the
    others are 10 % away from the cutoff) over the 27 images that a radius inside the cell's widths can reach."""
    h = np.asarray(h, dtype=np.float64)
    s, hl = _fractional(h, xyz)
    sd = s.astype(np.float64)
    n = len(sd)
    rc2 = LD(r_cut) * LD(r_cut)
    ci, cj, cn = [], [], []
    ds = sd[None, :, :] - sd[:, None, :]
    for img in IMAGES:
        d = (ds + img.astype(np.float64)) @ h
        near = (d * d).sum(axis=2) < 1.1 * float(rc2)
        if not img.any():
            near &= ~np.eye(n, dtype=bool)
        a, b = np.nonzero(near)
        ci.append(a), cj.append(b), cn.append(np.tile(img, (len(a), 1)))
    i, j, img = np.concatenate(ci), np.concatenate(cj), np.concatenate(cn)
    d = ((s[j] - s[i]) + img.astype(LD)) @ hl
    r2 = (d * d).sum(axis=1)
    gap_r = float((np.abs(r2 - rc2) / rc2).min()) if len(r2) else np.inf
    hit = (r2 > 0) & (r2 < rc2)
    return i[hit], j[hit], img[hit], gap_r


def _rows(n, i, j, img):
    """counts [n] and, per molecule, its edges (j, n_1, n_2, n_3) ascending: the entries between molecules of at most DEG entries."""
    counts = np.bincount(i, minlength=n)
    rows = [[] for _ in range(n)]
    for a, b, t in zip(i.tolist(), j.tolist(), img.tolist()):
        if counts[a] <= DEG and counts[b] <= DEG:
            rows[a].append((b, t[0], t[1], t[2]))
    return counts, [sorted(r) for r in rows]


def _readings(path):
    """The 2 L rooted, directed readings of a closed path as tuples of (molecule, n - n_root)."""
    L = len(path)
    out = []
    for s in range(L):
        r = path[s]
        for step in (1, -1):
            out.append(tuple((path[(s + step * k) % L][0], path[(s + step * k) % L][1] - r[1], path[(s + step * k) % L][2] - r[2],
                              path[(s + step * k) % L][3] - r[3]) for k in range(L)))
    return out


def rings_exact(h, xyz, r_cut):
    """dict of one box, lengths in bohr: hist [5], closed [5] int64, member [N, 5] int32, counts [N] int32, summary [4] int64
    (molecules over the cap, undirected edges per cell, primitive rings that needed the comparison of all readings, primitive
    rings), rings [R, 8] int32 (the complete list in the contract's order), closed_full (the closed paths that needed
    the comparison of all readings) and gap_r."""
    xyz = np.asarray(xyz, dtype=np.float64)
    n = len(xyz)
    i, j, img, gap_r = entries(h, xyz, r_cut)
    counts, rows = _rows(n, i, j, img)
    rowset = [set(r) for r in rows]
    hist, closed = np.zeros(5, dtype=np.int64), np.zeros(5, dtype=np.int64)
    member = np.zeros((n, 5), dtype=np.int32)
    rings, full, closed_full = [], 0, [0]

    def joined(u, w):
        return (w[0], w[1] - u[1], w[2] - u[2], w[3] - u[3]) in rowset[u[0]]

    def around(u):
        return {(e[0], u[1] + e[1], u[2] + e[2], u[3] + e[3]) for e in rows[u[0]]}

    def primitive(path):
        L = len(path)
        for a in range(L):
            for b in range(a + 1, L):
                dist = min(b - a, L - (b - a))
                if dist >= 2 and joined(path[a], path[b]):
                    return False
                if dist == 3 and around(path[a]) & around(path[b]):
                    return False
        return True

    def close(path):
        nonlocal full
        L = len(path)
        mine = tuple(path)
        if any(r < mine for r in _readings(path)):
            return
        closed[L - 3] += 1
        mols = [v[0] for v in path]
        need = mols.count(mols[0]) > 1 or mols[1] == mols[-1]          # not the common case of the contract
        closed_full[0] += need
        if not primitive(path):
            return
        hist[L - 3] += 1
        for m in mols:
            member[m, L - 3] += 1
        full += need
        rings.append([L] + mols + [-1] * (7 - L))

    def walk(root, path):
        u = path[-1]
        for e in rows[u[0]]:
            if e[0] < root:
                continue
            w = (e[0], u[1] + e[1], u[2] + e[2], u[3] + e[3])
            if w == path[0]:
                if len(path) >= 3:
                    close(path)
                continue
            if w in path:
                continue
            if len(path) < 7:
                path.append(w)
                walk(root, path)
                path.pop()

    for root in range(n):
        if rows[root]:
            walk(root, [(root, 0, 0, 0)])
    edges = sum(1 for a in range(n) for e in rows[a] if e[0] > a)
    summary = np.array([int((counts > DEG).sum()), edges, full, int(hist.sum())], dtype=np.int64)
    return dict(hist=hist, closed=closed, member=member, counts=counts.astype(np.int32), summary=summary,
                rings=np.array(rings, dtype=np.int32).reshape(-1, 8), gap_r=gap_r, closed_full=closed_full[0], max_count=int(counts.max(initial=0)))


def ring_list(ref, list_cap):
    """list [list_cap, 8] int32 of a rings_exact dict: the first list_cap rings, the unused rows -1."""
    out = np.full((list_cap, 8), -1, dtype=np.int32)
    k = min(list_cap, len(ref["rings"]))
    out[:k] = ref["rings"][:k]
    return out


def outputs(ref, list_cap):
    """The six outputs of the library for one box, in the order of mc_water_ls_mw_amd.rings.ring_statistics."""
    return ref["hist"], ref["closed"], ref["member"], ref["counts"], ref["summary"], ring_list(ref, list_cap)


# -- the inputs the GPU tests use (tests/test_gpu_rings.py), their preconditions and figures (tests/test_rings_ref.py) -------
#: goldens in which every molecule sits in twelve 6-rings at 3.5 Angstrom: hist = closed = (0, 0, 0, 2 N, 0)
ICE = ("ih8_small", "ic48", "ih48", "ih48_t020", "ic48_t015", "ic96", "ih1536_t012", "ic64_sheared")
#: (kind, reps, sigma in Angstrom, seed) of lattice.ice_box -> (hist, closed, largest n_i or None)
HOT = {
    ("ih", (2, 1, 1), 0.5, 6): ((9, 2, 2, 2, 4), (9, 8, 10, 12, 24), None),
    ("ih", (3, 2, 2), 0.5, 2): ((36, 2, 16, 45, 14), (36, 21, 29, 87, 152), 6),
    ("ic", (2, 2, 2), 0.5, 3): ((25, 5, 13, 17, 3), (25, 20, 37, 72, 113), 7),
    ("ih", (4, 3, 3), 0.6, 4): ((168, 28, 35, 59, 21), (168, 170, 219, 394, 752), 7),
}
#: (golden, boxes) of the batches of tests/test_gpu_rings.py, made by boo_ref.batch_set, at 3.5 Angstrom
BATCHES = (("ih48_t020", 9), ("ic96", 4))
#: the case with a molecule of exactly 8 entries (the most that keeps its edges) and another of 9 (the fewest that loses them)
AT_THE_CAP = "gas N = 257"
#: the cases in which some molecules are over the cap and some rings survive
PARTLY_CAPPED = ("gas N = 63", "gas N = 64", "gas N = 65", "gas N = 257")


def cases():
    """[(label, loader)]: every single box of tests/test_gpu_rings.py; loader() -> (h, xyz, r_cut in bohr)."""
    from conftest import load_golden
    from mc_water_ls_mw_amd import lattice as lat

    def golden(name, r_ang):
        def load():
            z = load_golden(name)
            return z["h"], z["xyz"], min(r_ang * ANG_TO_BOHR, 0.9999 * float(widths(z["h"]).min()))
        return load

    def hot(key):
        def load():
            h, xyz = lat.ice_box(key[0], key[1], key[2], seed=key[3])
            return h, xyz, min(R_ANG * ANG_TO_BOHR, 0.9999 * float(widths(h).min()))
        return load

    def gas(n, seed):
        def load():
            h, xyz = gas_box(n, seed)
            return h, xyz, min(R_ANG * ANG_TO_BOHR, 0.98 * float(widths(h).min()))
        return load

    out = [(f"{name} 3.5", golden(name, R_ANG)) for name in ICE]
    out += [(f"{k[0]}{k[1]} sigma {k[2]} seed {k[3]}", hot(k)) for k in HOT]
    out += [("ih1536_t012 4.8", golden("ih1536_t012", 4.8))]
    out += [(f"gas N = {n}", gas(n, 1000 + n)) for n in GAS_SIZES]
    return out


_CACHE = {}


def case_exact(case):
    """(h, xyz, r_cut, rings_exact dict) of a case, computed once per process."""
    if case[0] not in _CACHE:
        h, xyz, rc = case[1]()
        _CACHE[case[0]] = (h, xyz, rc, rings_exact(h, xyz, lib_radius(rc)))
    return _CACHE[case[0]]


def lib_radius(rc):
    """What the library sees of a radius in bohr that went through the wrapper's Angstrom."""
    return (rc * 0.5291772108) / 0.5291772108
