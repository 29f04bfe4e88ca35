"""A numpy reference in np.longdouble for the O-O-O angle histograms of include/mw_adf.h: the entry count of every molecule,
the histogram of cos(theta) over the pairs of kept entries of every centre, per group, and the four totals per group.
Vectorised over the molecules: the entries of a box are enumerated in the walk order of the contract (which decides the 32
kept entries of a molecule with more), padded to a table of unit vectors, and every pair is an element of its Gram matrix.

The fractional coordinates are formed, wrapped and differenced in long double from the double-precision positions, so a
cos(theta) of the reference is good to about 1e-18 and the device's differs from it by the rounding of its own double
arithmetic (1e-15).  An exact comparison of integer histograms therefore holds wherever no r^2 comes within that of r_cut^2
and no cos(theta) within that of a bin edge: ``adf_exact`` returns both gaps (and, where a molecule is over the cap, how far
the walk order is from changing), and tests/test_adf_ref.py asserts them against MARGIN for every input of
tests/test_gpu_adf.py.
"""
from __future__ import annotations

import numpy as np

from boo_ref import gas_box, widths

ANG_TO_BOHR = 1.0 / 0.5291772108
LD = np.longdouble
KEEP = 32                          # MW_ADF_KEEP
SMALL_N = 64                       # up to here: the small geometry
GAS_SIZES = (1, 2, 63, 64, 65, 255, 256, 257)
R_FIRST_ANG = 3.5
R_SECOND_ANG = 4.8
#: the margin of the preconditions: relative for r^2 against r_cut^2, absolute for cos(theta) against an edge
MARGIN = 1e-9


def edges_theta(nbins):
    """mc_water_ls_mw_amd.angles.adf_edges(nbins, "theta"), restated: bins uniform in theta, ascending in cos(theta)."""
    e = np.cos((nbins - np.arange(nbins + 1, dtype=np.float64)) * (np.pi / nbins))
    e[0], e[-1] = -1.0, 1.0
    return e


def edges_cos(nbins):
    e = -1.0 + 2.0 * np.arange(nbins + 1, dtype=np.float64) / nbins
    e[0], e[-1] = -1.0, 1.0
    return e


#: the two edge sets of the GPU tests
EDGE_SETS = {"cos97": edges_cos(97), "theta90": edges_theta(90)}


def cell_grid(h, r_cut, nwater):
    """(g_1, g_2, g_3) by the rule of mw_adf.h / mw_tet.h: floor(w_k / (r_cut (1 + 1e-9))), at least 1 and at most 1024 each,
    the largest (the first of equals) lowered until the product is at most max(64, 2 nwater)."""
    g = np.clip(np.floor(widths(h) / (r_cut * (1.0 + 1e-9))), 1, 1024).astype(np.int64)
    cap = max(64, 2 * nwater)
    while int(g.prod()) > cap:
        g[int(np.argmax(g))] -= 1
    return tuple(int(v) for v in g)


def _fractional(h, xyz):
    """s = H^-1 r reduced to [0, 1), in long double (the inverse by cofactors: numpy's LAPACK has no long double)."""
    hl = np.asarray(h, dtype=np.float64).astype(LD)
    a, b, c = hl
    det = (a * np.cross(b, c)).sum()
    inv = np.stack([np.cross(b, c), np.cross(c, a), np.cross(a, b)], axis=1) / det           # r = s @ h, s = r @ inv
    s = np.asarray(xyz, dtype=np.float64).astype(LD) @ inv
    s = s - np.floor(s)
    return np.where(s >= 1, LD(0), s), hl


def _walk_small(hl, s):
    """(i, j, d, order_gap): every candidate of the small geometry in its walk order -- i, then j in index order, then the eight
    combinations of the two images per axis, bit k choosing the second image along axis k."""
    n = len(s)
    e = s[None, :, :] - s[:, None, :]                                   # [i, j, 3]
    f = np.where(e > 0, e - 1, e + 1)
    out = []
    for c in range(8):
        pick = np.array([(c >> k) & 1 for k in range(3)], dtype=bool)
        out.append(np.where(pick, f, e) @ hl)                           # [i, j, 3]
    d = np.stack(out, axis=2).reshape(n * n * 8, 3)                     # (i, j, c) in C order: the walk
    i = np.repeat(np.arange(n), n * 8)
    j = np.tile(np.repeat(np.arange(n), 8), n)
    off = ~np.eye(n, dtype=bool)
    order_gap = min(float(np.abs(e[off]).min()) if n > 1 else np.inf, float(np.minimum(s, 1 - s).min()))
    return i, j, d, order_gap


def _walk_general(hl, s, g):
    """The same for the general geometry with the grid g: i, then the 27 cell offsets (z slowest, x fastest, each with its own
    image shift), then the members of the cell in index order."""
    n = len(s)
    g = np.asarray(g, dtype=np.int64)
    sg = s * g.astype(LD)
    c = np.clip(np.floor(sg).astype(np.int64), 0, g - 1)
    lin = (c[:, 2] * g[1] + c[:, 1]) * g[0] + c[:, 0]
    order = np.argsort(lin, kind="stable")                              # inside a cell by index
    ncell = int(g.prod())
    count = np.bincount(lin, minlength=ncell)
    start = np.concatenate([[0], np.cumsum(count)])
    kmax = int(count.max())
    members = np.full((ncell, kmax), -1, dtype=np.int64)
    members[lin[order], np.arange(n) - start[lin[order]]] = order
    out_i, out_j, out_d, out_o = [], [], [], []
    me = np.arange(n)
    o = 0
    for oz in (-1, 0, 1):
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                cc = c + np.array([ox, oy, oz])
                shift = np.floor_divide(cc, g)
                cc = cc - shift * g
                cand = members[(cc[:, 2] * g[1] + cc[:, 1]) * g[0] + cc[:, 0]]          # [n, kmax], ascending index
                a, b = np.nonzero(cand >= 0)
                j = cand[a, b]
                out_i.append(me[a]), out_j.append(j), out_o.append(np.full(len(a), o))
                out_d.append(((s[j] - s[a]) + shift[a].astype(LD)) @ hl)
                o += 1
    i, j, d, o = (np.concatenate(v) for v in (out_i, out_j, out_d, out_o))
    rank = np.lexsort((j, o, i))
    frac = sg - np.floor(sg)
    order_gap = float(np.minimum(frac, 1 - frac).min())                # a molecule this close to a cell wall could sit in the other cell
    return i[rank], j[rank], d[rank], order_gap


def adf_exact(h, xyz, r_cut, edges, group=None, ngroups=1, grid=None, keep="walk"):
    """dict: hist [ngroups, nbins] int64, counts [N] int32, summary [ngroups, 4] int64 (centres, pairs enumerated, pairs binned,
    centres over the cap) as include/mw_adf.h defines them for one box, lengths in bohr; and the preconditions of an exact
    comparison: gap_r = the smallest |r^2 - r_cut^2| / r_cut^2 over every candidate of the walk, gap_c = the smallest
    |c - edge| over every pair of kept entries of every molecule and every edge other than -1 and 1 (the clamp ends), gap_order
    = for a box with a molecule over the cap the smallest distance (fractional) of a molecule from changing the walk order --
    a cell wall, the cell's own wrap or, in the small geometry, ds_k = 0 -- and inf for a box without.  ``grid``: the cell
    grid (g_1, g_2, g_3) of the general geometry; None: the small geometry up to 64 molecules and `cell_grid` beyond.
    ``keep="nearest"`` keeps the 32 nearest entries instead of the first 32 of the walk (not the contract: what a test
    compares with to show that the order matters)."""
    h = np.asarray(h, dtype=np.float64)
    xyz = np.asarray(xyz, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    n, nbins = len(xyz), len(edges) - 1
    s, hl = _fractional(h, xyz)
    if grid is None and n <= SMALL_N:
        i, j, d, order_gap = _walk_small(hl, s)
    else:
        i, j, d, order_gap = _walk_general(hl, s, cell_grid(h, r_cut, n) if grid is None else grid)
    r2 = (d * d).sum(axis=1)
    rc2 = LD(r_cut) * LD(r_cut)
    positive = r2 > 0                                                   # (j, n) = (i, 0) is the only candidate at distance 0
    gap_r = float((np.abs(r2[positive] - rc2) / rc2).min()) if positive.any() else np.inf
    hit = positive & (r2 < rc2)
    i, j, d, r2 = i[hit], j[hit], d[hit], r2[hit]
    if keep == "nearest":
        by_r = np.lexsort((r2, i))
        i, j, d, r2 = i[by_r], j[by_r], d[by_r], r2[by_r]
    counts = np.bincount(i, minlength=n)
    first = np.concatenate([[0], np.cumsum(counts)])[:-1]
    slot = np.arange(len(i)) - first[i]                                 # place in the walk
    kept = slot < KEEP
    k = np.minimum(counts, KEEP)
    K = max(1, int(k.max(initial=0)))
    U = np.zeros((n, K, 3), dtype=LD)
    U[i[kept], slot[kept]] = d[kept] / np.sqrt(r2[kept])[:, None]
    grp = np.zeros(n, dtype=np.int64) if group is None else np.asarray(group, dtype=np.int64)
    assert grp.shape == (n,) and np.all((grp >= -1) & (grp < ngroups))
    hist = np.zeros((ngroups, nbins), dtype=np.int64)
    summary = np.zeros((ngroups, 4), dtype=np.int64)
    el = edges.astype(LD)
    inner = el[(edges != -1.0) & (edges != 1.0)]
    gap_c = np.inf
    a_idx, b_idx = np.triu_indices(K, 1)
    for m0 in range(0, n, 256):
        sl = slice(m0, m0 + 256)
        C = np.clip(np.einsum("iac,ibc->iab", U[sl], U[sl])[:, a_idx, b_idx], LD(-1), LD(1))      # [m, pairs]
        valid = b_idx[None, :] < k[sl, None]
        if len(inner) and valid.any():
            cv = C[valid]
            at = np.searchsorted(inner, cv)
            below, above = inner[np.clip(at - 1, 0, len(inner) - 1)], inner[np.clip(at, 0, len(inner) - 1)]
            gap_c = min(gap_c, float(np.minimum(np.abs(cv - below), np.abs(cv - above)).min()))
        binned = valid & (C >= el[0]) & (C <= el[-1])
        which = np.clip(np.searchsorted(el, C, side="right") - 1, 0, nbins - 1)
        for gi in range(ngroups):
            rows = grp[sl] == gi
            pick = binned & rows[:, None]
            hist[gi] += np.bincount(which[pick], minlength=nbins)
    for gi in range(ngroups):
        rows = grp == gi
        kk = k[rows]
        summary[gi] = (int(rows.sum()), int((kk * (kk - 1) // 2).sum()), int(hist[gi].sum()), int((counts[rows] > KEEP).sum()))
    capped = bool((counts > KEEP).any())
    return dict(hist=hist, counts=counts.astype(np.int32), summary=summary, gap_r=gap_r, gap_c=gap_c,
                gap_order=order_gap if capped else np.inf, max_count=int(counts.max(initial=0)))


def preconditions(ref):
    """(gap_r, gap_c, gap_order) of an adf_exact dict: each must exceed MARGIN."""
    return ref["gap_r"], ref["gap_c"], ref["gap_order"]


# -- the inputs the GPU tests use (tests/test_gpu_adf.py), and their preconditions (tests/test_adf_ref.py) -----------------
def cases():
    """[(label, golden name or None, gas size or None, radius in Angstrom, names of EDGE_SETS)]: every golden of
    tet_ref.cases() but the 4096-molecule ones at 3.5 Angstrom and at 4.8 Angstrom, and the gas boxes at 3.5 Angstrom, every
    radius held inside the narrowest width of the cell (`load_case`).  Both edge sets everywhere but on the ideal lattices at
    the second-shell radius, whose angles of exactly 60, 90 and 120 degrees lie on edges of the theta bins: those take the 97
    bins in cos(theta) only."""
    from conftest import golden_names
    out = []
    for name in golden_names():
        if any(t in name for t in ("4096", "32768")):
            continue
        thermal = "_t0" in name or name in ("gas20", "dimer", "single_atom")
        out.append((f"{name} 3.5", name, None, R_FIRST_ANG, ("cos97", "theta90")))
        out.append((f"{name} 4.8", name, None, R_SECOND_ANG, ("cos97", "theta90") if thermal else ("cos97",)))
    out += [(f"gas N = {n}", None, n, R_FIRST_ANG, ("cos97", "theta90")) for n in GAS_SIZES]
    # the general geometry with one cell along two axes, most molecules over the cap (radius None: 0.55 of the narrowest width)
    out += [("gas N = 65 in one cell", None, 65, None, ("cos97", "theta90"))]
    return out


def load_case(case):
    """(h, xyz, r_cut in bohr) of a case of `cases`: the radius is min(its Angstrom, 0.9999 of the narrowest width; 0.98 for a
    gas box), or 0.55 of the narrowest width where the case names none."""
    from conftest import load_golden
    label, name, gas, r_ang, _ = case
    if name is None:
        h, xyz = gas_box(gas, 1000 + gas)
    else:
        z = load_golden(name)
        h, xyz = z["h"], z["xyz"]
    w = float(widths(h).min())
    if r_ang is None:
        return h, xyz, 0.55 * w
    return h, xyz, min(r_ang * ANG_TO_BOHR, (0.98 if name is None else 0.9999) * w)


#: (golden, boxes) of the batches of tests/test_gpu_adf.py (tet_ref.BATCHES), made by boo_ref.batch_set
BATCHES = (("ih48_t020", 9), ("ic96", 4), ("ih1536_t012", 3))


def batch_radius(hs):
    """r_cut in bohr for a batch: 4.8 Angstrom, held inside the narrowest cell of the batch."""
    return min(R_SECOND_ANG * ANG_TO_BOHR, 0.9999 * min(float(widths(h).min()) for h in hs))


def cap_radius(h, xyz, want, lo=0.5, hi=None):
    """A radius (bohr) at which the largest entry count of the box is exactly `want`, by bisection over counts in the
    reference's own distances; None if the count jumps over `want`."""
    hi = 0.9999 * float(widths(h).min()) if hi is None else hi
    e = EDGE_SETS["cos97"]
    if adf_exact(h, xyz, hi, e)["max_count"] < want:
        return None
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        m = adf_exact(h, xyz, mid, e)["max_count"]
        if m == want:
            return mid
        lo, hi = (mid, hi) if m < want else (lo, mid)
    return None
