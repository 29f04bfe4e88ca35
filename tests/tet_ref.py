"""A numpy reference in np.longdouble for the nearest-neighbour order parameters of include/mw_tet.h: tetrahedral order q,
translational order s_k, fifth-neighbour distance d5, the local structure index, the four nearest neighbours and the entry
counts of every molecule, and the box summary.  Vectorised over the molecules: the entries of a box (boo_ref.entries) are
ranked by distance and padded to the largest n_search, and every value is an expression of that table.

The entries come from double-precision positions wrapped into the cell; their distances are then taken in long double and
ranked by them, so the reference knows the order of two entries wherever they differ by more than the rounding of a
difference of positions (1e-15 relative).  ``tet_exact`` therefore also returns what an exact comparison of counts and
neighbour sets needs to hold: per molecule the relative gap between ranks 4 and 5, per box how close any entry comes to
either radius.  tests/test_tet_ref.py asserts those for every input of tests/test_gpu_tet.py.
"""
from __future__ import annotations

import numpy as np

from boo_ref import entries, gas_box, widths

ANG_TO_BOHR = 1.0 / 0.5291772108
LD = np.longdouble
KEEP = 16                          # MW_TET_KEEP
R_SEARCH_ANG = 5.5
R_LSI_ANG = 3.7
GAS_SIZES = (1, 2, 63, 64, 65, 255, 256, 257)
#: the relative margin of the preconditions
MARGIN = 1e-9


def tet_exact(h, xyz, r_search, r_lsi, grid=None):
    """dict: order [N, 4] longdouble = (q, s_k, d5, lsi), NaN where not defined; near [N, 4] int (-1 where there is no such
    rank); counts [N, 2] int = (n_search, n_lsi); summary [8] longdouble; r [N, K] the ranked distances (inf beyond n_search);
    gap45 [N] = (r5 - r4) / r4 (inf where n_search < 5); gap_search, gap_lsi = the nearest | |d| - radius | / radius over every
    pair and image within 1.05 r_search.  ``grid``: a cell-grid search for the entries (default: beyond 256 molecules, where
    the cell holds three cells of 1.05 r_search per axis)."""
    h = np.asarray(h, dtype=np.float64)
    xyz = np.asarray(xyz, dtype=np.float64)
    nmol = len(xyz)
    wide = 1.05 * r_search
    if grid is None:
        grid = nmol > 256 and bool(np.all(np.floor(widths(h) / wide) >= 3))
    i, j, d = entries(h, xyz, wide, grid)
    dl = d.astype(LD)
    r = np.sqrt((dl * dl).sum(axis=1))
    gap_search = float(np.abs(r - r_search).min() / r_search) if len(r) else np.inf
    gap_lsi = float(np.abs(r - r_lsi).min() / r_lsi) if len(r) else np.inf
    keep = r < LD(r_search)
    i, j, dl, r = i[keep], j[keep], dl[keep], r[keep]
    rank = np.lexsort((r, i))                                           # by molecule, then by distance
    i, j, dl, r = i[rank], j[rank], dl[rank], r[rank]
    n = np.bincount(i, minlength=nmol)
    slot = np.arange(len(i)) - np.concatenate([[0], np.cumsum(n)])[:-1][i]
    K = max(KEEP + 1, int(n.max(initial=0)))
    R = np.full((nmol, K), np.inf, dtype=LD)
    J = np.full((nmol, K), -1, dtype=np.int64)
    D = np.zeros((nmol, K, 3), dtype=LD)
    R[i, slot], J[i, slot], D[i, slot] = r, j, dl
    n_lsi = (R < LD(r_lsi)).sum(axis=1)
    order = np.full((nmol, 4), np.nan, dtype=LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        four = n >= 4
        U = D[:, :4] / R[:, :4, None]
        acc = np.zeros(nmol, dtype=LD)
        for a in range(4):
            for b in range(a + 1, 4):
                acc += ((U[:, a] * U[:, b]).sum(axis=1) + LD(1) / 3) ** 2
        rbar = R[:, :4].sum(axis=1) / 4
        sk = 1 - ((R[:, :4] - rbar[:, None]) ** 2).sum(axis=1) / (12 * rbar ** 2)
        order[:, 0] = np.where(four, 1 - LD(3) / 8 * acc, np.nan)
        order[:, 1] = np.where(four, sk, np.nan)
        order[:, 2] = np.where(n >= 5, R[:, 4], np.nan)
        lsi_ok = (n_lsi >= 1) & (n_lsi + 1 <= np.minimum(n, KEEP))
        delta = R[:, 1:KEEP] - R[:, :KEEP - 1]                           # D_a, a = 1..15
        m = np.arange(KEEP - 1)[None, :] < n_lsi[:, None]
        delta = np.where(m & lsi_ok[:, None], delta, LD(0))
        nl = np.where(lsi_ok, n_lsi, 1).astype(LD)
        mean = delta.sum(axis=1) / nl
        var = (np.where(m, delta - mean[:, None], LD(0)) ** 2).sum(axis=1) / nl
        order[:, 3] = np.where(lsi_ok, var, np.nan)
        gap45 = np.where(n >= 5, ((R[:, 4] - R[:, 3]) / R[:, 3]).astype(np.float64), np.inf)
    summary = np.full(8, np.nan, dtype=LD)
    for k in range(4):
        ok = ~np.isnan(order[:, k])
        summary[4 + k] = ok.sum()
        if ok.any():
            summary[k] = order[ok, k].sum() / LD(int(ok.sum()))
    return dict(order=order, near=J[:, :4], counts=np.stack([n, n_lsi], axis=1), summary=summary, r=R, gap45=gap45,
                gap_search=gap_search, gap_lsi=gap_lsi)


# -- the inputs the GPU tests use (tests/test_gpu_tet.py), and their preconditions (tests/test_tet_ref.py) -----------------
def cases():
    """[(label, golden name or None, gas size or None, fraction of the narrowest width that bounds r_search, r_search as a
    fraction of the narrowest width or None, r_lsi in Angstrom or None for r_lsi = r_search)]: every input of
    tests/test_gpu_tet.py.  r_search is 5.5 Angstrom where the cell is wide enough, and r_lsi 3.7 Angstrom wherever r_search
    reaches that far (the narrowest boxes: r_lsi = r_search, the supported range's edge)."""
    from conftest import golden_names
    out = [(name, name, None, 0.9999, None, R_LSI_ANG) for name in golden_names() if not any(t in name for t in ("4096", "32768"))]
    out += [("ih4096_t015", "ih4096_t015", None, 0.9999, None, R_LSI_ANG)]
    out += [(f"gas N = {n}", None, n, 0.98, None, R_LSI_ANG) for n in GAS_SIZES]
    # the general geometry with one cell along two axes and every molecule with at least 16 entries
    out += [("gas N = 65 in one cell", None, 65, None, 0.55, R_LSI_ANG)]
    out += [("ih48_t020 without LSI", "ih48_t020", None, 0.9999, None, None)]
    return out


def load_case(case):
    """(h, xyz, r_search, r_lsi) of a case of `cases`, lengths in bohr."""
    from conftest import load_golden
    label, name, gas, bound, fraction, rl_ang = case
    if name is None:
        h, xyz = gas_box(gas, 1000 + gas)
    else:
        z = load_golden(name)
        h, xyz = z["h"], z["xyz"]
    w = float(widths(h).min())
    rs = fraction * w if fraction is not None else min(R_SEARCH_ANG * ANG_TO_BOHR, bound * w)
    rl = rs if rl_ang is None else min(rl_ang * ANG_TO_BOHR, rs)
    return h, xyz, rs, rl


def case_exact(case):
    """tet_exact of a case."""
    return tet_exact(*load_case(case))


#: (golden, boxes) of the batches of tests/test_gpu_tet.py, made by boo_ref.batch_set
BATCHES = (("ih48_t020", 9), ("ic96", 4), ("ih1536_t012", 3))


def batch_radii(hs):
    """(r_search, r_lsi) in bohr for a batch: 5.5 and 3.7 Angstrom, r_search held inside the narrowest cell of the batch."""
    w = min(float(widths(h).min()) for h in hs)
    rs = min(R_SEARCH_ANG * ANG_TO_BOHR, 0.9999 * w)
    return rs, min(R_LSI_ANG * ANG_TO_BOHR, rs)


def preconditions(ref):
    """(smallest 4/5 gap, gap to r_search, gap to r_lsi) of a tet_exact dict, all relative: each must exceed MARGIN."""
    return float(ref["gap45"].min()), ref["gap_search"], ref["gap_lsi"]
