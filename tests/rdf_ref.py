"""Numpy reference for the engine's pair-distance histogram (mw_rdf), written from the definition.

For a box with cell vectors h[0], h[1], h[2] (rows, bohr), positions xyz (bohr, wrapped or not), a range r_max and nbins:
hist[b] = the number of ORDERED triples (i, j, n) -- n = (n1, n2, n3) any integer lattice translation, (j, n) != (i, 0) -- with
d = |r_j + n1 h[0] + n2 h[1] + n3 h[2] - r_i|, 0 < d < r_max and b = floor(d nbins / r_max).

rdf_brute enumerates EVERY translation that can reach, with no wrapping and no rule: with s = r h^-1 the fractional
coordinates and w_k the perpendicular width of the cell along k (volume / |h_l x h_m|: the distance between the two faces),
a difference vector d has |d| >= |(s_j - s_i + n)_k| w_k for every k, so |d| < r_max needs
|n_k| < r_max / w_k + |s_j,k - s_i,k| <= r_max / w_k + (the spread of s_k over the box), and all of those are taken.

rdf_fast wraps the fractional difference to [-1/2, 1/2] per axis first (ds -= rint(ds)), which changes d by a whole
lattice translation only.  Then |(ds + n)_k| >= |n_k| - 1/2, so a translation n_k != 0 reaches inside r_max only if
(|n_k| - 1/2) w_k < r_max, i.e. |n_k| < r_max / w_k + 1/2.  Hence, per axis: n_k = 0 alone is complete when
r_max <= w_k / 2 (|n_k| = 1 would need r_max > w_k / 2), and n_k in {-1, 0, 1} is complete when r_max <= 1.5 w_k
(|n_k| = 2 would need r_max > 1.5 w_k).  The factor (1 + 1e-9) on r_max keeps rounding in w_k away from the thresholds.
That is the image rule of the kernels; rdf_fast refuses r_max (1 + 1e-9) > 1.5 min_k w_k.

Both return (hist int64 [nbins], edge int64 [nbins + 1]): edge[b] = the number of triples -- counted or not -- whose d lies
within EDGE_TOL = 1e-9 bohr of the bin edge b r_max / nbins (edge[nbins]: of r_max itself).  Two correct evaluations of d
differ by rounding, ~1e-12 bohr at these coordinates; a pair further than EDGE_TOL from every edge has ONE right bin.
"""
from __future__ import annotations

import numpy as np

ANG_TO_BOHR = 1.0 / 0.5291772108
EDGE_TOL = 1e-9


def widths(h):
    """Perpendicular widths of the cell along its three vectors (rows of h)."""
    h = np.asarray(h, dtype=np.float64)
    vol = abs(np.linalg.det(h))
    return np.array([vol / np.linalg.norm(np.cross(h[(k + 1) % 3], h[(k + 2) % 3])) for k in range(3)])


def image_range(r_max, w):
    """Images per axis by the rule: 0 (n_k = 0 alone) or 1 (n_k in -1, 0, 1); ValueError beyond 1.5 w."""
    r = r_max * (1.0 + 1e-9)
    if r <= 0.5 * w:
        return 0
    if r <= 1.5 * w:
        return 1
    raise ValueError(f"r_max = {r_max} beyond 1.5 x the cell width {w}")


def _accumulate(d, self_mask, r_max, nbins, hist, edge):
    """Add the distances d (any shape; self_mask marks the (i, i, 0) entries, which are no triples) to hist and edge."""
    d = d[~self_mask] if self_mask is not None else d.ravel()
    dr = r_max / nbins
    near = d < r_max + 2.0 * EDGE_TOL
    d = d[near]
    k = np.rint(d / dr).astype(np.int64)
    on = (np.abs(d - k * dr) <= EDGE_TOL) & (k <= nbins)
    edge += np.bincount(k[on], minlength=nbins + 1)[:nbins + 1]
    d = d[(d > 0.0) & (d < r_max)]
    b = np.minimum(np.floor(d * nbins / r_max).astype(np.int64), nbins - 1)
    hist += np.bincount(b, minlength=nbins)


def rdf_brute(h, xyz, r_max, nbins):
    h = np.asarray(h, dtype=np.float64)
    xyz = np.asarray(xyz, dtype=np.float64)
    n = len(xyz)
    s = xyz @ np.linalg.inv(h)
    spread = s.max(axis=0) - s.min(axis=0)
    reach = [int(np.floor(r_max / w + sp)) + 1 for w, sp in zip(widths(h), spread)]
    hist = np.zeros(nbins, dtype=np.int64)
    edge = np.zeros(nbins + 1, dtype=np.int64)
    eye = np.eye(n, dtype=bool)
    none = np.zeros((n, n), dtype=bool)
    for n1 in range(-reach[0], reach[0] + 1):
        for n2 in range(-reach[1], reach[1] + 1):
            for n3 in range(-reach[2], reach[2] + 1):
                t = n1 * h[0] + n2 * h[1] + n3 * h[2]
                d = (xyz[None, :, :] + t) - xyz[:, None, :]
                d = np.sqrt((d * d).sum(axis=2))
                _accumulate(d, eye if (n1, n2, n3) == (0, 0, 0) else none, r_max, nbins, hist, edge)
    return hist, edge


def rdf_fast(h, xyz, r_max, nbins, chunk=256, workers=1):
    """Wrapped fractional differences + the image rule, chunked over i (``workers`` threads, numpy releases the GIL)."""
    h = np.asarray(h, dtype=np.float64)
    xyz = np.asarray(xyz, dtype=np.float64)
    n = len(xyz)
    m = [image_range(r_max, w) for w in widths(h)]
    shifts = np.array([(a, b, c) for a in range(-m[0], m[0] + 1) for b in range(-m[1], m[1] + 1)
                       for c in range(-m[2], m[2] + 1)], dtype=np.float64)
    s = xyz @ np.linalg.inv(h)
    reach2 = (r_max + 2.0 * EDGE_TOL) ** 2

    def part(i0):
        hist = np.zeros(nbins, dtype=np.int64)
        edge = np.zeros(nbins + 1, dtype=np.int64)
        i1 = min(n, i0 + chunk)
        ds = s[None, :, :] - s[i0:i1, None, :]
        ds -= np.rint(ds)
        central = np.zeros(ds.shape[:2], dtype=bool)
        central[np.arange(i1 - i0), np.arange(i0, i1)] = True
        for sh in shifts:
            d = (ds + sh) @ h
            r2 = (d * d).sum(axis=2)
            keep = r2 < reach2
            if not sh.any():
                keep &= ~central
            _accumulate(np.sqrt(r2[keep]), None, r_max, nbins, hist, edge)
        return hist, edge

    starts = range(0, n, chunk)
    if workers > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(workers) as pool:
            parts = list(pool.map(part, starts))
    else:
        parts = [part(i0) for i0 in starts]
    return sum(p[0] for p in parts), sum(p[1] for p in parts)


def cumulative(hist):
    """C[b] = hist[:b].sum(), b = 0 .. nbins."""
    return np.concatenate([[0], np.cumsum(np.asarray(hist, dtype=np.int64))])


def assert_same(hist_a, hist_b, edge, what=""):
    """The comparison rule: a pair within EDGE_TOL of edge b may sit on either side of it and nothing else may differ --
    |C_a[b] - C_b[b]| <= edge[b] for b = 1 .. nbins; where edge is zero this is equality of the histograms."""
    ca, cb = cumulative(hist_a), cumulative(hist_b)
    assert ca.shape == cb.shape == edge.shape, (ca.shape, cb.shape, edge.shape)
    bad = np.nonzero(np.abs(ca - cb)[1:] > edge[1:])[0] + 1
    assert len(bad) == 0, (what, bad[:8], ca[bad[:8]], cb[bad[:8]], edge[bad[:8]])


def assert_cap(edge, what=""):
    """The rule must not hide a failure: at most ONE bin edge of an input has a pair near it."""
    assert np.count_nonzero(edge[1:]) <= 1, (what, np.nonzero(edge[1:])[0] + 1, edge[edge > 0])
