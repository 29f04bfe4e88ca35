"""Numpy / union-find reference for the engine's ice clusters (mw_ice_clusters.hip.h, DESIGN.md "Ice clusters"), from the
CHILL+ classes of one box and a neighbour table (xyz, ivect, nn, jn, vn) in the reference's list layout (1-based) -- brute
force (ice_ref.brute_neighbours) or the engine's own list -- the bond cutoff rc in bohr and a class mask.

Molecule i is selected iff bit cls[i] of the mask is set (classes 1..5 only: such a molecule has exactly four neighbour
entries with 0 < |d| < rc).  Selected i and selected j are bonded iff j is one of i's four entries or i is one of j's; an
entry that is an image of i itself is no bond, several images of one j are one bond.  label[i] = 0 for a molecule that is not
selected, else the 1-based index of the smallest molecule of its connected component; summary = (selected molecules,
clusters, size of the largest cluster, its label), a tie going to the smallest label, all 0 when nothing is selected.
"""
from __future__ import annotations

import numpy as np

MASK_ALL = 0b111110
MASK_DEFAULT = 0b1110          # cubic + hexagonal + interfacial ice


def neighbour_entries(xyz, ivect, nn, jn, vn, rc):
    """(count [N], j [N, 4]): the number of entries with 0 < |d| < rc of every molecule and the 0-based j of the first four,
    in list order, -1 past the count.  d is formed as the kernels (and ice_ref) form it."""
    xyz = np.asarray(xyz, dtype=np.float64)
    ivect = np.asarray(ivect, dtype=np.float64)
    nn, jn, vn = np.asarray(nn), np.asarray(jn), np.asarray(vn)
    n, smax = jn.shape
    live = np.arange(smax)[None, :] < nn[:, None]
    j = np.where(live, jn - 1, 0)
    v = np.where(live, vn - 1, 0)
    d = (xyz[j] + ivect[v]) - xyz[:, None, :]
    r2 = d[..., 2] * d[..., 2] + (d[..., 1] * d[..., 1] + d[..., 0] * d[..., 0])
    bond = live & (r2 < rc * rc) & (r2 > 0.0)
    count = bond.sum(axis=1)
    first = np.argsort(~bond, axis=1, kind="stable")[:, :4]
    if first.shape[1] < 4:
        first = np.pad(first, ((0, 0), (0, 4 - first.shape[1])))
    ok = np.arange(4)[None, :] < np.minimum(count, 4)[:, None]
    ok &= np.arange(4)[None, :] < smax
    return count, np.where(ok, np.take_along_axis(j, np.minimum(first, smax - 1), 1), -1)


def _find(parent, x):
    r = x
    while parent[r] != r:
        r = parent[r]
    while parent[x] != r:
        parent[x], x = r, parent[x]
    return r


def clusters_from_entries(cls, count, j4, mask):
    """(label int32 [N], summary int32 [4]) from the classes and the four neighbour entries of every molecule."""
    if mask <= 0 or mask & ~MASK_ALL:
        raise ValueError(f"mask {mask} is not a non-empty subset of classes 1..5")
    cls = np.asarray(cls)
    n = len(cls)
    sel = ((mask >> cls.astype(np.int64)) & 1).astype(bool)
    assert np.all(count[sel] == 4), "a molecule of class 1..5 has exactly four neighbours"
    parent = list(range(n))
    for i in np.nonzero(sel)[0]:
        for j in j4[i]:
            if j < 0 or j == i or not sel[j]:
                continue
            a, b = _find(parent, int(i)), _find(parent, int(j))
            if a != b:
                parent[max(a, b)] = min(a, b)
    label = np.zeros(n, dtype=np.int32)
    for i in np.nonzero(sel)[0]:
        label[i] = _find(parent, int(i)) + 1            # (the smaller root always wins: a root is its tree's smallest molecule)
    return label, summary_of(label)


def summary_of(label):
    lab = np.asarray(label)
    roots, sizes = np.unique(lab[lab > 0], return_counts=True)
    if len(roots) == 0:
        return np.zeros(4, dtype=np.int32)
    k = int(np.argmax(sizes))                            # first of the largest: roots ascend, so the smallest label
    return np.array([int((lab > 0).sum()), len(roots), int(sizes[k]), int(roots[k])], dtype=np.int32)


def clusters(cls, xyz, ivect, nn, jn, vn, rc, mask=MASK_DEFAULT):
    count, j4 = neighbour_entries(xyz, ivect, nn, jn, vn, rc)
    return clusters_from_entries(cls, count, j4, mask)


def sizes(label):
    """Cluster sizes, largest first."""
    lab = np.asarray(label)
    return sorted((int(s) for s in np.unique(lab[lab > 0], return_counts=True)[1]), reverse=True)


def permute_labels(label, perm):
    """The canonical labels of the box whose molecule k is molecule perm[k] of the box that ``label`` belongs to."""
    lab = np.asarray(label)[perm]
    out = np.zeros_like(lab)
    for root in np.unique(lab[lab > 0]):
        members = np.nonzero(lab == root)[0]
        out[members] = members.min() + 1
    return out


#: the defect box of the tests: Ih "AB" x 8 (16 bilayers of 8 molecules, 128 in all) with bilayers 3 and 9 displaced by a
#: Gaussian of 0.6 Angstrom, strongly enough to become class 0 almost throughout: the ice falls into two slabs of different
#: thickness and one lone ice-like molecule inside a displaced bilayer.  The seed was searched (400 seeds of three such
#: recipes gave three boxes) for the conditions tests/test_cluster_ref.py asserts: no bond value within 0.02 of a CHILL+
#: threshold (0.023 here), no pair distance within 0.01 Angstrom of r_c (0.024 here).
DEFECT = {"sequence": "AB" * 8, "reps_xy": (2, 1), "seed": 240, "sigma_ang": 0.6, "slabs": ((3, 4), (9, 10)), "singles": ()}


def defect_box():
    """(h, xyz) of the defect box."""
    from mc_water_ls_mw_amd import lattice as lat
    d = DEFECT
    h, xyz = lat.stacked_ice_box(d["sequence"], d["reps_xy"])
    rng = np.random.default_rng(d["seed"])
    per_bilayer = 4 * d["reps_xy"][0] * d["reps_xy"][1]
    moved = np.zeros(len(xyz), dtype=bool)
    for lo, hi in d["slabs"]:                                       # bilayers lo .. hi-1
        moved[lo * per_bilayer:hi * per_bilayer] = True
    moved[list(d["singles"])] = True
    disp = rng.normal(0.0, d["sigma_ang"] * lat.ANG_TO_BOHR, size=xyz.shape)
    return h, np.ascontiguousarray(np.where(moved[:, None], xyz + disp, xyz))
