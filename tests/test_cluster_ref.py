"""CPU: the union-find reference of tests/cluster_ref.py on boxes whose clusters are known in closed form, its behaviour
under a permutation of the molecule order, and the conditions the GPU tests need of the defect box -- all from brute-force
neighbours (ice_ref.brute_neighbours) and the reference classes (ice_ref.ice_classes) at r_c = 3.5 Angstrom."""
import functools

import numpy as np
import pytest

import cluster_ref as cr
from ice_ref import ANG_TO_BOHR, ECLIPSED, RC_ANG, STAGGERED, brute_neighbours, ice_classes, stacking_counts

RC = RC_ANG * ANG_TO_BOHR
SEQ160 = "ABCABCABABABCABCBCBC"
CUBIC, HEX = 0b10, 0b100


@functools.lru_cache(maxsize=None)
def _analysed(name):
    """(h, xyz, cls, bond values, neighbour count, four entries) of a named box."""
    from mc_water_ls_mw_amd import lattice as lat
    if name == "defect":
        h, xyz = cr.defect_box()
    else:
        seq, sigma = name.split(":")
        h, xyz = lat.stacked_ice_box(seq, (2, 1), sigma_ang=float(sigma))
    iv, nn, jn, vn = brute_neighbours(h, xyz, RC)
    cls, c, _ = ice_classes(xyz, iv, nn, jn, vn, RC)
    count, j4 = cr.neighbour_entries(xyz, iv, nn, jn, vn, RC)
    return h, xyz, cls, c, count, j4


def _sizes(name, mask):
    _, _, cls, _, count, j4 = _analysed(name)
    label, summary = cr.clusters_from_entries(cls, count, j4, mask)
    sz = cr.sizes(label)
    assert summary[0] == sum(sz) == int(((mask >> cls.astype(int)) & 1).sum()) and summary[1] == len(sz)
    assert summary[2] == (sz[0] if sz else 0)
    if sz:
        assert summary[3] == min(r for r in np.unique(label[label > 0]) if (label == r).sum() == sz[0])
        assert np.all(label[label > 0] <= np.nonzero(label > 0)[0] + 1)          # a label is its cluster's smallest molecule
        assert all(label[r - 1] == r for r in np.unique(label[label > 0]))
    return sz


def test_abcb_alternates_cubic_and_hexagonal_pairs_of_sublayers():
    cls = _analysed("ABCB:0")[2]
    assert len(cls) == 32 and stacking_counts("ABCB") == (16, 16)
    assert _sizes("ABCB:0", CUBIC) == [2] * 8
    assert _sizes("ABCB:0", HEX) == [2] * 8
    assert _sizes("ABCB:0", CUBIC | HEX) == [32]


@pytest.mark.parametrize("sigma", ["0", "0.08"])
def test_a_stacking_disordered_box_of_160(sigma):
    name = f"{SEQ160}:{sigma}"
    cls, c = _analysed(name)[2:4]
    assert np.array_equal(np.bincount(cls, minlength=6), [0, 96, 64, 0, 0, 0])
    assert _sizes(name, CUBIC) == [64, 32]
    assert _sizes(name, HEX) == [32, 32]
    for mask in (CUBIC | HEX, cr.MASK_DEFAULT, cr.MASK_ALL):
        assert _sizes(name, mask) == [160]
    live = (c != 2.0) & ~np.isnan(c)
    assert min(np.abs(c[live] - t).min() for t in (STAGGERED, *ECLIPSED)) > 0.1   # the classes are not a matter of rounding


def test_hexagonal_ice_of_64_bilayers_is_one_cluster():
    assert _sizes("AB" * 32 + ":0", HEX) == [512]
    assert _sizes("AB" * 32 + ":0", CUBIC) == []
    assert np.array_equal(cr.summary_of(np.zeros(7, dtype=np.int32)), [0, 0, 0, 0])


def test_a_bad_mask_is_refused():
    _, _, cls, _, count, j4 = _analysed("ABCB:0")
    for mask in (0, 1, 0b1111, 64, -2):
        with pytest.raises(ValueError):
            cr.clusters_from_entries(cls, count, j4, mask)


@pytest.mark.parametrize("name,mask", [(f"{SEQ160}:0.08", CUBIC), (f"{SEQ160}:0.08", HEX), ("defect", cr.MASK_DEFAULT)])
def test_labels_follow_a_permutation_of_the_molecule_order(name, mask):
    h, xyz, cls, _, count, j4 = _analysed(name)
    label, summary = cr.clusters_from_entries(cls, count, j4, mask)
    perm = np.random.default_rng(5).permutation(len(xyz))
    iv, nn, jn, vn = brute_neighbours(h, xyz[perm], RC)
    cls_p = ice_classes(xyz[perm], iv, nn, jn, vn, RC)[0]
    assert np.array_equal(cls_p, cls[perm])
    label_p, summary_p = cr.clusters(cls_p, xyz[perm], iv, nn, jn, vn, RC, mask)
    assert np.array_equal(label_p, cr.permute_labels(label, perm))
    assert cr.sizes(label_p) == cr.sizes(label) and np.array_equal(summary_p[:3], summary[:3])
    assert not np.array_equal(label_p, label[perm])                              # (the canonical labels did have to move)


def test_the_defect_box_is_a_fair_input():
    """What the GPU tests rely on: several clusters of several sizes, a lone selected molecule, and no class or bond that
    hangs on the last digits -- no bond value within 0.02 of a CHILL+ threshold, no pair distance within 0.01 Angstrom of r_c."""
    h, xyz, cls, c, count, j4 = _analysed("defect")
    assert len(xyz) <= 1024
    label, summary = cr.clusters_from_entries(cls, count, j4, cr.MASK_DEFAULT)
    sz = cr.sizes(label)
    assert summary[1] == len(sz) >= 3 and len(set(sz)) >= 2 and sz[-1] == 1, sz
    assert (cls == 0).any() and not np.isnan(c).any()
    live = c != 2.0
    assert min(np.abs(c[live] - t).min() for t in (STAGGERED, *ECLIPSED)) >= 0.02
    iv, nn, jn, vn = brute_neighbours(h, xyz, RC + 0.5 * ANG_TO_BOHR)
    held = np.arange(jn.shape[1])[None, :] < nn[:, None]
    d = (xyz[np.where(held, jn - 1, 0)] + iv[np.where(held, vn - 1, 0)]) - xyz[:, None, :]
    r = np.sqrt((d * d).sum(axis=2))[held]
    assert (r < RC).sum() == count.sum() and np.abs(r - RC).min() >= 0.01 * ANG_TO_BOHR
