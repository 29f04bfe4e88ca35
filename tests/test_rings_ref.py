"""CPU: the depth-first reference of the ring statistics (tests/rings_ref.py) against the figures include/mw_rings.h was
written to -- every molecule of ice in twelve 6-rings, and the counts of four hot boxes -- and against itself (member sums,
the list, an independent count of the closed paths), and the one precondition of the exact comparisons of
tests/test_gpu_rings.py for every input that file uses: no r^2 within 1e-9 relative of r_cut^2."""
import itertools

import numpy as np
import pytest

from boo_ref import batch_set, scaled_set, widths
from rings_ref import (ANG_TO_BOHR, AT_THE_CAP, BATCHES, DEG, HOT, ICE, MARGIN, PARTLY_CAPPED, SIZES, _rows, case_exact, cases,
                       entries, outputs, ring_list, rings_exact)

CASES = cases()


def _case(label):
    return next(c for c in CASES if c[0] == label)


def _consistent(ref, n):
    assert np.array_equal(ref["member"].sum(axis=0), np.array(SIZES) * ref["hist"])
    assert ref["summary"][3] == ref["hist"].sum() == len(ref["rings"]) and np.all(ref["hist"] <= ref["closed"])
    assert ref["summary"][0] == int((ref["counts"] > DEG).sum()) and ref["summary"][2] <= ref["closed_full"]
    rings = ref["rings"]
    if len(rings):
        L = rings[:, 0]
        assert np.array_equal(np.bincount(L, minlength=8)[3:], ref["hist"])
        assert np.all(np.diff(rings[:, 1]) >= 0)                           # by ascending root
        for row in rings:
            mols = row[1:1 + row[0]]
            assert mols.min() == mols[0] >= 0 and mols.max() < n and np.all(row[1 + row[0]:] == -1)
            assert np.all(ref["counts"][mols] <= DEG)                      # a molecule over the cap is in no ring


@pytest.mark.parametrize("name", ICE)
def test_every_molecule_of_ice_sits_in_twelve_six_rings(name):
    h, xyz, rc, ref = case_exact(_case(f"{name} 3.5"))
    n = len(xyz)
    assert ref["hist"].tolist() == ref["closed"].tolist() == [0, 0, 0, 2 * n, 0]
    assert np.all(ref["member"][:, 3] == 12) and np.all(ref["counts"] == 4) and ref["summary"].tolist()[:2] == [0, 2 * n]
    # only the 8-molecule box is narrow enough to hold a molecule twice in a ring: 8 of its 16 rings take the full comparison
    assert ref["summary"][2] == ref["closed_full"] == (8 if name == "ih8_small" else 0)
    _consistent(ref, n)


def test_a_sheared_cell_takes_its_columns_as_vectors():
    """Read with the transposed cell, the same positions of ic64_sheared are no ice."""
    h, xyz, rc, ref = case_exact(_case("ic64_sheared 3.5"))
    assert not np.allclose(h, h.T)
    wrong = rings_exact(h.T, xyz, min(rc, 0.9999 * float(widths(h.T).min())))
    assert wrong["hist"].tolist() != ref["hist"].tolist()


@pytest.mark.parametrize("key", list(HOT), ids=[f"{k[0]}{k[1]}" for k in HOT])
def test_the_figures_of_the_hot_boxes(key):
    h, xyz, rc, ref = case_exact(_case(f"{key[0]}{key[1]} sigma {key[2]} seed {key[3]}"))
    hist, closed, largest = HOT[key]
    assert tuple(ref["hist"]) == hist and tuple(ref["closed"]) == closed
    if largest is not None:
        assert ref["max_count"] == largest
    if key[1] == (2, 1, 1):
        assert len(xyz) == 16 and ref["closed_full"] == 1                  # one closed path by the full comparison; it is not primitive
    _consistent(ref, len(xyz))


def test_over_the_cap_there_are_no_edges():
    h, xyz, rc, ref = case_exact(_case("ih1536_t012 4.8"))
    n = len(xyz)
    assert ref["counts"].min() > DEG and ref["summary"].tolist() == [n, 0, 0, 0]
    assert not ref["hist"].any() and not ref["closed"].any() and not ref["member"].any() and len(ref["rings"]) == 0
    for label in PARTLY_CAPPED:
        h, xyz, rc, ref = case_exact(_case(label))
        assert 0 < ref["summary"][0] < len(xyz) and ref["summary"][3] > 0, label
        _consistent(ref, len(xyz))
    ref = case_exact(_case(AT_THE_CAP))[3]
    assert 8 in ref["counts"] and 9 in ref["counts"]


def test_the_list_is_cut_and_padded():
    ref = case_exact(_case("ic(2, 2, 2) sigma 0.5 seed 3"))[3]
    total = len(ref["rings"])
    assert total == 63
    assert ring_list(ref, 0).shape == (0, 8)
    short, ample = ring_list(ref, 10), ring_list(ref, total + 5)
    assert np.array_equal(short, ref["rings"][:10]) and np.array_equal(ample[:total], ref["rings"]) and np.all(ample[total:] == -1)
    assert [o.dtype for o in outputs(ref, 4)] == [np.int64, np.int64, np.int32, np.int32, np.int64, np.int32]


def _closed_by_sets(h, xyz, rc):
    """The closed paths of 3 ... 7 nodes, counted another way: every simple cycle through images of the molecules is
    collected as the set of its edges, shifted so that its smallest (molecule, image) node has image 0, and the sets counted."""
    n = len(xyz)
    i, j, img, _ = entries(h, xyz, rc)
    _, rows = _rows(n, i, j, img)
    seen = [set() for _ in SIZES]

    def walk(path):
        u = path[-1]
        for e in rows[u[0]]:
            w = (e[0], u[1] + e[1], u[2] + e[2], u[3] + e[3])
            if w == path[0] and len(path) >= 3:
                base = min(path)
                cyc = [(v[0], v[1] - base[1], v[2] - base[2], v[3] - base[3]) for v in path]
                seen[len(path) - 3].add(frozenset(frozenset((cyc[k], cyc[(k + 1) % len(cyc)])) for k in range(len(cyc))))
            elif w not in path and len(path) < 7:
                walk(path + [w])

    for root in range(n):
        walk([(root, 0, 0, 0)])
    return [len(s) for s in seen]


@pytest.mark.parametrize("label", ("ih8_small 3.5", "ih(2, 1, 1) sigma 0.5 seed 6", "ic(2, 2, 2) sigma 0.5 seed 3"))
def test_closed_paths_counted_another_way(label):
    """No pruning by index and no readings: cycles as edge sets modulo translation."""
    h, xyz, rc, ref = case_exact(_case(label))
    assert _closed_by_sets(h, xyz, rc) == ref["closed"].tolist()


def test_closed_paths_against_networkx():
    nx = pytest.importorskip("networkx")
    h, xyz, rc, ref = case_exact(_case("ih(2, 1, 1) sigma 0.5 seed 6"))    # 16 molecules: the graph over 7 x 7 x 7 cells stays small
    n = len(xyz)
    i, j, img, _ = entries(h, xyz, rc)
    _, rows = _rows(n, i, j, img)
    g = nx.Graph()
    shifts = list(itertools.product(range(-3, 4), repeat=3))      # a ring of 7 through the origin cell reaches 3 cells
    for a in range(n):
        for m in shifts:
            for e in rows[a]:
                g.add_edge((a, *m), (e[0], m[0] + e[1], m[1] + e[2], m[2] + e[3]))
    count = [0] * 5
    for a in range(n):                                                     # a ring of 7 through a node stays within 3 edges of it
        root = (a, 0, 0, 0)
        if root in g:
            for cyc in nx.simple_cycles(nx.ego_graph(g, root, radius=3), length_bound=7):
                if len(cyc) >= 3 and min(cyc) == root:
                    count[len(cyc) - 3] += 1
    assert count == ref["closed"].tolist()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_preconditions_of_every_gpu_case(case):
    h, xyz, rc, ref = case_exact(case)
    print(case[0], "gap r^2 %.2e" % ref["gap_r"], "largest count", ref["max_count"], "hist", ref["hist"].tolist())
    assert ref["gap_r"] > MARGIN and rc * (1.0 + 1e-9) <= float(widths(h).min())


def test_preconditions_of_every_batch():
    sets = [batch_set(name, n) for name, n in BATCHES]
    sets += [scaled_set("ih48_t020", 250, 0.3, 500), scaled_set("ic96", 3, 0.3, 70), scaled_set("ih48_t020", 6, 0.3, 70)]
    for hs, xs in sets:
        for b in range(len(hs)):
            assert entries(hs[b], xs[b], 3.5 * ANG_TO_BOHR)[3] > MARGIN, b
            assert 3.5 * ANG_TO_BOHR * (1.0 + 1e-9) <= float(widths(hs[b]).min())
