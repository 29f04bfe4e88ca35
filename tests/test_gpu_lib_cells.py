"""GPU: the four analysis libraries on csrc/mw_lib_cells.h (six more stand on it through mw_lib_forces.h: see
tests/test_gpu_lib_cells_forces.py) see the same entries.  For the same cells, positions and cutoff the entry count of every
molecule is the same number in libmw_adf.so (counts), libmw_rings.so (counts), libmw_boo.so (nn[..., 0]) and libmw_tet.so
(counts[..., 0], the entries within r_search), and it is the count of tests/adf_ref.py -- exactly: the shapes are the smallest
at which the grid, the sort and the two walks can go wrong (tests/lib_cells_cases.py: five boxes of its own, the grid shapes
and twelve random oblique boxes), and tests/test_lib_cells.py asserts that none of them has a pair within adf_ref.MARGIN of the
cutoff.  On the grid shapes and the random boxes each library is also held to its own mirror beyond the counts, at that mirror's
bar: a count does not see a wrong bond vector."""
import numpy as np
import pytest

from adf_ref import EDGE_SETS, MARGIN, cell_grid
from lib_cells_cases import CASES, LABELS, R2_ANG, R_ANG, RC, RC2, analysis_box, expected_plan, grid_reference, reference

pytestmark = pytest.mark.gpu

LD = np.longdouble
TOL = 1e-12                                      # the bar of tests/test_gpu_boo.py and tests/test_gpu_tet.py
NAN_BITS = 0x7ff8000000000000
#: label -> (small geometry, the grid of the first box or None where only its size matters)
EXPECT = {"n65_one_cell": (False, (1, 1, 1)), "n200_343_cells": (False, (7, 7, 7)), "n64_small": (True, None),
          "n96_three_cells": (False, (5, 5, 5)), "n200_shifted_on_planes": (False, (7, 7, 7))}
#: the grid shapes and the random boxes: the grid tests/lib_cells_cases.py names, which is adf_ref.cell_grid's (asserted on the CPU)
EXPECT.update({label: expected_plan(label, analysis_box(label)[0], len(analysis_box(label)[1]), RC) for label in LABELS})


@pytest.fixture(scope="module", autouse=True)
def _library_lifetime():
    """Each library is initialised by its first call here and finalised when this file is done."""
    yield
    from mc_water_ls_mw_amd import angles, bondorder, rings, tetrahedral
    for finalize in (angles.adf_finalize, rings.rings_finalize, bondorder.boo_finalize, tetrahedral.tet_finalize):
        finalize()


def _inputs(label):
    """(cells, pos, counts, gap_r) of a case of either table."""
    if label in CASES:
        return reference(label)
    (h, pos), ref = analysis_box(label), grid_reference(label)
    return h[None], pos[None], ref["counts"][None], ref["gap_r"]


def _lasts():
    from mc_water_ls_mw_amd.angles import adf_last
    from mc_water_ls_mw_amd.bondorder import boo_last
    from mc_water_ls_mw_amd.rings import rings_last
    from mc_water_ls_mw_amd.tetrahedral import tet_last
    return adf_last, rings_last, boo_last, tet_last


@pytest.mark.parametrize("label", sorted(CASES) + list(LABELS))
def test_the_four_libraries_count_the_same_entries(label):
    from mc_water_ls_mw_amd.angles import angle_counts
    from mc_water_ls_mw_amd.bondorder import bond_order
    from mc_water_ls_mw_amd.rings import ring_statistics
    from mc_water_ls_mw_amd.tetrahedral import tetrahedral_order
    cells, pos, want, gap_r = _inputs(label)
    assert gap_r > MARGIN
    small, grid = EXPECT[label]
    got = {"adf": angle_counts(cells, pos, R_ANG, np.array([-1.0, 1.0]))[1],
           "rings": ring_statistics(cells, pos, R_ANG)[3],
           "boo": bond_order(cells, pos, R_ANG, 0.5)[1][..., 0],
           "tet": tetrahedral_order(cells, pos, R_ANG, R_ANG)[2][..., 0]}
    for last in _lasts():                                                      # one batch, on the path the case is about
        p = last()
        assert p["small"] == small and p["chunks"] == 1 and p["boxes_per_chunk"] == len(cells), (label, p)
        if grid:
            assert (p["g1"], p["g2"], p["g3"]) == grid == cell_grid(cells[0], RC, pos.shape[1]), (label, p)
    for name, counts in got.items():
        print(label, name, "entries", int(counts.sum()), "wrong counts", int(np.count_nonzero(counts != want)))
        assert counts.shape == want.shape and np.array_equal(counts, want), (label, name)


@pytest.mark.parametrize("label", LABELS)
def test_each_library_is_its_mirrors_beyond_the_counts(label):
    """The histogram of cos(theta) of libmw_adf.so (exact), the ring counts, memberships and list of libmw_rings.so (exact), q4,
    q6 and their averaged forms of libmw_boo.so (1e-12 in q^2) and q, s_k, d5 and the LSI of libmw_tet.so with its four nearest
    (1e-12), on the grid shapes and the random boxes: every one of them is made of the bond vectors d, image shift included."""
    from boo_ref import boo_exact
    from rings_ref import outputs, rings_exact
    from tet_ref import tet_exact
    from mc_water_ls_mw_amd.angles import angle_counts
    from mc_water_ls_mw_amd.bondorder import bond_order
    from mc_water_ls_mw_amd.rings import ring_statistics
    from mc_water_ls_mw_amd.tetrahedral import tetrahedral_order
    h, pos = analysis_box(label)
    small, grid = EXPECT[label]
    lasts = dict(zip(("adf", "rings", "boo", "tet"), _lasts()))

    def on_its_path(name):
        p = lasts[name]()
        assert p["small"] == small and p["chunks"] == 1 and (p["g1"], p["g2"], p["g3"]) == grid, (label, name, p)

    # adf
    ref = grid_reference(label)
    hist, counts, summary = angle_counts(h, pos, R_ANG, EDGE_SETS["cos97"])
    on_its_path("adf")
    print(label, "adf: pairs binned", int(ref["summary"][0, 2]), "largest count", ref["max_count"], "wrong bins", int(np.count_nonzero(hist != ref["hist"])))
    assert np.array_equal(counts, ref["counts"]) and np.array_equal(hist, ref["hist"]) and np.array_equal(summary, ref["summary"]), label
    # rings
    ref = rings_exact(h, pos, RC)
    cap = len(ref["rings"]) + 3
    got = ring_statistics(h, pos, R_ANG, cap)
    on_its_path("rings")
    names = ("hist", "closed", "member", "counts", "summary", "list")
    print(label, "rings: hist", got[0].tolist(), "closed", got[1].tolist(), "summary", got[4].tolist(),
          "wrong", [name for name, g, w in zip(names, got, outputs(ref, cap)) if not np.array_equal(g, w)])
    for name, g, w in zip(names, got, outputs(ref, cap)):
        assert g.shape == w.shape and np.array_equal(g, w), (label, name)
    # boo
    ref = boo_exact(h, pos, RC, 0.5)
    q, nn, _ = bond_order(h, pos, R_ANG, 0.5)
    on_its_path("boo")
    dq = np.abs((q.astype(LD) ** 2 - ref["q2"]).astype(np.float64)).max(axis=0)
    print(label, "boo: max |d q^2| (q4, q6, qbar4, qbar6)", " ".join("%.2e" % v for v in dq), "(bar %.0e)" % TOL)
    assert np.array_equal(nn[:, 0], ref["n"]) and dq.max() <= TOL, label
    # tet
    ref = tet_exact(h, pos, RC, RC2)
    order, near, counts, _ = tetrahedral_order(h, pos, R_ANG, R2_ANG)
    on_its_path("tet")
    nan_ref = np.isnan(ref["order"].astype(np.float64))
    err = np.abs((order.astype(LD) - ref["order"]).astype(np.float64))
    worst = [float(np.max(err[~nan_ref[:, k], k], initial=0.0)) for k in range(4)]
    print(label, "tet: max |d| (q, s_k, d5, lsi)", " ".join("%.2e" % v for v in worst), "(bar %.0e)" % TOL,
          "wrong (counts, near)", int(np.count_nonzero(counts != ref["counts"])), int(np.count_nonzero(np.sort(near, axis=1) != np.sort(ref["near"], axis=1))))
    assert np.array_equal(counts, ref["counts"]) and np.array_equal(np.sort(near, axis=1), np.sort(ref["near"], axis=1)), label
    assert np.array_equal(np.isnan(order), nan_ref) and np.all(order.view(np.uint64)[nan_ref] == NAN_BITS) and max(worst) <= TOL, label
