"""GPU: the four libraries on csrc/mw_lib_cells.h see the same entries.  For the same cells, positions and cutoff the entry
count of every molecule is the same number in libmw_adf.so (counts), libmw_rings.so (counts), libmw_boo.so (nn[..., 0]) and
libmw_tet.so (counts[..., 0], the entries within r_search), and it is the count of tests/adf_ref.py -- exactly: the shapes are
the smallest at which the grid and the sort can go wrong (tests/lib_cells_cases.py), and tests/test_lib_cells.py asserts that
none of them has a pair within adf_ref.MARGIN of the cutoff."""
import numpy as np
import pytest

from adf_ref import MARGIN, cell_grid
from lib_cells_cases import CASES, R_ANG, RC, reference

pytestmark = pytest.mark.gpu

#: label -> (small geometry, the grid of the first box or None where only its size matters)
EXPECT = {"n65_one_cell": (False, (1, 1, 1)), "n200_343_cells": (False, (7, 7, 7)), "n64_small": (True, None),
          "n96_three_cells": (False, (5, 5, 5)), "n200_shifted_on_planes": (False, (7, 7, 7))}


@pytest.fixture(scope="module", autouse=True)
def _library_lifetime():
    """Each library is initialised by its first call here and finalised when this file is done."""
    yield
    from mc_water_ls_mw_amd import angles, bondorder, rings, tetrahedral
    for finalize in (angles.adf_finalize, rings.rings_finalize, bondorder.boo_finalize, tetrahedral.tet_finalize):
        finalize()


@pytest.mark.parametrize("label", sorted(CASES))
def test_the_four_libraries_count_the_same_entries(label):
    from mc_water_ls_mw_amd.angles import adf_last, angle_counts
    from mc_water_ls_mw_amd.bondorder import bond_order, boo_last
    from mc_water_ls_mw_amd.rings import ring_statistics, rings_last
    from mc_water_ls_mw_amd.tetrahedral import tet_last, tetrahedral_order
    cells, pos, want, gap_r = reference(label)
    assert gap_r > MARGIN
    small, grid = EXPECT[label]
    got = {"adf": angle_counts(cells, pos, R_ANG, np.array([-1.0, 1.0]))[1],
           "rings": ring_statistics(cells, pos, R_ANG)[3],
           "boo": bond_order(cells, pos, R_ANG, 0.5)[1][..., 0],
           "tet": tetrahedral_order(cells, pos, R_ANG, R_ANG)[2][..., 0]}
    for last in (adf_last, rings_last, boo_last, tet_last):                    # one batch, on the path the case is about
        p = last()
        assert p["small"] == small and p["chunks"] == 1 and p["boxes_per_chunk"] == len(cells), (label, p)
        if grid:
            assert (p["g1"], p["g2"], p["g3"]) == grid == cell_grid(cells[0], RC, pos.shape[1]), (label, p)
    for name, counts in got.items():
        print(label, name, "entries", int(counts.sum()), "wrong counts", int(np.count_nonzero(counts != want)))
        assert counts.shape == want.shape and np.array_equal(counts, want), (label, name)
