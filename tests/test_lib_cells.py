"""CPU: the cell layer the four cell-grid libraries share (csrc/mw_lib_cells.h) gives all of them one grid -- the grid fields
of mw_boo_plan, mw_tet_plan, mw_adf_plan and mw_rings_plan (none needs a device) agree with each other and with
adf_ref.cell_grid -- and each library still refuses a narrow cell in its own words.  Also the preconditions of
tests/test_gpu_lib_cells.py: no pair of its inputs within adf_ref.MARGIN of the cutoff."""
import numpy as np
import pytest

from adf_ref import MARGIN, cell_grid
from lib_cells_cases import BOHR_TO_ANG, CASES, R_ANG, RC, reference

TRICLINIC = np.array([[30.0, 0.0, 0.0], [12.0, 28.0, 0.0], [-9.0, 11.0, 33.0]])
#: (label, cell in bohr, radius in Angstrom, nwater)
GRID_CASES = (
    ("cubic", np.eye(3) * 40.0, R_ANG, 100),
    ("orthorhombic", np.diag([30.0, 41.0, 55.0]), R_ANG, 100),
    ("triclinic", TRICLINIC, R_ANG, 100),                            # widths 25.5, 26.6, 33 against edges 30, 30.5, 35.9
    ("one cell", np.eye(3) * (1.5 * RC), R_ANG, 65),                 # every width below twice the radius
    ("lowered", np.diag([400.0, 300.0, 100.0]), R_ANG, 100),         # (60, 45, 15) down to 200 cells, ties on the way
    ("lowered, equal axes", np.eye(3) * 70.0, R_ANG, 100),           # (10, 10, 10): every step but the last is a tie
    ("1024 holds", np.diag([8000.0, 20.0, 20.0]), R_ANG, 5000),      # 1209 cells along x cut to 1024; 9216 fit 10000
    ("1024, then lowered", np.diag([8000.0, 20.0, 20.0]), R_ANG, 100),
    ("second radius", np.eye(3) * 40.0, 5.5, 100),
    ("n = 64", TRICLINIC, R_ANG, 64),
    ("n = 65", TRICLINIC, R_ANG, 65),
)


def _plans():
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.angles import adf_plan
    from mc_water_ls_mw_amd.bondorder import boo_plan
    from mc_water_ls_mw_amd.rings import rings_plan
    from mc_water_ls_mw_amd.tetrahedral import tet_plan
    for builder in (build.build_boo, build.build_tet, build.build_adf, build.build_rings):
        builder()
    return {"rc": boo_plan, "r_search": tet_plan, "r_cut (adf)": adf_plan, "r_cut (rings)": rings_plan}


@pytest.mark.parametrize("case", GRID_CASES, ids=[c[0] for c in GRID_CASES])
def test_the_four_plans_report_one_grid(case):
    _, h, r_ang, n = case
    want = cell_grid(h, r_ang / BOHR_TO_ANG, n)
    for word, plan in _plans().items():
        p = plan(n, h, r_ang)
        assert (p["g1"], p["g2"], p["g3"]) == want and p["small"] == (n <= 64), (word, p, want)
    assert int(np.prod(want)) <= max(64, 2 * n) and max(want) <= 1024


def test_the_grid_cases_cover_what_they_claim():
    grids = {label: cell_grid(h, r / BOHR_TO_ANG, n) for label, h, r, n in GRID_CASES}
    assert grids["one cell"] == (1, 1, 1) and len(set(grids["orthorhombic"])) == 3
    assert grids["lowered"] == (5, 6, 6) and grids["lowered, equal axes"] == (5, 6, 6)          # the first of equals goes down first
    assert grids["1024 holds"] == (1024, 3, 3) and grids["1024, then lowered"][0] < 1024
    assert grids["n = 64"] == grids["n = 65"]


def test_a_narrow_cell_is_refused_in_each_library_s_own_words():
    from mc_water_ls_mw_amd.energy import MwError
    h = np.diag([40.0, 40.0, 0.99 * RC])
    for word, plan in _plans().items():
        name = word.split()[0]
        with pytest.raises(MwError, match=r"_plan: " + name + r" = \S+ bohr is beyond the narrowest width \S+ bohr of box 0 \(" + name + r" \(1 \+ 1e-9\)"):
            plan(100, h, R_ANG)


@pytest.mark.parametrize("label", sorted(CASES))
def test_no_pair_of_the_gpu_cases_is_at_the_cutoff(label):
    cells, pos, counts, gap_r = reference(label)
    print(label, "gap_r", gap_r, "entries per molecule", float(counts.mean()), "largest", int(counts.max()))
    assert gap_r > MARGIN
    assert counts.shape == pos.shape[:2] and counts.min() >= 0 and counts.sum() > 0 and counts.sum() % 2 == 0        # entries come in pairs
