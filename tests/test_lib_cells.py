"""CPU: the cell layer the ten cell-grid libraries share (csrc/mw_lib_cells.h) gives all of them one grid -- the grid fields
of mw_boo_plan, mw_tet_plan, mw_adf_plan and mw_rings_plan (none needs a device) agree with each other and with
adf_ref.cell_grid -- and each analysis library still refuses a narrow cell in its own words.  Also the preconditions of
tests/test_gpu_lib_cells.py and tests/test_gpu_lib_cells_forces.py: no pair of their inputs within adf_ref.MARGIN of the cutoff,
every grid-shape case of tests/lib_cells_cases.py on the grid it is named for in all ten plans, the force family's boxes no
closer than their floor, every case shown to tell a walk that loses images from one that keeps them, and the recorded spreads
of W and W_ab that the bars of the force family's boxes are made of."""
import numpy as np
import pytest

import lib_cells_cases as cases
import md_ref
from adf_ref import KEEP, MARGIN, _fractional, adf_exact, cell_grid
from boo_ref import widths
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


# -- the grid shapes of tests/lib_cells_cases.py --------------------------------------------------------------------------------
def _force_plans():
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.dynamics import md_plan
    from mc_water_ls_mw_amd.einstein import ti_plan
    from mc_water_ls_mw_amd.flexcell import flex_plan
    from mc_water_ls_mw_amd.npt import npt_plan
    from mc_water_ls_mw_amd.phonons import hess_plan
    from mc_water_ls_mw_amd.quench import quench_plan
    for builder in (build.build_quench, build.build_md, build.build_npt, build.build_flex, build.build_hess, build.build_ti):
        builder()
    return {"quench": quench_plan, "md": md_plan, "npt": npt_plan, "flex": flex_plan, "hess": hess_plan, "ti": ti_plan}


@pytest.mark.parametrize("label", cases.LABELS)
def test_every_grid_shape_is_on_its_grid_in_all_ten_plans(label):
    """adf_ref.cell_grid gives each case of GRID_SHAPES the grid it is named for, in both families; the two lowered cases start
    from the grid and stop at the cap they claim; and the ten plans (none needs a device) report that grid and geometry."""
    for family, box, r, plans in (("analysis", cases.analysis_box(label), RC, _plans()), ("force", cases.force_box(label), md_ref.A_SIGMA, _force_plans())):
        h, pos = box
        n = len(pos)
        small, grid = cases.expected_plan(label, h, n, r)
        w = widths(h) / r
        print(label, family, "N", n, "widths / r", np.round(w, 3).tolist(), "grid", grid, "small" if small else "general")
        assert grid == cell_grid(h, r, n) and small == (n <= 64) and w.min() >= 1.0 + 1e-9
        if label in cases.GRID_SHAPES:
            assert n == cases.GRID_SHAPES[label][2] and (cases.GRID_SHAPES[label][3] is None) == small
        if label in cases.UNLOWERED:
            full, cap = cases.UNLOWERED[label]
            assert tuple(int(v) for v in np.floor(w / (1.0 + 1e-9))) == full and cap == max(64, 2 * n) and int(np.prod(full)) > cap >= int(np.prod(grid))
        for word, plan in plans.items():
            p = plan(n, h, R_ANG) if family == "analysis" else plan(n, h)
            assert (p["g1"], p["g2"], p["g3"]) == grid and p.get("small", small) == small, (label, word, p)
    if label in cases.RANDOM_LABELS:
        assert 65 <= n <= 160


def _order_gap_off_the_planes(h, xyz, r):
    """adf_exact's gap_order without the coordinates that are exactly 0: how far a molecule is from changing the walk order,
    fractional.  A molecule on an s_k = 0 plane has s_k = 0 exactly on the device as in the reference (the rows of the inverse
    cell that form it hold exact zeros), and so has a difference of two of them: neither can fall on the other side."""
    s, _ = _fractional(h, xyz)
    s = s.astype(np.float64)
    n = len(s)
    if n <= 64:
        e = np.abs(s[None, :, :] - s[:, None, :])[~np.eye(n, dtype=bool)]
        v = np.concatenate([e[e != 0.0], np.minimum(s, 1.0 - s)[s != 0.0]])
    else:
        sg = s * np.array(cell_grid(h, r, n), dtype=np.float64)
        frac = sg - np.floor(sg)
        v = np.minimum(frac, 1.0 - frac)[s != 0.0]
    return float(v.min())


@pytest.mark.parametrize("label", cases.LABELS)
def test_no_pair_of_the_grid_shapes_is_at_a_cutoff(label):
    """What lets the device tests compare integers exactly: no r^2 within MARGIN of a radius (3.5 Angstrom, the second radius of
    the tetrahedral call and a sigma), no cos(theta) within MARGIN of a bin edge, no fourth and fifth neighbour within MARGIN of
    each other, no molecule of a box over the cap of 32 within MARGIN of changing the walk order."""
    from tet_ref import preconditions, tet_exact
    h, pos = cases.analysis_box(label)
    ref = cases.grid_reference(label)
    order = _order_gap_off_the_planes(h, pos, RC) if ref["max_count"] > KEEP else np.inf
    tet = preconditions(tet_exact(h, pos, RC, cases.RC2))
    hf, pf = cases.force_box(label)
    gap_f, _ = cases.cutoff_gap(hf, pf, md_ref.A_SIGMA)
    print(label, "gap_r", ref["gap_r"], "gap_c", ref["gap_c"], "order", order, "tet (4/5, r_search, r_lsi)", tet, "a sigma", gap_f,
          "entries per molecule", float(ref["counts"].mean()), "largest", ref["max_count"])
    assert ref["gap_r"] > MARGIN and ref["gap_c"] > MARGIN and order > MARGIN and min(tet) > MARGIN and gap_f > MARGIN
    assert ref["counts"].sum() > 0 and ref["counts"].sum() % 2 == 0
    assert np.array_equal(ref["counts"], cases.image_counts(h, pos, RC))            # the walk's entries are all 27 images'


@pytest.mark.parametrize("label", cases.LABELS)
def test_the_force_boxes_keep_their_floor_and_fit_the_mirrors_lists(label):
    h, pos = cases.force_box(label)
    _, nearest = cases.cutoff_gap(h, pos, md_ref.A_SIGMA)
    counts, e, f = cases.restricted_energy_forces(h, pos)
    ref = cases.force_reference(label)
    print(label, "nearest pair %.3f bohr (floor %.3f)" % (nearest, cases.MIN_SEP), "entries per molecule %.1f, largest %d" % (counts.mean(), counts.max()),
          "E %.6e largest |F| %.2e W %.4e" % (ref["e"], np.abs(ref["f"]).max(), ref["w"]))
    assert nearest >= cases.MIN_SEP and counts.max() <= 60
    assert np.array_equal(counts, adf_exact(h, pos, md_ref.A_SIGMA, np.array([-1.0, 1.0]))["counts"])
    # the mirror's lists (the C oracle's, over the wrapped positions) hold what all 27 images hold
    assert abs(e - ref["e"]) <= 1e-13 * abs(ref["e"]) and np.abs(f - ref["f"]).max() <= 1e-13
    assert abs(np.trace(ref["wab"]) - ref["w"]) <= 1e-12 * max(1.0, abs(ref["w"]))
    moved = np.abs(pos - cases.wrapped(h, pos)).max(axis=1) > 1.0
    s = pos @ np.linalg.inv(h)
    assert moved.sum() >= len(pos) // 4 and int((s == 0.0).any(axis=1).sum()) >= len(range(0, min(len(pos), 60), 10))


@pytest.mark.parametrize("label", cases.LABELS)
def test_every_grid_shape_tells_a_walk_that_loses_images(label):
    """With reference code alone: the entry counts -- and, in the force family, the energy -- of a walk that keeps the nearest
    image of every pair only, and of one that takes no image across the cell's boundary.  The second differs from the truth in
    every case; the first wherever a lattice vector is shorter than twice the radius (NARROW), where at least one pair must have
    two images in range.  An energy differs when it is more than a thousand energy bars (1e-10 relative) away."""
    for family, (h, pos), r in (("analysis", cases.analysis_box(label), RC), ("force", cases.force_box(label), md_ref.A_SIGMA)):
        true, nearest, inside = (cases.image_counts(h, pos, r, images) for images in ("all", "minimum", "none"))
        two = cases.pairs_with_two_images(h, pos, r)
        print(label, family, "entries", int(true.sum()), "pairs with two images", two, "molecules with other counts: minimum image", int((true != nearest).sum()),
              "no boundary", int((true != inside).sum()))
        assert not np.array_equal(true, inside)
        assert (two > 0) == (not np.array_equal(true, nearest))
        if label in cases.NARROW:
            assert two > 0
        if family == "force":
            e = cases.force_reference(label)["e"]
            e_min, e_in = (cases.restricted_energy_forces(h, pos, images)[1] for images in ("minimum", "none"))
            print(label, "E %.9e minimum image %.9e no boundary %.9e" % (e, e_min, e_in))
            assert abs(e_in - e) > 1e3 * 1e-10 * abs(e)
            if label in cases.NARROW:
                assert abs(e_min - e) > 1e3 * 1e-10 * abs(e)


def test_the_recorded_spreads_of_the_force_boxes_cover_the_measured_ones():
    """W and W_ab of every force box move by this much when the mirror's forces are perturbed by +-quench_ref.F_ATOL; the bar of
    a box is the larger of the mirror's own and ten times the recorded value, which is the measured one rounded up."""
    import flex_ref
    import npt_ref
    for label in cases.LABELS:
        w, wab = cases.measure_spreads(label)
        print(label, "W %.3e recorded %.3e bar %.3e   W_ab %.3e recorded %.3e bar %.3e" % (w, cases.W_SPREAD_MEASURED[label], cases.w_bar(label), wab,
                                                                                           cases.W_AB_SPREAD_MEASURED[label], cases.w_ab_bar(label)))
        assert w <= cases.W_SPREAD_MEASURED[label] <= 1.01 * w and wab <= cases.W_AB_SPREAD_MEASURED[label] <= 1.01 * wab
        assert cases.w_bar(label) >= npt_ref.W_TOL and cases.w_ab_bar(label) >= flex_ref.W_AB_TOL


def test_the_trajectory_box_sends_molecules_through_cell_walls():
    """The 20 steps of the mirror on g123's force box: at least three molecules end in another grid cell than they started in,
    so the device's run has to sort again on the way."""
    h, pos = cases.force_box(cases.TRAJECTORY_LABEL)
    ref = cases.trajectory_reference()
    grid = cases.GRID_SHAPES[cases.TRAJECTORY_LABEL][3]
    changed = int((cases.cells_of(h, pos, grid) != cases.cells_of(h, ref["pos"], grid)).sum())
    print("molecules in another cell after", cases.TRAJECTORY_STEPS, "steps:", changed, "status", tuple(ref["status"]))
    assert tuple(ref["status"]) == (cases.TRAJECTORY_STEPS, 0) and changed >= 3
