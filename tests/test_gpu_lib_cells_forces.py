"""GPU: the six force libraries on csrc/mw_lib_cells.h (through csrc/mw_lib_forces.h) on the grid shapes and the twelve random
oblique boxes of tests/lib_cells_cases.py, as single points: libmw_md.so (nsteps = 0), libmw_quench.so (max_iter = 0),
libmw_npt.so and libmw_flex.so (nsteps = 0, baro_every = 0), libmw_hess.so (the dense matrix and four products) and libmw_ti.so
(nsteps = 0).  Each library compiles its own copy of the two walks and has its own callback that turns the image shift of a
cell into a bond vector, so each is held to its mirror on every box: a two-cell axis, an axis of one cell beside wider ones, a
lowered grid, 128 and 130 cells in a row, oblique cells narrower than twice the cutoff in both geometries.  tests/test_lib_cells.py
asserts on the CPU that every box is on the grid it is named for, that its mirror would see a lost image, and the spreads the
bars of W and W_ab are made of.

Bars.  E: conftest.RTOL = 1e-10 relative.  Forces: quench_ref.F_ATOL.  W and W_ab: lib_cells_cases.w_bar and w_ab_bar, the larger
of the mirror's bar and ten times the box's own recorded spread.  H and H v: RTOL times the largest element of the reference, as
in tests/test_gpu_hess.py.  The mixed force of libmw_ti.so: 4 ulp of its two terms against libmw_md.so's forces, as in
tests/test_gpu_ti.py, and F_ATOL against the mirror's.  One trajectory, 20 NVE steps on g123's box: md_ref's bars."""
import numpy as np
import pytest

from conftest import RTOL
from quench_ref import F_ATOL
import hess_ref
import lib_cells_cases as cases
import md_ref
import ti_ref
from md_ref import BAR_DT

pytestmark = pytest.mark.gpu

LAMBDA, SPRING, SITE_SHIFT = 0.3, 0.02, 0.1


@pytest.fixture(scope="module", autouse=True)
def _library_lifetime():
    """The libraries are initialised by their first calls here and finalised when this file is done."""
    yield
    from mc_water_ls_mw_amd import dynamics, einstein, flexcell, npt, phonons, quench
    for finalize in (dynamics.md_finalize, quench.quench_finalize, npt.npt_finalize, flexcell.flex_finalize, phonons.hess_finalize, einstein.ti_finalize):
        finalize()


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _on_its_path(label, name, last, small, grid):
    p = last()
    assert p.get("small", small) == small and (p["g1"], p["g2"], p["g3"]) == grid and p["chunks"] == 1 and p["boxes_per_chunk"] == 1, (label, name, p)


def _held(label, name, e, f, ref):
    de, df = abs(e - ref["e"]), float(np.abs(f - ref["f"]).max())
    print(label, name, "|E - E_ref| %.2e (bar %.2e) max |F - F_ref| %.2e (bar %.0e)" % (de, RTOL * abs(ref["e"]), df, F_ATOL))
    assert de <= RTOL * abs(ref["e"]) and df <= F_ATOL, (label, name)


@pytest.mark.parametrize("label", cases.LABELS)
def test_md_quench_npt_and_flex_give_the_mirrors_single_point_and_one_set_of_force_bytes(label):
    from mc_water_ls_mw_amd.dynamics import md_last, molecular_dynamics
    from mc_water_ls_mw_amd.flexcell import flex_last, molecular_dynamics_flex, pressure_tensor
    from mc_water_ls_mw_amd.npt import molecular_dynamics_npt, npt_last
    from mc_water_ls_mw_amd.quench import inherent_structures, quench_last
    h, pos = cases.force_box(label)
    n = len(pos)
    small, grid = cases.expected_plan(label, h, n, md_ref.A_SIGMA)
    ref = cases.force_reference(label)
    # md
    pos_md, _, f_md, trace, status = molecular_dynamics(h, pos, 0, BAR_DT)
    _on_its_path(label, "md", md_last, small, grid)
    assert trace.shape == (1, 4) and tuple(status) == (0, 0) and _same(pos_md, np.ascontiguousarray(pos))
    _held(label, "md", trace[0, 0], f_md, ref)
    # quench
    pos_q, f_q, stats, iters = inherent_structures(h, pos, 1e-10, 0)
    _on_its_path(label, "quench", quench_last, small, grid)
    assert tuple(iters) == (0, 0) and stats[0] == stats[1] and _same(pos_q, np.ascontiguousarray(pos))
    _held(label, "quench", stats[1], f_q, ref)
    # npt
    _, _, f_npt, _, _, trace, status = molecular_dynamics_npt(h, pos, 0, BAR_DT, baro_every=0)
    _on_its_path(label, "npt", npt_last, small, grid)
    assert trace.shape == (1, 6) and tuple(status) == (0, 0) and trace[0, 1] == 0.0
    vol = trace[0, 4]
    w = trace[0, 5] * 3.0 * vol
    bar = cases.w_bar(label) + 4.0 * np.spacing(abs(w))                      # forming W back from P
    _held(label, "npt", trace[0, 0], f_npt, ref)
    print(label, "npt W %.12e mirror %.12e: %.2e (bar %.2e)" % (w, ref["w"], abs(w - ref["w"]), bar))
    assert abs(vol - abs(np.linalg.det(h))) <= 1e-13 * vol and abs(w - ref["w"]) <= bar
    # flex
    _, _, f_flex, _, _, trace, status = molecular_dynamics_flex(h, pos, 0, BAR_DT, baro_every=0)
    _on_its_path(label, "flex", flex_last, small, grid)
    assert trace.shape == (1, 15) and tuple(status) == (0, 0)
    wab = pressure_tensor(trace)[0] * trace[0, 4]
    bar_ab = cases.w_ab_bar(label) + 4.0 * np.spacing(float(np.abs(wab).max()))
    _held(label, "flex", trace[0, 0], f_flex, ref)
    print(label, "flex largest |W_ab| %.6e: against the mirror %.2e (bar %.2e), its trace against npt's W %.2e (bar %.2e)" % (
        np.abs(wab).max(), np.abs(wab - ref["wab"]).max(), bar_ab, abs(np.trace(wab) - w), bar))
    assert np.abs(wab - ref["wab"]).max() <= bar_ab and abs(np.trace(wab) - w) <= bar
    # the four share entry_force: for the same box the same bytes
    assert _same(f_md, f_q) and _same(f_md, f_npt) and _same(f_md, f_flex), label


@pytest.mark.parametrize("label", cases.LABELS)
def test_the_hessian_and_four_products_are_the_references(label):
    from mc_water_ls_mw_amd.phonons import hess_last, hessian, hessian_matvec
    h, pos = cases.force_box(label)
    n = len(pos)
    _, grid = cases.expected_plan(label, h, n, md_ref.A_SIGMA)
    energy = hess_ref.Energy(h, cases.wrapped(h, pos))                      # a whole lattice vector changes no second derivative
    ref = energy.dense()
    H, ef = hessian(h, pos)
    _on_its_path(label, "hess", hess_last, False, grid)
    bar = RTOL * float(np.abs(ref).max())
    point = cases.force_reference(label)
    print(label, "max |H_ref| %.4e max |H - H_ref| %.2e (bar %.2e) asymmetry %.2e |E - E_ref| %.2e" % (bar / RTOL, np.abs(H - ref).max(), bar, np.abs(H - H.T).max(),
                                                                                                  abs(ef[0] - point["e"])))
    assert H.shape == (3 * n, 3 * n) and np.all(np.isfinite(H)) and np.abs(H - ref).max() <= bar and np.abs(H - H.T).max() <= bar
    assert abs(ef[0] - point["e"]) <= RTOL * abs(point["e"]) and abs(ef[1] - np.abs(point["f"]).max()) <= F_ATOL
    vecs = np.random.default_rng(1000 + n).standard_normal((4, n, 3))
    vecs /= np.sqrt((vecs * vecs).sum(axis=(1, 2)))[:, None, None]
    want = energy.matvec(vecs)
    out, _ = hessian_matvec(h, pos, vecs)
    _on_its_path(label, "hess", hess_last, False, grid)
    bar = RTOL * float(np.abs(want).max())
    print(label, "max |H_ref v| %.4e max |H v - H_ref v| %.2e (bar %.2e)" % (bar / RTOL, np.abs(out - want).max(), bar))
    assert out.shape == vecs.shape and np.abs(out - want).max() <= bar


@pytest.mark.parametrize("label", cases.LABELS)
def test_the_einstein_library_mixes_the_same_forces_with_the_spring(label):
    from mc_water_ls_mw_amd.dynamics import molecular_dynamics
    from mc_water_ls_mw_amd.einstein import einstein_md, ti_last
    h, pos = cases.force_box(label)
    n = len(pos)
    small, grid = cases.expected_plan(label, h, n, md_ref.A_SIGMA)
    u = np.random.default_rng(300 + n).uniform(-SITE_SHIFT, SITE_SHIFT, size=pos.shape)
    sites = np.ascontiguousarray(pos - u)
    u = pos - sites                                                          # what the library forms
    pos_out, vel_out, forces, trace, blocks, status = einstein_md(h, sites, LAMBDA, SPRING, 0, BAR_DT, pos=pos)
    _on_its_path(label, "ti", ti_last, small, grid)
    f_md = molecular_dynamics(h, pos, 0, BAR_DT)[2]
    oml, nlk = 1.0 - LAMBDA, -(LAMBDA * SPRING)
    want = oml * f_md + nlk * u
    ulp = np.abs(forces - want) / np.spacing(np.abs(oml * f_md) + np.abs(nlk * u))
    ref = cases.force_reference(label)
    mirror = ti_ref.mixed_force(LAMBDA, SPRING, ref["f"], u)
    print(label, "ti: %.2f ulp of |oml F| + |nlk u| from libmw_md.so's forces (bar 4), max |F_tot - mirror| %.2e (bar %.0e), |E - E_ref| %.2e (bar %.2e)" % (
        ulp.max(), np.abs(forces - mirror).max(), F_ATOL, abs(trace[0, 0] - ref["e"]), RTOL * abs(ref["e"])))
    assert ulp.max() <= 4.0 and np.abs(forces - mirror).max() <= F_ATOL
    assert abs(trace[0, 0] - ref["e"]) <= RTOL * abs(ref["e"])
    assert _same(pos_out, np.ascontiguousarray(pos)) and np.all(vel_out == 0.0) and tuple(status) == (0, 0) and blocks.shape == (0, 5)


def test_twenty_steps_through_cell_walls_land_where_the_mirror_lands():
    """libmw_md.so sorts again at every step: on g123's box (one, two and three cells) molecules change their cell within the 20
    steps (tests/test_lib_cells.py asserts that at least three do in the mirror's run)."""
    from mc_water_ls_mw_amd.dynamics import md_last, molecular_dynamics
    label = cases.TRAJECTORY_LABEL
    h, pos = cases.force_box(label)
    n = len(pos)
    small, grid = cases.expected_plan(label, h, n, md_ref.A_SIGMA)
    ref = cases.trajectory_reference()
    pos_out, vel_out, forces, trace, status = molecular_dynamics(h, pos, cases.TRAJECTORY_STEPS, BAR_DT, vel=cases.trajectory_velocities())
    _on_its_path(label, "md", md_last, small, grid)
    dp, dv = float(np.abs(pos_out - ref["pos"]).max()), float(np.abs(vel_out - ref["vel"]).max())
    dt = np.abs(trace - ref["trace"]).max(axis=0)
    changed = int((cases.cells_of(h, pos, grid) != cases.cells_of(h, pos_out, grid)).sum())
    print(label, "status", tuple(status), "molecules in another cell", changed, "pos %.2e (bar %.2e) vel %.2e (bar %.2e)" % (dp, md_ref.POS_TOL, dv, md_ref.VEL_TOL),
          "trace", " ".join("%.2e" % v for v in dt), "bars", " ".join("%.2e" % v for v in md_ref.TRACE_TOL))
    assert tuple(status) == tuple(ref["status"]) == (cases.TRAJECTORY_STEPS, 0) and trace.shape == ref["trace"].shape and changed >= 3
    assert dp <= md_ref.POS_TOL and dv <= md_ref.VEL_TOL and np.all(dt <= np.array(md_ref.TRACE_TOL))
    assert np.abs(forces - ref["forces"]).max() <= md_ref.TRACE_TOL[3]
