"""CPU: the numpy references of tests/boo_ref.py for the bond-order parameters of include/mw_boo.h -- analytic values of the
ideal lattices, the symmetries of the definition, the two long-double routes against each other, the plain-double harmonic
tables against them (the noise floor the GPU tolerance sits a factor of ten above), and the preconditions that let
tests/test_gpu_boo.py compare neighbour and connection counts exactly."""
import numpy as np
import pytest

from conftest import load_golden
from boo_ref import (ANG_TO_BOHR, BATCHES, batch_set, gaps, boo_exact, case_exact, boo_tables, cases, entries, load_case, nearest_to_cutoff, real_harmonics, widths)

RC = 3.5 * ANG_TO_BOHR
CASES = cases()


def _f(a):
    return np.asarray(a, dtype=np.float64)


@pytest.fixture(scope="module")
def evaluated():
    """label -> (boo_exact, boo_tables, h, xyz, rc, thr) of every GPU input, computed once."""
    out = {}
    for case in CASES:
        h, xyz, rc, thr, grid = load_case(case)
        out[case[0]] = (case_exact(case), boo_tables(h, xyz, rc, thr, grid), h, xyz, rc, thr, grid)
    return out


@pytest.mark.parametrize("reps", [(2, 3, 1), (2, 3, 2), (4, 6, 8)])
def test_ideal_cubic_ice_has_the_tetrahedral_values(reps):
    """Ideal diamond lattices of 48, 96 and 1536 molecules (lattice.ice_box; the golden ic48 / ic96 / ic1536 are the
    reference program's slightly strained cells, q4^2 = 0.26024 there): n = 4, q4^2 = 7/27, q6^2 = 32/81, qbar = q = Q -- even l
    is blind to the inversion between the two sublattices -- and every s_ij = 1."""
    from mc_water_ls_mw_amd import lattice as lat
    h, xyz = lat.ice_box("ic", reps, 0.0)
    assert len(xyz) == 8 * reps[0] * reps[1] * reps[2]
    e = boo_exact(h, xyz, RC, 0.5, grid=len(xyz) > 256)
    want = np.array([7.0 / 27.0, 32.0 / 81.0] * 2)
    assert np.all(e["n"] == 4) and np.all(e["conn"] == 4)
    assert np.abs(_f(e["q2"]) - want).max() <= 1e-14
    assert np.abs(_f(e["summary"][:2]) - want[:2]).max() <= 1e-14
    assert np.abs(_f(e["summary"][2:]) - np.sqrt(want[:2])).max() <= 1e-14
    assert np.abs(_f(e["s"]) - 1.0).max() <= 1e-14
    t = boo_tables(h, xyz, RC, 0.5) if len(xyz) <= 96 else None
    if t is not None:
        assert np.abs(t["q2"] - want).max() <= 1e-14 and np.array_equal(t["conn"], e["conn"])


def test_ideal_hexagonal_ice_differs_only_in_the_average():
    from mc_water_ls_mw_amd import lattice as lat
    h, xyz = lat.ice_box("ih", (2, 3, 1), 0.0)
    e = boo_exact(h, xyz, RC, 0.5)
    assert np.all(e["n"] == 4)
    assert np.abs(_f(e["q2"][:, :2]) - [7.0 / 27.0, 32.0 / 81.0]).max() <= 1e-14
    assert np.all(_f(e["q2"][:, 3]) < 32.0 / 81.0 - 0.05) and np.all(_f(e["q2"][:, 2]) < 7.0 / 27.0 - 0.05)
    assert _f(e["summary"][1]) < 32.0 / 81.0 - 0.05


def test_a_single_atom_gives_zeros():
    z = load_golden("single_atom")
    for f in (boo_exact, boo_tables):
        e = f(z["h"], z["xyz"], RC, 0.5)
        assert e["n"].tolist() == [0] and e["conn"].tolist() == [0] and not np.any(_f(e["q2"])) and not np.any(_f(e["summary"]))


@pytest.mark.parametrize("name", ["ic48_t015", "ih48_t020", "gas20", "ih8_small"])
def test_rotations_and_lattice_translations_change_nothing(name):
    z = load_golden(name)
    h, xyz = z["h"], z["xyz"]
    rc = min(RC, 0.9999 * widths(h).min())
    e = boo_exact(h, xyz, rc, 0.5)
    rng = np.random.default_rng(5)
    rot, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    r = boo_exact(h @ rot.T, xyz @ rot.T, rc, 0.5)
    moved = xyz + rng.integers(-2, 3, xyz.shape).astype(np.float64) @ h
    m = boo_exact(h, moved, rc, 0.5)
    for o in (r, m):
        assert np.array_equal(o["n"], e["n"]) and np.array_equal(o["conn"], e["conn"])
        assert np.abs(_f(o["q2"] - e["q2"])).max() <= 1e-13 and np.abs(_f(o["summary"] - e["summary"])).max() <= 1e-13


def test_the_harmonic_tables_obey_the_addition_theorem():
    rng = np.random.default_rng(11)
    u = rng.normal(size=(200, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    x = u @ u.T
    for l, p in ((4, (35 * x ** 4 - 30 * x ** 2 + 3) / 8), (6, (231 * x ** 6 - 315 * x ** 4 + 105 * x ** 2 - 5) / 16)):
        Y = real_harmonics(l, u)
        assert Y.shape == (200, 2 * l + 1) and np.abs(Y @ Y.T - p).max() <= 1e-14


def test_the_grid_finds_the_entries_of_brute_force():
    z = load_golden("ih1536_t012")
    a, b = entries(z["h"], z["xyz"], RC, grid=False), entries(z["h"], z["xyz"], RC, grid=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.abs(a[2] - b[2]).max() <= 1e-12
    assert len(a[0]) == 4 * 1536


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_preconditions_of_the_exact_comparisons(case, evaluated):
    """No pair distance within 1e-9 rc of rc, no s_ij within 1e-6 of the threshold, rc inside the supported range."""
    e, _, h, xyz, rc, thr, grid = evaluated[case[0]]
    assert rc * (1.0 + 1e-9) <= widths(h).min()
    gap = nearest_to_cutoff(h, xyz, rc, grid)
    s = _f(e["s"])
    sgap = np.nanmin(np.abs(s - thr)) if np.any(np.isfinite(s)) else np.inf
    print(case[0], "N", len(xyz), "n", e["n"].min(), e["n"].max(), "nearest |d| - rc (rel)", gap / rc, "nearest s - thr", sgap)
    assert gap > 1e-9 * rc and sgap > 1e-6


@pytest.mark.parametrize("name,n", BATCHES)
def test_preconditions_of_the_batch_boxes_compared_exactly(name, n):
    """The last box of every batch of tests/test_gpu_boo.py is held to boo_exact with exact counts (3.5 Angstrom, 0.5)."""
    hs, xs = batch_set(name, n)
    grid = xs.shape[1] > 256
    ref = boo_exact(hs[-1], xs[-1], RC, 0.5, sums=False, grid=grid)
    gap, sgap = gaps(hs[-1], xs[-1], RC, 0.5, ref, grid)
    print(name, "box", n, "nearest |d| - rc (rel)", gap, "nearest s - thr", sgap)
    assert RC * (1.0 + 1e-9) <= widths(hs[-1]).min() and gap > 1e-9 and sgap > 1e-6


def test_the_special_inputs_are_what_they_are_meant_to_be(evaluated):
    e = evaluated["ih8_small at its width"][0]
    pairs = list(zip(e["i"].tolist(), e["j"].tolist()))
    assert len(set(pairs)) < len(pairs) and all(a != b for a, b in pairs)       # several images of one j, no self-image
    for label in ("ic48_t015 second shell", "ih48_t020 second shell"):
        n = evaluated[label][0]["n"]
        assert n.min() >= 12 and 16.0 <= n.mean() <= 20.0, label                 # 16 when ideal; thermal boxes add a few
    assert evaluated["gas N = 1"][0]["n"].tolist() == [0]
    assert any(evaluated[c[0]][0]["n"].min() == 0 for c in CASES) and max(evaluated[c[0]][0]["n"].max() for c in CASES) >= 16


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_noise_floor_of_a_double_evaluation(case, evaluated):
    """boo_tables (float64, explicit harmonics) within 1e-13 of the long-double sums on the squared invariants and on s_ij, and
    the two long-double routes within 1e-16 of each other.  Worst over all inputs: 1.0e-14 (recorded in DESIGN.md 3.9)."""
    e, t, h, xyz, rc, thr, grid = evaluated[case[0]]
    m = boo_exact(h, xyz, rc, thr, sums=False, grid=grid)
    if e["n"].max() > 8 and len(xyz) <= 48:
        e = boo_exact(h, xyz, rc, thr, sums=True, grid=grid)                       # the dense inputs took the moment route: the sums of the small ones
    worst = max(np.abs(_f(e["q2"]) - t["q2"]).max(), np.abs(_f(e["summary"]) - t["summary"]).max())
    if len(e["s"]):
        assert np.array_equal(np.isnan(_f(e["s"])), np.isnan(t["s"]))
        if np.any(np.isfinite(t["s"])):
            worst = max(worst, np.nanmax(np.abs(_f(e["s"]) - t["s"])))
    routes = max(np.abs(_f(e["q2"] - m["q2"])).max(), np.abs(_f(e["summary"] - m["summary"])).max())
    print(case[0], "tables - exact %.2e" % worst, "moments - sums %.2e" % routes)
    assert worst <= 1e-13 and routes <= 1e-16
    assert np.array_equal(e["n"], t["n"]) and np.array_equal(e["conn"], t["conn"]) and np.array_equal(e["conn"], m["conn"])
