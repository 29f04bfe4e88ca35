"""CPU: the numpy mirror of include/mw_nuc.h (tests/nuc_ref.py) and the preconditions of the device tests
(tests/test_gpu_nuc.py): the single-point inputs keep boo_ref's own distances from the cutoff and the threshold; the trajectory
inputs keep, at every evaluation of the mirror, ten times the measured spread of s_ij under flex_ref.POS_TOL; the union-find
agrees with a flood fill; the host helpers of mc_water_ls_mw_amd.nucleation do what they say."""
import math

import numpy as np
import pytest

import boo_ref
import flex_ref
import nuc_ref
from boo_ref import ANG_TO_BOHR
from quench_ref import load_case


def test_single_point_inputs_keep_away_from_the_cutoff_and_the_threshold():
    """boo_ref's bars: no |d| within 1e-9 rc of rc, no s_ij within 1e-6 of the threshold -- and every input is inside the
    library's range (N >= 65, rc (1 + 1e-9) <= a sigma <= every width) and has what its place in the list is for."""
    seen = {}
    for k, (label, h, xyz, rc_ang, thr, mc, grid) in enumerate(nuc_ref.single_cases()):
        rc = rc_ang * ANG_TO_BOHR
        o = nuc_ref.single_reference(k)
        gd, gs = nuc_ref.gaps(o, rc, thr, h, xyz, grid)
        print(label, len(xyz), "op", o["op"], "largest n_i", o["nn"][:, 0].max(), "gap to rc / rc %.2e, to the threshold %.2e" % (gd / rc, gs))
        assert len(xyz) >= 65 and rc * (1.0 + 1e-9) <= nuc_ref.A_SIGMA and nuc_ref.A_SIGMA * (1.0 + 1e-9) <= boo_ref.widths(h).min()
        assert gd / rc > 1e-9 and gs > 1e-6, label
        seen[label] = o
    shaken = seen["ic96 shaken"]["op"]
    assert shaken[1] >= 3 and shaken[0] < 96                                 # at least three clusters and a molecule that is not solid-like
    assert seen["gas N = 65, rc = 0.98 a sigma"]["nn"][:, 0].max() > 2 * 12  # far above the list the cluster pass keeps (MW_NUC_LIST)
    assert seen["gas N = 255"]["op"][1] > 3 and seen["defect box"]["op"][1] >= 2
    assert seen["seeded box"]["op"][2] >= 10


def test_s_ij_moves_by_the_recorded_spread_under_the_position_bar():
    worst = 0.0
    for k, (name, langevin) in enumerate(nuc_ref.TRAJ_RUNS):
        rc = nuc_ref.TRAJ_ORDER[name][0] * ANG_TO_BOHR
        h, xyz = load_case(name)
        r = nuc_ref.reference(name, langevin)
        a, b = nuc_ref.s_spread(h, xyz, rc, flex_ref.POS_TOL, 1), nuc_ref.s_spread(r["cell"], r["pos"], rc, flex_ref.POS_TOL, 2)
        print(name, langevin, "spread of s_ij at the input %.3e, at the end %.3e" % (a, b))
        worst = max(worst, a, b)
    print("worst %.3e, recorded %.3e" % (worst, nuc_ref.S_SPREAD_MEASURED))
    assert 0.5 * nuc_ref.S_SPREAD_MEASURED <= worst <= nuc_ref.S_SPREAD_MEASURED


@pytest.mark.parametrize("name,langevin", nuc_ref.TRAJ_RUNS)
def test_every_evaluation_of_the_mirror_keeps_ten_spreads_from_the_threshold(name, langevin):
    """... and ten shifts of a distance from the cutoff; the runs with bounds stop where the unbounded series says."""
    h, xyz = load_case(name)
    r = nuc_ref.reference(name, langevin)
    assert tuple(r["status"]) == (nuc_ref.BAR_STEPS, 0) and [e[0] for e in r["evals"]] == list(range(0, nuc_ref.BAR_STEPS + 1, nuc_ref.TRAJ_CHECK))
    for steps, op, gd, gs in r["evals"]:
        print(name, langevin, steps, tuple(int(v) for v in op), "gap to rc %.2e bohr (bar %.2e), to the threshold %.2e (bar %.2e)" % (gd, nuc_ref.D_GAP, gs, nuc_ref.S_GAP))
        assert gd >= nuc_ref.D_GAP and gs >= nuc_ref.S_GAP
    assert np.array_equal(r["trace"][::nuc_ref.TRAJ_CHECK, 15], [e[1][2] for e in r["evals"]])
    assert np.array_equal(r["trace"][1:nuc_ref.TRAJ_CHECK, 15], np.full(nuc_ref.TRAJ_CHECK - 1, r["evals"][0][1][2]))   # the latest evaluation at or before the row
    lo, hi = nuc_ref.bounds_from(r, len(xyz))
    b = nuc_ref.reference(name, langevin, lo, hi)
    lam = [int(e[1][2]) for e in r["evals"]]
    first = next((k for k, v in enumerate(lam) if v != lam[0]), 0)
    want = nuc_ref.REACHED_LO if first and lam[first] < lam[0] else nuc_ref.REACHED_HI
    assert tuple(b["status"]) == (first * nuc_ref.TRAJ_CHECK, want) and len(b["evals"]) == first + 1
    rows = b["trace"]
    assert np.all(rows[first * nuc_ref.TRAJ_CHECK:] == rows[first * nuc_ref.TRAJ_CHECK]) and np.array_equal(rows[:first * nuc_ref.TRAJ_CHECK + 1], r["trace"][:first * nuc_ref.TRAJ_CHECK + 1])
    assert np.array_equal(b["op"], r["evals"][first][1])


def test_bounds_off_the_mirror_is_flex_ref():
    name = "ic65_interstitial"
    r = nuc_ref.reference(name, True)
    f = flex_ref.reference(name, True, nuc_ref.TRAJ_BARO, flex_ref.ANISO, 2)
    for k in ("pos", "vel", "forces", "cell", "ref", "status"):
        assert np.array_equal(r[k], f[k]), k
    assert np.array_equal(r["trace"][:, :15], f["trace"])


def test_union_find_against_a_flood_fill():
    for k, (label, h, xyz, rc_ang, thr, mc, grid) in enumerate(nuc_ref.single_cases()):
        if len(xyz) > 300:
            continue
        o = nuc_ref.single_reference(k)
        assert np.array_equal(nuc_ref.clusters_flood_fill(o["solid"], o["i"], o["j"]), o["label"]), label
    rng = np.random.default_rng(5)
    for n, m in ((40, 30), (90, 70), (200, 140)):
        solid = rng.random(n) < 0.7
        i, j = rng.integers(0, n, m), rng.integers(0, n, m)
        a, b = nuc_ref.clusters_union_find(solid, i, j), nuc_ref.clusters_flood_fill(solid, i, j)
        assert np.array_equal(a, b) and np.all(a[~solid] == 0) and np.all((a[solid] >= 1) & (a[solid] <= np.arange(n)[solid] + 1))
        op = nuc_ref.op_of(a)
        sizes = np.bincount(a[a > 0])
        assert op[0] == solid.sum() and op[1] == len(np.unique(a[a > 0])) and op[2] == sizes.max() and op[3] == int(np.argmax(sizes))
    assert tuple(nuc_ref.op_of(np.array([0, 2, 2, 4, 4, 0]))) == (4, 2, 2, 2)   # a tie goes to the smallest label
    assert tuple(nuc_ref.op_of(np.zeros(5, dtype=np.int32))) == (0, 0, 0, 0)


def test_an_unthermalised_ice_box_is_one_cluster_at_the_default_parameters():
    from mc_water_ls_mw_amd import lattice as lat
    from mc_water_ls_mw_amd import nucleation as nu
    assert (nu.RC_ANG_DEFAULT, nu.THRESHOLD_DEFAULT, nu.MIN_CONN_DEFAULT) == (nuc_ref.RC_ANG, nuc_ref.THRESHOLD, nuc_ref.MIN_CONN)
    for kind in ("ih", "ic"):
        h, xyz = lat.ice_box(kind, (3, 2, 2))
        o = nuc_ref.order(h, xyz, nu.RC_ANG_DEFAULT * ANG_TO_BOHR, nu.THRESHOLD_DEFAULT, nu.MIN_CONN_DEFAULT)
        assert tuple(o["op"]) == (96, 1, 96, 1) and np.all(o["nn"][:, 0] == 4) and np.all(o["label"] == 1), kind
    doc = nu.__doc__
    assert "a choice" in doc


def test_seeded_box_keeps_its_distances_and_its_seed_is_found_again():
    from mc_water_ls_mw_amd import lattice as lat
    from mc_water_ls_mw_amd import nucleation as nu
    big_h, big = lat.ice_box("ih", (6, 4, 4), 0.7, seed=13)                  # 768 molecules, 26.7 Angstrom at its narrowest
    host_h, host = lat.ice_box("ih", nuc_ref.SEEDED["reps"], nuc_ref.SEEDED["sigma_ang"], seed=nuc_ref.SEEDED["seed"])
    rc = nuc_ref.RC_ANG * ANG_TO_BOHR
    for kind, radius in (("ic", 8.0), ("ih", 7.0)):
        # the host kept beyond the bond cutoff: no host molecule is an entry of a seed molecule, so the seed's order parameter is
        # that of the bare seed in an empty cell
        h, xyz, nseed = nu.seeded_box(big_h, big, kind, radius, d_min_ang=3.6)
        i, j, d = boo_ref.entries(h, xyz, 3.6 * ANG_TO_BOHR)
        r = np.sqrt((d * d).sum(axis=1))
        mixed = (i < nseed) != (j < nseed)
        assert nseed > 30 and len(xyz) < len(big) + nseed and not np.any(mixed)
        centre = 0.5 * h.sum(axis=0)
        assert np.all(np.linalg.norm(xyz[:nseed] - centre, axis=1) < radius * ANG_TO_BOHR)
        assert np.all(np.linalg.norm(nu._min_image(h, xyz[nseed:] - centre), axis=1) >= radius * ANG_TO_BOHR)
        bare = nuc_ref.order(np.eye(3) * 200.0, xyz[:nseed], rc, nuc_ref.THRESHOLD, nuc_ref.MIN_CONN)
        o = nuc_ref.order(h, xyz, rc, nuc_ref.THRESHOLD, nuc_ref.MIN_CONN)
        print(kind, "seed of", nseed, "in", len(xyz), ": bare", bare["op"], "in the host", o["op"])
        assert bare["op"][1] == 1 and bare["op"][2] >= 10                     # the seed alone: one cluster
        assert np.array_equal(o["label"][:nseed], bare["label"]) and np.array_equal(o["nn"][:nseed], bare["nn"])
        assert np.sum(o["label"] == bare["op"][3]) == bare["op"][2]           # and no host molecule joins it
    # the default d_min: no two molecules closer than it
    h, xyz, nseed = nu.seeded_box(host_h, host, "ic", 6.0)
    i, j, d = boo_ref.entries(h, xyz, 2.4 * ANG_TO_BOHR)
    assert not np.any((i < nseed) != (j < nseed)) and nseed == nuc_ref.seeded()[2]
    with pytest.raises(nu.MwError, match="fit"):
        nu.seeded_box(host_h, host, "ic", 30.0)


def test_rate_from_stages_and_the_binomial_error():
    from mc_water_ls_mw_amd import nucleation as nu
    assert nu.rate_from_stages(2.0e-6, (0.5, 0.25, 0.1)) == pytest.approx(2.5e-8, rel=1e-14)
    assert nu.rate_from_stages(3.0, ()) == 3.0
    assert nu.binomial_error(25, 100) == pytest.approx(math.sqrt(0.25 * 0.75 / 100.0), rel=1e-14)
    assert nu.binomial_error(0, 10) == 0.0 and nu.binomial_error(10, 10) == 0.0 and nu.binomial_error(0, 0) == 0.0
    lo, hi = nu._bounds(None, None, 3, 96)
    assert lo.tolist() == [-1, -1, -1] and hi.tolist() == [97, 97, 97] and lo.dtype == np.int32
    lo, hi = nu._bounds([1, 2, 3], 50, 3, 96)
    assert lo.tolist() == [1, 2, 3] and hi.tolist() == [50, 50, 50]
    with pytest.raises(nu.MwError, match="lam_lo"):
        nu._bounds([1, 2], 5, 3, 96)
    with pytest.raises(nu.MwError, match="lam_hi"):
        nu._bounds(1, 5.5, 3, 96)
