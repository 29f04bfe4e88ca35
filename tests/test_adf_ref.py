"""CPU: the long-double reference of the angle histograms (tests/adf_ref.py) against a known answer and against itself along
its two walks, the preconditions of the exact comparisons of tests/test_gpu_adf.py for every input that file uses, and the
host arithmetic of mc_water_ls_mw_amd.angles (adf_edges, adf_from_counts)."""
import numpy as np
import pytest

from adf_ref import (ANG_TO_BOHR, BATCHES, EDGE_SETS, MARGIN, adf_exact, batch_radius, cap_radius, cases, cell_grid, edges_cos,
                     edges_theta, load_case, preconditions)
from boo_ref import batch_set, gas_box

CASES = cases()
#: (molecules, seed) of the cap boxes of tests/test_gpu_adf.py: three of the small geometry, three of the general
CAP_BOXES = ((40, 2040), (56, 2056), (64, 2064), (65, 2065), (100, 2100), (130, 2130))


def test_ideal_cubic_ice_puts_every_pair_in_the_tetrahedral_bin():
    from mc_water_ls_mw_amd import lattice as lat
    from mc_water_ls_mw_amd.angles import adf_edges
    e = adf_edges(97, "cos")
    m = int(np.searchsorted(e, -1.0 / 3.0, side="right") - 1)
    assert e[m] < -1.0 / 3.0 < e[m + 1]
    for reps in ((2, 2, 2), (2, 2, 3), (3, 3, 3)):                          # 64 molecules: the small walk; 96 and 216: the grid walk
        h, xyz = lat.ice_box("ic", reps, 0.0, seed=1)
        n = len(xyz)
        ref = adf_exact(h, xyz, 3.5 * ANG_TO_BOHR, e)
        assert np.all(ref["counts"] == 4)
        want = np.zeros(97, dtype=np.int64)
        want[m] = 6 * n
        assert np.array_equal(ref["hist"][0], want) and ref["summary"].tolist() == [[n, 6 * n, 6 * n, 0]], reps
        assert min(preconditions(ref)) > MARGIN


def test_the_two_walks_agree_below_the_cap_and_differ_above_it():
    """Below the cap the walk order is immaterial: the small walk and the grid walk (any grid) give the same integers.  Above it
    the first 32 of the walk are not the 32 nearest."""
    e = EDGE_SETS["theta90"]
    h, xyz = gas_box(63, 1063)
    rc = 3.5 * ANG_TO_BOHR
    a = adf_exact(h, xyz, rc, e)
    for grid in (cell_grid(h, rc, 63), (1, 1, 1), (2, 1, 2)):
        b = adf_exact(h, xyz, rc, e, grid=grid)
        assert a["max_count"] <= 32 and all(np.array_equal(a[k], b[k]) for k in ("hist", "counts", "summary")), grid
    rc = cap_radius(h, xyz, 36)
    a, b, c = adf_exact(h, xyz, rc, e), adf_exact(h, xyz, rc, e, grid=cell_grid(h, rc, 63)), adf_exact(h, xyz, rc, e, keep="nearest")
    assert a["max_count"] == 36 and np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["summary"], b["summary"])
    assert a["summary"][0, 3] >= 1 and a["summary"][0, 1] == a["summary"][0, 2] == a["hist"].sum()
    assert not np.array_equal(a["hist"], b["hist"]) and not np.array_equal(a["hist"], c["hist"])


def test_groups_split_the_histogram():
    e = EDGE_SETS["cos97"]
    h, xyz, rc = load_case(next(c for c in CASES if c[0] == "ih48_t020 4.8"))
    rng = np.random.default_rng(5)
    group = rng.integers(-1, 3, len(xyz))
    whole = adf_exact(h, xyz, rc, e)
    parts = adf_exact(h, xyz, rc, e, group=group, ngroups=3)
    every = adf_exact(h, xyz, rc, e, group=np.where(group < 0, 2, group), ngroups=3)
    assert np.array_equal(parts["counts"], whole["counts"]) and np.array_equal(every["hist"].sum(axis=0), whole["hist"][0])
    assert np.array_equal(every["hist"][:2], parts["hist"][:2]) and parts["summary"][:, 0].tolist() == [int((group == g).sum()) for g in range(3)]
    narrow = adf_exact(h, xyz, rc, np.array([-0.6, -0.2, 0.2]))
    assert 0 < narrow["summary"][0, 2] < narrow["summary"][0, 1] == whole["summary"][0, 1]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_preconditions_of_every_gpu_case(case):
    h, xyz, rc = load_case(case)
    for name in case[4]:
        ref = adf_exact(h, xyz, rc, EDGE_SETS[name])
        print(case[0], name, "gaps (r^2, c, order) %.2e %.2e %.2e" % preconditions(ref), "largest count", ref["max_count"])
        assert min(preconditions(ref)) > MARGIN, (case[0], name)
        if "one cell" in case[0]:                                          # the walk of a grid of one and two cells, over the cap
            assert ref["summary"][0, 3] >= 1 and np.isfinite(ref["gap_order"])
        else:
            assert ref["max_count"] <= 32                                   # (the cap has cases of its own)


@pytest.mark.parametrize("name,n", BATCHES)
def test_preconditions_of_every_batch(name, n):
    hs, xs = batch_set(name, n)
    rc = batch_radius(hs)
    for b in range(n):
        for es in EDGE_SETS.values():
            ref = adf_exact(hs[b], xs[b], rc, es)
            assert min(preconditions(ref)) > MARGIN, (name, b, preconditions(ref))


@pytest.mark.parametrize("n,seed", CAP_BOXES)
def test_preconditions_of_the_cap_boxes(n, seed):
    """The radii at which the largest count is 31, 32 and 33: found, apart, and clear of every r^2, edge and cell wall."""
    h, xyz = gas_box(n, seed)
    for want in (31, 32, 33):
        rc = cap_radius(h, xyz, want)
        assert rc is not None, (n, want)
        ref = adf_exact(h, xyz, rc, EDGE_SETS["cos97"])
        print(n, want, "r_cut %.6f bohr" % rc, "gaps %.2e %.2e %.2e" % preconditions(ref), "capped", ref["summary"][0, 3])
        assert ref["max_count"] == want and min(preconditions(ref)) > MARGIN
        assert (ref["summary"][0, 3] >= 1) == (want == 33)


def test_adf_edges_and_adf_from_counts():
    from mc_water_ls_mw_amd.angles import MwError, adf_edges, adf_from_counts
    for nbins in (1, 2, 90, 97, 1024):
        for kind, mine in (("theta", edges_theta), ("cos", edges_cos)):
            e = adf_edges(nbins, kind)
            assert e.shape == (nbins + 1,) and e.dtype == np.float64 and np.all(np.diff(e) > 0) and e[0] == -1.0 and e[-1] == 1.0
            assert np.array_equal(e, mine(nbins))
    assert np.allclose(np.degrees(np.arccos(adf_edges(90, "theta"))), 180.0 - 2.0 * np.arange(91), atol=1e-10)
    assert np.array_equal(adf_edges(4, "cos"), [-1.0, -0.5, 0.0, 0.5, 1.0])
    with pytest.raises(MwError):
        adf_edges(0)
    with pytest.raises(MwError):
        adf_edges(10, "degrees")
    e = adf_edges(90, "theta")
    rng = np.random.default_rng(2)
    hist = rng.integers(0, 1000, (3, 2, 90))
    hist[1, 1] = 0
    theta, p_theta, cos_mid, p_cos = adf_from_counts(hist, e)
    assert theta.shape == cos_mid.shape == (90,) and p_theta.shape == p_cos.shape == (3, 2, 90)
    assert np.allclose(theta, 179.0 - 2.0 * np.arange(90)) and np.all(np.diff(cos_mid) > 0)
    norm_theta, norm_cos = (p_theta * 2.0).sum(axis=-1), (p_cos * np.diff(e)).sum(axis=-1)
    filled = hist.sum(axis=-1) > 0
    assert np.allclose(norm_theta[filled], 1.0, rtol=1e-12) and np.allclose(norm_cos[filled], 1.0, rtol=1e-12)
    assert np.all(p_theta[1, 1] == 0.0) and np.all(p_cos[1, 1] == 0.0) and np.all(np.isfinite(p_theta)) and np.all(np.isfinite(p_cos))
    one = adf_from_counts(hist[0, 0], e)
    assert np.array_equal(one[1], p_theta[0, 0])
    with pytest.raises(MwError):
        adf_from_counts(hist, e[:-1])
