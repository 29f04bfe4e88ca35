"""CPU: the mirror of include/mw_coll.h (tests/coll_ref.py) against a second, brute-force formulation and against its own
long-double reference; deliberately broken mirrors miss the bars or change a count; the inputs of the GPU tests keep every
distance away from every bin edge and every squared displacement away from a^2; and the host helpers of
``mc_water_ls_mw_amd.collective`` give their closed forms."""
import numpy as np
import pytest

import coll_ref
import sk_ref
from coll_ref import LD, evaluate, evaluate_brute, make_input, reference, worst

pytestmark = pytest.mark.skipif(not sk_ref.have_extended_precision(), reason="no extended precision on this platform")


def _cases():
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.collective import coll_plan
    build.build_coll()
    return coll_ref.cases(coll_plan(16, 8))


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def _mirror(case, **kw):
    cells, frames, nvec, r_max = make_input(case)
    return evaluate(cells, frames, case.nlags, case.every, nvec, r_max, case.nbins, case.hist_lags, case.a, **kw)


def test_the_cases_cross_every_boundary_of_the_plan():
    from mc_water_ls_mw_amd.collective import coll_plan
    plan = coll_plan(16, 8)
    tile, lb = plan["pair_tile"], plan["lag_block"]
    assert (tile, lb) == (256, 64) and len(BY_NAME) == len(CASES)
    nw = {c.nwater for c in CASES}
    assert {1, 2, 63, 64, 65, tile - 1, tile, tile + 1, 1025, 8193} <= nw
    assert {c.nframes for c in CASES} >= {1, 2} and {c.nlags for c in CASES} >= {1, 2, lb - 1, lb, lb + 1}
    assert {c.M for c in CASES} >= {0, 1} and {c.nbins for c in CASES} >= {1, 4096}
    assert any(c.every == 3 for c in CASES) and any(c.every > c.nframes for c in CASES)
    assert any(c.rfrac < 0.5 for c in CASES) and any(0.5 < c.rfrac < 1.5 for c in CASES)
    assert BY_NAME["farm600"].nboxes == 600 and BY_NAME["farm600"].nwater == 8
    for name in ("nwater_1025", "nwater_8193"):
        assert BY_NAME[name].nframes == 2 and BY_NAME[name].M == 3
    signs = np.array(coll_ref.VECTORS)
    assert np.array_equal(signs[0], -signs[1]) and np.array_equal(signs[2], -signs[3])


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_no_term_of_a_case_is_near_an_edge_and_the_mirror_is_within_the_bars(case):
    ref = reference(case)
    assert ref["near_edges"] == 0 and ref["near_a2"] == 0, (case.name, ref["near_edges"], ref["near_a2"])
    if case.nwater > 2000:
        return                                                             # the reference alone; the mirror's tables would be large
    got = _mirror(case)
    rows = worst(got, ref)
    print(case.name, {k: "%.2e / %.2e (%.2f)" % v for k, v in rows.items()})
    assert all(v[2] <= 1.0 for v in rows.values()), rows
    for name in ("gd", "qsum", "q2sum"):
        assert np.array_equal(got[name], ref[name]), name
    if case.M:
        assert np.all(ref["bar_rho"] > 0.0) and np.all(ref["bar_fkt"] > 0.0)
        # the bars ask something: far below the size of what they bound
        assert np.all(ref["bar_rho"] < 1e-9 * case.nwater) and np.all(ref["bar_fkt"] < 1e-9 * case.nwater)
    for h, lag in enumerate(case.hist_lags):
        if case.rfrac > 1.0:
            assert np.all(ref["gd"][:, h].sum(axis=-1) > 0)


@pytest.mark.parametrize("name", ("nwater_2", "nwater_65", "nframes_1", "nframes_2", "every3", "every_far", "M1", "nbins_1", "nlags_block+1"))
def test_the_mirror_is_the_brute_force_formulation(name):
    case = BY_NAME[name]
    cells, frames, nvec, r_max = make_input(case)
    ref = reference(case)
    brute = evaluate_brute(cells, frames, case.nlags, case.every, nvec, r_max, case.nbins, case.hist_lags, case.a)
    rows = worst(brute, ref)
    assert all(v[2] <= 1.0 for v in rows.values()), rows
    for key in ("gd", "qsum", "q2sum"):
        assert np.array_equal(brute[key], ref[key]), key


@pytest.mark.parametrize("wrong", coll_ref.WRONG)
def test_a_broken_mirror_misses_a_bar_or_changes_a_count(wrong):
    case = BY_NAME["every3"]
    ref = reference(case)
    bad = _mirror(case, wrong=wrong)
    rows = worst(bad, ref)
    floats = any(v[2] > 1.0 for v in rows.values())
    counts = {k: not np.array_equal(bad[k], ref[k]) for k in ("gd", "qsum", "q2sum")}
    expected = dict(origin=("fkt", "gd", "qsum", "q2sum"), lag=("fkt", "gd", "qsum", "q2sum"), self=("gd",), images=("gd",), conj=("fkt",),
                    q2tile=("q2sum",))[wrong]
    for k in expected:
        assert (rows["fkt"][2] > 1.0) if k == "fkt" else counts[k], (wrong, k, rows)
    assert floats or any(counts.values())
    if wrong in ("self", "images", "q2tile"):
        assert not floats and not counts["qsum"]


def test_lag_zero_is_the_pair_histogram_of_every_origin_and_minus_n_is_the_conjugate():
    import rdf_ref
    case = BY_NAME["every3"]
    cells, frames, nvec, r_max = make_input(case)
    got = _mirror(case)
    h0 = case.hist_lags.index(0)
    for b in range(case.nboxes):
        total = np.zeros(case.nbins, dtype=np.int64)
        for t0 in coll_ref.origins(case.nframes, 0, case.every):
            hist, edge = rdf_ref.rdf_fast(cells[b], frames[t0, b], r_max, case.nbins)
            assert not edge[1:].any()
            total += hist
        assert np.array_equal(got["gd"][b, h0], total)
    ref = reference(case)
    assert np.array_equal(ref["fkt"][:, :, 0], np.conj(ref["fkt"][:, :, 1])) and np.array_equal(ref["rho"][:, :, 2], np.conj(ref["rho"][:, :, 3]))
    assert np.all(ref["qsum"][:, 0] == coll_ref.n_origins(case.nframes, 0, case.every) * case.nwater)


# ---- the host helpers ---------------------------------------------------------------------------------------------------------------
def test_a_frozen_trajectory_gives_unit_normalised_scattering_and_no_susceptibility():
    from mc_water_ls_mw_amd import collective
    case = BY_NAME["every3"]
    cells, frames, nvec, r_max = make_input(case)
    frozen = np.ascontiguousarray(np.broadcast_to(frames[:1], frames.shape))
    out = evaluate(cells, frozen, case.nlags, case.every, nvec, r_max, case.nbins, case.hist_lags, case.a)
    q = collective.wave_numbers(nvec, cells)
    edges = np.array([0.0, 0.5 * (q.min() + q.max()), q.max() * 1.01])
    q_mid, F, norm, count = collective.coherent_scattering(out["fkt"], nvec, cells, edges)
    assert F.shape == (case.nboxes, case.nlags, 2) and np.all(count.sum(axis=1) == case.M) and np.all(count > 0)
    assert np.allclose(norm, 1.0, rtol=0, atol=1e-12) and np.all(F[:, 0] > 0)
    o = coll_ref.n_origins(case.nframes, np.arange(case.nlags), case.every)
    assert np.array_equal(collective.n_origins(case.nframes, np.arange(case.nlags), case.every), o)
    mean, chi4 = collective.chi4_from_sums(out["qsum"], out["q2sum"], o, case.nwater)
    assert np.all(mean == 1.0) and np.all(chi4 == 0.0)
    tau = collective.relaxation_time(F.transpose(0, 2, 1), 2.0)
    assert np.all(np.isnan(tau))                                           # it never decays


def test_uniform_counts_give_unit_distinct_van_hove():
    from mc_water_ls_mw_amd import collective
    cells = np.array([np.diag([10.0, 11.0, 12.0]), np.diag([9.0, 9.0, 9.0])])
    nbins, r_max, n, o = 20, 4.0, 50, np.array([7, 3])
    edges = r_max * np.arange(nbins + 1) / nbins
    shell = 4.0 * np.pi / 3.0 * (edges[1:] ** 3 - edges[:-1] ** 3)
    vol = np.array([1320.0, 729.0])
    counts = o[None, :, None] * n * (n / vol)[:, None, None] * shell[None, None, :]
    r_mid, g = collective.distinct_van_hove_from_counts(counts, cells, n, r_max, o)
    assert np.allclose(g, 1.0, rtol=1e-13, atol=0) and np.allclose(r_mid, 0.5 * (edges[1:] + edges[:-1]))


def test_a_single_cosine_gives_the_dynamic_structure_factor_a_single_peak():
    from mc_water_ls_mw_amd import collective
    nl, dt, k0 = 65, 0.5, 9
    lags = np.arange(nl)
    F = np.cos(np.pi * k0 * lags / (nl - 1))
    omega, S = collective.dynamic_structure_factor(F, dt, window=None)
    assert omega.shape == S.shape == (nl,) and np.isclose(omega[k0], np.pi * k0 / ((nl - 1) * dt))
    assert np.argmax(S) == k0 and np.isclose(S[k0], 0.5 * (nl - 1) * dt / np.pi)
    rest = np.delete(S, k0)
    assert np.all(np.abs(rest) < 1e-12 * S[k0] + 1e-12)
    _, Sh = collective.dynamic_structure_factor(np.stack([F, F]), dt)
    assert Sh.shape == (2, nl) and np.argmax(Sh[0]) == k0 and np.array_equal(Sh[0], Sh[1])
    with pytest.raises(collective.MwError, match="window"):
        collective.dynamic_structure_factor(F, dt, window="boxcar")
    tau = collective.relaxation_time(np.exp(-lags / 10.0), 2.0)
    assert abs(float(tau) - 20.0) < 0.05                                   # (linear interpolation of an exponential)
