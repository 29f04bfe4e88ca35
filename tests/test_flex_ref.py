"""CPU: the preconditions of tests/test_gpu_flex.py and the bars it uses, measured again with the numpy mirror of
tests/flex_ref.py and held against the constants recorded there.  Every figure is printed before it is asserted."""
import math

import numpy as np
import pytest

import flex_ref
import md_ref
import npt_ref
from forces_ref import strained
from md_ref import BAR_DT, BAR_STEPS
from quench_ref import BAR_CASES, load_case
from test_npt_ref import _held, _triclinic


# -- (a) the virial tensor is the strain derivative of the energy ------------------------------------
@pytest.mark.parametrize("name", md_ref.TRAJECTORY_CASES + ("triclinic",))
def test_the_mirrors_stress_is_minus_the_strain_derivative_of_the_energy(name):
    """Under x -> (I + eta) x, h -> (I + eta) h: dE = -sum W_ab d eta_ab.  A stretch of axis a (eta_aa = d) gives W_aa, the
    symmetric shear eta_ab = eta_ba = d / 2 gives W_ab.  Central differences at d and d / 2.  The quotient at d / 2 carries a
    truncation error of a third of the difference of the two (second order) and the rounding error of two energies over d: E is a
    sum over the n molecules, each addition rounds by up to half an ulp of |E|, and with six quotients per box the rounding term is
    taken at its bound, max(n, 8) ulp of |E| over d, where tests/test_npt_ref.py takes 8 for its single quotient.  The bar is the
    whole difference plus that.  ic64_sheared, ic65_interstitial and the triclinic box have shears of W that are not zero."""
    h, xyz = _triclinic() if name == "triclinic" else load_case(name)
    e0, _, w = flex_ref.energy_forces_stress(h, xyz)
    assert np.allclose(w, w.T, rtol=0, atol=1e-12 * max(1.0, np.abs(w).max()))
    if name in ("ic64_sheared", "triclinic"):
        assert min(abs(w[0, 1]), abs(w[0, 2]), abs(w[1, 2])) > 1e-6, w

    def quotient(a, b, d):
        eta = np.zeros((3, 3))
        eta[a, b] += d / 2.0
        eta[b, a] += d / 2.0
        ep = flex_ref.energy_forces_stress(*strained(h, xyz, eta))[0]
        em = flex_ref.energy_forces_stress(*strained(h, xyz, -eta))[0]
        return (ep - em) / (2.0 * d)

    d = 2e-5
    for a, b in flex_ref.PAIRS:
        q1, q2 = quotient(a, b, d), quotient(a, b, d / 2.0)
        bar = abs(q1 - q2) + max(len(xyz), 8) * np.spacing(abs(e0)) / d
        print(name, "W_%d%d %.12e  -dE/d eta %.12e  difference %.2e (bar %.2e)" % (a, b, w[a, b], -q2, abs(w[a, b] + q2), bar))
        assert abs(w[a, b] + q2) <= bar and bar < 1e-5 * max(np.abs(w).max(), 1e-3)


@pytest.mark.parametrize("name", npt_ref.POINT_CASES[:-1])
def test_the_trace_of_the_tensor_is_npt_refs_virial(name):
    h, xyz = load_case(name)
    e, f, w = flex_ref.energy_forces_stress(h, xyz)
    e2, f2, w2 = npt_ref.energy_forces_virial(h, xyz)
    assert e == e2 and np.array_equal(f, f2) and float(np.trace(w)) == w2
    r = flex_ref.run(h, xyz, 0, BAR_DT, vel=md_ref.maxwell_boltzmann(1, len(xyz), md_ref.BAR_KT, seed=3)[0])
    t = r["trace"][0]
    assert t.shape == (15,) and abs(t[6] + t[7] + t[8] - 3.0 * t[5]) <= 1e-14 * np.abs(t[6:9]).max() + 4.0 * np.spacing(abs(t[5]))
    assert np.allclose(t[12:], np.linalg.norm(h, axis=1), rtol=1e-15)


# -- (b) the barostat's stationary law ---------------------------------------------------------------
@pytest.mark.parametrize("coupling", (flex_ref.ANISO, flex_ref.SEMI, flex_ref.UNIAXIAL), ids=("aniso", "semi", "uniaxial"))
def test_the_free_ensemble_has_the_mean_and_the_variance_of_its_law_in_every_coupling(coupling):
    """N = 20 molecules without forces: p(V) ~ V^N exp(-pressure V / kT) whatever the groups are.  The final volumes of
    FREE_BOXES boxes after 4 relaxation times from the mean volume; the same at half the cb (and twice the applications) for the
    Euler bias.  No box of the mirror freezes, and the freely diffusing shapes stay above twice the cutoff: the device test's boxes
    keep a grid of at least two cells each way."""
    n, nb, apps = flex_ref.FREE_N, flex_ref.FREE_BOXES, flex_ref.FREE_APPLICATIONS[coupling]
    rate = flex_ref.FREE_RATE / (3.0 if coupling == flex_ref.UNIAXIAL else 1.0)          # of ln V per application
    assert apps * rate >= 4.0
    assert flex_ref.MAX_DLNL >= 7.5 * math.sqrt(2.0 * flex_ref.FREE_RATE / (3.0 * (n + 1)))      # cn_1 / sqrt(V) at the mean volume
    la, small_a, refused_a = flex_ref.free_lengths(nb, flex_ref.FREE_CB, apps, 5, coupling)
    lb, small_b, refused_b = flex_ref.free_lengths(nb, flex_ref.FREE_CB / 2.0, 2 * apps, 6, coupling)
    assert not refused_a and not refused_b
    print("smallest length %.1f and %.1f bohr against twice the cutoff %.1f" % (small_a, small_b, 2.0 * npt_ref.A_SIGMA))
    assert min(small_a, small_b) > 2.0 * npt_ref.A_SIGMA * npt_ref.GUARD
    va, vb = la.prod(axis=1), lb.prod(axis=1)
    mean, var = (n + 1) * flex_ref.FREE_KT / flex_ref.FREE_PRESSURE, (n + 1) * (flex_ref.FREE_KT / flex_ref.FREE_PRESSURE) ** 2
    assert math.isclose(mean, flex_ref.FREE_VOLUME, rel_tol=1e-14) and math.isclose(flex_ref.FREE_SIDE ** 3, mean, rel_tol=1e-14)
    se_mean = math.sqrt(var / nb) / mean
    se_var = math.sqrt((2.0 + 6.0 / (n + 1)) / nb)            # a gamma law of shape N + 1: excess kurtosis 6 / (N + 1)
    for v, what in ((va, "cb"), (vb, "cb / 2")):
        dm, dv = v.mean() / mean - 1.0, v.var() / var - 1.0
        print(what, "mean %.3e (5 se %.3e + bias %.3e)  variance %.3e (5 se %.3e + bias %.3e)" % (dm, 5 * se_mean, flex_ref.FREE_BIAS[coupling], dv, 5 * se_var,
                                                                                                 flex_ref.FREE_VAR_BIAS[coupling]))
        assert abs(dm) <= 5.0 * se_mean + flex_ref.FREE_BIAS[coupling]
        assert abs(dv) <= 5.0 * se_var + flex_ref.FREE_VAR_BIAS[coupling]
    _held((va.mean() - vb.mean()) / mean, flex_ref.FREE_HALVING_MEASURED[coupling], "the halving difference of the mean")
    _held((va.var() - vb.var()) / var, flex_ref.FREE_VAR_HALVING_MEASURED[coupling], "the halving difference of the variance")
    assert flex_ref.FREE_BIAS[coupling] == 2.0 * abs(flex_ref.FREE_HALVING_MEASURED[coupling])
    # the shapes: an axis that no group holds keeps its length, the others have moved apart
    spread = np.log(la).std(axis=0)
    print("spread of ln L per axis", spread)
    if coupling == flex_ref.UNIAXIAL:
        assert np.all(la[:, :2] == flex_ref.FREE_SIDE) and spread[2] > 0.1
    else:
        assert np.all(spread > 0.1)
    if coupling == flex_ref.SEMI:
        assert np.array_equal(la[:, 0], la[:, 1])                          # one factor for the pair


# -- (c) the bars ----------------------------------------------------------------------------------
def test_the_spreads_under_force_noise_are_the_recorded_ones():
    pos, vel, cell, trace = 0.0, 0.0, 0.0, np.zeros(15)
    for name in md_ref.TRAJECTORY_CASES:
        for coupling, axis in flex_ref.BAR_COUPLINGS + (flex_ref.EXTRA_COUPLING,):
            for langevin in (False, True):
                for every in npt_ref.BAR_BARO:
                    a, b = flex_ref.reference(name, langevin, every, coupling, axis), flex_ref.reference(name, langevin, every, coupling, axis, True)
                    dp, dv, dc = (float(np.abs(a[k] - b[k]).max()) for k in ("pos", "vel", "cell"))
                    dt = np.abs(a["trace"] - b["trace"]).max(axis=0)
                    print(name, coupling, axis, "langevin" if langevin else "deterministic", every,
                          "pos %.2e vel %.2e cell %.2e trace %s" % (dp, dv, dc, " ".join("%.2e" % t for t in dt)))
                    assert tuple(a["status"]) == (BAR_STEPS, 0) and abs(a["trace"][-1, 4] / a["trace"][0, 4] - 1.0) > 1e-5     # the cell moved
                    if name in BAR_CASES and (coupling, axis) in flex_ref.BAR_COUPLINGS:
                        pos, vel, cell, trace = max(pos, dp), max(vel, dv), max(cell, dc), np.maximum(trace, dt)
                    else:                                                  # held to the bar, not part of it
                        assert dp <= flex_ref.POS_TOL and dv <= flex_ref.VEL_TOL and dc <= flex_ref.CELL_TOL and np.all(dt <= np.array(flex_ref.TRACE_TOL))
    _held(pos, flex_ref.POS_SPREAD_MEASURED, "positions")
    _held(vel, flex_ref.VEL_SPREAD_MEASURED, "velocities")
    _held(cell, flex_ref.CELL_SPREAD_MEASURED, "cells")
    for k in range(15):
        _held(trace[k], flex_ref.TRACE_SPREAD_MEASURED[k], "trace column %d" % k)
    assert flex_ref.POS_TOL == 10.0 * flex_ref.POS_SPREAD_MEASURED and flex_ref.VEL_TOL == 10.0 * flex_ref.VEL_SPREAD_MEASURED
    assert flex_ref.CELL_TOL == 10.0 * flex_ref.CELL_SPREAD_MEASURED and flex_ref.TRACE_TOL == tuple(10.0 * s for s in flex_ref.TRACE_SPREAD_MEASURED)


def test_the_spread_of_the_virial_tensor_is_the_recorded_one():
    worst = 0.0
    for name in npt_ref.POINT_CASES:
        if name == "ih1536_t012":
            continue                                                       # (the device test's; 1536 molecules are not part of the bar)
        w, wn = flex_ref.point(name)[2], flex_ref.point(name, True)[2]
        d = float(np.abs(w - wn).max())
        print(name, "largest |W_ab| %.9e moved by %.2e" % (np.abs(w).max(), d))
        if name in BAR_CASES:
            worst = max(worst, d)
        else:
            assert d <= flex_ref.W_AB_TOL
    _held(worst, flex_ref.W_AB_SPREAD_MEASURED, "W_ab")
    assert flex_ref.W_AB_TOL == 10.0 * flex_ref.W_AB_SPREAD_MEASURED


# -- the mirror itself --------------------------------------------------------------------------------
def test_in_coupling_0_and_without_the_barostat_the_mirror_is_npt_refs():
    h, xyz = load_case("ic64_sheared")
    kw = dict(vel=md_ref.bar_velocities("ic64_sheared"), stream=9, **npt_ref.bar_kwargs(True, 5))
    a, b = flex_ref.run(h, xyz, 12, BAR_DT, coupling=flex_ref.ISO, axis=1, **kw), npt_ref.run(h, xyz, 12, BAR_DT, **kw)
    for key in ("pos", "vel", "cell", "ref", "status"):
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(a["trace"][:, :5], b["trace"][:, :5]) and np.allclose(a["trace"][:, 5], b["trace"][:, 5], rtol=1e-13)
    kw["baro_every"] = 0
    for coupling in (1, 2, 3):
        a = flex_ref.run(h, xyz, 6, BAR_DT, coupling=coupling, **kw)
        b = md_ref.run(h, xyz, 6, BAR_DT, md_ref.BAR_KT, md_ref.BAR_GAMMA, vel=kw["vel"], seed=kw["seed"], stream=9)
        assert np.array_equal(a["pos"], b["pos"]) and np.array_equal(a["vel"], b["vel"]) and np.array_equal(a["trace"][:, :4], b["trace"])
        assert np.array_equal(a["cell"], h) and np.array_equal(a["ref"], xyz)


@pytest.mark.parametrize("coupling,axis", flex_ref.BAR_COUPLINGS + (flex_ref.EXTRA_COUPLING,))
def test_a_run_of_the_mirror_equals_its_halves_on_and_off_a_barostat_step(coupling, axis):
    name = "ih48_t020"
    h, xyz = load_case(name)
    kw = dict(stream=9, coupling=coupling, axis=axis, **npt_ref.bar_kwargs(True, 5))
    v0 = md_ref.bar_velocities(name)
    whole = flex_ref.run(h, xyz, 12, BAR_DT, step0=48, vel=v0, **kw)
    assert not np.array_equal(whole["cell"], h)
    for k in (2, 5):                                                       # the chain point on (step 49: (49 + 1) % 5 == 0) and off a barostat step
        a = flex_ref.run(h, xyz, k, BAR_DT, step0=48, vel=v0, **kw)
        b = flex_ref.run(a["cell"], a["pos"], 12 - k, BAR_DT, step0=48 + k, pos_ref=a["ref"], vel=a["vel"], **kw)
        for key in ("pos", "vel", "cell", "ref"):
            assert np.array_equal(b[key], whole[key]), (k, key)
        assert np.array_equal(b["trace"], whole["trace"][k:])
    # which columns of the cell an application moves
    moved = [not np.array_equal(whole["cell"][:, a], np.asarray(h)[:, a]) for a in range(3)]
    assert moved == ([a == axis for a in range(3)] if coupling == flex_ref.UNIAXIAL else [True, True, True])
    if coupling == flex_ref.SEMI:
        a, b = [k for k in range(3) if k != axis]
        assert math.isclose(whole["cell"][a, a] / h[a, a], whole["cell"][b, b] / h[b, b], rel_tol=1e-14)      # one factor for the pair


def test_the_groups_and_their_normals():
    assert flex_ref.groups(0, 1) == ((0, 1, 2),) and flex_ref.groups(1, 0) == ((0,), (1,), (2,))
    assert flex_ref.groups(2, 2) == ((0, 1), (2,)) and flex_ref.groups(2, 0) == ((1, 2), (0,)) and flex_ref.groups(2, 1) == ((0, 2), (1,))
    assert flex_ref.groups(3, 1) == ((1,),)
    # the fourth words 1 (isotropic), 2, 3 and 4 give different normals, and word 1 is npt_ref's
    xi = [flex_ref.group_normal(5, 7, 11, w) for w in (1, 2, 3, 4)]
    assert len(set(xi)) == 4 and xi[0] == npt_ref.box_normal(5, 7, 11)
    z = np.array([flex_ref.group_normal(5, s, t, 3) for s in range(40) for t in range(50)])
    print("mean %.4f variance %.4f" % (z.mean(), z.var()))
    assert abs(z.mean()) < 5.0 / math.sqrt(z.size) and abs(z.var() - 1.0) < 5.0 * math.sqrt(2.0 / z.size)
    cb, cn, cb3, cn1, cn2 = flex_ref.barostat_constants(BAR_DT, md_ref.BAR_KT, npt_ref.BAR_TAU_P, npt_ref.BAR_BETA_T, 5)
    assert cb3 == cb / 3.0 and math.isclose(cn1 * cn1 * 3.0, cn * cn, rel_tol=1e-15) and math.isclose(cn2 * cn2 * 2.0, cn1 * cn1, rel_tol=1e-15)


def test_the_mirrors_barostat_guard_freezes_a_box_before_the_application():
    h, xyz = load_case("ic48_t015")
    v0 = md_ref.bar_velocities("ic48_t015")
    for coupling in (1, 2, 3):
        r = flex_ref.run(h, xyz, 6, BAR_DT, pressure=1.0, baro_every=2, sample_every=2, vel=v0, coupling=coupling)      # |de_G| >> 0.1 at the first application
        assert tuple(r["status"]) == (2, 2) and np.array_equal(r["cell"], h) and np.array_equal(r["ref"], xyz)
        assert np.all(r["trace"][1:] == r["trace"][1]) and not np.array_equal(r["trace"][0], r["trace"][1])
        free = md_ref.run(h, xyz, 2, BAR_DT, vel=v0)
        assert np.array_equal(r["pos"], free["pos"]) and np.array_equal(r["vel"], free["vel"])
    # |de_G| between 0.1 and 0.3: the per-axis stage refuses what the isotropic one accepts
    stiff = dict(beta_T=300.0 * npt_ref.BAR_BETA_T, baro_every=4, vel=v0, pressure=npt_ref.ATM)
    r = flex_ref.run(h, xyz, 4, BAR_DT, coupling=1, **stiff)
    de = [abs((flex_ref.barostat_constants(BAR_DT, 0.0, npt_ref.BAR_TAU_P, stiff["beta_T"], 4)[2]) * (npt_ref.ATM - r["trace"][4, 6 + a])) for a in range(3)]
    print("|de| per axis", de)
    assert tuple(r["status"]) == (4, 2) and 1.2 * flex_ref.MAX_DLNL < max(de) < npt_ref.MAX_DLNV
    assert tuple(flex_ref.run(h, xyz, 4, BAR_DT, coupling=0, **stiff)["status"]) == (4, 0)
    # a cell just above the rule along x, under pressure: refused when x is in a group, untouched when it is not
    for n in (4, 65):
        h, xyz = npt_ref.narrow_gas(n)
        kw = dict(pressure=100.0 * npt_ref.ATM, baro_every=3, step0=1)
        assert tuple(flex_ref.run(h, xyz, 10, BAR_DT, coupling=1, **kw)["status"]) == (2, 2)
        assert tuple(flex_ref.run(h, xyz, 10, BAR_DT, coupling=3, axis=0, **kw)["status"]) == (2, 2)
        r = flex_ref.run(h, xyz, 10, BAR_DT, coupling=3, axis=2, **kw)
        assert tuple(r["status"]) == (10, 0) and np.array_equal(r["cell"][:, :2], h[:, :2]) and r["cell"][2, 2] < h[2, 2]


def test_the_grid_edge_boxes_cross_their_multiples_within_the_run():
    """The boxes of the device's grid-edge test: the mirror's width along the axis crosses the multiple of a sigma (1 + 1e-9) it
    starts next to, and the other two widths keep their number of cutoffs."""
    for (axis, multiple, margin, pressure), crosses in zip(flex_ref.EDGE_CASES, (-1, 1)):
        h, xyz = flex_ref.at_a_grid_edge("ic96", axis, multiple, margin)
        r = flex_ref.edge_reference(axis, multiple, margin, pressure)
        u0, u1 = (npt_ref.widths(c) / (npt_ref.A_SIGMA * npt_ref.GUARD) for c in (h, r["cell"]))
        print("axis", axis, "widths / (a sigma (1 + 1e-9)):", u0, "->", u1, "status", r["status"])
        assert tuple(r["status"]) == (BAR_STEPS, 0)
        assert (u0[axis] > multiple > u1[axis]) if crosses < 0 else (u0[axis] < multiple < u1[axis])
        others = [k for k in range(3) if k != axis]
        assert np.array_equal(np.floor(u0[others]), np.floor(u1[others])) and np.array_equal(r["cell"][:, others], h[:, others])
