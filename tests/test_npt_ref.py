"""CPU: the preconditions of tests/test_gpu_npt.py and the bars it uses, measured again with the numpy mirror of tests/npt_ref.py
and held against the constants recorded there.  Every figure is printed before it is asserted."""
import math

import numpy as np
import pytest

import md_ref
import npt_ref
from forces_ref import strained
from md_ref import BAR_DT, BAR_STEPS
from quench_ref import BAR_CASES, load_case


def _held(measured, recorded, what):
    """The recorded constant is the measured value rounded to three figures: within 1 % of it."""
    print(what, "measured %.4e recorded %.4e" % (measured, recorded))
    assert abs(measured - recorded) <= 0.01 * abs(recorded), what


def _triclinic():
    """ic96 under a homogeneous shear and strain: a cell with three oblique angles."""
    h, xyz = load_case("ic96")
    return strained(h, xyz, np.array([[0.02, 0.08, 0.05], [0.0, -0.01, -0.06], [0.0, 0.0, 0.015]]))


# -- (a) the virial is the volume derivative of the energy --------------------------------------
@pytest.mark.parametrize("name", md_ref.TRAJECTORY_CASES + ("triclinic",))
def test_the_mirrors_virial_is_minus_three_v_de_dv(name):
    """Under x -> lam x, h -> lam h: V = lam^3 V0, so -3 V dE/dV = -dE/dlam at lam = 1.  Central differences at d and d / 2; the
    quotient at d / 2 carries a truncation error of a third of their difference (second order) and a rounding error of a few
    ulp of E over d: the bar is the whole difference plus 8 ulp of |E| over d."""
    h, xyz = _triclinic() if name == "triclinic" else load_case(name)
    if name == "triclinic":
        ang = [math.degrees(math.acos(h[i] @ h[j] / np.linalg.norm(h[i]) / np.linalg.norm(h[j]))) for i, j in ((0, 1), (0, 2), (1, 2))]
        assert all(abs(a - 90.0) > 2.0 for a in ang), ang
    e0, _, w = npt_ref.energy_forces_virial(h, xyz)

    def quotient(d):
        return (npt_ref.energy_forces_virial((1.0 + d) * h, (1.0 + d) * xyz)[0] - npt_ref.energy_forces_virial((1.0 - d) * h, (1.0 - d) * xyz)[0]) / (2.0 * d)

    d = 2e-5
    q1, q2 = quotient(d), quotient(d / 2.0)
    bar = abs(q1 - q2) + 8.0 * np.spacing(abs(e0)) / d
    print(name, "W %.12e  -dE/dlam %.12e  difference %.2e (bar %.2e)" % (w, -q2, abs(w + q2), bar))
    assert abs(w + q2) <= bar and bar < 1e-5 * max(abs(w), 1e-3)


# -- (b) the barostat's stationary law ---------------------------------------------------------------
def test_the_free_ensemble_has_the_mean_and_the_variance_of_its_law_and_the_recorded_bias():
    """N = 20 molecules without forces: p(V) ~ V^N exp(-pressure V / kT), <V> = (N + 1) kT / pressure, var V = (N + 1) (kT /
    pressure)^2.  The final volumes of FREE_BOXES boxes after 24 relaxation times; the same at half the cb (and twice the
    applications) for the Euler bias."""
    n, nb = npt_ref.FREE_N, npt_ref.FREE_BOXES
    assert npt_ref.FREE_APPLICATIONS * npt_ref.FREE_RATE >= 20.0
    assert npt_ref.MAX_DLNV >= 8.0 * math.sqrt(2.0 * npt_ref.FREE_RATE / (n + 1))        # cn / sqrt(V) at the mean volume
    va, refused_a = npt_ref.free_volumes(nb, npt_ref.FREE_CB, npt_ref.FREE_APPLICATIONS, 5)
    vb, refused_b = npt_ref.free_volumes(nb, npt_ref.FREE_CB / 2.0, 2 * npt_ref.FREE_APPLICATIONS, 6)
    assert not refused_a and not refused_b                                             # no box of the mirror freezes
    mean, var = (n + 1) * npt_ref.FREE_KT / npt_ref.FREE_PRESSURE, (n + 1) * (npt_ref.FREE_KT / npt_ref.FREE_PRESSURE) ** 2
    assert math.isclose(mean, npt_ref.FREE_VOLUME, rel_tol=1e-14)
    se_mean = math.sqrt(var / nb) / mean
    se_var = math.sqrt((2.0 + 6.0 / (n + 1)) / nb)            # a gamma law of shape N + 1: excess kurtosis 6 / (N + 1)
    for v, what in ((va, "cb"), (vb, "cb / 2")):
        dm, dv = v.mean() / mean - 1.0, v.var() / var - 1.0
        print(what, "mean %.3e (5 se %.3e + bias %.3e)  variance %.3e (5 se %.3e + bias %.3e)" % (dm, 5 * se_mean, npt_ref.FREE_BIAS, dv, 5 * se_var,
                                                                                                 npt_ref.FREE_VAR_BIAS))
        assert abs(dm) <= 5.0 * se_mean + npt_ref.FREE_BIAS
        assert abs(dv) <= 5.0 * se_var + npt_ref.FREE_VAR_BIAS
    _held((va.mean() - vb.mean()) / mean, npt_ref.FREE_HALVING_MEASURED, "the halving difference of the mean")
    _held((va.var() - vb.var()) / var, npt_ref.FREE_VAR_HALVING_MEASURED, "the halving difference of the variance")
    assert npt_ref.FREE_BIAS == 2.0 * abs(npt_ref.FREE_HALVING_MEASURED)


def test_the_second_virial_coefficient_of_the_pair_term_is_the_recorded_one():
    b2 = npt_ref.second_virial(npt_ref.FREE_KT)
    _held(b2, npt_ref.FREE_B2_MEASURED, "B2")
    assert abs(npt_ref.second_virial(npt_ref.FREE_KT, 400000) - b2) < 1e-6 * abs(b2)      # the rule has converged
    se = 1.0 / math.sqrt((npt_ref.FREE_N + 1) * 4096)
    print("N |B2| / V = %.2e against a tenth of the device test's standard error %.2e" % (npt_ref.FREE_N * abs(b2) / npt_ref.FREE_VOLUME, 0.1 * se))
    assert npt_ref.FREE_N * abs(b2) / npt_ref.FREE_VOLUME < 0.1 * se


# -- (c) the bars ----------------------------------------------------------------------------------
def test_the_spreads_under_force_noise_are_the_recorded_ones():
    pos, vel, cell, trace = 0.0, 0.0, 0.0, np.zeros(6)
    for name in md_ref.TRAJECTORY_CASES:
        for langevin in (False, True):
            for every in npt_ref.BAR_BARO:
                a, b = npt_ref.reference(name, langevin, every), npt_ref.reference(name, langevin, every, True)
                dp, dv, dc = (float(np.abs(a[k] - b[k]).max()) for k in ("pos", "vel", "cell"))
                dt = np.abs(a["trace"] - b["trace"]).max(axis=0)
                print(name, "langevin" if langevin else "deterministic", every, "pos %.2e vel %.2e cell %.2e trace %s" % (dp, dv, dc, " ".join("%.2e" % t for t in dt)))
                assert tuple(a["status"]) == (BAR_STEPS, 0) and abs(a["trace"][-1, 4] / a["trace"][0, 4] - 1.0) > 1e-4     # the cell moved
                if name in BAR_CASES:
                    pos, vel, cell, trace = max(pos, dp), max(vel, dv), max(cell, dc), np.maximum(trace, dt)
                else:                                                      # held to the bar, not part of it
                    assert dp <= npt_ref.POS_TOL and dv <= npt_ref.VEL_TOL and dc <= npt_ref.CELL_TOL and np.all(dt <= np.array(npt_ref.TRACE_TOL))
    _held(pos, npt_ref.POS_SPREAD_MEASURED, "positions")
    _held(vel, npt_ref.VEL_SPREAD_MEASURED, "velocities")
    _held(cell, npt_ref.CELL_SPREAD_MEASURED, "cells")
    for k in range(6):
        _held(trace[k], npt_ref.TRACE_SPREAD_MEASURED[k], "trace column %d" % k)
    assert npt_ref.POS_TOL == 10.0 * npt_ref.POS_SPREAD_MEASURED and npt_ref.VEL_TOL == 10.0 * npt_ref.VEL_SPREAD_MEASURED
    assert npt_ref.CELL_TOL == 10.0 * npt_ref.CELL_SPREAD_MEASURED and npt_ref.TRACE_TOL == tuple(10.0 * s for s in npt_ref.TRACE_SPREAD_MEASURED)


def test_the_spread_of_the_virial_is_the_recorded_one():
    worst = 0.0
    for name in npt_ref.POINT_CASES:
        if name == "ih1536_t012":
            continue                                                       # (the device test's; 1536 molecules are not part of the bar)
        w, wn = npt_ref.point(name)[2], npt_ref.point(name, True)[2]
        print(name, "W %.9e moved by %.2e" % (w, abs(w - wn)))
        if name in BAR_CASES:
            worst = max(worst, abs(w - wn))
        else:
            assert abs(w - wn) <= npt_ref.W_TOL
    _held(worst, npt_ref.W_SPREAD_MEASURED, "W")
    assert npt_ref.W_TOL == 10.0 * npt_ref.W_SPREAD_MEASURED


# -- the mirror itself --------------------------------------------------------------------------------
def test_without_the_barostat_the_mirror_is_md_refs():
    h, xyz = load_case("ih48_t020")
    kw = dict(kT=md_ref.BAR_KT, gamma=md_ref.BAR_GAMMA, seed=4, stream=9, vel=md_ref.bar_velocities("ih48_t020"))
    a, b = npt_ref.run(h, xyz, 6, BAR_DT, baro_every=0, **kw), md_ref.run(h, xyz, 6, BAR_DT, **kw)
    assert np.array_equal(a["pos"], b["pos"]) and np.array_equal(a["vel"], b["vel"]) and np.array_equal(a["trace"][:, :4], b["trace"])
    assert np.array_equal(a["cell"], h) and np.array_equal(a["ref"], xyz)


def test_a_run_of_the_mirror_equals_its_halves_on_and_off_a_barostat_step():
    name = "ih48_t020"
    h, xyz = load_case(name)
    kw = dict(vel=None, **npt_ref.bar_kwargs(True, 5))
    kw.update(stream=9)
    v0 = md_ref.bar_velocities(name)
    whole = npt_ref.run(h, xyz, 12, BAR_DT, step0=48, **dict(kw, vel=v0))
    for k in (2, 5):                                                       # steps 48, 49 | ...: the chain point on (49: (49 + 1) % 5 == 0) and off a barostat step
        a = npt_ref.run(h, xyz, k, BAR_DT, step0=48, **dict(kw, vel=v0))
        b = npt_ref.run(a["cell"], a["pos"], 12 - k, BAR_DT, step0=48 + k, pos_ref=a["ref"], **dict(kw, vel=a["vel"]))
        for key in ("pos", "vel", "cell", "ref"):
            assert np.array_equal(b[key], whole[key]), (k, key)
        assert np.array_equal(b["trace"], whole["trace"][k:])


def test_the_mirrors_barostat_guard_freezes_a_box_before_the_application():
    h, xyz = load_case("ic48_t015")
    r = npt_ref.run(h, xyz, 6, BAR_DT, pressure=1.0, baro_every=2, sample_every=2, vel=md_ref.bar_velocities("ic48_t015"))      # |de| >> 0.3 at the first application
    assert tuple(r["status"]) == (2, 2) and np.array_equal(r["cell"], h) and np.array_equal(r["ref"], xyz)
    assert np.all(r["trace"][1:] == r["trace"][1]) and not np.array_equal(r["trace"][0], r["trace"][1])
    free = md_ref.run(h, xyz, 2, BAR_DT, vel=md_ref.bar_velocities("ic48_t015"))
    assert np.array_equal(r["pos"], free["pos"]) and np.array_equal(r["vel"], free["vel"])
    # a cell just above the rule, under pressure: refused at the first application, when its width would fall below a sigma (1 + 1e-9)
    for n in (4, 65):
        h, xyz = npt_ref.narrow_gas(n)
        assert npt_ref.cell_ok(h)
        e, f, w = npt_ref.energy_forces_virial(h, xyz)
        assert e == 0.0 and w == 0.0 and not f.any()
        r = npt_ref.run(h, xyz, 10, BAR_DT, pressure=100.0 * npt_ref.ATM, baro_every=3, step0=1)
        assert tuple(r["status"]) == (2, 2) and np.array_equal(r["cell"], h) and np.array_equal(r["pos"], xyz)


def test_the_grid_edge_boxes_cross_their_multiples_within_the_run():
    """The boxes of the device's grid-edge test: the mirror's width crosses the multiple of a sigma (1 + 1e-9) it starts next to."""
    for (axis, multiple, margin, pressure), crosses in zip(npt_ref.EDGE_CASES, (-1, 1)):
        h, xyz = npt_ref.at_a_grid_edge("ic96", axis, multiple, margin)
        r = npt_ref.edge_reference(axis, multiple, margin, pressure)
        u0, u1 = (npt_ref.widths(c)[axis] / (npt_ref.A_SIGMA * npt_ref.GUARD) for c in (h, r["cell"]))
        print("axis", axis, "width / (a sigma (1 + 1e-9)): %.5f -> %.5f" % (u0, u1), "status", r["status"])
        assert tuple(r["status"]) == (BAR_STEPS, 0)
        assert (u0 > multiple > u1) if crosses < 0 else (u0 < multiple < u1)


def test_the_barostats_normal_comes_from_a_counter_no_molecule_has():
    xi = np.array([npt_ref.box_normal(5, s, t) for s in range(40) for t in range(50)])
    print("mean %.4f variance %.4f" % (xi.mean(), xi.var()))
    assert abs(xi.mean()) < 5.0 / math.sqrt(xi.size) and abs(xi.var() - 1.0) < 5.0 * math.sqrt(2.0 / xi.size)
    w = md_ref.philox4x32_10(7, 0, 0xFFFFFFFF, 1, 5, 0)
    assert not np.array_equal(np.array(w), np.array(md_ref.philox4x32_10(7, 0, 0xFFFFFFFF, 0, 5, 0)))
    assert (1 << 22) <= 0xFFFFFFFF                                          # molecule indices end below 2^22


def test_the_smoke_runs_spreads_are_the_recorded_ones():
    a, b = npt_ref.smoke_reference(), npt_ref.smoke_reference(True)
    assert tuple(a["status"]) == (npt_ref.SMOKE_STEPS, 0) and a["trace"].shape == (npt_ref.SMOKE_STEPS // npt_ref.SMOKE_EVERY + 1, 6)
    v = a["trace"][:, 4]
    print("V from %.1f to %.1f bohr^3" % (v.min(), v.max()))
    assert v.max() - v.min() > 1e-3 * v[0]                                 # the cell breathes
    _held(float(np.abs(v - b["trace"][:, 4]).max()), npt_ref.SMOKE_V_SPREAD_MEASURED, "V")
    _held(float(np.abs(npt_ref.enthalpy(a["trace"]) - npt_ref.enthalpy(b["trace"])).max()), npt_ref.SMOKE_H_SPREAD_MEASURED, "E + K + pressure V")
    assert npt_ref.SMOKE_V_TOL == 10.0 * npt_ref.SMOKE_V_SPREAD_MEASURED and npt_ref.SMOKE_H_TOL == 10.0 * npt_ref.SMOKE_H_SPREAD_MEASURED
