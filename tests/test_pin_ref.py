"""CPU: the preconditions of tests/test_gpu_pin.py and the bars it uses, measured again with the numpy mirror of tests/pin_ref.py
and held against the constants recorded there.  Every figure is printed before it is asserted."""
import math

import numpy as np
import pytest

import flex_ref
import md_ref
import pin_ref
import sk_ref
from md_ref import BAR_DT, BAR_STEPS
from quench_ref import BAR_CASES, load_case
from test_npt_ref import _held

EPS = 2.0 ** -52
#: (case, skew) of every biased box the device test holds to the mirror
DEVICE_CASES = (("ih48_t020", False), ("ic96", False), ("ic64_sheared", False), ("ic64_sheared", True), ("ic65_interstitial", False))


# -- (a) the bars ------------------------------------------------------------------------------------
def test_the_spreads_under_force_noise_are_the_recorded_ones():
    pos, vel, cell, trace, blocks = 0.0, 0.0, 0.0, np.zeros(17), np.zeros(4)
    for name, skew in tuple((n, False) for n in BAR_CASES) + DEVICE_CASES[3:]:
        for coupling, axis, every in pin_ref.BAR_RUNS:
            for langevin in (False, True):
                a = pin_ref.reference(name, langevin, every, coupling, axis, True, False, skew)
                b = pin_ref.reference(name, langevin, every, coupling, axis, True, True, skew)
                dp, dv, dc = (float(np.abs(a[k] - b[k]).max()) for k in ("pos", "vel", "cell"))
                dt, db = np.abs(a["trace"] - b["trace"]).max(axis=0), np.abs(a["blocks"] - b["blocks"]).max(axis=0)
                print(name, skew, coupling, every, "langevin" if langevin else "deterministic",
                      "pos %.2e vel %.2e cell %.2e trace %s blocks %s" % (dp, dv, dc, " ".join("%.2e" % t for t in dt), " ".join("%.2e" % t for t in db)))
                assert tuple(a["status"]) == (BAR_STEPS, 0) and a["blocks"].shape == (4, 4) and abs(a["trace"][-1, 4] / a["trace"][0, 4] - 1.0) > 1e-6
                if name in BAR_CASES and not skew:
                    pos, vel, cell, trace, blocks = max(pos, dp), max(vel, dv), max(cell, dc), np.maximum(trace, dt), np.maximum(blocks, db)
                else:                                                      # held to the bar, not part of it
                    assert dp <= pin_ref.POS_TOL and dv <= pin_ref.VEL_TOL and dc <= pin_ref.CELL_TOL
                    assert np.all(dt <= np.array(pin_ref.TRACE_TOL)) and np.all(db <= np.array(pin_ref.BLOCK_TOL))
    _held(pos, pin_ref.POS_SPREAD_MEASURED, "positions")
    _held(vel, pin_ref.VEL_SPREAD_MEASURED, "velocities")
    _held(cell, pin_ref.CELL_SPREAD_MEASURED, "cells")
    for k in range(17):
        _held(trace[k], pin_ref.TRACE_SPREAD_MEASURED[k], "trace column %d" % k)
    for k in range(4):
        _held(blocks[k], pin_ref.BLOCK_SPREAD_MEASURED[k], "block field %d" % k)
    assert pin_ref.POS_TOL == 10.0 * pin_ref.POS_SPREAD_MEASURED and pin_ref.TRACE_TOL[15] == 10.0 * pin_ref.TRACE_SPREAD_MEASURED[15]


# -- (b) the bias is what the header says ----------------------------------------------------------------
@pytest.mark.parametrize("name,skew", DEVICE_CASES)
def test_the_force_of_the_bias_is_minus_the_gradient_of_its_energy_and_sums_to_zero(name, skew):
    """Central differences of the mirror's U_b at d and d / 2 along every Cartesian direction of six molecules.  The quotient at
    d / 2 carries a truncation error of a third of the difference of the two (second order) and the rounding of two energies over d:
    rho is a sum of N phasors (N ulp), Q - a = -0.25 a loses a factor 5 to cancellation and is squared, so U_b rounds by up to
    32 N eps (1/2 kappa Q^2); the bar is the whole difference of the two quotients plus that over d / 2.  d = 1e-3 bohr: the
    phase moves by k d = 1e-3, the truncation term (k d)^2 / 6 relative is 2e-7."""
    h, xyz = load_case(name)
    nvec, kappa, anchor, q0 = pin_ref.bias_case(name, skew)
    n = len(xyz)
    q, u, fb = pin_ref.bias(h, xyz, nvec, kappa, anchor)
    assert q == q0 and math.isclose(u, 0.5 * kappa * (0.2 * q0) ** 2, rel_tol=1e-12)
    total = np.abs(fb.sum(axis=0)).max()
    print(name, nvec, "max |F_b| %.3e  |sum F_b| %.2e (bar %.2e)" % (np.abs(fb).max(), total, 4.0 * n * EPS * np.abs(fb).max()))
    assert total <= 4.0 * n * EPS * np.abs(fb).max()

    def quotient(j, a, d):
        xp, xm = xyz.copy(), xyz.copy()
        xp[j, a] += d
        xm[j, a] -= d
        return (pin_ref.bias(h, xp, nvec, kappa, anchor)[1] - pin_ref.bias(h, xm, nvec, kappa, anchor)[1]) / (2.0 * d)

    d, worst = 1e-3, 0.0
    for j in (0, 1, n // 3, n // 2, n - 2, n - 1):
        for a in range(3):
            q1, q2 = quotient(j, a, d), quotient(j, a, d / 2.0)
            bar = abs(q1 - q2) + 32.0 * n * EPS * (0.5 * kappa * q * q) / (d / 2.0)
            worst = max(worst, abs(fb[j, a] + q2) / bar)
            assert abs(fb[j, a] + q2) <= bar and bar < 1e-4 * np.abs(fb).max(), (j, a, fb[j, a], -q2, bar)
    print(name, "largest |F_b + dU_b/dx| over its bar: %.2f" % worst)


@pytest.mark.parametrize("name,skew", DEVICE_CASES)
def test_the_bias_energy_does_not_change_under_any_scaling_of_the_barostat(name, skew):
    """The zero virial: h and x scaled together by every coupling's factors (and by a shear, which no coupling applies) leave s, so
    Q and U_b, where they were to rounding -- 32 N eps (1/2 kappa Q^2) as above, the phases being formed again from the scaled
    arrays -- while the force does change: k follows the cell."""
    h, xyz = load_case(name)
    nvec, kappa, anchor, _ = pin_ref.bias_case(name, skew)
    q, u, fb = pin_ref.bias(h, xyz, nvec, kappa, anchor)
    bar = 32.0 * len(xyz) * EPS * (0.5 * kappa * q * q)
    for coupling, axis in ((flex_ref.ISO, 2), (flex_ref.ANISO, 2), (flex_ref.SEMI, 2), (flex_ref.SEMI, 0), (flex_ref.UNIAXIAL, 2), (flex_ref.UNIAXIAL, 1)):
        mu = np.ones(3)
        for k, g in enumerate(flex_ref.groups(coupling, axis)):
            mu[list(g)] = 1.0 + 0.03 * (k + 1)
        q2, u2, fb2 = pin_ref.bias(h * mu[None, :], xyz * mu[None, :], nvec, kappa, anchor)
        print(name, coupling, axis, "U_b %.6e changes by %.2e (bar %.2e), F_b by %.2e" % (u, abs(u2 - u), bar, np.abs(fb2 - fb).max()))
        assert abs(u2 - u) <= bar and abs(q2 - q) <= 32.0 * len(xyz) * EPS * q
        assert np.allclose(fb2, fb / mu[None, :], rtol=1e-9, atol=1e-12 * np.abs(fb).max())
    a = np.eye(3) + np.array([[0.0, 0.02, -0.01], [0.0, 0.0, 0.03], [0.0, 0.0, 0.0]])
    assert abs(pin_ref.bias(h @ a, xyz @ a, nvec, kappa, anchor)[1] - u) <= bar


@pytest.mark.parametrize("name", ("ih48_t020", "ic96"))
def test_without_a_thermostat_the_total_energy_with_the_bias_is_conserved(name):
    """E_mW + K + U_b over the 40 steps at fixed cell.  The bar is three times the drift of the unbiased mirror on the same case:
    the bias adds a force whose largest component is the median of the mW ones, along a mode whose phases move by k v dt < 0.05
    per step, so it integrates no worse than the forces next to it; the factor allows for the different trajectory."""
    h, xyz = load_case(name)
    nvec, kappa, anchor, _ = pin_ref.bias_case(name)
    vel = md_ref.bar_velocities(name)
    drift = {}
    for biased in (False, True):
        r = pin_ref.run(h, xyz, nvec, kappa if biased else 0.0, anchor, BAR_STEPS, BAR_DT, vel=vel)
        t = r["trace"]
        total = t[:, 0] + t[:, 1] + t[:, 16]
        drift[biased] = float(np.abs(total - total[0]).max())
        assert tuple(r["status"]) == (BAR_STEPS, 0) and (np.ptp(t[:, 16]) > 10.0 * drift[biased] if biased else np.all(t[:, 16] == 0.0))
    print(name, "drift of E + K + U_b: unbiased %.3e, biased %.3e (bar %.3e)" % (drift[False], drift[True], 3.0 * drift[False]))
    assert drift[True] <= 3.0 * drift[False]


# -- (c) the conditions on every biased case the device runs --------------------------------------------------
@pytest.mark.parametrize("name,skew", DEVICE_CASES)
def test_every_biased_case_of_the_device_test_has_a_bias_that_matters(name, skew):
    h, xyz = load_case(name)
    nvec, kappa, anchor, q0 = pin_ref.bias_case(name, skew)
    # the triple: choose_wavevector's, restated over sk_ref
    cand = pin_ref.half_space(pin_ref.NMAX)
    if skew:
        assert name == pin_ref.SKEW_CASE and all(v != 0 for v in nvec) and min(nvec) < 0
        cand = cand[np.all(cand != 0, axis=1) & np.any(cand < 0, axis=1)]
    S = sk_ref.sk_tables(h, xyz, cand)[1]
    best = int(np.argmax(S))
    assert tuple(cand[best]) == nvec and math.isclose(math.sqrt(S[best]), q0, rel_tol=1e-12)
    assert np.sort(S)[-2] < S[best] * (1.0 - 1e-9)                        # no tie for a device's S to break the other way
    assert all(abs(v) <= 255 for v in nvec) and anchor == 0.8 * q0 and kappa > 0.0
    f_mw = flex_ref.energy_forces_stress(h, xyz)[1]
    fb = pin_ref.bias(h, xyz, nvec, kappa, anchor)[2]
    ratio = np.abs(fb).max() / np.median(np.abs(f_mw))
    print(name, nvec, "kappa %.4e anchor %.4f Q_0 %.4f  max |F_b| / median |F_mW| = %.3f" % (kappa, anchor, q0, ratio))
    assert 0.1 <= ratio <= 10.0
    # a device that drops the bias cannot pass: the unbiased mirror is 100 bars away in positions and velocities
    for coupling, axis, every in pin_ref.BAR_RUNS:
        for langevin in (False, True):
            a = pin_ref.reference(name, langevin, every, coupling, axis, True, False, skew)
            b = pin_ref.reference(name, langevin, every, coupling, axis, False, False, skew)
            dp, dv = np.abs(a["pos"] - b["pos"]).max(), np.abs(a["vel"] - b["vel"]).max()
            print("   ", coupling, every, langevin, "kappa = 0 misses by pos %.2e (%.0f bars) vel %.2e (%.0f bars) Q %.2e (%.0f bars)"
                  % (dp, dp / pin_ref.POS_TOL, dv, dv / pin_ref.VEL_TOL, abs(a["trace"][-1, 15]), abs(a["trace"][-1, 15]) / pin_ref.TRACE_TOL[15]))
            assert dp >= 100.0 * pin_ref.POS_TOL and dv >= 100.0 * pin_ref.VEL_TOL
            assert np.all(b["trace"][:, 15:] == 0.0) and np.all(b["blocks"][:, :2] == 0.0) and np.all(a["blocks"][:, 0] > 1.0)


# -- (d) the free ensemble ---------------------------------------------------------------------------
def test_the_free_ensembles_reference_law_is_sharp_and_the_mirror_follows_it():
    """The direct draw's own standard errors are below a fifth of those of the device's ensemble of FREE_BOXES boxes; the mirror's
    step at dt and at dt / 2 lands on the law within 5 standard errors plus the recorded halving differences, which are measured
    again here."""
    mean, var, se_mean, se_var = pin_ref.free_law()
    nb = pin_ref.FREE_HALVING_BOXES
    qa = pin_ref.free_q(nb, pin_ref.FREE_DT, pin_ref.FREE_STEPS, 5)
    qb = pin_ref.free_q(nb, pin_ref.FREE_DT / 2.0, 2 * pin_ref.FREE_STEPS, 6)
    m4 = float(((qa - qa.mean()) ** 4).mean())
    dev_se_mean = math.sqrt(var / pin_ref.FREE_BOXES)
    dev_se_var = math.sqrt((m4 - var * var) / pin_ref.FREE_BOXES)
    print("law: <Q> = %.5f +- %.1e, var Q = %.5f +- %.1e; a device ensemble of %d boxes: +- %.1e and +- %.1e" % (mean, se_mean, var, se_var, pin_ref.FREE_BOXES,
                                                                                                                dev_se_mean, dev_se_var))
    assert se_mean <= 0.2 * dev_se_mean and se_var <= 0.2 * dev_se_var
    unbiased = math.sqrt(math.pi) / 2.0                                     # <Q> of a Rayleigh law with <Q^2> = 1, N large
    assert mean > unbiased + 0.4                                            # the bias moves the law far beyond every error here
    s = math.sqrt(pin_ref.FREE_BOXES / nb)
    for q, what in ((qa, "dt"), (qb, "dt / 2")):
        dm, dv = q.mean() - mean, q.var() - var
        print(what, "mean %.3e (5 se %.3e + bias %.3e)  variance %.3e (5 se %.3e + bias %.3e)" % (dm, 5 * s * dev_se_mean, pin_ref.FREE_BIAS, dv, 5 * s * dev_se_var,
                                                                                                 pin_ref.FREE_VAR_BIAS))
        assert abs(dm) <= 5.0 * s * dev_se_mean + pin_ref.FREE_BIAS and abs(dv) <= 5.0 * s * dev_se_var + pin_ref.FREE_VAR_BIAS
    _held(qa.mean() - qb.mean(), pin_ref.FREE_HALVING_MEASURED, "the halving difference of the mean")
    _held(qa.var() - qb.var(), pin_ref.FREE_VAR_HALVING_MEASURED, "the halving difference of the variance")
    assert pin_ref.FREE_BIAS == 2.0 * abs(pin_ref.FREE_HALVING_MEASURED) and pin_ref.FREE_VAR_BIAS == 2.0 * abs(pin_ref.FREE_VAR_HALVING_MEASURED)
