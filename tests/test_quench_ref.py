"""CPU: the preconditions of tests/test_gpu_quench.py.  For every case the device's quench is compared against the mirror at
(quench_ref.QUENCH_CASES): the mirror at ftol 1e-10 and an independent minimiser -- scipy's L-BFGS-B on the same energy and
forces; where scipy is absent, the mirror with dt0 and dtmax doubled -- reach the same minimum, the energy within
conftest.RTOL relative and the positions within quench_ref.POS_TOL, and the centre of mass is kept.  Energy and forces of
the mirror are central differences of each other at one case.  The position bar is measured here again: ten times the
spread max |x(ftol 1e-10) - x(ftol 1e-12)| of the mirror.

Measured on the CPU with the defaults (iterations to fmax <= 1e-10, spread, |x - x(L-BFGS-B)|, bohr):
  ic48_t015 168 4.2e-8 1.1e-7 | ih48_t020 177 1.8e-8 7.6e-8 | ic64_sheared 177 2.5e-8 7.5e-8 | ic96 142 4.3e-8 5.1e-8 |
  ih96_disordered 181 4.3e-8 4.6e-8 | ic65_interstitial 307 2.2e-7 2.3e-7;  the energies agree to 2e-15 Hartree or better.
FIRE is not monotone (3 to 11 of those steps raise E): nothing here asserts monotonicity."""
import numpy as np
import pytest

from conftest import RTOL
from quench_ref import COM_TOL, FTOL, POS_SPREAD_MEASURED, POS_TOL, QUENCH_CASES, BAR_CASES, energy_forces, load_case, quench, reference, widths


def _independent_minimum(h, x0):
    """(positions, energy, what) of the minimum below x0 by a minimiser that is not the mirror's FIRE at its defaults."""
    try:
        from scipy.optimize import minimize
    except ImportError:
        r = quench(h, x0, FTOL, fire=(40.0, 400.0, 0.2, 0.1, 0.99, 1.1, 0.5, 5.0))
        return r["pos"], float(r["stats"][1]), "FIRE with dt0 and dtmax doubled"

    def fun(p):
        e, f = energy_forces(h, p.reshape(-1, 3))
        return e, -f.ravel()

    res = minimize(fun, x0.ravel(), jac=True, method="L-BFGS-B", options=dict(maxiter=5000, gtol=1e-11, ftol=1e-16, maxcor=20))
    x = res.x.reshape(-1, 3)
    return x, energy_forces(h, x)[0], "L-BFGS-B"


@pytest.mark.parametrize("name", QUENCH_CASES)
def test_the_mirror_and_an_independent_minimiser_reach_the_same_minimum(name):
    h, x0 = load_case(name)
    assert widths(h).min() >= 8.13808 * (1.0 + 1e-9) + 1e-3                # inside the supported range of the library
    r = reference(name)
    x, e, what = _independent_minimum(h, x0)
    de = abs(r["stats"][1] - e) / abs(e)
    dx = float(np.abs(r["pos"] - x).max())
    com = float(np.abs(r["pos"].mean(axis=0) - x0.mean(axis=0)).max())
    print(name, len(x0), "iterations", int(r["iters"][0]), "steps that raise E", int((np.diff(r["energies"]) > 0).sum()), what,
          "dE/E %.1e" % de, "max |dx| %.2e" % dx, "centre of mass %.1e" % com)
    assert tuple(r["iters"]) == (len(r["energies"]) - 1, 1) and r["stats"][3] <= FTOL
    assert r["stats"][1] < r["stats"][0] and r["stats"][3] < r["stats"][2]
    assert de <= RTOL
    assert dx <= POS_TOL
    assert com <= COM_TOL


def test_the_position_bar_is_ten_times_the_measured_spread():
    """The bar comes from the five cases that were there before any device result (BAR_CASES); the 65-molecule box, which is
    this suite's own choice, is held to it: its own spread and its distance to the independent minimum are inside the bar."""
    spread = {}
    for name in QUENCH_CASES:
        h, x0 = load_case(name)
        spread[name] = float(np.abs(reference(name)["pos"] - quench(h, x0, 1e-12)["pos"]).max())
    print(" ".join("%s %.2e" % kv for kv in spread.items()))
    largest = max(spread[name] for name in BAR_CASES)
    assert POS_TOL == 10.0 * POS_SPREAD_MEASURED
    assert 0.8 * POS_SPREAD_MEASURED <= largest <= 1.05 * POS_SPREAD_MEASURED, largest
    assert max(spread.values()) <= POS_TOL


def test_energy_and_forces_of_the_mirror_are_central_differences_of_each_other():
    h, x0 = load_case("ic48_t015")
    e, f = energy_forces(h, x0)
    step = 1e-5
    rng = np.random.default_rng(7)
    worst = 0.0
    for i, c in zip(rng.integers(0, len(x0), 12), rng.integers(0, 3, 12)):
        xp, xm = x0.copy(), x0.copy()
        xp[i, c] += step
        xm[i, c] -= step
        fd = -(energy_forces(h, xp)[0] - energy_forces(h, xm)[0]) / (2 * step)
        worst = max(worst, abs(fd - f[i, c]))
    print("max |F - central difference| %.2e of max |F| %.2e" % (worst, np.abs(f).max()))
    assert worst <= 1e-7 * np.abs(f).max()                                 # (the bar of tests/test_forces_ref.py at the same step)
    assert np.abs(f.sum(axis=0)).max() <= 1e-12 * np.abs(f).sum()          # the forces add up to zero: the centre of mass stays


def test_max_iter_zero_is_a_single_point_and_max_iter_stops_unconverged():
    h, x0 = load_case("ih48_t020")
    e, f = energy_forces(h, x0)
    r = quench(h, x0, FTOL, 0)
    assert tuple(r["iters"]) == (0, 0) and np.array_equal(r["pos"], x0) and np.array_equal(r["forces"], f)
    assert r["stats"][0] == r["stats"][1] == e and r["stats"][2] == r["stats"][3] == np.abs(f).max() and r["stats"][4] == r["stats"][5] == 0.0
    r = quench(h, x0, FTOL, 10)
    assert tuple(r["iters"]) == (10, 0) and len(r["energies"]) == 11
    assert np.array_equal(r["pos"], reference("ih48_t020")["pos"]) is False
    r = quench(h, x0, 1.0, 10)
    assert tuple(r["iters"]) == (0, 1)                                     # already below ftol: converged before any step
