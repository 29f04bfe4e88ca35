"""CPU: the preconditions of tests/test_gpu_ti.py and the bars it uses, measured again with the numpy mirror of tests/ti_ref.py and
held against the constants recorded there.  Every figure is printed before it is asserted."""
import numpy as np

import md_ref
import ti_ref
from md_ref import BAR_DT, BAR_GAMMA, BAR_KT, BAR_STEPS, MASS_WATER
from quench_ref import BAR_CASES, load_case


def _held(measured, recorded, what):
    """The recorded constant is the measured value rounded to three figures: within 1 % of it."""
    print(what, "measured %.4e recorded %.4e" % (measured, recorded))
    assert abs(measured - recorded) <= 0.01 * recorded, what


def test_the_spreads_under_force_noise_are_the_recorded_ones():
    """The experiment of the bars (ti_ref's docstring): the mirror against itself with every F_mW perturbed by +-F_ATOL."""
    for name in ti_ref.TRAJECTORY_CASES:
        for lam in ti_ref.BAR_LAMBDAS:
            for langevin in (False, True):
                r = ti_ref.reference(name, langevin, lam)
                assert tuple(r["status"]) == (BAR_STEPS, 0) and r["trace"].shape == (BAR_STEPS + 1, 5) and r["blocks"].shape == (5, 5)
                assert r["trace"][0, 2] > 0.01 and r["trace"][0, 4] > 0.0              # u is not zero at step 0
    pos, vel, trace, blocks = ti_ref.spreads()
    _held(pos, ti_ref.SPREAD_POS, "positions")
    _held(vel, ti_ref.SPREAD_VEL, "velocities")
    for k in range(5):
        _held(trace[k], ti_ref.SPREAD_TRACE[k], "trace column %d" % k)
        _held(blocks[k], ti_ref.SPREAD_BLOCKS[k], "block column %d" % k)
    p, v, t, b = ti_ref.spreads(("ic65_interstitial",))                            # held to the bars, not part of them
    print("ic65_interstitial pos %.2e vel %.2e trace %s blocks %s" % (p, v, t, b))
    assert p <= ti_ref.POS_TOL and v <= ti_ref.VEL_TOL and np.all(t <= np.array(ti_ref.TRACE_TOL)) and np.all(b <= np.array(ti_ref.BLOCKS_TOL))
    assert ti_ref.POS_TOL == 10.0 * ti_ref.SPREAD_POS and ti_ref.VEL_TOL == 10.0 * ti_ref.SPREAD_VEL
    assert ti_ref.TRACE_TOL == tuple(10.0 * s for s in ti_ref.SPREAD_TRACE) and ti_ref.BLOCKS_TOL == tuple(10.0 * s for s in ti_ref.SPREAD_BLOCKS)
    assert ti_ref.BAR_CASES == BAR_CASES and ti_ref.BAR_LAMBDAS == (0.3, 0.8) and ti_ref.BAR_SPRING == 0.02


def test_the_blocks_are_the_sequential_sums_of_the_rows():
    r = ti_ref.reference("ih48_t020", True, 0.3)
    for j in range(5):
        acc = np.zeros(5)
        for s in range(ti_ref.BAR_EQUIL + 7 * j, ti_ref.BAR_EQUIL + 7 * j + 7):
            acc = acc + r["trace"][s + 1]
        assert np.array_equal(r["blocks"][j], acc / 7.0)
    assert ti_ref.nblocks_of(40, 5, 7) == 5 and ti_ref.nblocks_of(40, 41, 7) == 0 and ti_ref.nblocks_of(40, 5, 0) == 0 and ti_ref.nblocks_of(40, 40, 1) == 0


def test_the_mirror_at_lambda_0_is_md_ref():
    for name in ("ih48_t020", "ic96"):
        h, xyz = load_case(name)
        s, v0 = ti_ref.bar_sites(name), md_ref.bar_velocities(name)
        for kT, gamma in ((0.0, 0.0), (BAR_KT, BAR_GAMMA)):
            a = ti_ref.run(h, s, 0.0, 0.02, 12, BAR_DT, kT, gamma, pos=xyz, vel=v0, seed=5, stream=2, step0=9, sample_every=3)
            b = md_ref.run(h, xyz, 12, BAR_DT, kT, gamma, vel=v0, seed=5, stream=2, step0=9, sample_every=3, pos_ref=s)
            assert all(np.array_equal(a[k], b[k]) for k in ("pos", "vel", "forces", "status")) and np.array_equal(a["trace"][:, :4], b["trace"])
            u = (a["pos"] - s).sum(axis=0) / len(s)
            assert a["trace"][-1, 4] == (u * u).sum()


def test_the_mirror_at_lambda_1_is_the_matrix_power():
    """200 NVE steps at lambda = 1: positions and velocities equal the 2 x 2 step matrix raised to the 200th power to 1e-12
    relative to the amplitudes; the energy of the Einstein crystal is conserved by the modified Hamiltonian only, and the forces
    are -k u whatever mW says."""
    name = "ih48_t020"
    h, xyz = load_case(name)
    s, v0 = ti_ref.bar_sites(name), md_ref.bar_velocities(name)
    for k in (0.005, 0.02, 0.1):
        a = ti_ref.run(h, s, 1.0, k, 200, BAR_DT, pos=xyz, vel=v0)
        u, v = ti_ref.nve_exact(xyz - s, v0, k, BAR_DT, 200)
        amp_u = np.sqrt(((xyz - s) ** 2 + MASS_WATER / k * v0 ** 2).max())
        amp_v = amp_u * np.sqrt(k / MASS_WATER)
        du, dv = np.abs(a["pos"] - s - u).max() / amp_u, np.abs(a["vel"] - v).max() / amp_v
        print("k", k, "positions %.2e velocities %.2e of the amplitude" % (du, dv))
        assert tuple(a["status"]) == (200, 0) and du <= 1e-12 and dv <= 1e-12
        assert np.array_equal(a["forces"], -(1.0 * k) * (a["pos"] - s))
        assert abs(np.linalg.det(ti_ref.nve_matrix(k, BAR_DT)) - 1.0) <= 1e-15              # symplectic


def test_baoab_samples_the_positions_of_the_einstein_crystal_exactly_and_the_velocities_not():
    """The stationary covariance of the lambda = 1 Langevin step from its Lyapunov equation, checked by iterating the map."""
    for k, vv in ((0.005, 0.998), (0.02, 0.993), (0.1, 0.967)):
        u2, v2, uv = ti_ref.langevin_stationary(k, BAR_DT, BAR_KT, BAR_GAMMA)
        print("k", k, "k <u^2> / kT - 1 = %.2e, m <v^2> / kT = %.6f, <u v> = %.2e" % (k * u2 / BAR_KT - 1.0, MASS_WATER * v2 / BAR_KT, uv))
        assert abs(k * u2 / BAR_KT - 1.0) <= 1e-13 and abs(MASS_WATER * v2 / BAR_KT - vv) <= 1e-3
        # the covariance the step carries from zero settles there
        hk, hd, c1, c2, _ = md_ref.constants(BAR_DT, MASS_WATER, BAR_KT, BAR_GAMMA)
        a = hk * k
        A, D, O = np.array([[1.0, 0.0], [-a, 1.0]]), np.array([[1.0, hd], [0.0, 1.0]]), np.diag([1.0, c1])
        T, g = A @ D @ O @ D @ A, (A @ D)[:, 1] * c2
        S = np.zeros((2, 2))
        for _ in range(4000):                                                      # 200 relaxation times
            S = T @ S @ T.T + np.outer(g, g)
        assert np.allclose(S, [[u2, uv], [uv, v2]], rtol=1e-10, atol=1e-12 * np.sqrt(u2 * v2))


def test_a_frozen_box_fills_its_blocks_with_its_last_row():
    """Two molecules 0.5 bohr apart at lambda = 0.3: the first kick is beyond the guard, the box is frozen before its first drift
    and every block is the row of step 0."""
    h, xyz = load_case("ic48_t015")
    close = np.array(xyz)
    close[1] = close[0] + np.array([0.5, 0.0, 0.0])
    r = ti_ref.run(h, ti_ref.bar_sites("ic48_t015"), 0.3, 0.02, 20, BAR_DT, pos=close, equil_steps=2, block_steps=4)
    assert tuple(r["status"]) == (0, 1) and r["blocks"].shape == (4, 5) and np.array_equal(r["pos"], close)
    acc = np.zeros(5)
    for _ in range(4):
        acc = acc + r["trace"][0]
    assert np.all(r["trace"] == r["trace"][0]) and np.all(r["blocks"] == acc / 4.0)
