"""CPU: the preconditions of tests/test_gpu_md.py and the bars it uses, measured again with the numpy mirror of tests/md_ref.py and
held against the constants recorded there.  Every figure is printed before it is asserted."""
import math

import numpy as np
import pytest

import md_ref
from md_ref import BAR_DT, BAR_KT, BAR_STEPS, MASS_WATER
from quench_ref import BAR_CASES, load_case


def _held(measured, recorded, what):
    """The recorded constant is the measured value rounded to three figures: within 1 % of it."""
    print(what, "measured %.4e recorded %.4e" % (measured, recorded))
    assert abs(measured - recorded) <= 0.01 * recorded, what


def test_the_spreads_under_force_noise_are_the_recorded_ones():
    """The experiment of the trajectory bar (md_ref's docstring): the mirror against itself with forces perturbed by +-F_ATOL."""
    pos, vel, trace = 0.0, 0.0, np.zeros(4)
    for name in md_ref.TRAJECTORY_CASES:
        for langevin in (False, True):
            a, b = md_ref.reference(name, langevin), md_ref.reference(name, langevin, True)
            dp, dv = float(np.abs(a["pos"] - b["pos"]).max()), float(np.abs(a["vel"] - b["vel"]).max())
            dt = np.abs(a["trace"] - b["trace"]).max(axis=0)
            print(name, "langevin" if langevin else "nve", "pos %.2e vel %.2e trace %s" % (dp, dv, " ".join("%.2e" % t for t in dt)))
            assert tuple(a["status"]) == (BAR_STEPS, 0)
            if name in BAR_CASES:
                pos, vel, trace = max(pos, dp), max(vel, dv), np.maximum(trace, dt)
            else:                                                          # held to the bar, not part of it
                assert dp <= md_ref.POS_TOL and dv <= md_ref.VEL_TOL and np.all(dt <= np.array(md_ref.TRACE_TOL))
    _held(pos, md_ref.POS_SPREAD_MEASURED, "positions")
    _held(vel, md_ref.VEL_SPREAD_MEASURED, "velocities")
    for k in range(4):
        _held(trace[k], md_ref.TRACE_SPREAD_MEASURED[k], "trace column %d" % k)
    assert md_ref.POS_TOL == 10.0 * md_ref.POS_SPREAD_MEASURED and md_ref.VEL_TOL == 10.0 * md_ref.VEL_SPREAD_MEASURED
    assert md_ref.TRACE_TOL == tuple(10.0 * s for s in md_ref.TRACE_SPREAD_MEASURED)


def test_the_mirror_conserves_energy_to_second_order():
    """NVE: E + K stays within a small fraction of K, and halving the step divides the largest error by 4.0019 on ih48_t020 (a
    second-order scheme: 4); the force noise moves that ratio by 3.03e-7."""
    ratio, a, b = md_ref.energy_ratio("ih48_t020")
    noisy, _, _ = md_ref.energy_ratio("ih48_t020", noisy=True)
    k0 = 0.5 * MASS_WATER * float((md_ref.bar_velocities("ih48_t020") ** 2).sum())
    print("ih48_t020: drift %.6e at 5 fs, %.6e at 2.5 fs, ratio %.7f, with force noise %.7f (difference %.3e); K(0) %.4e" % (a, b, ratio, noisy, abs(ratio - noisy), k0))
    assert a < 0.05 * k0 and b < a
    assert abs(ratio - 4.0) < 0.05
    assert abs(ratio - md_ref.ENERGY_RATIO_MEASURED) <= 1e-6
    _held(abs(ratio - noisy), md_ref.ENERGY_RATIO_NOISE_MEASURED, "the noise in the ratio")
    assert md_ref.ENERGY_RATIO_TOL == 10.0 * md_ref.ENERGY_RATIO_NOISE_MEASURED


def test_the_mirror_runs_backwards_to_its_start():
    worst = 0.0
    for name in BAR_CASES:
        h, xyz = load_case(name)
        v0 = md_ref.bar_velocities(name)
        fwd = md_ref.run(h, xyz, BAR_STEPS, BAR_DT, vel=v0)
        back = md_ref.run(h, fwd["pos"], BAR_STEPS, BAR_DT, vel=-fwd["vel"])
        dx = float(np.abs(back["pos"] - xyz).max())
        print(name, "return error %.3e bohr, moved %.3e" % (dx, np.abs(fwd["pos"] - xyz).max()))
        assert np.abs(fwd["pos"] - xyz).max() > 1e-3
        worst = max(worst, dx)
    _held(worst, md_ref.REVERSAL_RETURN_MEASURED, "the return error")
    assert md_ref.REVERSAL_TOL == 10.0 * md_ref.REVERSAL_RETURN_MEASURED


def test_philox_reproduces_the_oracles_uniforms():
    """With stream identity 0 the counter (step, molecule, 0) under the key `seed` is the oracle's (move, walker, call 0) under
    its seed: its first two uniforms are the 53-bit fractions of the word pairs."""
    from oracle import SweepOracle
    C = SweepOracle()

    def u53(a, b):
        return ((int(a) >> 5) * 67108864.0 + (int(b) >> 6)) / 9007199254740992.0

    for seed, step in ((1, 0), (424242, 17), ((1 << 40) + 3, (5 << 32) + 9)):
        w = md_ref.words(seed, 0, step, 5)
        for m in range(5):
            u = C.uniforms(seed, m, step)
            assert u53(w[0][m], w[1][m]) == u[0] and u53(w[2][m], w[3][m]) == u[1], (seed, step, m)
    # the key is stream XOR seed, word by word
    assert np.array_equal(md_ref.words(0x1234567800000005, 0x00000000FFFFFFFF, 3, 4), md_ref.words(0x12345678FFFFFFFA, 0, 3, 4))
    assert not np.array_equal(md_ref.words(1, 2, 3, 4), md_ref.words(1, 3, 3, 4))


def test_the_normals_are_normal():
    xi = np.concatenate([md_ref.normals(5, s, 0, 64) for s in range(400)])            # 76800 numbers
    n = xi.size
    print("mean %.4f variance %.4f fourth moment %.4f" % (xi.mean(), xi.var(), (xi ** 4).mean()))
    assert abs(xi.mean()) < 5.0 / math.sqrt(n) and abs(xi.var() - 1.0) < 5.0 * math.sqrt(2.0 / n) and abs((xi ** 4).mean() - 3.0) < 5.0 * math.sqrt(96.0 / n)
    assert np.abs(np.corrcoef(xi.T)[np.triu_indices(3, 1)]).max() < 5.0 / math.sqrt(len(xi))


def test_the_mirrors_thermostat_settles_a_gas_inside_the_bar_the_device_is_held_to():
    """The experiment of the device test with the mirror's noise: 1024 boxes of 20 free molecules from v = 0, 200 steps at
    gamma dt = 0.1; the mean kinetic energy is 3 N kT / 2 within 5 standard errors sqrt(2 / (3 * 20 * 1024))."""
    nb, n, dt = 1024, 20, BAR_DT
    _, _, c1, c2, hm = md_ref.constants(dt, MASS_WATER, BAR_KT, 0.1 / dt)
    assert c1 ** 400 < 1e-17
    key = np.uint64(11) ^ np.arange(1000, 1000 + nb, dtype=np.uint64)
    v = np.zeros((nb, n, 3))
    mol = np.arange(n, dtype=np.uint64)[None, :]
    for s in range(200):
        w = md_ref.philox4x32_10(s, 0, mol, 0, (key & np.uint64(0xFFFFFFFF))[:, None], (key >> np.uint64(32))[:, None])
        u = (np.array(w).astype(np.float64) + 0.5) * 2.0 ** -32
        r0, t0 = np.sqrt(-2.0 * np.log(u[0])), (2.0 * math.pi) * u[1]
        r1, t1 = np.sqrt(-2.0 * np.log(u[2])), (2.0 * math.pi) * u[3]
        v = c1 * v + c2 * np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1)], axis=2)
    assert np.array_equal(np.array(w)[:, 3, :], md_ref.words(11, 1003, 199, n))       # the batched words are those of `words`
    k = hm * (v * v).sum(axis=(1, 2))
    want, se = 1.5 * n * BAR_KT, math.sqrt(2.0 / (3.0 * n * nb))
    print("mean K / (3 N kT / 2) - 1 = %.2e, standard error %.2e" % (k.mean() / want - 1.0, se))
    assert abs(k.mean() / want - 1.0) <= 5.0 * se


def test_the_mirrors_guard_freezes_a_box_and_repeats_its_row():
    h, xyz = load_case("ic48_t015")
    close = np.array(xyz)
    close[1] = close[0] + np.array([0.5, 0.0, 0.0])
    r = md_ref.run(h, close, 6, BAR_DT, vel=md_ref.bar_velocities("ic48_t015"), sample_every=2)
    assert tuple(r["status"]) == (0, 1) and np.array_equal(r["pos"], close) and np.all(np.isfinite(r["vel"]))
    assert r["trace"].shape == (4, 4) and np.all(r["trace"] == r["trace"][0])


@pytest.mark.parametrize("name", ("ih48_t020",))
def test_a_run_of_the_mirror_equals_its_halves(name):
    h, xyz = load_case(name)
    kw = dict(kT=BAR_KT, gamma=md_ref.BAR_GAMMA, seed=4, stream=9)
    whole = md_ref.run(h, xyz, 10, BAR_DT, vel=md_ref.bar_velocities(name), step0=50, **kw)
    a = md_ref.run(h, xyz, 4, BAR_DT, vel=md_ref.bar_velocities(name), step0=50, **kw)
    b = md_ref.run(h, a["pos"], 6, BAR_DT, vel=a["vel"], step0=54, pos_ref=xyz, **kw)
    assert np.array_equal(b["pos"], whole["pos"]) and np.array_equal(b["vel"], whole["vel"]) and np.array_equal(b["trace"], whole["trace"][4:])
