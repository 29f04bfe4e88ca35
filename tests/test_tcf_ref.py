"""CPU: the numpy mirror of include/mw_tcf.h (tests/tcf_ref.py) gives the analytic results of ballistic, harmonic and diffusive
motion, the host helpers of ``timecorr`` read the right numbers off them, and on every input of the GPU tests the float64 mirror
lies within the a-priori bar of the long-double reference, every deliberately wrong mirror misses it by 10^3 or more, and no
squared displacement lies near a histogram edge."""
import numpy as np
import pytest

import tcf_ref
from tcf_ref import evaluate, make_input, n_origins, reference, worst


def _plan():
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.timecorr import tcf_plan
    build.build_tcf()
    return tcf_plan(16, 8)


def _cases():
    return tcf_ref.cases(_plan())


def test_ballistic_molecules():
    rng = np.random.default_rng(1)
    T, B, N, dt, speed = 9, 2, 7, 0.5, 0.3
    u = rng.normal(size=(B, N, 3))
    v = speed * u / np.linalg.norm(u, axis=-1, keepdims=True)
    frames = rng.uniform(0, 20, (1, B, N, 3)) + v[None] * (dt * np.arange(T))[:, None, None, None]
    vel = np.broadcast_to(v, (T, B, N, 3))
    q = np.array([0.7, 2.9])
    r = evaluate(frames, vel, T, 2, q)
    lag = np.arange(T)
    assert np.allclose(r["msd"], (speed * lag * dt) ** 2, rtol=1e-12, atol=1e-13)
    assert np.allclose(r["mqd"], (speed * lag * dt) ** 4, rtol=1e-12, atol=1e-13)
    assert np.allclose(r["vacf"], speed ** 2, rtol=1e-13)
    x = q[None, :] * (speed * lag * dt)[:, None]
    assert np.allclose(r["fs"], np.sinc(x / np.pi)[None], rtol=0, atol=1e-12)
    assert np.all(r["msd"][:, 0] == 0.0) and np.all(r["fs"][:, 0] == 1.0)
    from mc_water_ls_mw_amd.timecorr import non_gaussian
    assert np.allclose(non_gaussian(r["msd"], r["mqd"])[:, 1:], -0.4, atol=1e-10)      # one speed: 3 / 5 - 1


def test_harmonic_coordinate_and_the_helpers_recover_omega():
    from mc_water_ls_mw_amd.timecorr import vdos
    T, N, dt, omega = 257, 8, 0.1, 2.0 * np.pi * 10 / 25.6                  # ten periods in the 256 intervals
    phase = 2.0 * np.pi * np.arange(N) / N
    t = dt * np.arange(T)
    vel = np.zeros((T, 1, N, 3))
    vel[:, 0, :, 0] = np.cos(omega * t[:, None] + phase[None, :])
    frames = np.zeros((T, 1, N, 3))
    frames[:, 0, :, 0] = np.sin(omega * t[:, None] + phase[None, :]) / omega
    r = evaluate(frames, vel, T, 1)
    assert np.allclose(r["vacf"][0], 0.5 * np.cos(omega * t), rtol=0, atol=1e-12)
    assert np.allclose(r["msd"][0], (1.0 - np.cos(omega * t)) / omega ** 2, rtol=0, atol=1e-12)
    w, spec = vdos(r["vacf"], dt)
    assert abs(w[np.argmax(spec[0])] - omega) <= 0.5 * (w[1] - w[0]) + 1e-12
    w, spec = vdos(r["vacf"], dt, window=None)
    assert abs(w[np.argmax(spec[0])] - omega) <= 0.5 * (w[1] - w[0]) + 1e-12


def test_gaussian_random_walks_diffuse_and_are_gaussian():
    from mc_water_ls_mw_amd.timecorr import diffusion_from_msd, non_gaussian
    rng = np.random.default_rng(2)
    T, B, N, sigma, nlags = 13, 4096, 8, 0.25, 7
    steps = rng.normal(0.0, sigma, (T, B, N, 3))
    steps[0] = 0.0
    r = evaluate(np.cumsum(steps, axis=0), None, nlags, 1)
    lag = np.arange(nlags)
    mean, err = r["msd"].mean(axis=0), r["msd"].std(axis=0, ddof=1) / np.sqrt(B)
    assert np.all(np.abs(mean - 3.0 * sigma ** 2 * lag) <= 5.0 * err), (mean, err)
    q_mean, q_err = r["mqd"].mean(axis=0), r["mqd"].std(axis=0, ddof=1) / np.sqrt(B)
    alpha = non_gaussian(mean, q_mean)
    alpha_err = (1.0 + alpha[1:]) * np.sqrt((q_err[1:] / q_mean[1:]) ** 2 + (2.0 * err[1:] / mean[1:]) ** 2)
    assert alpha[0] == 0.0 and np.all(np.abs(alpha[1:]) <= 5.0 * alpha_err), (alpha, alpha_err)
    dt = 0.4
    d, d_err = diffusion_from_msd(mean, dt, (1, nlags - 1)), err.max() / (6.0 * dt)
    assert abs(d - sigma ** 2 / (2.0 * dt)) <= 5.0 * d_err


def test_a_uniform_drift_vanishes_when_the_centre_is_removed():
    case = next(c for c in _cases() if c.name == "every3")
    frames, vel, q, edges = make_input(case)
    drift = np.array([3.0, -2.0, 5.0]) * np.arange(case.nframes)[:, None, None, None]
    a = evaluate(frames, vel, case.nlags, case.every, q, remove_com=True, dtype=np.longdouble)
    b = evaluate(frames + drift, vel + 0.01, case.nlags, case.every, q, remove_com=True, dtype=np.longdouble)
    for name in ("msd", "mqd", "vacf", "fs"):
        assert np.all(np.abs(a[name] - b[name]) <= a["bar_" + name] + b["bar_" + name]), name
    c = evaluate(frames + drift, vel, case.nlags, case.every, q, remove_com=False)
    assert np.all(c["msd"][:, 1:] > 10.0 * a["msd"][:, 1:])


def test_each_histogram_row_adds_up_to_the_terms_of_its_lag():
    for case in _cases():
        if not case.nedges:
            continue
        hist = reference(case)["hist"]
        for h, lag in enumerate(case.hist_lags):
            assert np.all(hist[:, h].sum(axis=-1) == n_origins(case.nframes, lag, case.every) * case.nwater), (case.name, lag)
        assert max(case.hist_lags) == 0 or hist[:, :, 1:-1].sum() > 0, case.name     # (lag 0: every displacement is 0, below the first edge)


def test_the_helpers():
    from mc_water_ls_mw_amd.timecorr import MwError, diffusion_from_msd, diffusion_from_vacf, non_gaussian, van_hove_from_counts
    t = 0.2 * np.arange(50)
    assert abs(diffusion_from_msd(6.0 * 0.37 * t + 1.5, 0.2) - 0.37) < 1e-12
    assert np.allclose(diffusion_from_msd(np.stack([6.0 * 0.37 * t, 6.0 * 0.11 * t]), 0.2, (10, 40)), [0.37, 0.11], rtol=1e-12)
    with pytest.raises(MwError, match="fit"):
        diffusion_from_msd(t, 0.2, (10, 10))
    tau = 1.3
    assert abs(diffusion_from_vacf(0.9 * np.exp(-0.01 * np.arange(4000) / tau), 0.01) - 0.9 * tau / 3.0) < 1e-4
    rng = np.random.default_rng(3)
    d2 = (rng.normal(size=(200000, 3)) ** 2).sum(axis=1)
    assert abs(non_gaussian(d2.mean(), (d2 * d2).mean())) < 0.02
    edges = np.linspace(0.5, 2.5, 21)
    counts = np.bincount(np.searchsorted(edges, np.sqrt(d2), side="right"), minlength=len(edges) + 1)
    r_mid, p = van_hove_from_counts(counts, edges)
    assert len(r_mid) == 20 and abs((p * np.diff(edges)).sum() + (counts[0] + counts[-1]) / counts.sum() - 1.0) < 1e-12
    maxwell = np.sqrt(2.0 / np.pi) * r_mid ** 2 * np.exp(-0.5 * r_mid ** 2)
    assert np.all(np.abs(p - maxwell) < 0.02)
    assert np.all(van_hove_from_counts(np.zeros((3, 22), dtype=np.int64), edges)[1] == 0.0)


def test_long_double_has_a_64_bit_mantissa_or_fsum_stands_in():
    if np.finfo(np.longdouble).nmant >= 63:
        return
    case = _cases()[0]
    frames, vel, q, _ = make_input(case)
    a, b = evaluate(frames, vel, case.nlags, case.every, q), tcf_ref.evaluate_fsum(frames, vel, case.nlags, case.every, q)
    assert np.allclose(a["msd"], b["msd"], rtol=1e-12)


def test_the_mirror_is_within_the_bar_of_the_reference_on_every_gpu_input():
    names = set()
    for case in _cases():
        frames, vel, q, edges = make_input(case)
        assert frames.shape == (case.nframes, case.nboxes, case.nwater, 3) and vel.shape == frames.shape
        ref = reference(case)
        got = evaluate(frames, vel, case.nlags, case.every, q, edges * edges, case.hist_lags, case.remove_com)
        rows = worst(got, ref)
        print(case.name, {k: f"{v[0]:.2e} / {v[1]:.2e}" for k, v in rows.items()})
        assert rows and all(v[2] <= 1.0 for v in rows.values()), (case.name, rows)
        assert np.array_equal(got["hist"], ref["hist"]), case.name
        for name in ("msd", "mqd", "vacf", "fs"):
            assert np.all(np.isfinite(ref[name])) and np.all(ref["bar_" + name] >= 0), (case.name, name)
            assert np.all(ref["bar_" + name] <= 1e-9 * np.maximum(np.abs(ref[name]), 1e-3) * max(1.0, np.abs(frames).max()) ** 2), (case.name, name)
        names.add(case.name)
    assert len(names) == len(_cases())


def test_no_squared_displacement_lies_near_an_edge():
    for case in _cases():
        if case.nedges and case.hist_lags:
            assert reference(case)["margin"] > 1e-9, (case.name, reference(case)["margin"])


@pytest.mark.parametrize("wrong,name", [("origin", "nwater_tile+1"), ("lag", "nwater_tile+1"), ("every", "every3"), ("com", "every3"), ("molecule", "nwater_tile+1"),
                                        ("frame", "nwater_tile+1"), ("origin", "nframes_300"), ("lag", "nframes_300"), ("molecule", "nwater_200"),
                                        ("com", "farm600")])
def test_every_wrong_mirror_misses_the_bar_by_a_thousand(wrong, name):
    case = next(c for c in _cases() if c.name == name)
    frames, vel, q, edges = make_input(case)
    got = evaluate(frames, vel, case.nlags, case.every, q, edges * edges, case.hist_lags, case.remove_com, wrong=wrong)
    rows = worst(got, reference(case))
    assert max(v[2] for v in rows.values()) >= 1e3, rows
    assert rows["msd"][2] >= 1e3, rows
