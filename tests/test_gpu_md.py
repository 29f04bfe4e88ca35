"""GPU: the molecular dynamics of libmw_md.so (dynamics.molecular_dynamics / _torch, EnergyModule.molecular_dynamics,
WalkerFarm.molecular_dynamics) against the numpy mirror of tests/md_ref.py, against the engine and the quench library, and the
bit rules of include/mw_md.h.

Bars.  Energies: conftest.RTOL = 1e-10 relative; forces of a single point: quench_ref.F_ATOL = 1e-10 Hartree / bohr.  After 40
steps: md_ref.POS_TOL = 3.81e-7 bohr, md_ref.VEL_TOL = 2.79e-10 bohr per atomic time unit and md_ref.TRACE_TOL per column, ten
times the largest deviation the mirror shows against itself with its forces perturbed by +-F_ATOL (measured on the CPU,
tests/md_ref.py; tests/test_md_ref.py measures it again).  Reversal: md_ref.REVERSAL_TOL = 3.56e-13 bohr, ten times the mirror's
own return error.  Energy conservation: the ratio of the largest |E + K - (E + K)(0)| at 5 fs and at 2.5 fs within
md_ref.ENERGY_RATIO_TOL = 3.03e-6 of the mirror's ratio for the same box, ten times what the force noise moves it by.  The
noise: NOISE_ULP below.  None of these figures comes from a device result but NOISE_ULP, which compares two
implementations of log, sin and cos and can only be measured on the device: the largest distance seen between the device's normals and numpy's was 2 ulp (of the normal), and
the bar is four times that."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from conftest import RTOL, load_golden
from boo_ref import scaled_set
from quench_ref import BAR_CASES, F_ATOL, energy_forces, load_case
import md_ref
from md_ref import BAR_DT, BAR_GAMMA, BAR_KT, BAR_SEED, BAR_STEPS, MASS_WATER

pytestmark = pytest.mark.gpu

#: the largest distance between a normal of the device and the mirror's, in ulp of the latter: measured 2 over the 60 normals
#: of md_ref.free_gas20 at four (seed, stream, step) triples; times four
NOISE_ULP_MEASURED = 2
NOISE_ULP = 4 * NOISE_ULP_MEASURED
ZERO_STEP_CASES = ("single_atom", "dimer", "gas20", "ic48_t015", "ic64_sheared", "ic65_interstitial", "ic96", "ih1536_t012")


@pytest.fixture(scope="module", autouse=True)
def _library_lifetime():
    """The libraries are initialised by their first calls here and finalised when this file is done."""
    yield
    from mc_water_ls_mw_amd import dynamics, quench
    dynamics.md_finalize()
    quench.quench_finalize()


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _all_same(a, b):
    return all(_same(x, y) for x, y in zip(a, b))


def _engine(h, xyz):
    """(E, F) of one box from the engine's two passes over its own lists."""
    from mc_water_ls_mw_amd.energy import load_boxes
    em = load_boxes([h], [xyz])
    try:
        e, f, _ = em.forces_batch()
        return float(e[0]), f[0].copy()
    finally:
        em.energy_deinit()


def _md(*a, **kw):
    from mc_water_ls_mw_amd.dynamics import molecular_dynamics
    return molecular_dynamics(*a, **kw)


# -- 1. nsteps = 0 ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ZERO_STEP_CASES)
def test_zero_steps_is_a_single_point_and_leaves_the_state_alone(name):
    from mc_water_ls_mw_amd.dynamics import md_last, maxwell_boltzmann
    from mc_water_ls_mw_amd.quench import inherent_structures
    h, xyz = load_case(name)
    n = len(xyz)
    vel = maxwell_boltzmann(1, n, BAR_KT, seed=3)[0]
    pos_out, vel_out, forces, trace, status = _md(h, xyz, 0, BAR_DT, vel=vel)
    assert pos_out.shape == (n, 3) and vel_out.shape == (n, 3) and forces.shape == (n, 3) and trace.shape == (1, 4) and status.shape == (2,)
    assert md_last()["small"] == (n <= 64) and md_last()["chunks"] == 1
    assert _same(pos_out, np.ascontiguousarray(xyz)) and _same(vel_out, vel) and tuple(status) == (0, 0)
    e_ref, f_ref = energy_forces(h, xyz)
    e_eng, f_eng = _engine(h, xyz)
    print(name, n, "E %.15g" % trace[0, 0], "dE/E (reference, engine) %.1e %.1e" % (abs(trace[0, 0] - e_ref) / max(abs(e_ref), 1e-300),
                                                                                    abs(trace[0, 0] - e_eng) / max(abs(e_eng), 1e-300)),
          "max |dF| (reference, engine) %.1e %.1e" % (np.abs(forces - f_ref).max(), np.abs(forces - f_eng).max()))
    assert abs(trace[0, 0] - e_ref) <= RTOL * abs(e_ref) and abs(trace[0, 0] - e_eng) <= RTOL * abs(e_eng)
    assert np.abs(forces - f_ref).max() <= F_ATOL and np.abs(forces - f_eng).max() <= F_ATOL
    k_ref = 0.5 * MASS_WATER * float((vel * vel).sum())
    assert abs(trace[0, 1] - k_ref) <= 1e-13 * max(k_ref, 1e-300) and trace[0, 2] == 0.0 and trace[0, 3] == np.abs(forces).max()
    # the quench library's single point: the same device routines, the same bytes
    _, f_q, stats_q, _ = inherent_structures(h, xyz, 1e-10, 0)
    assert _same(forces, f_q) and trace[0, 0] == stats_q[0] and trace[0, 3] == stats_q[2]


# -- 2. short trajectories against the mirror -------------------------------------------------
@pytest.mark.parametrize("langevin", (False, True), ids=("nve", "langevin"))
@pytest.mark.parametrize("name", md_ref.TRAJECTORY_CASES)
def test_forty_steps_land_where_the_mirror_lands(name, langevin):
    h, xyz = load_case(name)
    ref = md_ref.reference(name, langevin)                                 # (computed once per process, read-only)
    got = _md(h, xyz, BAR_STEPS, BAR_DT, BAR_KT if langevin else 0.0, BAR_GAMMA if langevin else 0.0, vel=md_ref.bar_velocities(name), seed=BAR_SEED,
              streams=[3])
    pos_out, vel_out, forces, trace, status = got
    dx, dv = float(np.abs(pos_out - ref["pos"]).max()), float(np.abs(vel_out - ref["vel"]).max())
    dt = np.abs(trace - ref["trace"]).max(axis=0)
    print(name, "langevin" if langevin else "nve", "max |dx| %.2e (bar %.2e)" % (dx, md_ref.POS_TOL), "max |dv| %.2e (bar %.2e)" % (dv, md_ref.VEL_TOL),
          "trace", " ".join("%.2e" % v for v in dt), "bars", " ".join("%.2e" % v for v in md_ref.TRACE_TOL))
    assert tuple(status) == (BAR_STEPS, 0) and tuple(ref["status"]) == (BAR_STEPS, 0) and trace.shape == (BAR_STEPS + 1, 4)
    assert dx <= md_ref.POS_TOL
    assert dv <= md_ref.VEL_TOL
    assert np.all(dt <= np.array(md_ref.TRACE_TOL))
    assert np.abs(forces - ref["forces"]).max() <= 10.0 * md_ref.TRACE_SPREAD_MEASURED[3] + F_ATOL
    assert not _same(pos_out, np.ascontiguousarray(xyz)) and trace[-1, 2] > 0.0


# -- 3. reversibility ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", BAR_CASES)
def test_nve_runs_backwards_to_its_start(name):
    h, xyz = load_case(name)
    v0 = md_ref.bar_velocities(name)
    fwd = _md(h, xyz, BAR_STEPS, BAR_DT, vel=v0)
    back = _md(h, fwd[0], BAR_STEPS, BAR_DT, vel=-fwd[1])
    dx, dv = float(np.abs(back[0] - xyz).max()), float(np.abs(back[1] + v0).max())
    print(name, "return error %.2e bohr (bar %.2e), velocities %.2e" % (dx, md_ref.REVERSAL_TOL, dv), "moved %.2e" % np.abs(fwd[0] - xyz).max())
    assert np.abs(fwd[0] - xyz).max() > 1e-3
    assert dx <= md_ref.REVERSAL_TOL


# -- 4. energy conservation ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ("ih48_t020", "ic96"))
def test_the_energy_error_falls_fourfold_with_half_the_step_as_the_mirrors_does(name):
    h, xyz = load_case(name)
    v0 = md_ref.bar_velocities(name)
    a = md_ref.energy_drift(_md(h, xyz, md_ref.ENERGY_STEPS, BAR_DT, vel=v0)[3])
    b = md_ref.energy_drift(_md(h, xyz, 2 * md_ref.ENERGY_STEPS, BAR_DT / 2.0, vel=v0)[3])
    ratio_ref, a_ref, b_ref = md_ref.energy_ratio(name)                    # the mirror: 1200 evaluations, a few seconds
    print(name, "device: %.6e / %.6e = %.7f" % (a, b, a / b), "mirror: %.6e / %.6e = %.7f" % (a_ref, b_ref, ratio_ref),
          "difference %.2e (bar %.2e)" % (abs(a / b - ratio_ref), md_ref.ENERGY_RATIO_TOL))
    assert abs(a / b - ratio_ref) <= md_ref.ENERGY_RATIO_TOL
    if name == "ih48_t020":
        assert abs(ratio_ref - md_ref.ENERGY_RATIO_MEASURED) <= 1e-6


# -- 5. the noise stream exactly ------------------------------------------------------------------
def test_one_thermostat_step_of_a_gas_is_the_mirrors_normals():
    """md_ref.free_gas20: 20 molecules out of each other's reach, every force exactly zero (the golden gas20 is a dense gas with
    E = 7.0 Hartree and cannot serve).  From v = 0 with gamma dt = 50, c1 = exp(-50) multiplies a zero and 1 - c1^2 rounds to 1,
    so after one step v = c2 xi with c2 = sqrt(kT / mass) to the last bit."""
    h, xyz = md_ref.free_gas20()
    n = len(xyz)
    dt = BAR_DT
    gamma = 50.0 / dt
    _, _, c1, c2, _ = md_ref.constants(dt, MASS_WATER, BAR_KT, gamma)
    assert 1.0 - c1 * c1 == 1.0 and c2 == math.sqrt(BAR_KT / MASS_WATER)
    worst, got = 0.0, {}
    for seed, stream, step0 in ((1, 0, 0), (1, 5, 0), (2, 5, 0), ((1 << 40) + 17, (1 << 63) + 12345, (1 << 33) + 7)):
        pos_out, vel_out, forces, trace, status = _md(h, xyz, 1, dt, BAR_KT, gamma, seed=seed, streams=[stream], step0=step0)
        assert tuple(status) == (1, 0) and np.all(forces == 0.0)
        want = c2 * md_ref.normals(seed, stream, step0, n)
        ulp = np.abs(vel_out - want) / np.spacing(np.abs(want))
        worst = max(worst, float(ulp.max()))
        print("seed", seed, "stream", stream, "step0", step0, "largest distance %.1f ulp" % ulp.max())
        got[(seed, stream, step0)] = vel_out
        assert _same(_md(h, xyz, 1, dt, BAR_KT, gamma, seed=seed, streams=[stream], step0=step0)[1], vel_out)      # the same: the same bytes
        assert np.allclose(pos_out - xyz, 0.5 * dt * vel_out, rtol=0, atol=1e-12)                                  # only the second half drift moved it
    print("largest distance to the mirror's normals: %.1f ulp (bar %d)" % (worst, NOISE_ULP))
    assert worst <= NOISE_ULP
    keys = list(got)
    for i in range(len(keys)):
        for j in range(i):
            assert not np.any(got[keys[i]] == got[keys[j]]), (keys[i], keys[j])        # another stream, seed or step: other normals
    # stream NULL is the box's index in the call
    two = _md(np.array([h, h]), np.array([xyz, xyz]), 1, dt, BAR_KT, gamma, seed=1)
    assert _same(two[1][0], got[(1, 0, 0)]) and _same(two[1][1], _md(h, xyz, 1, dt, BAR_KT, gamma, seed=1, streams=[1])[1])


# -- 6. the thermostat's stationary state ----------------------------------------------------------
def test_the_thermostat_settles_a_gas_at_its_temperature():
    """1024 copies of md_ref.free_gas20 (every force exactly zero) from v = 0, 200 steps at gamma dt = 0.1: with zero forces every velocity component is an exact
    Ornstein-Uhlenbeck chain with stationary variance kT / mass at any dt, the transient is 0.905^200 < 1e-17, and K of a box is
    kT / 2 times a chi-square of 3 N = 60 degrees: mean 3 N kT / 2, relative standard error of the mean over 1024 boxes
    sqrt(2 / (3 * 20 * 1024)) = 5.7e-3.  (tests/test_md_ref.py confirms that the mirror's noise is inside 5 of these.)"""
    h, xyz = md_ref.free_gas20()
    nb, n = 1024, len(xyz)
    dt = BAR_DT
    pos_out, vel_out, forces, trace, status = _md(np.tile(h, (nb, 1, 1)), np.tile(xyz, (nb, 1, 1)), 200, dt, BAR_KT, 0.1 / dt, seed=11,
                                                  streams=np.arange(1000, 1000 + nb), sample_every=200)
    assert trace.shape == (nb, 2, 4) and np.all(status == (200, 0)) and np.all(forces == 0.0) and np.all(trace[:, 0, 1] == 0.0)
    want = 1.5 * n * BAR_KT
    se = math.sqrt(2.0 / (3.0 * n * nb))
    k = trace[:, 1, 1]
    print("mean K / (3 N kT / 2) - 1 = %.2e, standard error %.2e" % (k.mean() / want - 1.0, se))
    assert abs(k.mean() / want - 1.0) <= 5.0 * se
    assert np.allclose(k, 0.5 * MASS_WATER * (vel_out * vel_out).sum(axis=(1, 2)), rtol=1e-13, atol=0)


# -- 7. the guard -----------------------------------------------------------------------------------
def _just_under_the_guard(v, fraction):
    """v plus a common velocity along x such that the fastest molecule's half drift is `fraction` of a sigma / 4."""
    limit = fraction * (md_ref.A_SIGMA / 4.0) / (BAR_DT / 2.0)
    s = limit
    for _ in range(50):
        s += limit - np.sqrt(((v + np.array([s, 0.0, 0.0])) ** 2).sum(axis=1)).max()
    return v + np.array([s, 0.0, 0.0])


@pytest.mark.parametrize("name", ("ic48_t015", "ic65_interstitial"), ids=("small", "general"))
def test_a_box_that_blows_up_is_frozen_and_its_neighbour_is_untouched(name):
    """Box 0 moves as a whole at 0.99 of the speed the guard allows, so its thermal motion carries a molecule over the limit
    after some steps (the mirror: 28 for ic48_t015, 43 for ic65_interstitial); box 2 has two molecules 0.5 bohr apart, which
    the first kick sends off at 4 bohr per atomic time unit; boxes 1 and 3 are healthy.  NVE.  The guard is ordinary arithmetic:
    nothing here is out of range for any kernel, and the sort clamps every cell index."""
    h, xyz = load_case(name)
    close = np.array(xyz)
    close[1] = close[0] + np.array([0.5, 0.0, 0.0])
    v = md_ref.bar_velocities(name)
    fast = _just_under_the_guard(v, 0.99)
    hs = np.array([h, h, h, h])
    xs = np.array([xyz, xyz, close, xyz])
    vs = np.array([fast, v, v, -v])
    nsteps = 60
    pos_out, vel_out, forces, trace, status = got = _md(hs, xs, nsteps, BAR_DT, vel=vs)
    print(name, "status", status.tolist())
    assert all(np.all(np.isfinite(o)) for o in (pos_out, vel_out, forces, trace))
    assert status[0, 1] == 1 and 0 < status[0, 0] < nsteps                # some steps, then too fast
    assert tuple(status[2]) == (0, 1)                                     # too fast after the first kick
    assert tuple(status[1]) == (nsteps, 0) and tuple(status[3]) == (nsteps, 0)
    for b in (0, 2):
        s = status[b, 0]
        assert np.all(trace[b, s:] == trace[b, s]) and (s == 0 or not np.all(trace[b, s] == trace[b, s - 1])), b     # rows after the freeze repeat the last completed step's
    assert np.array_equal(pos_out[2], close)                              # frozen before its first drift
    for b in (1, 3):                                                      # a healthy box has the bytes it has alone
        assert _all_same(_md(hs[b], xs[b], nsteps, BAR_DT, vel=vs[b]), [o[b] for o in got]), b
    # the mirror freezes both at the same steps
    assert tuple(md_ref.run(h, xyz, nsteps, BAR_DT, vel=fast)["status"]) == tuple(status[0])
    assert tuple(md_ref.run(h, close, nsteps, BAR_DT, vel=v)["status"]) == tuple(status[2])


# -- 8. bit rules -----------------------------------------------------------------------------------
def _batches():
    """One batch per geometry: (cells, positions, velocities)."""
    out = []
    for name in ("ih48_t020", "ic96"):
        hs, xs = scaled_set(name, 5, 0.1, 40)
        out.append((hs, xs, md_ref.maxwell_boltzmann(len(xs), xs.shape[1], BAR_KT, seed=21)))
    return out


LANGEVIN = dict(kT=BAR_KT, gamma=BAR_GAMMA, seed=77)


@pytest.mark.parametrize("k", (0, 1), ids=("small", "general"))
def test_a_batch_equals_the_single_calls_and_a_run_equals_its_halves_bit_for_bit(k):
    hs, xs, vs = _batches()[k]
    streams = np.array([11, 3, 2 ** 40, 5, 0], dtype=np.uint64)
    got = _md(hs, xs, 30, BAR_DT, vel=vs, streams=streams, sample_every=3, **LANGEVIN)
    assert got[3].shape == (5, 11, 4) and np.all(got[4] == (30, 0))
    assert _all_same(_md(hs, xs, 30, BAR_DT, vel=vs, streams=streams, sample_every=3, **LANGEVIN), got)          # the same call twice
    for b in range(5):
        alone = _md(hs[b], xs[b], 30, BAR_DT, vel=vs[b], streams=streams[b:b + 1], sample_every=3, **LANGEVIN)
        assert _all_same(alone, [o[b] for o in got]), b
    assert _all_same(_md(hs[2:], xs[2:], 30, BAR_DT, vel=vs[2:], streams=streams[2:], sample_every=3, **LANGEVIN), [o[2:] for o in got])
    # 30 steps = 12 + 18 chained through pos_out, vel_out, pos_ref and step0
    first = _md(hs, xs, 12, BAR_DT, vel=vs, streams=streams, sample_every=3, step0=100, **LANGEVIN)
    second = _md(hs, first[0], 18, BAR_DT, vel=first[1], streams=streams, sample_every=3, step0=112, pos_ref=xs, **LANGEVIN)
    whole = _md(hs, xs, 30, BAR_DT, vel=vs, streams=streams, sample_every=3, step0=100, **LANGEVIN)
    assert _all_same(second[:3], whole[:3])
    assert _same(first[3], whole[3][:, :5]) and _same(second[3], whole[3][:, 4:])
    assert not _same(whole[0], got[0])                                     # another step0: another noise


def test_device_tensors_and_null_outputs_give_the_bits_of_the_host_entry():
    import torch
    from mc_water_ls_mw_amd.dynamics import load_md_library, molecular_dynamics_torch
    dev = torch.device("cuda:0")
    for hs, xs, vs in _batches():
        streams = np.array([4, 9, 1, 7, 2 ** 50], dtype=np.uint64)
        got = _md(hs, xs, 20, BAR_DT, vel=vs, streams=streams, pos_ref=xs + 0.25, **LANGEVIN)
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)       # noqa: E731
        t = molecular_dynamics_torch(to(hs), to(xs), 20, BAR_DT, vel_t=to(vs), streams_t=to(streams.view(np.int64)), pos_ref_t=to(xs + 0.25), **LANGEVIN)
        assert all(v.is_cuda for v in t) and t[3].dtype == torch.float64 and t[4].dtype == torch.int32
        assert _all_same([v.cpu().numpy() for v in t], got)
        L = load_md_library()
        cells, pos, vel, ref = (np.ascontiguousarray(a) for a in (hs, xs, vs, xs + 0.25))
        for keep in range(5):
            outs = [np.zeros_like(o) for o in got]
            ptrs = [o.ctypes.data if j == keep else None for j, o in enumerate(outs)]
            assert L.mw_md_run(len(xs), xs.shape[1], cells.ctypes.data, pos.ctypes.data, vel.ctypes.data, ref.ctypes.data, streams.ctypes.data, 77, 0, 20, 1,
                               BAR_DT, MASS_WATER, BAR_KT, BAR_GAMMA, *ptrs) == 0, L.mw_md_last_error()
            assert _same(outs[keep], got[keep]), keep
        # vel NULL is v = 0, pos_ref NULL is pos
        assert _all_same(_md(hs, xs, 5, BAR_DT, vel=np.zeros_like(xs), pos_ref=xs), _md(hs, xs, 5, BAR_DT))


def _switch_cases():
    """More boxes of each geometry than 1 MiB of scratch holds: (cells, positions, velocities)."""
    out = []
    for name, count in (("ic48_t015", 320), ("ic96", 50)):
        hs, xs = scaled_set(name, count, 0.05, 300)
        out.append((hs, xs, md_ref.maxwell_boltzmann(count, xs.shape[1], BAR_KT, seed=31)))
    return out


SWITCH_STEPS = 70                                                          # more than one launch of 64 steps


def _switch_run(hs, xs, vs):
    return _md(hs, xs, SWITCH_STEPS, BAR_DT, vel=vs, sample_every=7, **LANGEVIN)


def test_chunks_and_slices_do_not_change_a_byte(tmp_path):
    """Fresh processes with 1, 7 and 64 steps per launch of the small geometry, the first with 1 MiB of scratch (several chunks,
    the last one ragged; the streams are then the boxes' indices in the call, not in the chunk), return the bytes of this
    process."""
    from mc_water_ls_mw_amd.dynamics import md_last
    got, fits = [], []
    for hs, xs, vs in _switch_cases():
        got.append(_switch_run(hs, xs, vs))
        last = md_last()
        assert last["chunks"] == 1 and last["boxes_per_chunk"] == len(xs) and last["steps_per_launch"] == (64 if last["small"] else 1)
        fits.append((1 << 20) // last["scratch_bytes_per_box"])
        assert 1 < fits[-1] < len(xs) and len(xs) % fits[-1] != 0
        assert np.all(got[-1][4] == (SWITCH_STEPS, 0))
    for mb, piece in (("1", "1"), ("", "7"), ("", "64")):
        out = tmp_path / f"switch_{piece}.npz"
        env = dict(os.environ, MW_MD_SCRATCH_MB=mb, MW_MD_SLICE=piece)
        res = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], capture_output=True, text=True, timeout=300, env=env)
        assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-3000:])
        z = np.load(out)
        for k in range(2):
            if mb:
                assert int(z[f"boxes_per_chunk{k}"]) == fits[k] and int(z[f"chunks{k}"]) == -(-len(got[k][0]) // fits[k]) >= 2
            else:
                assert int(z[f"chunks{k}"]) == 1
            assert int(z[f"steps_per_launch{k}"]) == (int(piece) if k == 0 else 1)
            assert _all_same([z[f"out{k}_{j}"] for j in range(5)], got[k]), (mb, piece, k)


# -- 9. several workgroups per box ----------------------------------------------------------------
def test_a_box_of_several_workgroups_conserves_energy_as_the_mirror_does():
    h, xyz = load_case("ih1536_t012")
    v0 = md_ref.bar_velocities("ih1536_t012")
    pos_out, vel_out, forces, trace, status = _md(h, xyz, 20, BAR_DT, vel=v0)
    ref = md_ref.run(h, xyz, 20, BAR_DT, vel=v0)
    drift, drift_ref = md_ref.energy_drift(trace), md_ref.energy_drift(ref["trace"])
    bar = md_ref.ENERGY_RATIO_TOL / md_ref.ENERGY_RATIO_MEASURED * drift_ref       # the margin of the ratio as a fraction of the drift
    print("ih1536_t012 drift %.6e mirror %.6e difference %.2e (bar %.2e)" % (drift, drift_ref, abs(drift - drift_ref), bar))
    assert tuple(status) == (20, 0) and abs(drift - drift_ref) <= bar
    e0, _ = _engine(h, xyz)
    e1, f1 = _engine(h, pos_out)
    assert abs(trace[0, 0] - e0) <= RTOL * abs(e0) and abs(trace[-1, 0] - e1) <= RTOL * abs(e1)
    assert np.abs(forces - f1).max() <= F_ATOL


# -- 10. with the engine in the same process ------------------------------------------------------
def _farm(nw=2):
    from mc_water_ls_mw_amd import lattice as lat
    from mc_water_ls_mw_amd.energy import load_boxes
    from mc_water_ls_mw_amd.sweep import MuGrid, WalkerFarm
    z1, z2 = load_golden("ic48"), load_golden("ih48")                      # the boxes of ls_pair48
    boxes = []
    for w in range(nw):
        boxes += [(z1["h"], lat.thermalise(z1["xyz"], 0.06, 760 + w)), (z2["h"], lat.thermalise(z2["xyz"], 0.06, 780 + w))]
    em = load_boxes([b[0] for b in boxes], [b[1] for b in boxes])
    farm = WalkerFarm(em, 2, 200.0, 1.1, grid=MuGrid(101, -400.0, 400.0), weight=np.zeros(101), pressure_au=1.0 / 2.90363081e8)
    farm.options(record=True, samplerun=False, always_switch=True, npt=True, wl_factor=0.05)
    farm.moves(trans_prob=0.5, vol_prob=0.2, dv_max_ang=0.924)
    for w in range(1, nw + 1):
        farm.set_state(w, 1 + (w % 2), farm.initial_mu(w))
    return em, farm


def test_the_engine_and_the_farm_give_what_the_arrays_give():
    em, farm = _farm()
    try:
        farm.sweep(96, seed=41)
        nb = em.num_lattices
        e0 = em.model_energy_batch(1, nb).copy()
        vel = md_ref.maxwell_boltzmann(nb, 48, BAR_KT, seed=9)
        kw = dict(kT=BAR_KT, gamma=BAR_GAMMA, vel=vel, seed=13, sample_every=5)
        pos_f, vel_f, trace_f, status_f = farm.molecular_dynamics(25, BAR_DT, first_global_walker=6, **kw)
        hs = farm.sync_cells()
        pos = np.array([farm.positions(b + 1) for b in range(nb)])
        streams = 6 * 2 + np.arange(nb)                                    # (global walker) * lattices + lattice
        want = _md(hs, pos, 25, BAR_DT, streams=streams, **kw)
        assert pos_f.shape == (2, 2, 48, 3) and trace_f.shape == (2, 2, 6, 4) and status_f.shape == (2, 2, 2)
        assert _same(pos_f.reshape(nb, 48, 3), want[0]) and _same(vel_f.reshape(nb, 48, 3), want[1])
        assert _same(trace_f.reshape(nb, 6, 4), want[3]) and _same(status_f.reshape(nb, 2), want[4]) and np.all(status_f[:, :, 0] == 25)
        assert _all_same(em.molecular_dynamics(1, nb, 25, BAR_DT, streams=streams, **kw), want)
        kw2 = dict(kT=BAR_KT, gamma=BAR_GAMMA, vel=vel[1:3], seed=13, streams=[100, 200])
        assert _all_same(em.molecular_dynamics(2, 2, 10, BAR_DT, **kw2), _md(hs[1:3], pos[1:3], 10, BAR_DT, **kw2))
        # the engine's own boxes are where they were
        assert np.array_equal(em.model_energy_batch(1, nb), e0) and np.array_equal(np.array([farm.positions(b + 1) for b in range(nb)]), pos)
    finally:
        em.energy_deinit()


if __name__ == "__main__":
    # the child of test_chunks_and_slices_do_not_change_a_byte: the switches are set, mw_md_init reads them
    from mc_water_ls_mw_amd.dynamics import md_finalize, md_last
    out = {}
    for k, (hs, xs, vs) in enumerate(_switch_cases()):
        r = _switch_run(hs, xs, vs)
        last = md_last()
        out.update({f"out{k}_{j}": r[j] for j in range(5)})
        out.update({f"chunks{k}": last["chunks"], f"boxes_per_chunk{k}": last["boxes_per_chunk"], f"steps_per_launch{k}": last["steps_per_launch"]})
    md_finalize()
    np.savez(sys.argv[1], **out)
