"""GPU: the Einstein-crystal thermodynamic integration of libmw_ti.so (einstein.einstein_md / _torch, EnergyModule.einstein_md,
WalkerFarm.einstein_free_energies) against the numpy mirror of tests/ti_ref.py, against libmw_md.so, against the closed forms of
the lambda = 1 step, and the bit rules of include/mw_ti.h.

Bars.  After 40 steps at lambda = 0.3 and 0.8: ti_ref.POS_TOL, VEL_TOL, TRACE_TOL and BLOCKS_TOL, ten times the largest deviation
the mirror shows against itself with every F_mW perturbed by +-quench_ref.F_ATOL (measured on the CPU, tests/ti_ref.py;
tests/test_ti_ref.py measures it again).  lambda = 1, NVE: 1e-11 of the amplitude against the matrix power (the mirror itself is
within 1e-12, tests/test_ti_ref.py).  A single point: 4 ulp of |oml F| + |nlk u| per component -- one rounding of the product,
one of the fma and the two of the reference expression.  Stationarity: 5 standard errors of the mean of 49152 independent
chi-square variables of one degree, 5 sqrt(2 / 49152) = 3.2 %, around the Lyapunov values of ti_ref.langevin_stationary.  None of
these figures comes from a device result."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from conftest import load_golden
from boo_ref import scaled_set
from quench_ref import F_ATOL, load_case
import md_ref
import ti_ref
from md_ref import BAR_DT, BAR_GAMMA, BAR_KT, BAR_SEED, BAR_STEPS, MASS_WATER

pytestmark = pytest.mark.gpu

LAMBDAS8 = np.array([0.0, 1.0, 0.3, 0.3, 1.0, 0.0, 0.8, 0.5])
SPRINGS8 = np.array([0.02, 0.03, 0.01, 0.04, 0.005, 0.06, 0.025, 0.015])
STREAMS8 = np.array([11, 3, 2 ** 40, 5, 0, 77, 2 ** 63 + 9, 8], dtype=np.uint64)
LANGEVIN = dict(kT=BAR_KT, gamma=BAR_GAMMA, seed=77)


@pytest.fixture(scope="module", autouse=True)
def _library_lifetime():
    """The libraries are initialised by their first calls here and finalised when this file is done."""
    yield
    from mc_water_ls_mw_amd import dynamics, einstein, quench
    einstein.ti_finalize()
    dynamics.md_finalize()
    quench.quench_finalize()


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _all_same(a, b):
    return all(_same(x, y) for x, y in zip(a, b))


def _ti(*a, **kw):
    from mc_water_ls_mw_amd.einstein import einstein_md
    return einstein_md(*a, **kw)


def _md(*a, **kw):
    from mc_water_ls_mw_amd.dynamics import molecular_dynamics
    return molecular_dynamics(*a, **kw)


def _sequential_blocks(trace, equil, per, nblocks):
    """The block means of a trace with sample_every = 1 as the header forms them: one row after the other, then the division."""
    out = np.zeros(trace.shape[:-2] + (nblocks, 5))
    for j in range(nblocks):
        acc = np.zeros(trace.shape[:-2] + (5,))
        for s in range(equil + j * per, equil + (j + 1) * per):
            acc = acc + trace[..., s + 1, :]
        out[..., j, :] = acc / float(per)
    return out


# -- 1. short trajectories against the mirror ---------------------------------------------------------------------------------
@pytest.mark.parametrize("langevin", (False, True), ids=("nve", "langevin"))
@pytest.mark.parametrize("lam", ti_ref.BAR_LAMBDAS)
@pytest.mark.parametrize("name", ti_ref.TRAJECTORY_CASES)
def test_forty_steps_land_where_the_mirror_lands(name, lam, langevin):
    """equil_steps = 5, block_steps = 7 and sample_every = 3: block, sample and launch boundaries do not coincide."""
    from mc_water_ls_mw_amd.einstein import ti_last
    h, xyz = load_case(name)
    ref = ti_ref.reference(name, langevin, lam)                            # (computed once per process, read-only; sample_every = 1)
    got = _ti(h, ti_ref.bar_sites(name), lam, ti_ref.BAR_SPRING, BAR_STEPS, BAR_DT, BAR_KT if langevin else 0.0, BAR_GAMMA if langevin else 0.0, pos=xyz,
              vel=md_ref.bar_velocities(name), seed=BAR_SEED, streams=[ti_ref.BAR_STREAM], sample_every=3, equil_steps=ti_ref.BAR_EQUIL,
              block_steps=ti_ref.BAR_BLOCK)
    pos_out, vel_out, forces, trace, blocks, status = got
    assert ti_last()["small"] == (len(xyz) <= 64)
    assert tuple(status) == (BAR_STEPS, 0) and trace.shape == (BAR_STEPS // 3 + 1, 5) and blocks.shape == (5, 5)
    dx, dv = float(np.abs(pos_out - ref["pos"]).max()), float(np.abs(vel_out - ref["vel"]).max())
    dt = np.abs(trace - ref["trace"][::3]).max(axis=0)
    db = np.abs(blocks - ref["blocks"]).max(axis=0)
    print(name, lam, "langevin" if langevin else "nve", "max |dx| %.2e (bar %.2e)" % (dx, ti_ref.POS_TOL), "max |dv| %.2e (bar %.2e)" % (dv, ti_ref.VEL_TOL),
          "trace", " ".join("%.2e" % v for v in dt), "bars", " ".join("%.2e" % v for v in ti_ref.TRACE_TOL),
          "blocks", " ".join("%.2e" % v for v in db), "bars", " ".join("%.2e" % v for v in ti_ref.BLOCKS_TOL))
    assert dx <= ti_ref.POS_TOL
    assert dv <= ti_ref.VEL_TOL
    assert np.all(dt <= np.array(ti_ref.TRACE_TOL))
    assert np.all(db <= np.array(ti_ref.BLOCKS_TOL))
    assert np.abs(forces - ref["forces"]).max() <= ti_ref.TRACE_TOL[3] + F_ATOL
    assert trace[0, 2] > 0.01 and trace[0, 4] > 0.0 and not _same(pos_out, np.ascontiguousarray(xyz))


# -- 2. lambda = 0 is libmw_md.so ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("ic64_sheared", "ic65_interstitial"), ids=("small", "general"))
def test_lambda_0_has_the_bytes_of_molecular_dynamics(name):
    h, xyz = load_case(name)
    sites, v0 = ti_ref.bar_sites(name), md_ref.bar_velocities(name)
    for kw in (dict(), LANGEVIN):
        got = _ti(h, sites, 0.0, 0.02, 30, BAR_DT, pos=xyz, vel=v0, streams=[5], sample_every=3, step0=17, equil_steps=4, block_steps=5, **kw)
        want = _md(h, xyz, 30, BAR_DT, vel=v0, streams=[5], sample_every=3, step0=17, pos_ref=sites, **kw)
        assert _same(got[0], want[0]) and _same(got[1], want[1]) and _same(got[2], want[2]) and _same(got[5], want[4])
        assert _same(np.ascontiguousarray(got[3][:, :4]), want[3]) and tuple(got[5]) == (30, 0)
        assert np.all(got[3][:, 4] > 0.0) and got[4].shape == (5, 5)


# -- 3. lambda = 1 in closed form -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("ic64_sheared", "ic65_interstitial"), ids=("small", "general"))
def test_lambda_1_nve_is_the_matrix_power_and_its_energy_is_mw_at_those_positions(name):
    h, xyz = load_case(name)
    sites, v0 = ti_ref.bar_sites(name), md_ref.bar_velocities(name)
    k = ti_ref.BAR_SPRING
    pos_out, vel_out, forces, trace, blocks, status = _ti(h, sites, 1.0, k, 200, BAR_DT, pos=xyz, vel=v0, sample_every=200)
    u, v = ti_ref.nve_exact(xyz - sites, v0, k, BAR_DT, 200)
    amp_u = np.sqrt(((xyz - sites) ** 2 + MASS_WATER / k * v0 ** 2).max())
    amp_v = amp_u * math.sqrt(k / MASS_WATER)
    du, dv = float(np.abs(pos_out - sites - u).max() / amp_u), float(np.abs(vel_out - v).max() / amp_v)
    print(name, "positions %.2e velocities %.2e of the amplitude (bar 1e-11)" % (du, dv))
    assert tuple(status) == (200, 0) and trace.shape == (2, 5)
    assert du <= 1e-11
    assert dv <= 1e-11
    single = _md(h, pos_out, 0, BAR_DT)
    assert trace[-1, 0] == single[3][0, 0] and trace[0, 0] == _md(h, xyz, 0, BAR_DT)[3][0, 0]
    assert np.array_equal(forces, -(1.0 * k) * (pos_out - sites)) and trace[-1, 3] == np.abs(forces).max()


# -- 4. a single point ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("ic48_t015", "ic64_sheared", "ic65_interstitial", "ih96_disordered"))
def test_a_single_point_mixes_the_forces_of_molecular_dynamics_with_the_spring(name):
    h, xyz = load_case(name)
    sites = ti_ref.bar_sites(name)
    lam, k = 0.5, 0.037
    pos_out, vel_out, forces, trace, blocks, status = _ti(h, sites, lam, k, 0, BAR_DT, pos=xyz)
    f_md = _md(h, xyz, 0, BAR_DT)[2]
    u = xyz - sites
    oml, nlk = 1.0 - lam, -(lam * k)
    want = oml * f_md + nlk * u
    ulp = np.abs(forces - want) / np.spacing(np.abs(oml * f_md) + np.abs(nlk * u))
    print(name, "largest distance %.2f ulp of |oml F| + |nlk u| (bar 4)" % ulp.max())
    assert ulp.max() <= 4.0
    assert _same(pos_out, np.ascontiguousarray(xyz)) and np.all(vel_out == 0.0) and tuple(status) == (0, 0) and blocks.shape == (0, 5)
    n = len(xyz)
    c = u.sum(axis=0) / n
    assert trace.shape == (1, 5) and trace[0, 1] == 0.0 and trace[0, 3] == np.abs(forces).max()
    assert abs(trace[0, 2] - (u * u).sum() / n) <= 1e-14 * trace[0, 2] and abs(trace[0, 4] - (c * c).sum()) <= 1e-13 * trace[0, 4] + 1e-30
    # pos NULL: the box starts on its sites, u = 0 and the force is (1 - lambda) F_mW there
    on = _ti(h, sites, lam, k, 0, BAR_DT)
    assert _same(on[0], sites) and on[3][0, 2] == 0.0 and on[3][0, 4] == 0.0 and np.array_equal(on[2], oml * _md(h, sites, 0, BAR_DT)[2])


# -- 5. - 7. bit rules ------------------------------------------------------------------------------------------------------------
def _batch(k):
    """Eight boxes of one geometry: (cells, sites, positions, velocities)."""
    hs, xs = scaled_set(("ih48_t020", "ic96")[k], 8, 0.1, 40)
    sites = xs - np.random.default_rng(17).uniform(-0.2, 0.2, size=xs.shape)
    return hs, np.ascontiguousarray(sites), xs, md_ref.maxwell_boltzmann(len(xs), xs.shape[1], BAR_KT, seed=21)


def _batch_run(hs, sites, xs, vs, nsteps=30, sel=slice(None), **kw):
    full = dict(pos=xs[sel], vel=vs[sel], streams=STREAMS8[sel], sample_every=1, equil_steps=4, block_steps=5, **LANGEVIN)
    full.update(kw)
    return _ti(hs[sel], sites[sel], LAMBDAS8[sel], SPRINGS8[sel], nsteps, BAR_DT, **full)


@pytest.mark.parametrize("k", (0, 1), ids=("small", "general"))
def test_a_batch_of_mixed_lambdas_equals_the_single_calls_and_its_blocks_are_the_sums_of_its_rows(k):
    hs, sites, xs, vs = _batch(k)
    got = _batch_run(hs, sites, xs, vs)
    assert got[3].shape == (8, 31, 5) and got[4].shape == (8, 5, 5) and np.all(got[5] == (30, 0))
    assert _all_same(_batch_run(hs, sites, xs, vs), got)                   # the same call twice
    for b in range(8):
        alone = _batch_run(hs, sites, xs, vs, sel=slice(b, b + 1))
        assert _all_same([o[0] for o in alone], [o[b] for o in got]), b
    assert _all_same(_batch_run(hs, sites, xs, vs, sel=slice(3, 8)), [o[3:] for o in got])
    # the blocks are the sequential sums of the rows, byte for byte, and do not depend on sample_every
    assert _same(got[4], _sequential_blocks(got[3], 4, 5, 5))
    sparse = _batch_run(hs, sites, xs, vs, sample_every=7)
    assert _same(sparse[4], got[4]) and _same(sparse[3], np.ascontiguousarray(got[3][:, ::7])) and _all_same(sparse[:3], got[:3])
    # the boxes with lambda = 0 are molecular dynamics
    for b in (0, 5):
        want = _md(hs[b], xs[b], 30, BAR_DT, vel=vs[b], streams=STREAMS8[b:b + 1], pos_ref=sites[b], **LANGEVIN)
        assert _same(got[0][b], want[0]) and _same(got[1][b], want[1]) and _same(got[2][b], want[2]) and _same(np.ascontiguousarray(got[3][b, :, :4]), want[3])
    # and those with lambda = 1 feel no mW force
    for b in (1, 4):
        assert np.array_equal(got[2][b], -(1.0 * SPRINGS8[b]) * (got[0][b] - sites[b]))


@pytest.mark.parametrize("k", (0, 1), ids=("small", "general"))
def test_a_run_equals_its_halves_and_device_pointers_the_host_entry_bit_for_bit(k):
    import torch
    from mc_water_ls_mw_amd.einstein import einstein_md_torch
    hs, sites, xs, vs = _batch(k)
    # 30 steps = 12 + 18 chained through pos_out, vel_out and step0 (blocks belong to a call)
    whole = _batch_run(hs, sites, xs, vs, sample_every=3, step0=100)
    first = _batch_run(hs, sites, xs, vs, nsteps=12, sample_every=3, step0=100)
    second = _batch_run(hs, sites, first[0], first[1], nsteps=18, sample_every=3, step0=112)
    assert _all_same(second[:3], whole[:3]) and _same(second[5], np.array([[18, 0]] * 8, dtype=np.int32))
    assert _same(first[3], whole[3][:, :5]) and _same(second[3], whole[3][:, 4:])
    assert not _same(whole[0], _batch_run(hs, sites, xs, vs, sample_every=3)[0])        # another step0: another noise
    # device pointers
    dev = torch.device("cuda:0")
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)       # noqa: E731
    t = einstein_md_torch(to(hs), to(sites), to(LAMBDAS8), to(SPRINGS8), 30, BAR_DT, pos_t=to(xs), vel_t=to(vs), streams_t=to(STREAMS8.view(np.int64)),
                          sample_every=3, step0=100, equil_steps=4, block_steps=5, **LANGEVIN)
    assert all(v.is_cuda for v in t) and t[3].dtype == torch.float64 and t[5].dtype == torch.int32
    assert _all_same([v.cpu().numpy() for v in t], whole)
    # pos NULL and vel NULL through both entries
    a = _ti(hs, sites, LAMBDAS8, SPRINGS8, 10, BAR_DT, streams=STREAMS8, equil_steps=0, block_steps=5, **LANGEVIN)
    b = einstein_md_torch(to(hs), to(sites), to(LAMBDAS8), to(SPRINGS8), 10, BAR_DT, streams_t=to(STREAMS8.view(np.int64)), equil_steps=0, block_steps=5,
                          **LANGEVIN)
    assert _all_same([v.cpu().numpy() for v in b], a)
    assert _all_same(_ti(hs, sites, LAMBDAS8, SPRINGS8, 10, BAR_DT, pos=sites, vel=np.zeros_like(sites), streams=STREAMS8, equil_steps=0, block_steps=5,
                         **LANGEVIN), a)


def _switch_cases():
    """More boxes of each geometry than 1 MiB of scratch holds: (cells, sites, positions, velocities, lambdas, springs)."""
    out = []
    for name, count in (("ic48_t015", 320), ("ic96", 50)):
        hs, xs = scaled_set(name, count, 0.05, 300)
        sites = np.ascontiguousarray(xs - np.random.default_rng(19).uniform(-0.2, 0.2, size=xs.shape))
        out.append((hs, sites, xs, md_ref.maxwell_boltzmann(count, xs.shape[1], BAR_KT, seed=31), np.resize(LAMBDAS8, count), np.resize(SPRINGS8, count)))
    return out


SWITCH_STEPS = 70                                                          # more than one launch of 64 steps


def _switch_run(hs, sites, xs, vs, lambdas, springs):
    return _ti(hs, sites, lambdas, springs, SWITCH_STEPS, BAR_DT, pos=xs, vel=vs, sample_every=7, equil_steps=5, block_steps=9, **LANGEVIN)


def test_chunks_and_slices_do_not_change_a_byte(tmp_path):
    """A fresh process with one step per launch of the small geometry and 1 MiB of scratch (several chunks, the last one ragged;
    the streams are then the boxes' indices in the call, not in the chunk, and the block accumulators cross 70 launches) returns
    the bytes of this process with its 64 steps per launch and one chunk."""
    from mc_water_ls_mw_amd.einstein import ti_last
    got, fits = [], []
    for case in _switch_cases():
        got.append(_switch_run(*case))
        last = ti_last()
        assert last["chunks"] == 1 and last["boxes_per_chunk"] == len(case[0]) and last["steps_per_launch"] == (64 if last["small"] else 1)
        fits.append((1 << 20) // last["scratch_bytes_per_box"])
        assert 1 < fits[-1] < len(case[0]) and len(case[0]) % fits[-1] != 0
        assert np.all(got[-1][5] == (SWITCH_STEPS, 0)) and got[-1][4].shape[1:] == (7, 5)
    out = tmp_path / "switch.npz"
    env = dict(os.environ, MW_TI_SCRATCH_MB="1", MW_TI_SLICE="1")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-3000:])
    z = np.load(out)
    for k in range(2):
        assert int(z[f"boxes_per_chunk{k}"]) == fits[k] and int(z[f"chunks{k}"]) == -(-len(got[k][0]) // fits[k]) >= 2
        assert int(z[f"steps_per_launch{k}"]) == 1
        assert _all_same([z[f"out{k}_{j}"] for j in range(6)], got[k]), k


# -- 8. the stationary state of the Einstein crystal ---------------------------------------------------------------------------
def test_the_einstein_crystal_settles_at_the_lyapunov_values():
    """256 boxes of 64 sites at lambda = 1, streams 0..255, k = 0.02, 250 K, gamma = 1 / (100 fs), 2000 steps of 5 fs (100 relaxation
    times) from the sites at rest: 49152 independent coordinates.  The means of k u^2 / kT and m v^2 / kT from pos_out and vel_out
    alone lie within 5 standard errors, 5 sqrt(2 / 49152) = 3.2 %, of the stationary values of the discrete step."""
    h, xyz = load_case("ic64_sheared")
    nb, n, k = 256, 64, 0.02
    pos_out, vel_out, forces, trace, blocks, status = _ti(np.tile(h, (nb, 1, 1)), np.tile(xyz, (nb, 1, 1)), 1.0, k, 2000, BAR_DT, BAR_KT, BAR_GAMMA, seed=11,
                                                          streams=np.arange(nb), sample_every=2000, equil_steps=1000, block_steps=500)
    assert np.all(status == (2000, 0)) and blocks.shape == (nb, 2, 5)
    u2, v2, _ = ti_ref.langevin_stationary(k, BAR_DT, BAR_KT, BAR_GAMMA)
    u = pos_out - xyz
    se = math.sqrt(2.0 / (3 * n * nb))
    got_u, got_v = float((u * u).mean()), float((vel_out * vel_out).mean())
    print("k <u^2> / kT = %.5f (Lyapunov %.5f), m <v^2> / kT = %.5f (Lyapunov %.5f), 5 standard errors %.4f"
          % (k * got_u / BAR_KT, k * u2 / BAR_KT, MASS_WATER * got_v / BAR_KT, MASS_WATER * v2 / BAR_KT, 5.0 * se))
    assert 3 * n * nb == 49152
    assert abs(got_u / u2 - 1.0) <= 5.0 * se
    assert abs(got_v / v2 - 1.0) <= 5.0 * se
    assert np.allclose(trace[:, 1, 2], (u * u).sum(axis=(1, 2)) / n, rtol=1e-13, atol=0)


# -- 9. coinciding molecules that no longer interact ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("ic48_t015", "ic65_interstitial"), ids=("small", "general"))
def test_two_molecules_on_one_point_at_lambda_1_stay_out_of_the_state(name):
    """Box 1 of four starts with molecule 1 on molecule 0 at lambda = 1: E_mW and F_mW of it are evaluated (and are what they are),
    F_tot is the springs' alone, and the state stays finite; the other boxes have the bytes they have alone, and the next call
    passes.  Everything here is ordinary arithmetic on finite positions: no kernel forms an address from a distance."""
    h, xyz = load_case(name)
    sites, v0 = ti_ref.bar_sites(name), md_ref.bar_velocities(name)
    on_top = np.array(xyz)
    on_top[1] = on_top[0]
    hs, ss = np.array([h] * 4), np.array([sites] * 4)
    xs, vs = np.array([xyz, on_top, xyz, xyz]), np.array([v0, v0, -v0, v0])
    lams, ks = np.array([0.3, 1.0, 1.0, 0.0]), np.array([0.02, 0.02, 0.03, 0.02])
    kw = dict(pos=xs, vel=vs, streams=np.arange(4), sample_every=4, equil_steps=2, block_steps=6, **LANGEVIN)
    got = _ti(hs, ss, lams, ks, 20, BAR_DT, **kw)
    pos_out, vel_out, forces, trace, blocks, status = got
    print(name, "status", status.tolist(), "E_mW of the box", trace[1, 0, 0])
    assert status[1, 1] == 1 or (tuple(status[1]) == (20, 0) and np.all(np.isfinite(pos_out[1])))
    assert np.all(np.isfinite(pos_out)) and np.all(np.isfinite(vel_out)) and np.all(np.isfinite(forces))
    if not status[1, 1]:
        assert np.array_equal(forces[1], -(1.0 * ks[1]) * (pos_out[1] - sites))
    for b in (0, 2, 3):
        alone = _ti(hs[b], ss[b], lams[b], ks[b], 20, BAR_DT, pos=xs[b], vel=vs[b], streams=[b], sample_every=4, equil_steps=2, block_steps=6, **LANGEVIN)
        assert _all_same(alone, [o[b] for o in got]) and tuple(status[b]) == (20, 0), b
    again = _ti(hs, ss, lams, ks, 20, BAR_DT, **kw)
    assert _all_same([o[[0, 2, 3]] for o in again], [o[[0, 2, 3]] for o in got])


@pytest.mark.parametrize("name", ("ic48_t015", "ic65_interstitial"), ids=("small", "general"))
def test_a_frozen_box_fills_its_blocks_with_its_last_row(name):
    """Box 1 has two molecules 0.5 bohr apart at lambda = 0.3 (the case of the molecular-dynamics suite): the first kick is beyond
    the guard and the box is frozen before its first drift, as the mirror's is.  Its trace repeats the row of step 0 and every
    block is that row added block_steps times, over 70 steps (two launches of the small geometry); box 0 is healthy and has the
    bytes it has alone.  The guard is ordinary arithmetic: nothing here is out of range for any kernel."""
    h, xyz = load_case(name)
    sites = ti_ref.bar_sites(name)
    close = np.array(xyz)
    close[1] = close[0] + np.array([0.5, 0.0, 0.0])
    kw = dict(sample_every=1, equil_steps=3, block_steps=8)
    got = _ti(np.array([h, h]), np.array([sites, sites]), 0.3, 0.02, 70, BAR_DT, pos=np.array([xyz, close]), vel=np.array([md_ref.bar_velocities(name)] * 2), **kw)
    pos_out, vel_out, forces, trace, blocks, status = got
    assert tuple(status[0]) == (70, 0) and tuple(status[1]) == (0, 1) and blocks.shape == (2, 8, 5)
    assert tuple(ti_ref.run(h, sites, 0.3, 0.02, 3, BAR_DT, pos=close, vel=md_ref.bar_velocities(name))["status"]) == (0, 1)
    assert np.array_equal(pos_out[1], close) and np.all(trace[1] == trace[1, 0]) and np.all(np.isfinite(trace[1]))
    assert _same(blocks, _sequential_blocks(trace, 3, 8, 8))
    alone = _ti(h, sites, 0.3, 0.02, 70, BAR_DT, pos=xyz, vel=md_ref.bar_velocities(name), **kw)
    assert _all_same(alone, [o[0] for o in got])


# -- 10. with the engine in the same process ------------------------------------------------------------------------------------
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


def test_the_engine_and_the_farm_integrate_what_the_arrays_integrate():
    from mc_water_ls_mw_amd import einstein
    em, farm = _farm()
    try:
        nb = em.num_lattices
        e0 = em.model_energy_batch(1, nb).copy()
        pos = np.array([farm.positions(b + 1) for b in range(nb)])
        hs = farm.sync_cells()
        # the module: a lambda integration of one box from the positions the device holds
        lam, w = einstein.gauss_legendre(4)
        kw = dict(kT=BAR_KT, gamma=BAR_GAMMA, seed=13, equil_steps=10, block_steps=10)
        got = em.einstein_md(2, lam, 0.02, 50, BAR_DT, **kw)
        want = _ti(np.repeat(hs[1:2], 4, axis=0), np.repeat(pos[1:2], 4, axis=0), lam, 0.02, 50, BAR_DT, **kw)
        assert got[3].shape == (4, 51, 5) and got[4].shape == (4, 4, 5) and _all_same(got, want)
        # the farm
        kT = 100.0 * md_ref.KELVIN
        args = dict(nodes=4, nsteps=60, equil_steps=20, block_steps=10, seed=3)
        F, err, f_ti = farm.einstein_free_energies(kT, **args)
        assert F.shape == (2, 2) and err.shape == (2, 2) and f_ti.shape == (2,)
        assert np.all(np.isfinite(F)) and np.all(np.isfinite(err)) and np.all(err > 0.0) and np.allclose(f_ti, F.mean(axis=0), rtol=1e-15)
        print("F", F.tolist(), "err", err.tolist())
        again = farm.einstein_free_energies(kT, **args)
        assert _all_same(again, (F, err, f_ti))                            # the same seed: the same bytes
        other = farm.einstein_free_energies(kT, spring=0.02, **dict(args, seed=4))
        assert not _same(other[0], F)
        # the engine's own boxes are where they were
        assert np.array_equal(em.model_energy_batch(1, nb), e0) and np.array_equal(np.array([farm.positions(b + 1) for b in range(nb)]), pos)
    finally:
        em.energy_deinit()


if __name__ == "__main__":
    # the child of test_chunks_and_slices_do_not_change_a_byte: the switches are set, mw_ti_init reads them
    from mc_water_ls_mw_amd.einstein import ti_finalize, ti_last
    out = {}
    for k, case in enumerate(_switch_cases()):
        r = _switch_run(*case)
        last = ti_last()
        out.update({f"out{k}_{j}": r[j] for j in range(6)})
        out.update({f"chunks{k}": last["chunks"], f"boxes_per_chunk{k}": last["boxes_per_chunk"], f"steps_per_launch{k}": last["steps_per_launch"]})
    ti_finalize()
    np.savez(sys.argv[1], **out)
