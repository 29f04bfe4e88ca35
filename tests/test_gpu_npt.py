"""GPU: the constant-pressure molecular dynamics of libmw_npt.so (npt.molecular_dynamics_npt / _torch,
EnergyModule.molecular_dynamics_npt, WalkerFarm.molecular_dynamics_npt) against libmw_md.so, against the numpy mirror of
tests/npt_ref.py, against the engine's virial, and the bit rules of include/mw_npt.h.

Bars.  Every one is npt_ref's: ten times the spread the mirror shows against itself with its forces perturbed by +-F_ATOL,
measured on the CPU (tests/test_npt_ref.py measures them again); the ensemble's is 5 standard errors plus the recorded Euler bias.
None comes from a device result."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from boo_ref import scaled_set
from quench_ref import load_case
import lib_cells_cases
import md_ref
import npt_ref
from md_ref import BAR_DT, BAR_GAMMA, BAR_KT, BAR_SEED, BAR_STEPS, MASS_WATER

pytestmark = pytest.mark.gpu

NAMES = ("pos", "vel", "forces", "cell", "ref", "trace", "status")


@pytest.fixture(scope="module", autouse=True)
def _library_lifetime():
    """The libraries are initialised by their first calls here and finalised when this file is done."""
    yield
    from mc_water_ls_mw_amd import dynamics, npt
    npt.npt_finalize()
    dynamics.md_finalize()


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _all_same(a, b):
    return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))


def _npt(*a, **kw):
    from mc_water_ls_mw_amd.npt import molecular_dynamics_npt
    return molecular_dynamics_npt(*a, **kw)


def _md(*a, **kw):
    from mc_water_ls_mw_amd.dynamics import molecular_dynamics
    return molecular_dynamics(*a, **kw)


def _batches():
    """One batch per geometry: (cells, positions, velocities)."""
    out = []
    for name in ("ih48_t020", "ic96"):
        hs, xs = scaled_set(name, 5, 0.1, 40)
        out.append((hs, xs, md_ref.maxwell_boltzmann(len(xs), xs.shape[1], BAR_KT, seed=21)))
    return out


LANGEVIN = dict(kT=BAR_KT, gamma=BAR_GAMMA, seed=77)
BARO = dict(pressure=npt_ref.BAR_PRESSURE, tau_p=npt_ref.BAR_TAU_P, beta_T=npt_ref.BAR_BETA_T)


# -- 1. without the barostat: libmw_md.so, byte for byte ---------------------------------------------
@pytest.mark.parametrize("langevin", (False, True), ids=("nve", "langevin"))
@pytest.mark.parametrize("k", (0, 1), ids=("small", "general"))
def test_without_the_barostat_the_bytes_are_those_of_mw_md_run(k, langevin):
    hs, xs, vs = _batches()[k]
    streams = np.array([11, 3, 2 ** 40, 5, 0], dtype=np.uint64)
    kw = dict(vel=vs, streams=streams, sample_every=3, step0=17, pos_ref=xs + 0.25, **(LANGEVIN if langevin else {}))
    want = _md(hs, xs, 30, BAR_DT, **kw)
    pos, vel, forces, cells, ref, trace, status = _npt(hs, xs, 30, BAR_DT, baro_every=0, pressure=1e-3, **kw)
    assert _same(pos, want[0]) and _same(vel, want[1]) and _same(forces, want[2]) and _same(status, want[4]) and np.all(status == (30, 0))
    assert trace.shape == (5, 11, 6) and _same(np.ascontiguousarray(trace[:, :, :4]), want[3])
    assert _same(cells, np.ascontiguousarray(hs)) and _same(ref, xs + 0.25)
    vol = np.abs(np.linalg.det(hs))
    assert np.all(np.abs(trace[:, :, 4] - vol[:, None]) <= 1e-13 * vol[:, None]) and np.all(trace[:, :, 4] == trace[:, :1, 4])
    assert not _same(pos, np.ascontiguousarray(xs))


# -- 2. the single point: the virial -----------------------------------------------------------------
def _engine_virial(h, xyz):
    from mc_water_ls_mw_amd.energy import load_boxes
    em = load_boxes([h], [xyz])
    try:
        _, _, vir = em.forces_batch()
        return float(np.trace(vir[0]))
    finally:
        em.energy_deinit()


@pytest.mark.parametrize("name", npt_ref.POINT_CASES)
def test_the_pressure_of_a_single_point_is_the_mirrors_and_the_engines_virial(name):
    """nsteps = 0: P 3 V - 2 K is W.  Orthorhombic (ic48_t015, ic96, ih1536_t012 ...) and triclinic (ic64_sheared,
    ic65_interstitial) cells, both geometries."""
    from mc_water_ls_mw_amd.npt import npt_last
    h, xyz = load_case(name)
    n = len(xyz)
    vel = md_ref.maxwell_boltzmann(1, n, BAR_KT, seed=3)[0]
    pos, vel_out, forces, cell, ref, trace, status = _npt(h, xyz, 0, BAR_DT, vel=vel, baro_every=1, **BARO)
    assert trace.shape == (1, 6) and tuple(status) == (0, 0) and npt_last()["small"] == (n <= 64)
    assert _same(pos, np.ascontiguousarray(xyz)) and _same(vel_out, vel) and _same(cell, np.ascontiguousarray(h)) and _same(ref, np.ascontiguousarray(xyz))
    e, k, _, _, vol, p = trace[0]
    w = p * 3.0 * vol - 2.0 * k
    e_ref, f_ref, w_ref = npt_ref.point(name)
    w_eng = _engine_virial(h, xyz)
    slack = 4.0 * np.spacing(2.0 * k + abs(w))                                # forming W back from P
    print(name, n, "W %.12e mirror %.12e engine %.12e: %.2e %.2e (bar %.2e)" % (w, w_ref, w_eng, abs(w - w_ref), abs(w - w_eng), npt_ref.W_TOL))
    assert abs(vol - abs(np.linalg.det(h))) <= 1e-13 * vol and abs(k - 0.5 * MASS_WATER * float((vel * vel).sum())) <= 1e-13 * k
    assert abs(e - e_ref) <= 1e-10 * abs(e_ref) and np.abs(forces - f_ref).max() <= 1e-10
    assert abs(w - w_ref) <= npt_ref.W_TOL + slack
    assert abs(w - w_eng) <= npt_ref.W_TOL + slack


@pytest.mark.parametrize("label", ("n96_three_cells", "n64_small"))
def test_the_virial_of_the_cell_layers_gas_boxes_is_the_mirrors(label):
    """The boxes of tests/lib_cells_cases.py (an orthorhombic, a flat and a triclinic cell; molecules outside the cell): dense
    gases with W of some hundred Hartree, held to the same absolute bar."""
    cells, xs = lib_cells_cases.CASES[label]()
    scale = md_ref.A_SIGMA * (1.0 + 1e-6) / lib_cells_cases.RC                # their cells are sized in units of another radius
    cells, xs = cells * max(scale, 1.0), xs * max(scale, 1.0)
    _, _, _, _, _, trace, status = _npt(cells, xs, 0, BAR_DT, baro_every=0)
    for b, (h, xyz) in enumerate(zip(cells, xs)):
        e_ref, _, w_ref = npt_ref.energy_forces_virial(h, xyz)
        w = trace[b, 0, 5] * 3.0 * trace[b, 0, 4]
        print(label, b, "E %.9e W %.12e mirror %.12e: %.2e (bar %.2e)" % (trace[b, 0, 0], w, w_ref, abs(w - w_ref), npt_ref.W_TOL))
        assert abs(trace[b, 0, 0] - e_ref) <= 1e-10 * abs(e_ref) and abs(w - w_ref) <= npt_ref.W_TOL + 4.0 * np.spacing(abs(w))


# -- 3. trajectories against the mirror ------------------------------------------------------------
def _hold_to(got, ref, label):
    pos, vel, forces, cell, refp, trace, status = got
    d = dict(pos=float(np.abs(pos - ref["pos"]).max()), vel=float(np.abs(vel - ref["vel"]).max()), cell=float(np.abs(cell - ref["cell"]).max()),
             ref=float(np.abs(refp - ref["ref"]).max()))
    dt = np.abs(trace - ref["trace"]).max(axis=0)
    print(label, "status", tuple(status), "pos %.2e (bar %.2e) vel %.2e (bar %.2e) cell %.2e (bar %.2e)" % (d["pos"], npt_ref.POS_TOL, d["vel"], npt_ref.VEL_TOL,
                                                                                                          d["cell"], npt_ref.CELL_TOL),
          "trace", " ".join("%.2e" % v for v in dt), "bars", " ".join("%.2e" % v for v in npt_ref.TRACE_TOL))
    assert tuple(status) == tuple(ref["status"])
    assert d["pos"] <= npt_ref.POS_TOL and d["ref"] <= npt_ref.POS_TOL
    assert d["vel"] <= npt_ref.VEL_TOL
    assert d["cell"] <= npt_ref.CELL_TOL
    assert np.all(dt <= np.array(npt_ref.TRACE_TOL))


@pytest.mark.parametrize("every", npt_ref.BAR_BARO)
@pytest.mark.parametrize("langevin", (False, True), ids=("deterministic", "langevin"))
@pytest.mark.parametrize("name", md_ref.TRAJECTORY_CASES)
def test_forty_steps_with_the_barostat_land_where_the_mirror_lands(name, langevin, every):
    h, xyz = load_case(name)
    ref = npt_ref.reference(name, langevin, every)                             # (computed once per process, read-only)
    got = _npt(h, xyz, BAR_STEPS, BAR_DT, vel=md_ref.bar_velocities(name), streams=[3], **npt_ref.bar_kwargs(langevin, every))
    _hold_to(got, ref, "%s %s every %d" % (name, "langevin" if langevin else "deterministic", every))
    assert tuple(got[6]) == (BAR_STEPS, 0) and abs(got[5][-1, 4] / got[5][0, 4] - 1.0) > 1e-4 and not _same(got[3], np.ascontiguousarray(h))


@pytest.mark.parametrize("name", ("ic48_t015", "ic96"), ids=("small", "general"))
def test_steps_and_step0_that_are_no_multiples_of_baro_every(name):
    """23 steps from step index 7 with the barostat every 5: applications after the steps 9, 14, 19, 24 and 29 -- the third, 8th, ...
    of the call --, sampled every 4."""
    h, xyz = load_case(name)
    kw = dict(vel=md_ref.bar_velocities(name), step0=7, sample_every=4, **npt_ref.bar_kwargs(True, 5))
    ref = npt_ref.run(h, xyz, 23, BAR_DT, stream=6, **kw)
    _hold_to(_npt(h, xyz, 23, BAR_DT, streams=[6], **kw), ref, name)
    # one step less ends before the last application: another cell
    short = npt_ref.run(h, xyz, 22, BAR_DT, stream=6, **kw)
    assert not np.array_equal(short["cell"], ref["cell"])
    _hold_to(_npt(h, xyz, 22, BAR_DT, streams=[6], **kw), short, name + " 22 steps")


# -- 4. the grid's edges ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", (0, 1), ids=("shrinking", "expanding"))
def test_a_width_that_crosses_a_multiple_of_the_cutoff_changes_nothing_but_the_grid(case):
    """ic96 scaled until a width lies 0.5 % from a multiple of a sigma (1 + 1e-9) and driven across it (tests/test_npt_ref.py checks
    that the mirror crosses): the device's grid changes on the way, the mirror has none."""
    from mc_water_ls_mw_amd.npt import npt_plan
    axis, multiple, margin, pressure = npt_ref.EDGE_CASES[case]
    h, xyz = npt_ref.at_a_grid_edge("ic96", axis, multiple, margin)
    ref = npt_ref.edge_reference(axis, multiple, margin, pressure)
    got = _npt(h, xyz, BAR_STEPS, BAR_DT, vel=md_ref.bar_velocities("ic96"), pressure=pressure, tau_p=npt_ref.BAR_TAU_P, beta_T=npt_ref.BAR_BETA_T,
               baro_every=1)
    g0, g1 = npt_plan(96, h), npt_plan(96, got[3])
    print("grid", [g0[k] for k in ("g1", "g2", "g3")], "->", [g1[k] for k in ("g1", "g2", "g3")])
    assert g1["g%d" % (axis + 1)] - g0["g%d" % (axis + 1)] == (-1 if case == 0 else 1)
    _hold_to(got, ref, "ic96 at the edge, axis %d" % axis)


@pytest.mark.parametrize("n", (4, 65), ids=("small", "general"))
def test_a_cell_that_would_fall_below_the_cutoff_freezes_its_box_with_status_2(n):
    h, xyz = npt_ref.narrow_gas(n)
    kw = dict(pressure=100.0 * npt_ref.ATM, tau_p=npt_ref.BAR_TAU_P, beta_T=npt_ref.BAR_BETA_T, baro_every=3, step0=1)
    ref = npt_ref.run(h, xyz, 10, BAR_DT, **kw)
    pos, vel, forces, cell, refp, trace, status = _npt(h, xyz, 10, BAR_DT, **kw)
    assert tuple(ref["status"]) == (2, 2) and tuple(status) == (2, 2)
    assert _same(cell, np.ascontiguousarray(h)) and _same(pos, xyz) and _same(refp, xyz) and not vel.any() and not forces.any()
    assert np.all(trace == trace[0]) and math.isclose(trace[0, 4], abs(np.linalg.det(h)), rel_tol=1e-13) and not trace[:, (0, 1, 2, 3, 5)].any()
    # at a thousandth of that pressure the first application passes: the margin is 1e-6 in the width
    assert tuple(_npt(h, xyz, 3, BAR_DT, **dict(kw, pressure=0.1 * npt_ref.ATM))[6]) == (3, 0)


# -- 5. the guards ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("ic48_t015", "ic65_interstitial"), ids=("small", "general"))
def test_the_guards_freeze_their_boxes_and_leave_the_neighbours_alone(name):
    """Boxes 0, 2 and 3: healthy, with other velocities each.  Box 1: two molecules 0.5 bohr apart, which the first kick sends off:
    the drift guard, status (0, 1).  Then the same call with beta_T / tau_p 10^4 times the bars': cb = 2.6e6 bohr^3 / Hartree against
    |pressure - P| of 10^-6 .. 10^-5 Hartree / bohr^3 makes |de| > 0.3 at the first application, which freezes the healthy boxes with
    status 2 after `every` steps, at the state libmw_md.so reaches there."""
    h, xyz = load_case(name)
    close = np.array(xyz)
    close[1] = close[0] + np.array([0.5, 0.0, 0.0])
    v = md_ref.bar_velocities(name)
    hs, xs, vs = np.array([h, h, h, h]), np.array([xyz, close, xyz, xyz]), np.array([v, v, -v, 0.5 * v])
    every, nsteps = 4, 14
    kw = dict(vel=vs, baro_every=every, sample_every=2, **BARO)
    got = _npt(hs, xs, nsteps, BAR_DT, **kw)
    pos, vel, forces, cell, ref, trace, status = got
    print(name, "status", status.tolist())
    assert all(np.all(np.isfinite(o)) for o in got[:6])
    assert tuple(status[1]) == (0, 1) and np.array_equal(pos[1], close) and np.all(trace[1] == trace[1, 0]) and _same(cell[1], np.ascontiguousarray(h))
    for b in (0, 2, 3):
        assert tuple(status[b]) == (nsteps, 0)
        assert _all_same(_npt(hs[b], xs[b], nsteps, BAR_DT, **dict(kw, vel=vs[b])), [o[b] for o in got]), b      # the bytes it has alone
    # the barostat guard
    stiff = dict(kw, beta_T=1e4 * npt_ref.BAR_BETA_T)
    got = _npt(hs, xs, nsteps, BAR_DT, **stiff)
    pos, vel, forces, cell, ref, trace, status = got
    print(name, "status", status.tolist())
    free = _md(hs, xs, every, BAR_DT, vel=vs, sample_every=2)
    assert tuple(status[1]) == (0, 1)
    for b in (0, 2, 3):
        assert tuple(status[b]) == (every, 2) and tuple(npt_ref.run(h, xs[b], nsteps, BAR_DT, **dict(stiff, vel=vs[b]))["status"]) == (every, 2)
        assert _same(pos[b], free[0][b]) and _same(vel[b], free[1][b]) and _same(forces[b], free[2][b])          # the state before the application
        assert _same(cell[b], np.ascontiguousarray(h)) and _same(ref[b], xs[b])
        rows = every // 2
        assert _same(np.ascontiguousarray(trace[b, :rows + 1, :4]), free[3][b]) and np.all(trace[b, rows:] == trace[b, rows])
        assert not np.all(trace[b, rows] == trace[b, rows - 1])


# -- 6. bit rules -----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (0, 1), ids=("small", "general"))
def test_a_batch_equals_the_single_calls_and_a_run_equals_its_halves_bit_for_bit(k):
    hs, xs, vs = _batches()[k]
    streams = np.array([11, 3, 2 ** 40, 5, 0], dtype=np.uint64)
    kw = dict(streams=streams, sample_every=2, baro_every=5, **LANGEVIN, **BARO)
    got = _npt(hs, xs, 24, BAR_DT, vel=vs, step0=100, **kw)
    assert got[5].shape == (5, 13, 6) and np.all(got[6] == (24, 0)) and not np.any(got[3] == hs)
    assert _all_same(_npt(hs, xs, 24, BAR_DT, vel=vs, step0=100, **kw), got)                                    # the same call twice
    for b in range(5):
        alone = _npt(hs[b], xs[b], 24, BAR_DT, vel=vs[b], step0=100, **dict(kw, streams=streams[b:b + 1]))
        assert _all_same(alone, [o[b] for o in got]), b
    assert _all_same(_npt(hs[2:], xs[2:], 24, BAR_DT, vel=vs[2:], step0=100, **dict(kw, streams=streams[2:])), [o[2:] for o in got])
    # 24 steps = 10 + 14 (the first run ends with the application after step 109) and = 12 + 12 (it ends between two)
    for first_steps in (10, 12):
        a = _npt(hs, xs, first_steps, BAR_DT, vel=vs, step0=100, **kw)
        assert np.all(a[6] == (first_steps, 0)) and not _same(a[4], np.ascontiguousarray(xs))                  # the origin was scaled with the cell
        b = _npt(a[3], a[0], 24 - first_steps, BAR_DT, vel=a[1], step0=100 + first_steps, pos_ref=a[4], **kw)
        assert _all_same(b[:5], got[:5]), first_steps
        r = first_steps // 2
        assert _same(a[5], np.ascontiguousarray(got[5][:, :r + 1])) and _same(b[5], np.ascontiguousarray(got[5][:, r:])), first_steps
    assert not _same(_npt(hs, xs, 24, BAR_DT, vel=vs, step0=101, **kw)[0], got[0])


def test_device_tensors_and_null_outputs_give_the_bits_of_the_host_entry():
    import torch
    from mc_water_ls_mw_amd.npt import load_npt_library, molecular_dynamics_npt_torch
    dev = torch.device("cuda:0")
    for hs, xs, vs in _batches():
        streams = np.array([4, 9, 1, 7, 2 ** 50], dtype=np.uint64)
        kw = dict(baro_every=3, **LANGEVIN, **BARO)
        got = _npt(hs, xs, 20, BAR_DT, vel=vs, streams=streams, pos_ref=xs + 0.25, **kw)
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)       # noqa: E731
        t = molecular_dynamics_npt_torch(to(hs), to(xs), 20, BAR_DT, vel_t=to(vs), streams_t=to(streams.view(np.int64)), pos_ref_t=to(xs + 0.25), **kw)
        assert all(v.is_cuda for v in t) and t[5].dtype == torch.float64 and t[6].dtype == torch.int32
        assert _all_same([v.cpu().numpy() for v in t], got)
        L = load_npt_library()
        cells, pos, vel, ref = (np.ascontiguousarray(a) for a in (hs, xs, vs, xs + 0.25))
        for keep in range(7):
            outs = [np.zeros_like(o) for o in got]
            ptrs = [o.ctypes.data if j == keep else None for j, o in enumerate(outs)]
            assert L.mw_npt_run(len(xs), xs.shape[1], cells.ctypes.data, pos.ctypes.data, vel.ctypes.data, ref.ctypes.data, streams.ctypes.data, 77, 0, 20, 1,
                                BAR_DT, MASS_WATER, BAR_KT, BAR_GAMMA, BARO["pressure"], BARO["tau_p"], BARO["beta_T"], 3, *ptrs) == 0, L.mw_npt_last_error()
            assert _same(outs[keep], got[keep]), keep
        # vel NULL is v = 0, pos_ref NULL is pos
        assert _all_same(_npt(hs, xs, 6, BAR_DT, vel=np.zeros_like(xs), pos_ref=xs, baro_every=2, **BARO), _npt(hs, xs, 6, BAR_DT, baro_every=2, **BARO))


def _switch_cases():
    """More boxes of each geometry than 1 MiB of scratch holds: (cells, positions, velocities)."""
    out = []
    for name, count in (("ic48_t015", 260), ("ic96", 50)):
        hs, xs = scaled_set(name, count, 0.05, 300)
        out.append((hs, xs, md_ref.maxwell_boltzmann(count, xs.shape[1], BAR_KT, seed=31)))
    return out


SWITCH_STEPS = 70                                                          # more than one launch of 64 steps


def _switch_run(hs, xs, vs):
    return _npt(hs, xs, SWITCH_STEPS, BAR_DT, vel=vs, sample_every=7, baro_every=9, step0=5, **LANGEVIN, **BARO)


def test_chunks_and_slices_do_not_change_a_byte(tmp_path):
    """Fresh processes with 3 and 64 steps per launch of the small geometry, the first with 1 MiB of scratch (several chunks, the
    last one ragged), return the bytes of this process (64 steps per launch, 256 MiB)."""
    from mc_water_ls_mw_amd.npt import npt_last
    got, fits = [], []
    for hs, xs, vs in _switch_cases():
        got.append(_switch_run(hs, xs, vs))
        last = npt_last()
        assert last["chunks"] == 1 and last["boxes_per_chunk"] == len(xs) and last["steps_per_launch"] == (64 if last["small"] else 1)
        fits.append((1 << 20) // last["scratch_bytes_per_box"])
        assert 1 < fits[-1] < len(xs) and len(xs) % fits[-1] != 0
        assert np.all(got[-1][6] == (SWITCH_STEPS, 0))
    for mb, piece in (("1", "3"), ("", "64")):
        out = tmp_path / f"switch_{piece}.npz"
        env = dict(os.environ, MW_NPT_SCRATCH_MB=mb, MW_NPT_SLICE=piece)
        res = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], capture_output=True, text=True, timeout=300, env=env)
        assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-3000:])
        z = np.load(out)
        for k in range(2):
            if mb:
                assert int(z[f"boxes_per_chunk{k}"]) == fits[k] and int(z[f"chunks{k}"]) == -(-len(got[k][0]) // fits[k]) >= 2
            else:
                assert int(z[f"chunks{k}"]) == 1
            assert int(z[f"steps_per_launch{k}"]) == (int(piece) if k == 0 else 1)
            assert _all_same([z[f"out{k}_{j}"] for j in range(7)], got[k]), (mb, piece, k)


# -- 7. the ensemble --------------------------------------------------------------------------------
def test_the_barostat_holds_a_dilute_gas_at_the_mean_volume_of_its_law():
    """4096 copies of md_ref.free_gas20 three times as wide (360 x 450 x 90 bohr: 20 molecules 90 bohr apart) at kT = 0.05 Hartree,
    thermostatted, the barostat every step with cb pressure = 0.01 for 2400 steps = 24 relaxation times: npt_ref's free ensemble.
    <V> = (N + 1) kT / pressure within 5 standard errors 1 / sqrt((N + 1) 4096) = 3.4e-3 plus the recorded Euler bias 1.1e-3.  The
    molecules meet now and then: the pair term's B2 at this temperature is -3.80 bohr^3 (npt_ref.second_virial, midpoint rule;
    tests/test_npt_ref.py), so the second-virial correction N B2 / V = 5.2e-6 is far below a tenth of the standard error."""
    h, xyz = md_ref.free_gas20()
    h, xyz = npt_ref.FREE_SCALE * h, npt_ref.FREE_SCALE * xyz
    nb, n = 4096, len(xyz)
    assert n == npt_ref.FREE_N and math.isclose(abs(np.linalg.det(h)), npt_ref.FREE_VOLUME, rel_tol=1e-12)
    se = 1.0 / math.sqrt((n + 1) * nb)
    assert n * abs(npt_ref.FREE_B2_MEASURED) / npt_ref.FREE_VOLUME < 0.1 * se
    dt = npt_ref.FREE_DT
    beta_T = 1.0 / npt_ref.FREE_PRESSURE
    tau_p = beta_T * dt / npt_ref.FREE_CB
    assert math.isclose(npt_ref.barostat_constants(dt, npt_ref.FREE_KT, tau_p, beta_T, 1)[0], npt_ref.FREE_CB, rel_tol=1e-12)
    pos, vel, forces, cell, ref, trace, status = _npt(np.tile(h, (nb, 1, 1)), np.tile(xyz, (nb, 1, 1)), npt_ref.FREE_APPLICATIONS, dt,
                                                      pressure=npt_ref.FREE_PRESSURE, kT=npt_ref.FREE_KT, gamma=npt_ref.FREE_GAMMA_DT / dt, tau_p=tau_p,
                                                      beta_T=beta_T, baro_every=1, seed=11, streams=np.arange(1000, 1000 + nb),
                                                      sample_every=npt_ref.FREE_APPLICATIONS)
    vol = trace[:, 1, 4]
    dm, dv = vol.mean() / npt_ref.FREE_VOLUME - 1.0, vol.var() * (n + 1) / npt_ref.FREE_VOLUME ** 2 - 1.0
    print("frozen", int((status[:, 1] != 0).sum()), "mean V / ((N + 1) kT / p) - 1 = %.3e (5 se %.3e + bias %.3e), variance %.3e" % (dm, 5 * se, npt_ref.FREE_BIAS, dv),
          "K / (3 N kT / 2) - 1 = %.3e" % (trace[:, 1, 1].mean() / (1.5 * n * npt_ref.FREE_KT) - 1.0))
    assert np.all(status == (npt_ref.FREE_APPLICATIONS, 0))                    # no box is frozen
    assert np.allclose(vol, np.abs(np.linalg.det(cell)), rtol=1e-13, atol=0)
    assert abs(dm) <= 5.0 * se + npt_ref.FREE_BIAS


# -- 8. physics smoke ---------------------------------------------------------------------------------
def test_an_ice_box_at_one_atmosphere_breathes_as_the_mirrors_does():
    """ic96 at 250 K (mW ice melts at 274 K) and 1 atm, 300 steps of 5 fs, thermostat and barostat: with the same noise the
    thermostat keeps device and mirror together, so V stays inside the mirror's range and E + K + pressure V follows the mirror's
    within the bars measured for this run (npt_ref.SMOKE_*)."""
    h, xyz = load_case(npt_ref.SMOKE_CASE)
    ref = npt_ref.smoke_reference()
    pos, vel, forces, cell, refp, trace, status = _npt(h, xyz, npt_ref.SMOKE_STEPS, BAR_DT, vel=md_ref.bar_velocities(npt_ref.SMOKE_CASE), streams=[3],
                                                       sample_every=npt_ref.SMOKE_EVERY, **npt_ref.bar_kwargs(True, npt_ref.SMOKE_EVERY))
    v, vr = trace[:, 4], ref["trace"][:, 4]
    hd, hr = npt_ref.enthalpy(trace), npt_ref.enthalpy(ref["trace"])
    slope = lambda y: float(np.polyfit(np.arange(len(y)), y, 1)[0])        # noqa: E731
    print("V %.2f .. %.2f (mirror %.2f .. %.2f), max |dV| %.2e (bar %.2e); H trend per row %.3e (mirror %.3e), max |dH| %.2e (bar %.2e)"
          % (v.min(), v.max(), vr.min(), vr.max(), np.abs(v - vr).max(), npt_ref.SMOKE_V_TOL, slope(hd), slope(hr), np.abs(hd - hr).max(), npt_ref.SMOKE_H_TOL))
    assert tuple(status) == (npt_ref.SMOKE_STEPS, 0)
    assert vr.min() - npt_ref.SMOKE_V_TOL <= v.min() and v.max() <= vr.max() + npt_ref.SMOKE_V_TOL
    assert abs(slope(hd) - slope(hr)) * (len(hd) - 1) <= npt_ref.SMOKE_H_TOL
    assert np.abs(hd - hr).max() <= npt_ref.SMOKE_H_TOL


# -- with the engine in the same process -------------------------------------------------------------
def test_the_engine_and_the_farm_give_what_the_arrays_give():
    from test_gpu_md import _farm
    from mc_water_ls_mw_amd.npt import npt_elapsed_ms
    em, farm = _farm()
    try:
        farm.sweep(96, seed=41)
        nb = em.num_lattices
        e0 = em.model_energy_batch(1, nb).copy()
        vel = md_ref.maxwell_boltzmann(nb, 48, BAR_KT, seed=9)
        kw = dict(kT=BAR_KT, gamma=BAR_GAMMA, vel=vel, seed=13, sample_every=5, baro_every=5, tau_p=npt_ref.BAR_TAU_P, beta_T=npt_ref.BAR_BETA_T)
        pos_f, vel_f, cells_f, trace_f, status_f = farm.molecular_dynamics_npt(25, BAR_DT, first_global_walker=6, **kw)
        hs = farm.sync_cells()
        pos = np.array([farm.positions(b + 1) for b in range(nb)])
        streams = 6 * 2 + np.arange(nb)
        want = _npt(hs, pos, 25, BAR_DT, streams=streams, pressure=farm.pressure, **kw)
        assert pos_f.shape == (2, 2, 48, 3) and cells_f.shape == (2, 2, 3, 3) and trace_f.shape == (2, 2, 6, 6) and status_f.shape == (2, 2, 2)
        assert _same(pos_f.reshape(nb, 48, 3), want[0]) and _same(vel_f.reshape(nb, 48, 3), want[1]) and _same(cells_f.reshape(nb, 3, 3), want[3])
        assert _same(trace_f.reshape(nb, 6, 6), want[5]) and _same(status_f.reshape(nb, 2), want[6]) and np.all(status_f[:, :, 0] == 25)
        assert not np.any(cells_f.reshape(nb, 3, 3)[:, 0, 0] == hs[:, 0, 0])
        assert _all_same(em.molecular_dynamics_npt(1, nb, 25, BAR_DT, streams=streams, pressure=farm.pressure, **kw), want)
        t = npt_elapsed_ms()
        assert len(t) == 5 and t[2] > 0.0 and t[4] > 0.0
        # the engine's own boxes and cells are where they were
        assert np.array_equal(em.model_energy_batch(1, nb), e0) and np.array_equal(farm.sync_cells(), hs)
    finally:
        em.energy_deinit()


if __name__ == "__main__":
    # the child of test_chunks_and_slices_do_not_change_a_byte: the switches are set, mw_npt_init reads them
    from mc_water_ls_mw_amd.npt import npt_finalize, npt_last
    out = {}
    for k, (hs, xs, vs) in enumerate(_switch_cases()):
        r = _switch_run(hs, xs, vs)
        last = npt_last()
        out.update({f"out{k}_{j}": r[j] for j in range(7)})
        out.update({f"chunks{k}": last["chunks"], f"boxes_per_chunk{k}": last["boxes_per_chunk"], f"steps_per_launch{k}": last["steps_per_launch"]})
    npt_finalize()
    np.savez(sys.argv[1], **out)
