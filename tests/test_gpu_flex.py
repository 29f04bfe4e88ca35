"""GPU: the per-axis constant-pressure molecular dynamics of libmw_flex.so (flexcell.molecular_dynamics_flex / _torch,
EnergyModule.molecular_dynamics_flex, WalkerFarm.molecular_dynamics_flex) against libmw_md.so and libmw_npt.so (bytes), against
the numpy mirror of tests/flex_ref.py, against the engine's virial tensor, and the bit rules of include/mw_flex.h.

Bars.  Every one is flex_ref's: ten times the spread the mirror shows against itself with its forces perturbed by +-F_ATOL,
measured on the CPU (tests/test_flex_ref.py measures them again); the ensemble's is 5 standard errors plus the recorded Euler
bias.  None comes from a device result."""
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
import flex_ref
import md_ref
import npt_ref
from md_ref import BAR_DT, BAR_GAMMA, BAR_KT, BAR_STEPS, MASS_WATER

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _library_lifetime():
    """The libraries are initialised by their first calls here and finalised when this file is done."""
    yield
    from mc_water_ls_mw_amd import dynamics, flexcell, npt
    flexcell.flex_finalize()
    npt.npt_finalize()
    dynamics.md_finalize()


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _all_same(a, b):
    return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))


def _flex(*a, **kw):
    from mc_water_ls_mw_amd.flexcell import molecular_dynamics_flex
    return molecular_dynamics_flex(*a, **kw)


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
COUPLINGS = flex_ref.BAR_COUPLINGS + (flex_ref.EXTRA_COUPLING,)
IDS = ("aniso", "semi_z", "uniaxial_z", "semi_x")


def _cols(trace, k):
    return np.ascontiguousarray(trace[..., :k])


# -- 1. the isotropic paths: libmw_md.so and libmw_npt.so, byte for byte --------------------------------
@pytest.mark.parametrize("langevin", (False, True), ids=("nve", "langevin"))
@pytest.mark.parametrize("k", (0, 1), ids=("small", "general"))
def test_without_the_barostat_the_bytes_are_those_of_mw_md_run(k, langevin):
    hs, xs, vs = _batches()[k]
    streams = np.array([11, 3, 2 ** 40, 5, 0], dtype=np.uint64)
    kw = dict(vel=vs, streams=streams, sample_every=3, step0=17, pos_ref=xs + 0.25, **(LANGEVIN if langevin else {}))
    want = _md(hs, xs, 30, BAR_DT, **kw)
    for coupling in (0, 1, 3):
        pos, vel, forces, cells, ref, trace, status = _flex(hs, xs, 30, BAR_DT, baro_every=0, pressure=1e-3, coupling=coupling, **kw)
        assert _same(pos, want[0]) and _same(vel, want[1]) and _same(forces, want[2]) and _same(status, want[4]) and np.all(status == (30, 0))
        assert trace.shape == (5, 11, 15) and _same(_cols(trace, 4), want[3])
        assert _same(cells, np.ascontiguousarray(hs)) and _same(ref, xs + 0.25)
    assert not _same(pos, np.ascontiguousarray(xs))


@pytest.mark.parametrize("every", (1, 5))
@pytest.mark.parametrize("langevin", (False, True), ids=("nve", "langevin"))
@pytest.mark.parametrize("k", (0, 1), ids=("small", "general"))
def test_in_coupling_0_the_bytes_are_those_of_mw_npt_run(k, langevin, every):
    hs, xs, vs = _batches()[k]
    streams = np.array([11, 3, 2 ** 40, 5, 0], dtype=np.uint64)
    kw = dict(vel=vs, streams=streams, sample_every=3, step0=17, pos_ref=xs + 0.25, baro_every=every, **(LANGEVIN if langevin else {}), **BARO)
    want = _npt(hs, xs, 30, BAR_DT, **kw)
    for axis in (0, 2):
        got = _flex(hs, xs, 30, BAR_DT, coupling="iso", axis=axis, **kw)
        for j in (0, 1, 2, 3, 4, 6):
            assert _same(got[j], want[j]), j
        assert got[5].shape == (5, 11, 15) and _same(_cols(got[5], 6), want[5])
    assert np.all(want[6] == (30, 0)) and not np.any(want[3] == hs)
    # the tensor's columns agree with the scalar ones: tr P / 3 = P, and the lengths are those of cells_out
    t = got[5]
    assert np.all(np.abs(t[..., 6:9].sum(axis=-1) / 3.0 - t[..., 5]) <= 1e-12 * np.abs(t[..., 6:9]).max())
    assert np.allclose(t[:, -1, 12:], np.linalg.norm(got[3], axis=2), rtol=1e-15, atol=0)


# -- 2. the single point: the virial tensor ----------------------------------------------------------
def _engine_virial(h, xyz):
    from mc_water_ls_mw_amd.energy import load_boxes
    em = load_boxes([h], [xyz])
    try:
        _, _, vir = em.forces_batch()
        return np.array(vir[0], dtype=np.float64)
    finally:
        em.energy_deinit()


@pytest.mark.parametrize("name", npt_ref.POINT_CASES)
def test_the_pressure_tensor_of_a_single_point_is_the_mirrors_and_the_engines_virial(name):
    """nsteps = 0: P_ab V - 2 K_ab is W_ab.  Orthorhombic and triclinic (ic64_sheared, ic65_interstitial) cells, both geometries,
    one and several workgroups per box (ih1536_t012)."""
    from mc_water_ls_mw_amd.flexcell import flex_last, pressure_tensor
    h, xyz = load_case(name)
    n = len(xyz)
    vel = md_ref.maxwell_boltzmann(1, n, BAR_KT, seed=3)[0]
    pos, vel_out, forces, cell, ref, trace, status = _flex(h, xyz, 0, BAR_DT, vel=vel, baro_every=1, coupling="aniso", **BARO)
    assert trace.shape == (1, 15) and tuple(status) == (0, 0) and flex_last()["small"] == (n <= 64)
    assert _same(pos, np.ascontiguousarray(xyz)) and _same(vel_out, vel) and _same(cell, np.ascontiguousarray(h)) and _same(ref, np.ascontiguousarray(xyz))
    want = _npt(h, xyz, 0, BAR_DT, vel=vel, baro_every=1, **BARO)
    assert _same(_cols(trace, 6), want[5]) and _same(forces, want[2])          # fields 0 - 5 are libmw_npt.so's bits
    vol = trace[0, 4]
    kab = 0.5 * MASS_WATER * (vel.T @ vel)
    w = pressure_tensor(trace)[0] * vol - 2.0 * kab
    w_ref = flex_ref.point(name)[2]
    w_eng = _engine_virial(h, xyz)
    slack = 4.0 * np.spacing(2.0 * np.abs(kab).max() + np.abs(w).max())       # forming W_ab back from P_ab
    print(name, n, "largest |W_ab| %.6e: against the mirror %.2e, against the engine %.2e (bar %.2e)" % (np.abs(w).max(), np.abs(w - w_ref).max(),
                                                                                                           np.abs(w - w_eng).max(), flex_ref.W_AB_TOL))
    assert np.abs(w - w_ref).max() <= flex_ref.W_AB_TOL + slack
    assert np.abs(w - w_eng).max() <= flex_ref.W_AB_TOL + slack
    assert abs(np.trace(w) - (trace[0, 5] * 3.0 * vol - 2.0 * trace[0, 1])) <= 8.0 * slack
    assert np.allclose(trace[0, 12:], np.linalg.norm(h, axis=1), rtol=1e-15, atol=0)
    if name in ("ic64_sheared", "ic65_interstitial"):
        assert np.abs(w[np.triu_indices(3, 1)]).min() > 100.0 * flex_ref.W_AB_TOL       # the shears are there to be compared


# -- 3. trajectories against the mirror ------------------------------------------------------------
def _hold_to(got, ref, label):
    pos, vel, forces, cell, refp, trace, status = got
    d = dict(pos=float(np.abs(pos - ref["pos"]).max()), vel=float(np.abs(vel - ref["vel"]).max()), cell=float(np.abs(cell - ref["cell"]).max()),
             ref=float(np.abs(refp - ref["ref"]).max()))
    dt = np.abs(trace - ref["trace"]).max(axis=0)
    print(label, "status", tuple(status), "pos %.2e (bar %.2e) vel %.2e (bar %.2e) cell %.2e (bar %.2e)" % (d["pos"], flex_ref.POS_TOL, d["vel"], flex_ref.VEL_TOL,
                                                                                                          d["cell"], flex_ref.CELL_TOL),
          "trace", " ".join("%.2e" % v for v in dt), "bars", " ".join("%.2e" % v for v in flex_ref.TRACE_TOL))
    assert tuple(status) == tuple(ref["status"])
    assert d["pos"] <= flex_ref.POS_TOL and d["ref"] <= flex_ref.POS_TOL
    assert d["vel"] <= flex_ref.VEL_TOL
    assert d["cell"] <= flex_ref.CELL_TOL
    assert np.all(dt <= np.array(flex_ref.TRACE_TOL))


@pytest.mark.parametrize("every", npt_ref.BAR_BARO)
@pytest.mark.parametrize("langevin", (False, True), ids=("deterministic", "langevin"))
@pytest.mark.parametrize("coupling,axis", COUPLINGS, ids=IDS)
@pytest.mark.parametrize("name", md_ref.TRAJECTORY_CASES)
def test_forty_steps_with_the_barostat_land_where_the_mirror_lands(name, coupling, axis, langevin, every):
    h, xyz = load_case(name)
    ref = flex_ref.reference(name, langevin, every, coupling, axis)            # (computed once per process, read-only)
    got = _flex(h, xyz, BAR_STEPS, BAR_DT, vel=md_ref.bar_velocities(name), streams=[3], coupling=coupling, axis=axis, **npt_ref.bar_kwargs(langevin, every))
    _hold_to(got, ref, "%s coupling %d axis %d %s every %d" % (name, coupling, axis, "langevin" if langevin else "deterministic", every))
    cell = got[3]
    assert tuple(got[6]) == (BAR_STEPS, 0) and abs(got[5][-1, 4] / got[5][0, 4] - 1.0) > 1e-5
    for a in range(3):                                                       # the columns of the cell that moved: those of the groups
        moved = not _same(np.ascontiguousarray(cell[:, a]), np.ascontiguousarray(h[:, a]))
        assert moved == (coupling != flex_ref.UNIAXIAL or a == axis), a


# -- 4. uniaxial: the fixed axes keep their bits ------------------------------------------------------
@pytest.mark.parametrize("name", ("ic64_sheared", "ic65_interstitial"), ids=("small", "general"))
def test_the_fixed_axes_of_a_uniaxial_run_keep_the_bits_of_the_input_after_every_call(name):
    """Three chained calls on a triclinic cell, the barostat every second step, axis 1: columns 0 and 2 of the cell and of
    pos_ref are the input's bytes after each, column 1 moves each time."""
    h, xyz = load_case(name)
    cell, pos, vel, ref = np.array(h), np.array(xyz), md_ref.bar_velocities(name), np.array(xyz)
    for call in range(3):
        out = _flex(cell, pos, 6, BAR_DT, vel=vel, pos_ref=ref, step0=6 * call, baro_every=2, coupling="uniaxial", axis=1, streams=[4], **LANGEVIN, **BARO)
        assert tuple(out[6]) == (6, 0)
        for a in (0, 2):
            assert _same(np.ascontiguousarray(out[3][:, a]), np.ascontiguousarray(h[:, a])), (call, a)
            assert _same(np.ascontiguousarray(out[4][:, a]), np.ascontiguousarray(xyz[:, a])), (call, a)
        assert not _same(np.ascontiguousarray(out[3][:, 1]), np.ascontiguousarray(cell[:, 1])) and not _same(np.ascontiguousarray(out[4][:, 1]), np.ascontiguousarray(ref[:, 1]))
        pos, vel, cell, ref = out[0], out[1], out[3], out[4]


# -- 5. the grid's edges ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", (0, 1), ids=("shrinking", "expanding"))
def test_one_width_that_crosses_a_multiple_of_the_cutoff_changes_that_grid_count_alone(case):
    """ic96 with one axis scaled until its width lies 0.3 % from a multiple of a sigma (1 + 1e-9) and driven across it by the
    uniaxial barostat (tests/test_flex_ref.py checks that the mirror crosses): the device's grid changes along that axis on
    the way and along no other; the mirror has no grid."""
    from mc_water_ls_mw_amd.flexcell import flex_plan
    axis, multiple, margin, pressure = flex_ref.EDGE_CASES[case]
    h, xyz = flex_ref.at_a_grid_edge("ic96", axis, multiple, margin)
    ref = flex_ref.edge_reference(axis, multiple, margin, pressure)
    got = _flex(h, xyz, BAR_STEPS, BAR_DT, vel=md_ref.bar_velocities("ic96"), pressure=pressure, tau_p=npt_ref.BAR_TAU_P, beta_T=npt_ref.BAR_BETA_T,
                baro_every=1, coupling="uniaxial", axis=axis)
    g0, g1 = flex_plan(96, h), flex_plan(96, got[3])
    print("grid", [g0[k] for k in ("g1", "g2", "g3")], "->", [g1[k] for k in ("g1", "g2", "g3")])
    for a in range(3):
        assert g1["g%d" % (a + 1)] - g0["g%d" % (a + 1)] == ((-1 if case == 0 else 1) if a == axis else 0), a
    _hold_to(got, ref, "ic96 at the edge, axis %d" % axis)


# -- 6. the guards ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (4, 65), ids=("small", "general"))
def test_an_axis_that_would_fall_below_the_cutoff_freezes_its_box_with_status_2(n):
    h, xyz = npt_ref.narrow_gas(n)                                            # x is 1e-6 above the cell rule
    kw = dict(pressure=100.0 * npt_ref.ATM, tau_p=npt_ref.BAR_TAU_P, beta_T=npt_ref.BAR_BETA_T, baro_every=3, step0=1)
    for coupling, axis in ((1, 2), (3, 0), (2, 1)):
        ref = flex_ref.run(h, xyz, 10, BAR_DT, coupling=coupling, axis=axis, **kw)
        pos, vel, forces, cell, refp, trace, status = _flex(h, xyz, 10, BAR_DT, coupling=coupling, axis=axis, **kw)
        assert tuple(ref["status"]) == (2, 2) and tuple(status) == (2, 2)
        assert _same(cell, np.ascontiguousarray(h)) and _same(pos, xyz) and _same(refp, xyz) and not vel.any() and not forces.any()
        assert np.all(trace == trace[0]) and math.isclose(trace[0, 4], abs(np.linalg.det(h)), rel_tol=1e-13) and not trace[:, (0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11)].any()
    # with x outside every group the same box shrinks along z and goes on
    got = _flex(h, xyz, 10, BAR_DT, coupling=3, axis=2, **kw)
    assert tuple(got[6]) == (10, 0) and _same(np.ascontiguousarray(got[3][:, :2]), np.ascontiguousarray(h[:, :2])) and got[3][2, 2] < h[2, 2]
    _hold_to(got, flex_ref.run(h, xyz, 10, BAR_DT, coupling=3, axis=2, **kw), "narrow gas, z alone")


@pytest.mark.parametrize("name", ("ic48_t015", "ic65_interstitial"), ids=("small", "general"))
def test_the_guards_freeze_their_boxes_and_leave_the_neighbours_alone(name):
    """Boxes 0, 2 and 3: healthy, with other velocities each.  Box 1: two molecules 0.5 bohr apart, which the first kick sends
    off: the drift guard, status (0, 1).  Then the same call with beta_T 300 times the bars': the largest |de_G| is 0.12 .. 0.7 at the
    first application (the mirror's figures; at least 20 % from MW_FLEX_MAX_DLNL), which freezes the healthy boxes with status 2 after
    `every` steps, at the state libmw_md.so reaches there; what the isotropic stage does with the same step is the mirror's verdict."""
    h, xyz = load_case(name)
    close = np.array(xyz)
    close[1] = close[0] + np.array([0.5, 0.0, 0.0])
    v = md_ref.bar_velocities(name)
    hs, xs, vs = np.array([h, h, h, h]), np.array([xyz, close, xyz, xyz]), np.array([v, v, -v, 0.5 * v])
    every, nsteps = 4, 14
    kw = dict(vel=vs, baro_every=every, sample_every=2, coupling="aniso", **BARO)
    got = _flex(hs, xs, nsteps, BAR_DT, **kw)
    pos, vel, forces, cell, ref, trace, status = got
    print(name, "status", status.tolist())
    assert all(np.all(np.isfinite(o)) for o in got[:6])
    assert tuple(status[1]) == (0, 1) and np.array_equal(pos[1], close) and np.all(trace[1] == trace[1, 0]) and _same(cell[1], np.ascontiguousarray(h))
    for b in (0, 2, 3):
        assert tuple(status[b]) == (nsteps, 0)
        assert _all_same(_flex(hs[b], xs[b], nsteps, BAR_DT, **dict(kw, vel=vs[b])), [o[b] for o in got]), b      # the bytes it has alone
    # the barostat guard
    stiff = dict(kw, beta_T=300.0 * npt_ref.BAR_BETA_T)
    got = _flex(hs, xs, nsteps, BAR_DT, **stiff)
    pos, vel, forces, cell, ref, trace, status = got
    print(name, "status", status.tolist())
    free = _md(hs, xs, every, BAR_DT, vel=vs, sample_every=2)
    assert tuple(status[1]) == (0, 1)
    frozen = 0
    for b in (0, 2, 3):
        want = flex_ref.run(h, xs[b], nsteps, BAR_DT, **dict(stiff, vel=vs[b], coupling=1))
        assert tuple(status[b]) == tuple(want["status"])
        if tuple(status[b]) != (every, 2):
            continue
        frozen += 1
        assert _same(pos[b], free[0][b]) and _same(vel[b], free[1][b]) and _same(forces[b], free[2][b])          # the state before the application
        assert _same(cell[b], np.ascontiguousarray(h)) and _same(ref[b], xs[b])
        rows = every // 2
        assert _same(np.ascontiguousarray(trace[b, :rows + 1, :4]), free[3][b]) and np.all(trace[b, rows:] == trace[b, rows])
        assert not np.all(trace[b, rows] == trace[b, rows - 1])
        iso = tuple(flex_ref.run(h, xs[b], every, BAR_DT, **dict(stiff, vel=vs[b], coupling=0))["status"])
        assert tuple(_flex(hs[b], xs[b], every, BAR_DT, **dict(stiff, vel=vs[b], coupling="iso"))[6]) == iso
    assert frozen == 3


# -- 7. bit rules -----------------------------------------------------------------------------------
@pytest.mark.parametrize("coupling,axis", COUPLINGS[:3], ids=IDS[:3])
@pytest.mark.parametrize("k", (0, 1), ids=("small", "general"))
def test_a_batch_equals_the_single_calls_and_a_run_equals_its_halves_bit_for_bit(k, coupling, axis):
    hs, xs, vs = _batches()[k]
    streams = np.array([11, 3, 2 ** 40, 5, 0], dtype=np.uint64)
    kw = dict(streams=streams, sample_every=2, baro_every=5, coupling=coupling, axis=axis, **LANGEVIN, **BARO)
    got = _flex(hs, xs, 24, BAR_DT, vel=vs, step0=100, **kw)
    assert got[5].shape == (5, 13, 15) and np.all(got[6] == (24, 0)) and not np.any(got[3][:, axis, axis] == hs[:, axis, axis])
    assert _all_same(_flex(hs, xs, 24, BAR_DT, vel=vs, step0=100, **kw), got)                                   # the same call twice
    for b in range(5):
        alone = _flex(hs[b], xs[b], 24, BAR_DT, vel=vs[b], step0=100, **dict(kw, streams=streams[b:b + 1]))
        assert _all_same(alone, [o[b] for o in got]), b
    assert _all_same(_flex(hs[2:], xs[2:], 24, BAR_DT, vel=vs[2:], step0=100, **dict(kw, streams=streams[2:])), [o[2:] for o in got])
    # 24 steps = 10 + 14 (the first run ends with the application after step 109) and = 12 + 12 (it ends between two)
    for first_steps in (10, 12):
        a = _flex(hs, xs, first_steps, BAR_DT, vel=vs, step0=100, **kw)
        assert np.all(a[6] == (first_steps, 0)) and not _same(a[4], np.ascontiguousarray(xs))                  # the origin was scaled with the cell
        b = _flex(a[3], a[0], 24 - first_steps, BAR_DT, vel=a[1], step0=100 + first_steps, pos_ref=a[4], **kw)
        assert _all_same(b[:5], got[:5]), first_steps
        r = first_steps // 2
        assert _same(a[5], np.ascontiguousarray(got[5][:, :r + 1])) and _same(b[5], np.ascontiguousarray(got[5][:, r:])), first_steps
    assert not _same(_flex(hs, xs, 24, BAR_DT, vel=vs, step0=101, **kw)[0], got[0])


def test_device_tensors_and_null_outputs_give_the_bits_of_the_host_entry():
    import torch
    from mc_water_ls_mw_amd.flexcell import load_flex_library, molecular_dynamics_flex_torch
    dev = torch.device("cuda:0")
    for hs, xs, vs in _batches():
        streams = np.array([4, 9, 1, 7, 2 ** 50], dtype=np.uint64)
        kw = dict(baro_every=3, coupling="semi", axis=1, **LANGEVIN, **BARO)
        got = _flex(hs, xs, 20, BAR_DT, vel=vs, streams=streams, pos_ref=xs + 0.25, **kw)
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)       # noqa: E731
        t = molecular_dynamics_flex_torch(to(hs), to(xs), 20, BAR_DT, vel_t=to(vs), streams_t=to(streams.view(np.int64)), pos_ref_t=to(xs + 0.25), **kw)
        assert all(v.is_cuda for v in t) and t[5].dtype == torch.float64 and t[6].dtype == torch.int32
        assert _all_same([v.cpu().numpy() for v in t], got)
        L = load_flex_library()
        cells, pos, vel, ref = (np.ascontiguousarray(a) for a in (hs, xs, vs, xs + 0.25))
        for keep in range(7):
            outs = [np.zeros_like(o) for o in got]
            ptrs = [o.ctypes.data if j == keep else None for j, o in enumerate(outs)]
            assert L.mw_flex_run(len(xs), xs.shape[1], cells.ctypes.data, pos.ctypes.data, vel.ctypes.data, ref.ctypes.data, streams.ctypes.data, 77, 0, 20, 1,
                                 BAR_DT, MASS_WATER, BAR_KT, BAR_GAMMA, BARO["pressure"], BARO["tau_p"], BARO["beta_T"], 3, 2, 1, *ptrs) == 0, L.mw_flex_last_error()
            assert _same(outs[keep], got[keep]), keep
        # vel NULL is v = 0, pos_ref NULL is pos
        assert _all_same(_flex(hs, xs, 6, BAR_DT, vel=np.zeros_like(xs), pos_ref=xs, baro_every=2, **BARO), _flex(hs, xs, 6, BAR_DT, baro_every=2, **BARO))


def _switch_cases():
    """More boxes of each geometry than 1 MiB of scratch holds: (cells, positions, velocities)."""
    out = []
    for name, count in (("ic48_t015", 260), ("ic96", 50)):
        hs, xs = scaled_set(name, count, 0.05, 300)
        out.append((hs, xs, md_ref.maxwell_boltzmann(count, xs.shape[1], BAR_KT, seed=31)))
    return out


SWITCH_STEPS = 70                                                          # more than one launch of 64 steps


def _switch_run(hs, xs, vs):
    return _flex(hs, xs, SWITCH_STEPS, BAR_DT, vel=vs, sample_every=7, baro_every=9, step0=5, coupling="aniso", **LANGEVIN, **BARO)


def test_chunks_and_slices_do_not_change_a_byte(tmp_path):
    """Fresh processes with 3 and 64 steps per launch of the small geometry, the first with 1 MiB of scratch (several chunks, the
    last one ragged), return the bytes of this process (64 steps per launch, 256 MiB)."""
    from mc_water_ls_mw_amd.flexcell import flex_last
    got, fits = [], []
    for hs, xs, vs in _switch_cases():
        got.append(_switch_run(hs, xs, vs))
        last = flex_last()
        assert last["chunks"] == 1 and last["boxes_per_chunk"] == len(xs) and last["steps_per_launch"] == (64 if last["small"] else 1)
        fits.append((1 << 20) // last["scratch_bytes_per_box"])
        assert 1 < fits[-1] < len(xs) and len(xs) % fits[-1] != 0
        assert np.all(got[-1][6] == (SWITCH_STEPS, 0))
    for mb, piece in (("1", "3"), ("", "64")):
        out = tmp_path / f"switch_{piece}.npz"
        env = dict(os.environ, MW_FLEX_SCRATCH_MB=mb, MW_FLEX_SLICE=piece)
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


# -- 8. the ensemble --------------------------------------------------------------------------------
@pytest.mark.parametrize("coupling", (flex_ref.ANISO, flex_ref.SEMI, flex_ref.UNIAXIAL), ids=("aniso", "semi", "uniaxial"))
def test_the_barostat_holds_a_dilute_gas_at_the_mean_and_the_variance_of_its_law(coupling):
    """4096 boxes of the 20 molecules of md_ref.free_gas20 spread over a cube of npt_ref's free volume (244 bohr) at kT = 0.05
    Hartree, thermostatted, the barostat every step with cb pressure = 0.005 for 4 relaxation times of ln V: flex_ref's free
    ensemble.  <V> = (N + 1) kT / pressure and var V = (N + 1) (kT / pressure)^2 within 5 standard errors plus the recorded Euler
    biases; no box is frozen; the shapes diffuse (tests/test_flex_ref.py: in the mirror every length stays above twice the cutoff).
    The second-virial correction is that of tests/test_gpu_npt.py's gas: the volume and the temperature are the same."""
    h0, xyz0 = md_ref.free_gas20()
    side = flex_ref.FREE_SIDE
    h, xyz = np.eye(3) * side, xyz0 / np.diag(h0) * side + np.array([0.0, 0.0, 0.45 * side])
    nb, n = 4096, len(xyz)
    assert n == flex_ref.FREE_N and math.isclose(abs(np.linalg.det(h)), flex_ref.FREE_VOLUME, rel_tol=1e-12)
    se = 1.0 / math.sqrt((n + 1) * nb)
    se_var = math.sqrt((2.0 + 6.0 / (n + 1)) / nb)
    assert n * abs(npt_ref.FREE_B2_MEASURED) / flex_ref.FREE_VOLUME < 0.1 * se
    dt, apps = flex_ref.FREE_DT, flex_ref.FREE_APPLICATIONS[coupling]
    beta_T = 1.0 / flex_ref.FREE_PRESSURE
    tau_p = beta_T * dt / flex_ref.FREE_CB
    assert math.isclose(flex_ref.barostat_constants(dt, flex_ref.FREE_KT, tau_p, beta_T, 1)[0], flex_ref.FREE_CB, rel_tol=1e-12)
    vel = md_ref.maxwell_boltzmann(nb, n, flex_ref.FREE_KT, seed=8)
    pos, vel, forces, cell, ref, trace, status = _flex(np.tile(h, (nb, 1, 1)), np.tile(xyz, (nb, 1, 1)), apps, dt, vel=vel, pressure=flex_ref.FREE_PRESSURE,
                                                       kT=flex_ref.FREE_KT, gamma=flex_ref.FREE_GAMMA_DT / dt, tau_p=tau_p, beta_T=beta_T, baro_every=1, seed=11,
                                                       streams=np.arange(1000, 1000 + nb), sample_every=apps, coupling=coupling, axis=2)
    vol = trace[:, 1, 4]
    dm, dv = vol.mean() / flex_ref.FREE_VOLUME - 1.0, vol.var() * (n + 1) / flex_ref.FREE_VOLUME ** 2 - 1.0
    lengths = trace[:, 1, 12:]
    spread = np.log(lengths).std(axis=0)
    print("coupling", coupling, "frozen", int((status[:, 1] != 0).sum()), "mean V / ((N + 1) kT / p) - 1 = %.3e (5 se %.3e + bias %.3e), variance %.3e (5 se %.3e + bias %.3e)"
          % (dm, 5 * se, flex_ref.FREE_BIAS[coupling], dv, 5 * se_var, flex_ref.FREE_VAR_BIAS[coupling]), "spread of ln L", spread, "smallest length %.1f" % lengths.min(),
          "K / (3 N kT / 2) - 1 = %.3e" % (trace[:, 1, 1].mean() / (1.5 * n * flex_ref.FREE_KT) - 1.0))
    assert np.all(status == (apps, 0))                                         # no box is frozen
    assert np.allclose(vol, np.abs(np.linalg.det(cell)), rtol=1e-13, atol=0) and np.allclose(lengths, np.linalg.norm(cell, axis=2), rtol=1e-15, atol=0)
    assert abs(dm) <= 5.0 * se + flex_ref.FREE_BIAS[coupling]
    assert abs(dv) <= 5.0 * se_var + flex_ref.FREE_VAR_BIAS[coupling]
    if coupling == flex_ref.UNIAXIAL:
        assert np.all(cell[:, 0, 0] == side) and np.all(cell[:, 1, 1] == side) and spread[2] > 0.1
    else:
        assert np.all(spread > 0.1)                                            # the shapes diffuse
    if coupling == flex_ref.SEMI:
        assert np.array_equal(cell[:, 0, 0], cell[:, 1, 1])


# -- 9. with the engine in the same process -----------------------------------------------------------
def test_the_engine_and_the_farm_give_what_the_arrays_give():
    from test_gpu_md import _farm
    from mc_water_ls_mw_amd.flexcell import flex_elapsed_ms, surface_tension
    em, farm = _farm()
    try:
        farm.sweep(96, seed=41)
        nb = em.num_lattices
        e0 = em.model_energy_batch(1, nb).copy()
        vel = md_ref.maxwell_boltzmann(nb, 48, BAR_KT, seed=9)
        kw = dict(kT=BAR_KT, gamma=BAR_GAMMA, vel=vel, seed=13, sample_every=5, baro_every=5, tau_p=npt_ref.BAR_TAU_P, beta_T=npt_ref.BAR_BETA_T,
                  coupling="semi", axis=2)
        pos_f, vel_f, cells_f, trace_f, status_f = farm.molecular_dynamics_flex(25, BAR_DT, first_global_walker=6, **kw)
        hs = farm.sync_cells()
        pos = np.array([farm.positions(b + 1) for b in range(nb)])
        streams = 6 * 2 + np.arange(nb)
        want = _flex(hs, pos, 25, BAR_DT, streams=streams, pressure=farm.pressure, **kw)
        assert pos_f.shape == (2, 2, 48, 3) and cells_f.shape == (2, 2, 3, 3) and trace_f.shape == (2, 2, 6, 15) and status_f.shape == (2, 2, 2)
        assert _same(pos_f.reshape(nb, 48, 3), want[0]) and _same(vel_f.reshape(nb, 48, 3), want[1]) and _same(cells_f.reshape(nb, 3, 3), want[3])
        assert _same(trace_f.reshape(nb, 6, 15), want[5]) and _same(status_f.reshape(nb, 2), want[6]) and np.all(status_f[:, :, 0] == 25)
        assert not np.any(cells_f.reshape(nb, 3, 3)[:, 0, 0] == hs[:, 0, 0])
        assert _all_same(em.molecular_dynamics_flex(1, nb, 25, BAR_DT, streams=streams, pressure=farm.pressure, **kw), want)
        t = flex_elapsed_ms()
        assert len(t) == 5 and t[2] > 0.0 and t[4] > 0.0
        g = surface_tension(want[5], axis=2)
        assert g.shape == (nb, 6) and np.all(np.isfinite(g))
        # the engine's own boxes and cells are where they were
        assert np.array_equal(em.model_energy_batch(1, nb), e0) and np.array_equal(farm.sync_cells(), hs)
    finally:
        em.energy_deinit()


if __name__ == "__main__":
    # the child of test_chunks_and_slices_do_not_change_a_byte: the switches are set, mw_flex_init reads them
    from mc_water_ls_mw_amd.flexcell import flex_finalize, flex_last
    out = {}
    for k, (hs, xs, vs) in enumerate(_switch_cases()):
        r = _switch_run(hs, xs, vs)
        last = flex_last()
        out.update({f"out{k}_{j}": r[j] for j in range(7)})
        out.update({f"chunks{k}": last["chunks"], f"boxes_per_chunk{k}": last["boxes_per_chunk"], f"steps_per_launch{k}": last["steps_per_launch"]})
    flex_finalize()
    np.savez(sys.argv[1], **out)
