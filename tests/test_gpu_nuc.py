"""GPU: the nucleus-size molecular dynamics of libmw_nuc.so (nucleation.nucleus_md / _torch, largest_cluster, shoot,
basin_crossings, EnergyModule.nucleus_md, WalkerFarm.nucleus_md) against libmw_flex.so (bytes, with the bounds disabled and for
every stopped box), against libmw_boo.so (neighbour and connection counts), against the numpy mirror of tests/nuc_ref.py
(integers exactly, the state within flex_ref's bars), and the bit rules of include/mw_nuc.h.

Bars.  The state's are flex_ref's, measured on the CPU; the integers are compared exactly, which the preconditions that
tests/test_nuc_ref.py asserts on the CPU make legitimate.  None comes from a device result."""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from boo_ref import ANG_TO_BOHR, scaled_set
from quench_ref import load_case
import flex_ref
import md_ref
import npt_ref
import nuc_ref
from md_ref import BAR_DT, BAR_GAMMA, BAR_KT, BAR_STEPS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _library_lifetime():
    """The libraries are initialised by their first calls here and finalised when this file is done."""
    yield
    from mc_water_ls_mw_amd import bondorder, flexcell, nucleation
    nucleation.nuc_finalize()
    flexcell.flex_finalize()
    bondorder._dev.finalize()


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _all_same(a, b):
    return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))


def _nuc(*a, **kw):
    from mc_water_ls_mw_amd.nucleation import nucleus_md
    return nucleus_md(*a, **kw)


def _flex(*a, **kw):
    from mc_water_ls_mw_amd.flexcell import molecular_dynamics_flex
    return molecular_dynamics_flex(*a, **kw)


def _batch():
    """Five thermalised, rescaled ic96 boxes, as tests/test_gpu_flex.py's: (cells, positions, velocities)."""
    hs, xs = scaled_set("ic96", 5, 0.1, 40)
    return hs, xs, md_ref.maxwell_boltzmann(len(xs), xs.shape[1], BAR_KT, seed=21)


LANGEVIN = dict(kT=BAR_KT, gamma=BAR_GAMMA, seed=77)
BARO = dict(pressure=npt_ref.BAR_PRESSURE, tau_p=npt_ref.BAR_TAU_P, beta_T=npt_ref.BAR_BETA_T)
STREAMS = np.array([11, 3, 2 ** 40, 5, 0], dtype=np.uint64)
#: the state of a box in the results of nucleus_md and of molecular_dynamics_flex: pos, vel, forces, cells, ref
STATE = (0, 1, 2, 3, 4)


# -- 1. bounds disabled: libmw_flex.so, byte for byte ---------------------------------------------------
@pytest.mark.parametrize("check", (1, 5))
@pytest.mark.parametrize("every", (0, 5))
@pytest.mark.parametrize("langevin", (False, True), ids=("nve", "langevin"))
def test_with_the_bounds_disabled_the_bytes_are_those_of_mw_flex_run(langevin, every, check):
    hs, xs, vs = _batch()
    kw = dict(vel=vs, streams=STREAMS, sample_every=3, step0=17, pos_ref=xs + 0.25, baro_every=every, **(LANGEVIN if langevin else {}), **BARO)
    for coupling in (0, 1, 3):
        want = _flex(hs, xs, 30, BAR_DT, coupling=coupling, axis=1, **kw)
        got = _nuc(hs, xs, 30, BAR_DT, check_every=check, coupling=coupling, axis=1, **kw)
        for j in STATE + (6,):
            assert _same(got[j], want[j]), (coupling, j)
        assert got[5].shape == (5, 11, 18) and _same(np.ascontiguousarray(got[5][..., :15]), want[5])
        assert np.all(want[6] == (30, 0)) and (every == 0 or not np.any(want[3][:, 1, 1] == hs[:, 1, 1]))
        lam = got[5][..., 15]
        assert np.all(lam == np.round(lam)) and np.all((lam >= 0) & (lam <= 96)) and np.all(got[5][:, -1, 15] == got[9][:, 2]) and np.all(got[5][:, -1, 16] == got[9][:, 0])


# -- 2. the single point against the mirror and against libmw_boo.so -------------------------------------
@pytest.mark.parametrize("k", range(len(nuc_ref.single_cases())), ids=[c[0].replace(" ", "_") for c in nuc_ref.single_cases()])
def test_a_single_point_has_the_mirrors_counts_labels_and_clusters(k):
    from mc_water_ls_mw_amd.bondorder import bond_order
    from mc_water_ls_mw_amd.nucleation import largest_cluster, nuc_last
    label, h, xyz, rc_ang, thr, mc, _ = nuc_ref.single_cases()[k]
    ref = nuc_ref.single_reference(k)                                        # (computed once per process, read-only)
    nn, lab, op = largest_cluster(h, xyz, rc_ang, thr, mc)
    last = nuc_last()
    print(label, len(xyz), "op", op, "mirror", ref["op"], "largest n_i", nn[:, 0].max(), "rounds", last["cluster_rounds"], "grid", last["g1"], last["g2"], last["g3"])
    assert nn.dtype == np.int32 and np.array_equal(nn, ref["nn"])
    assert np.array_equal(lab, ref["label"]) and np.array_equal(op, ref["op"])
    assert np.array_equal(bond_order(h, xyz, rc_ang, thr)[1], nn)
    assert last["cluster_rounds"] >= 1 and last["labels_in_lds"] == 1 and not last["small"]
    if "0.98" in label:
        assert nn[:, 0].max() > 12                                           # molecules above the list of the cluster pass: they walk


def test_a_single_point_leaves_the_state_alone_and_fills_row_zero():
    h, xyz = nuc_ref.shaken_ic96()
    got = _nuc(h, xyz, 0, BAR_DT, baro_every=1)
    plain = _flex(h, xyz, 0, BAR_DT, baro_every=1)
    for j in STATE + (6,):
        assert _same(got[j], plain[j]), j
    ref = nuc_ref.order(h, xyz, nuc_ref.RC_ANG * ANG_TO_BOHR, nuc_ref.THRESHOLD, nuc_ref.MIN_CONN)
    assert got[5].shape == (1, 18) and tuple(got[5][0, 15:]) == (ref["op"][2], ref["op"][0], ref["op"][1]) and tuple(got[6]) == (0, 0)


# -- 3. the stopping rule, device against device --------------------------------------------------------
def test_each_box_stops_at_its_first_crossing_with_the_state_of_a_flex_run_of_that_length():
    """An unbounded run gives every box's series of lambda; bounds chosen from it make box 0 stop at entry, box 1 never, box 2
    at the first evaluation that reaches its maximum (lam_hi), boxes 3 and 4 at the first that falls to their minimum (lam_lo)."""
    hs, xs, vs = nuc_ref.stop_batch()
    n, every = xs.shape[1], 5
    kw = dict(vel=vs, streams=np.array(nuc_ref.STOP_STREAMS, dtype=np.uint64), check_every=every, baro_every=5, step0=3, **LANGEVIN, **BARO)
    free = _nuc(hs, xs, 40, BAR_DT, **kw)
    lam = free[5][:, ::every, 15].astype(np.int64)
    print("lambda\n", lam)
    assert np.all(free[6] == (40, 0)) and np.all(free[5][:, 1:every, 15] == free[5][:, :1, 15])   # the latest evaluation at or before the row
    lo, hi = np.full(5, -1, dtype=np.int32), np.full(5, n + 1, dtype=np.int32)
    hi[0] = lam[0, 0]
    hi[2] = lam[2].max()
    lo[3], lo[4] = lam[3].min(), lam[4].min()
    first = lambda b: next((k for k in range(lam.shape[1]) if lam[b, k] >= hi[b] or lam[b, k] <= lo[b]), None)   # noqa: E731
    where = [first(b) for b in range(5)]
    assert where[0] == 0 and where[1] is None and where[2] > 0 and where[3] > 0 and where[4] > 0, where
    got = _nuc(hs, xs, 40, BAR_DT, lam_lo=lo, lam_hi=hi, **kw)
    print("status\n", got[6])
    for b in range(5):
        if where[b] is None:
            assert tuple(got[6][b]) == (40, 0) and _all_same([o[b] for o in got], [o[b] for o in free])
            continue
        done = where[b] * every
        assert tuple(got[6][b]) == (done, 3 if lam[b, where[b]] >= hi[b] else 4), b
        flex = _flex(hs[b], xs[b], done, BAR_DT, vel=vs[b], streams=[nuc_ref.STOP_STREAMS[b]], baro_every=5, step0=3, **LANGEVIN, **BARO)
        for j in STATE:
            assert _same(got[j][b], flex[j]), (b, j)
        assert _same(got[5][b, :done + 1], free[5][b, :done + 1]) and np.all(got[5][b, done:] == got[5][b, done])   # the trace repeats its last row
        assert got[9][b, 2] == lam[b, where[b]] == got[5][b, done, 15]
        alone = _nuc(hs[b], xs[b], done, BAR_DT, vel=vs[b], streams=[nuc_ref.STOP_STREAMS[b]], check_every=every, baro_every=5, step0=3, **LANGEVIN, **BARO)
        assert _same(alone[7], got[7][b]) and _same(alone[8], got[8][b]) and _same(alone[9], got[9][b])             # nn, label, op of the final state


# -- 4. forty steps against the mirror ------------------------------------------------------------------
def _hold_to(got, ref, label):
    pos, vel, forces, cell, refp, trace, status, nn, lab, op = got
    d = dict(pos=float(np.abs(pos - ref["pos"]).max()), vel=float(np.abs(vel - ref["vel"]).max()), cell=float(np.abs(cell - ref["cell"]).max()),
             ref=float(np.abs(refp - ref["ref"]).max()))
    dt = np.abs(trace[:, :15] - ref["trace"][:, :15]).max(axis=0)
    print(label, "status", tuple(status), "op", tuple(op), "pos %.2e (bar %.2e) vel %.2e (bar %.2e) cell %.2e (bar %.2e)" % (d["pos"], flex_ref.POS_TOL, d["vel"], flex_ref.VEL_TOL,
                                                                                                                           d["cell"], flex_ref.CELL_TOL),
          "trace", " ".join("%.2e" % v for v in dt), "bars", " ".join("%.2e" % v for v in flex_ref.TRACE_TOL))
    assert tuple(status) == tuple(ref["status"])
    assert np.array_equal(trace[:, 15:], ref["trace"][:, 15:]) and np.array_equal(op, ref["op"]) and np.array_equal(nn, ref["nn"]) and np.array_equal(lab, ref["label"])
    assert d["pos"] <= flex_ref.POS_TOL and d["ref"] <= flex_ref.POS_TOL and d["vel"] <= flex_ref.VEL_TOL and d["cell"] <= flex_ref.CELL_TOL
    assert np.all(dt <= np.array(flex_ref.TRACE_TOL))


@pytest.mark.parametrize("bounded", (False, True), ids=("free", "bounded"))
@pytest.mark.parametrize("name,langevin", nuc_ref.TRAJ_RUNS, ids=[n + ("_langevin" if l else "") for n, l in nuc_ref.TRAJ_RUNS])
def test_forty_steps_land_where_the_mirror_lands(name, langevin, bounded):
    """65 molecules in a triclinic cell and 96 in an orthorhombic one, a barostat application before every check; free, and with
    the bounds that stop the mirror at the first evaluation whose lambda differs from the entry's."""
    h, xyz = load_case(name)
    rc_ang, thr, mc, kw = nuc_ref.traj_kwargs(name, langevin)
    lo, hi = nuc_ref.bounds_from(nuc_ref.reference(name, langevin), len(xyz)) if bounded else (-1, None)
    ref = nuc_ref.reference(name, langevin, lo, hi)                          # (computed once per process, read-only)
    got = _nuc(h, xyz, BAR_STEPS, BAR_DT, lam_lo=lo, lam_hi=hi, check_every=nuc_ref.TRAJ_CHECK, rc_ang=rc_ang, threshold=thr, min_conn=mc,
               vel=md_ref.bar_velocities(name), streams=[3], coupling="aniso", axis=2, **kw)
    _hold_to(got, ref, "%s %s %s" % (name, "langevin" if langevin else "deterministic", "bounded" if bounded else "free"))


# -- 5. the byte equalities ----------------------------------------------------------------------------
def test_two_runs_of_k_steps_are_one_run_of_2k():
    hs, xs, vs = _batch()
    kw = dict(streams=STREAMS, check_every=5, baro_every=5, coupling="semi", **LANGEVIN, **BARO)
    whole = _nuc(hs, xs, 20, BAR_DT, vel=vs, step0=4, **kw)
    a = _nuc(hs, xs, 10, BAR_DT, vel=vs, step0=4, **kw)
    assert np.all(a[6] == (10, 0))
    b = _nuc(a[3], a[0], 10, BAR_DT, vel=a[1], pos_ref=a[4], step0=14, **kw)
    for j in STATE + (6, 7, 8, 9):
        assert _same(b[j] if j != 6 else b[j] + np.array([10, 0], dtype=np.int32), whole[j]), j
    assert _same(a[5], np.ascontiguousarray(whole[5][:, :11])) and _same(np.ascontiguousarray(b[5][:, 1:]), np.ascontiguousarray(whole[5][:, 11:]))


def _stop_bounds():
    return np.array([-1, 30, -1, 80, 70], dtype=np.int32), np.array([60, 97, 97, 97, 97], dtype=np.int32)


def test_host_pointers_device_pointers_and_a_box_alone_give_the_same_bytes():
    import torch
    from mc_water_ls_mw_amd.nucleation import nucleus_md_torch
    hs, xs, vs = nuc_ref.stop_batch()
    lo, hi = _stop_bounds()
    streams = np.array(nuc_ref.STOP_STREAMS, dtype=np.uint64)
    kw = dict(check_every=5, baro_every=5, sample_every=2, **LANGEVIN, **BARO)
    got = _nuc(hs, xs, 40, BAR_DT, lam_lo=lo, lam_hi=hi, vel=vs, streams=streams, **kw)
    print("status\n", got[6])
    assert len(set(got[6][:, 1].tolist())) >= 2                              # stopped and running boxes in one call
    t = lambda a, dt=torch.float64: torch.tensor(a, dtype=dt, device="cuda")   # noqa: E731
    dev = nucleus_md_torch(t(hs), t(xs), 40, BAR_DT, t(lo, torch.int32), t(hi, torch.int32), vel_t=t(vs), streams_t=t(streams.astype(np.int64), torch.int64), **kw)
    assert _all_same([o.cpu().numpy() for o in dev], got)
    for b in (0, 3):
        alone = _nuc(hs[b], xs[b], 40, BAR_DT, lam_lo=int(lo[b]), lam_hi=int(hi[b]), vel=vs[b], streams=[streams[b]], **kw)
        assert _all_same(alone, [o[b] for o in got]), b


def _switch_case():
    """More boxes than 1 MiB of scratch holds, with bounds that stop some of them: (cells, positions, velocities, lam_lo, lam_hi)."""
    count = 50
    hs, xs = scaled_set("ic96", count, 0.3, 300)
    k = np.arange(count)
    return hs, xs, md_ref.maxwell_boltzmann(count, xs.shape[1], 4.0 * BAR_KT, seed=31), np.where(k % 3 == 0, 60, -1).astype(np.int32), np.where(k % 3 == 1, 90, 97).astype(np.int32)


def _switch_run(hs, xs, vs, lo, hi):
    return _nuc(hs, xs, 20, BAR_DT, lam_lo=lo, lam_hi=hi, vel=vs, check_every=5, sample_every=4, baro_every=5, step0=5, coupling="uniaxial", **LANGEVIN, **BARO)


def test_chunks_and_where_the_labels_live_do_not_change_a_byte(tmp_path):
    """A fresh process with 1 MiB of scratch (several chunks, the last one ragged) and one with the labels in global memory
    return the bytes of this process (256 MiB, labels in LDS)."""
    from mc_water_ls_mw_amd.nucleation import nuc_last
    case = _switch_case()
    got = _switch_run(*case)
    last = nuc_last()
    fits = (1 << 20) // last["scratch_bytes_per_box"]
    print("status codes", np.bincount(got[6][:, 1], minlength=5), "boxes per MiB", fits)
    assert last["chunks"] == 1 and last["labels_in_lds"] == 1 and 1 < fits < len(case[1]) and len(case[1]) % fits != 0
    assert len(set(got[6][:, 1].tolist())) >= 2
    for env, chunks, lds in ((dict(MW_NUC_SCRATCH_MB="1"), -(-len(case[1]) // fits), 1), (dict(MW_NUC_LABELS_LDS="0"), 1, 0)):
        out = tmp_path / ("switch%d%d.npz" % (chunks, lds))
        res = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
        assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-3000:])
        z = np.load(out)
        assert int(z["chunks"]) == chunks and int(z["labels_in_lds"]) == lds
        assert _all_same([z[f"out{j}"] for j in range(10)], got), env


# -- 6. the host helpers on a tiny input ----------------------------------------------------------------
def test_shoot_and_basin_crossings_add_up_and_repeat():
    from mc_water_ls_mw_amd.nucleation import basin_crossings, largest_cluster, shoot
    hs, xs, vs = nuc_ref.stop_batch()
    kw = dict(check_every=5, baro_every=0, **{k: v for k, v in LANGEVIN.items() if k != "seed"})
    res = shoot(hs[:3], xs[:3], vs[:3], 40, BAR_DT, 5, 70, trials=3, seed=9, **kw)
    again = shoot(hs[:3], xs[:3], vs[:3], 40, BAR_DT, 5, 70, trials=3, seed=9, **kw)
    print("shoot", {k: v for k, v in res.items() if np.isscalar(v)})
    assert res["total"] == 9 == res["reached_hi"] + res["reached_lo"] + res["undecided"] + res["frozen"] and res["reached_hi"] >= 1
    assert res["fraction"] == res["reached_hi"] / 9 and res["error"] == pytest.approx(np.sqrt(res["fraction"] * (1 - res["fraction"]) / 9), rel=1e-14)
    assert len(res["pos"]) == res["reached_hi"] == len(res["parent"]) and np.all(res["parent"] < 3)
    assert np.all(largest_cluster(res["cells"], res["pos"])[2][:, 2] >= 70)
    assert all(_same(np.asarray(res[k]), np.asarray(again[k])) for k in res)
    other = shoot(hs[:3], xs[:3], vs[:3], 40, BAR_DT, 5, 70, trials=3, seed=10, **kw)
    assert other["reached_hi"] == 0 or not _same(other["pos"][:1], res["pos"][:1])               # another seed, other trajectories
    flux = basin_crossings(hs[3:], xs[3:], vs[3:], 85, 90, 10, BAR_DT, calls=6, seed=9, **kw)
    same = basin_crossings(hs[3:], xs[3:], vs[3:], 85, 90, 10, BAR_DT, calls=6, seed=9, **kw)
    print("basin_crossings", {k: v for k, v in flux.items() if np.isscalar(v)})
    assert flux["crossings"] == len(flux["pos"]) == len(flux["cells"]) >= 2 and 0 < flux["steps"] <= 2 * 6 * 10 and flux["steps"] % 5 == 0
    assert flux["time"] == flux["steps"] * BAR_DT and flux["flux"] == flux["crossings"] / flux["time"] and flux["frozen"] == 0
    assert np.all(largest_cluster(flux["cells"], flux["pos"])[2][:, 2] >= 90)
    assert all(_same(np.asarray(flux[k]), np.asarray(same[k])) for k in flux)


# -- 7. with the engine in the same process -------------------------------------------------------------
def test_the_engine_gives_what_the_arrays_give_and_a_small_farm_gets_the_librarys_message():
    from mc_water_ls_mw_amd.energy import MwError, load_boxes
    from mc_water_ls_mw_amd.nucleation import nuc_elapsed_ms
    from test_gpu_md import _farm
    hs, xs, vs = nuc_ref.stop_batch()
    lo, hi = _stop_bounds()
    kw = dict(lam_lo=lo, lam_hi=hi, vel=vs, check_every=5, baro_every=5, sample_every=5, **LANGEVIN, **BARO)
    em = load_boxes(list(hs), list(xs))
    try:
        e0 = em.model_energy_batch(1, 5).copy()
        want = _nuc(hs, xs, 20, BAR_DT, **kw)
        assert _all_same(em.nucleus_md(1, 5, 20, BAR_DT, **kw), want)
        t = nuc_elapsed_ms()
        assert len(t) == 7 and t[2] > 0.0 and t[5] > 0.0 and t[6] > 0.0
        assert np.array_equal(em.model_energy_batch(1, 5), e0)
    finally:
        em.energy_deinit()
    em, farm = _farm()                                                       # 48 molecules
    try:
        with pytest.raises(MwError, match="nwater = 48.*out of scope"):
            farm.nucleus_md(10, BAR_DT, check_every=5)
    finally:
        em.energy_deinit()


if __name__ == "__main__":
    # the child of test_chunks_and_where_the_labels_live_do_not_change_a_byte: the switches are set, mw_nuc_init reads them
    from mc_water_ls_mw_amd.nucleation import nuc_finalize, nuc_last
    r = _switch_run(*_switch_case())
    last = nuc_last()
    out = {f"out{j}": r[j] for j in range(10)}
    out.update(chunks=last["chunks"], labels_in_lds=last["labels_in_lds"])
    nuc_finalize()
    np.savez(sys.argv[1], **out)
