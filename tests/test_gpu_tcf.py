"""GPU: the time correlation functions of libmw_tcf.so (timecorr.time_correlations / _torch, dynamics.trajectory,
EnergyModule.time_correlations, WalkerFarm.time_correlations) against the long-double reference of tests/tcf_ref.py and the bit
rules of include/mw_tcf.h.

Bars.  Every floating output is held to the a-priori rounding bound that tests/tcf_ref.py derives (u = 2^-53, the number of
terms, the sum of their magnitudes, the inputs' magnitudes; nothing measured on a device), the histograms to equality -- the
inputs keep every squared displacement a relative 10^-9 away from every edge, which tests/test_tcf_ref.py asserts on the CPU.
The inputs are synthetic random walks with a drift (tcf_ref.cases: the smallest shapes at which each boundary of
timecorr.tcf_plan -- tile, lag block, frame window, origin chunk -- is crossed).  Two values that are each a fixed-order sum of
the same terms (REMOVE_COM with and without a drift; this library's msd and the MD library's trace column) are held to the
sum of their two bars.

Measured on an MI355X, the largest |device - reference| beside the bar of that value over the 25 cases: msd 1.82e-12 / 1.63e-11,
mqd 2.98e-08 / 4.73e-07, vacf 6.78e-21 / 2.80e-19, fs 1.44e-15 / 8.12e-14; the largest ratio of a difference to its bar was 0.19,
and with molecular dynamics 0.04."""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from conftest import load_golden
from quench_ref import load_case
import md_ref
import tcf_ref
from md_ref import BAR_DT, BAR_GAMMA, BAR_KT
from tcf_ref import make_input, reference, worst

pytestmark = pytest.mark.gpu


def _cases():
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.timecorr import tcf_plan
    build.build_tcf()
    return tcf_ref.cases(tcf_plan(16, 8))


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


@pytest.fixture(scope="module", autouse=True)
def _library_lifetime():
    """The libraries are initialised by their first calls here and finalised when this file is done."""
    yield
    from mc_water_ls_mw_amd import dynamics, timecorr
    timecorr.tcf_finalize()
    dynamics.md_finalize()


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _all_same(a, b):
    return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))


def _compute(case, frames=None, vel=True, boxes=slice(None)):
    """The five results of a case through the host entry; ``frames``: other positions of the case's shape; ``boxes``: a part."""
    from mc_water_ls_mw_amd.timecorr import time_correlations
    f, v, q, edges = make_input(case)
    f = f if frames is None else frames
    return time_correlations(f[:, boxes], v[:, boxes] if vel else None, case.nlags, case.every, q if case.nq else None, edges if case.nedges else None,
                             case.hist_lags, case.remove_com)


def _named(out):
    return dict(zip(("msd", "mqd", "vacf", "fs", "hist"), out))


# -- 1. against the reference, and host entry = device entry -------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_every_output_is_within_its_bar_and_the_histograms_are_exact(case):
    import torch
    from mc_water_ls_mw_amd.timecorr import tcf_last, time_correlations_torch
    ref = reference(case)
    out = _compute(case)
    got = _named(out)
    last = tcf_last()
    assert last["tiles"] == -(-case.nwater // last["tile"]) and last["lag_blocks"] == -(-case.nlags // last["lag_block"]) and last["chunks"] == 1
    rows = worst(got, ref)
    print(case.name, {k: "%.2e / %.2e (%.2f)" % v for k, v in rows.items()})
    assert all(v[2] <= 1.0 for v in rows.values()), rows
    assert got["msd"].shape == (case.nboxes, case.nlags) and got["vacf"].shape == (case.nboxes, case.nlags)
    assert np.all(got["msd"][:, 0] == 0.0) and np.all(got["mqd"][:, 0] == 0.0)
    if case.nq:
        assert got["fs"].shape == (case.nboxes, case.nlags, case.nq) and np.all(got["fs"][:, 0] == 1.0)
    else:
        assert got["fs"] is None
    if case.nedges and case.hist_lags:
        assert got["hist"].dtype == np.int64 and np.array_equal(got["hist"], ref["hist"])
        for h, lag in enumerate(case.hist_lags):
            assert np.all(got["hist"][:, h].sum(axis=-1) == tcf_ref.n_origins(case.nframes, lag, case.every) * case.nwater)
    else:
        assert got["hist"] is None
    f, v, q, edges = make_input(case)
    dev = time_correlations_torch(torch.tensor(f).cuda(), torch.tensor(v).cuda(), case.nlags, case.every, q if case.nq else None,
                                  edges if case.nedges else None, case.hist_lags, case.remove_com)
    assert _all_same([None if t is None else t.cpu().numpy() for t in dev], out)


# -- 2. byte equalities ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("every3", "nwater_200"))
def test_a_batch_is_its_boxes_one_at_a_time_whatever_the_other_boxes_hold(name):
    case = BY_NAME[name]
    full = _compute(case)
    for b in range(case.nboxes):
        one = _compute(case, boxes=slice(b, b + 1))
        assert _all_same(one, [a[b:b + 1] for a in full]), (name, b)
    f = make_input(case)[0]
    other = np.array(f[:, ::-1] * 1.5 + 2.0)                                 # every other box is replaced, box 2 stays
    other[:, 2] = f[:, 2]
    changed = _compute(case, frames=other)
    assert _all_same([a[2] for a in changed], [a[2] for a in full]) and not _same(changed[0][0], full[0][0])


def test_a_null_output_does_not_change_the_others():
    from mc_water_ls_mw_amd.timecorr import load_tcf_library
    case = BY_NAME["every3"]
    full = _named(_compute(case))
    assert _same(_compute(case, vel=False)[0], full["msd"]) and _compute(case, vel=False)[2] is None
    L = load_tcf_library()
    f, v, q, edges = make_input(case)
    e2, hl = np.ascontiguousarray(edges * edges), np.asarray(case.hist_lags, dtype=np.int32)
    for keep in (("fs",), ("hist",), ("vacf",), ("mqd", "hist"), ("msd",)):
        bufs = {k: np.full_like(a, -7) for k, a in full.items()}
        rc_ = L.mw_tcf_compute(case.nframes, case.nboxes, case.nwater, f.ctypes.data, v.ctypes.data, case.nlags, case.every, len(q), q.ctypes.data,
                               len(e2), e2.ctypes.data, len(hl), hl.ctypes.data, 1 if case.remove_com else 0,
                               *[bufs[k].ctypes.data if k in keep else None for k in ("msd", "mqd", "vacf", "fs", "hist")])
        assert rc_ == 0, L.mw_tcf_last_error().decode()
        for k in full:
            assert _same(bufs[k], full[k]) if k in keep else np.all(bufs[k] == -7), (keep, k)


def _chunk_run():
    from mc_water_ls_mw_amd.timecorr import tcf_last
    out = _compute(BY_NAME["farm600"])
    return out, tcf_last()


def test_the_scratch_budget_does_not_change_a_byte(tmp_path):
    """A fresh process with 1 MiB of scratch takes the 600 boxes in several chunks, the last one ragged, and returns the bytes of
    this process, which takes them in one."""
    out, last = _chunk_run()
    fit = (1 << 20) // last["scratch_bytes_per_box"]
    assert last["chunks"] == 1 and 1 < fit < 600 and 600 % fit != 0
    path = tmp_path / "chunks.npz"
    res = subprocess.run([sys.executable, os.path.abspath(__file__), str(path)], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, MW_TCF_SCRATCH_MB="1"))
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-3000:])
    z = np.load(path)
    assert int(z["boxes_per_chunk"]) == fit and int(z["chunks"]) == -(-600 // fit) >= 2
    assert _all_same([z[f"out{j}"] for j in range(5)], out)


# -- 3. semantics ------------------------------------------------------------------------------------------------------------------
def test_a_large_uniform_drift_vanishes_when_the_centre_is_removed():
    case = BY_NAME["every3"]
    assert case.remove_com
    f, v, q, edges = make_input(case)
    drift = np.array([300.0, -200.0, 500.0]) * np.arange(case.nframes)[:, None, None, None]
    moved = np.ascontiguousarray(f + drift)
    a, b = _named(_compute(case)), _named(_compute(case, frames=moved))
    ref_a = reference(case)
    ref_b = tcf_ref.evaluate(moved, v, case.nlags, case.every, q, remove_com=True, dtype=np.longdouble)
    for name in ("msd", "mqd", "fs"):
        assert np.all(np.abs(a[name] - b[name]) <= ref_a["bar_" + name] + ref_b["bar_" + name]), name
        assert np.all(np.abs(b[name] - ref_b[name]) <= ref_b["bar_" + name]), name
    assert _same(a["vacf"], b["vacf"])


# -- 4. with molecular dynamics ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,thermostat", (("ih48_t020", False), ("ih48_t020", True), ("ic96", False), ("ic96", True)))
def test_a_recorded_run_is_the_uninterrupted_run_and_its_msd_is_the_trace(name, thermostat):
    import torch
    from mc_water_ls_mw_amd.dynamics import molecular_dynamics_torch, trajectory
    from mc_water_ls_mw_amd.timecorr import time_correlations_torch
    h, xyz = load_case(name)
    v0 = md_ref.bar_velocities(name)
    kw = dict(kT=BAR_KT, gamma=BAR_GAMMA, seed=5) if thermostat else {}
    cells_t, pos_t, vel_t = (torch.tensor(a[None]).cuda().contiguous() for a in (h, xyz, v0))
    frames, vel_frames, trace, status = trajectory(cells_t, pos_t, 9, 5, BAR_DT, vel_t=vel_t, **kw)
    pos_out, vel_out, _, trace_one, status_one = molecular_dynamics_torch(cells_t, pos_t, 40, BAR_DT, vel_t=vel_t, **kw)
    assert frames.shape == (9, 1, len(xyz), 3) and torch.equal(frames[0], pos_t) and torch.equal(vel_frames[0], vel_t)
    assert torch.equal(frames[8], pos_out) and torch.equal(vel_frames[8], vel_out)
    assert torch.equal(trace, trace_one) and torch.equal(status, status_one) and status.cpu().tolist() == [[40, 0]]
    msd, mqd, vacf, fs, hist = time_correlations_torch(frames, vel_frames, origin_every=9, q=[1.7])
    ref = tcf_ref.evaluate(frames.cpu().numpy(), vel_frames.cpu().numpy(), 9, 9, [1.7], dtype=np.longdouble)
    got = dict(msd=msd.cpu().numpy(), mqd=mqd.cpu().numpy(), vacf=vacf.cpu().numpy(), fs=fs.cpu().numpy())
    rows = worst(got, ref)
    print(name, thermostat, {k: "%.2e / %.2e (%.2f)" % v for k, v in rows.items()})
    assert all(v[2] <= 1.0 for v in rows.values()), rows
    column = trace.cpu().numpy()[0, ::5, 2]                                  # the mean squared displacement at the steps 0, 5, ..., 40
    assert column.shape == (9,) and np.all(np.abs(got["msd"][0] - column) <= 2.0 * ref["bar_msd"][0]), (got["msd"][0] - column, ref["bar_msd"][0])
    assert got["msd"][0, 8] > 0.0 and hist is None


def test_the_engine_and_the_farm_give_what_the_arrays_give():
    import torch
    from mc_water_ls_mw_amd import lattice as lat
    from mc_water_ls_mw_amd.dynamics import trajectory
    from mc_water_ls_mw_amd.energy import load_boxes
    from mc_water_ls_mw_amd.sweep import MuGrid, WalkerFarm
    from mc_water_ls_mw_amd.timecorr import time_correlations_torch
    z1, z2 = load_golden("ic48"), load_golden("ih48")                      # the boxes of ls_pair48, two walkers of two lattices
    boxes = []
    for w in range(2):
        boxes += [(z1["h"], lat.thermalise(z1["xyz"], 0.06, 760 + w)), (z2["h"], lat.thermalise(z2["xyz"], 0.06, 780 + w))]
    em = load_boxes([b[0] for b in boxes], [b[1] for b in boxes])
    try:
        farm = WalkerFarm(em, 2, 200.0, 1.1, grid=MuGrid(101, -400.0, 400.0), weight=np.zeros(101), pressure_au=1.0 / 2.90363081e8)
        farm.options(record=True, samplerun=False, always_switch=True, npt=True, wl_factor=0.05)
        farm.moves(trans_prob=0.5, vol_prob=0.2, dv_max_ang=0.924)
        for w in range(1, 3):
            farm.set_state(w, 1 + (w % 2), farm.initial_mu(w))
        farm.sweep(96, seed=41)
        nb = em.num_lattices
        pos = np.array([farm.positions(b + 1) for b in range(nb)])
        e0 = em.model_energy_batch(1, nb).copy()
        vel = md_ref.maxwell_boltzmann(nb, 48, BAR_KT, seed=9)
        edges = np.linspace(0.05, 1.5, 8)
        kw = dict(kT=BAR_KT, gamma=BAR_GAMMA, vel=vel, seed=13, q=[1.7, 3.0], edges=edges, hist_lags=(1, 5), origin_every=2, remove_com=True)
        msd, mqd, vacf, fs, hist, status = farm.time_correlations(6, 4, BAR_DT, first_global_walker=6, **kw)
        assert msd.shape == (2, 6) and fs.shape == (2, 6, 2) and hist.shape == (2, 2, 9) and status.shape == (2, 2, 2) and np.all(status == (20, 0))
        # walker by walker, as ranks holding one walker each would run them: the stream is (global walker) x lattices + lattice
        hs = farm.sync_cells()
        per = []
        for w in range(2):
            kw_w = dict(kw, vel=vel[2 * w:2 * w + 2], streams=[(6 + w) * 2, (6 + w) * 2 + 1])
            curves, st = em.time_correlations(1 + 2 * w, 2, 6, 4, BAR_DT, **kw_w)
            assert np.all(st == (20, 0))
            per.append(curves)
            up = lambda a, dtype=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()   # noqa: E731
            frames, vel_frames, _, _ = trajectory(up(hs[2 * w:2 * w + 2]), up(pos[2 * w:2 * w + 2]), 6, 4, BAR_DT, kT=BAR_KT, gamma=BAR_GAMMA, seed=13,
                                                  vel_t=up(vel[2 * w:2 * w + 2]), streams_t=up(kw_w["streams"], torch.int64))
            arrays = time_correlations_torch(frames, vel_frames, None, 2, [1.7, 3.0], edges, (1, 5), True)
            assert _all_same([t.cpu().numpy() for t in arrays], curves)
        for k, got in enumerate((msd, mqd, vacf, fs)):
            assert _same(got, np.stack([per[0][k], per[1][k]]).mean(axis=0)), k
        assert _same(hist, per[0][4] + per[1][4]) and np.all(hist.sum(axis=-1) == 2 * 48 * np.array([3, 1]))
        assert msd[0, 5] > 0.0 and not _same(per[0][0], per[1][0])
        # the engine's own boxes are where they were
        assert np.array_equal(em.model_energy_batch(1, nb), e0) and np.array_equal(np.array([farm.positions(b + 1) for b in range(nb)]), pos)
    finally:
        em.energy_deinit()


if __name__ == "__main__":
    # the child of test_the_scratch_budget_does_not_change_a_byte: MW_TCF_SCRATCH_MB is set, mw_tcf_init reads it
    from mc_water_ls_mw_amd.timecorr import tcf_finalize
    res, last_ = _chunk_run()
    tcf_finalize()
    np.savez(sys.argv[1], chunks=last_["chunks"], boxes_per_chunk=last_["boxes_per_chunk"], **{f"out{j}": res[j] for j in range(5)})
