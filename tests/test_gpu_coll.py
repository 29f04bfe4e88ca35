"""GPU: the collective time correlations of libmw_coll.so (collective.collective_correlations / _torch,
EnergyModule.collective_correlations, WalkerFarm.collective_correlations) against the long-double reference of
tests/coll_ref.py, against the libraries that hold their static limits (libmw_sk.so, mw_rdf, libmw_tcf.so) and against the bit
rules of include/mw_coll.h.

Bars.  rho and fkt are held to the a-priori bounds that tests/coll_ref.py derives (nothing measured on a device); gd, qsum and
q2sum to equality -- the inputs keep every distance a relative 10^-9 away from every bin edge and from r_max and every squared
displacement from a^2, which tests/test_coll_ref.py asserts on the CPU.  The inputs are synthetic random walks in oblique cells
(coll_ref.cases: the smallest shapes at which each boundary of collective.coll_plan is crossed)."""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from conftest import load_golden
import coll_ref
import md_ref
from coll_ref import make_input, reference, worst
from md_ref import BAR_DT, BAR_GAMMA, BAR_KT

pytestmark = pytest.mark.gpu

NAMES = ("rho", "fkt", "gd", "qsum", "q2sum")


def _cases():
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.collective import coll_plan
    build.build_coll()
    return coll_ref.cases(coll_plan(16, 8))


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


@pytest.fixture(scope="module", autouse=True)
def _library_lifetime():
    """The libraries are initialised by their first calls here and finalised when this file is done."""
    yield
    from mc_water_ls_mw_amd import collective, dynamics, structure, timecorr
    collective.coll_finalize()
    timecorr.tcf_finalize()
    structure.sk_finalize()
    dynamics.md_finalize()


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _all_same(a, b):
    return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))


def _compute(case, frames=None, boxes=slice(None), outputs=NAMES):
    """The five results of a case through the host entry; ``frames``: other positions of the case's shape; ``boxes``: a part."""
    from mc_water_ls_mw_amd.collective import collective_correlations
    cells, f, nvec, r_max = make_input(case)
    f = f if frames is None else frames
    return collective_correlations(cells[boxes], f[:, boxes], case.nlags, case.every, nvec, r_max, case.nbins, case.hist_lags, case.a, outputs)


def _named(out):
    return dict(zip(NAMES, out))


# -- 1. against the reference, and host entry = device entry -------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_every_output_is_within_its_bar_and_the_counts_are_exact(case):
    import torch
    from mc_water_ls_mw_amd.collective import coll_last, collective_correlations_torch
    ref = reference(case)
    out = _compute(case)
    got = _named(out)
    last = coll_last()
    assert last["chunks"] == 1 and last["pair_small"] == (case.nwater <= 64) and last["pair_tiles"] == (1 if case.nwater <= 64 else -(-case.nwater // last["pair_tile"]))
    assert last["segments"] == (1 if case.nwater <= 64 else -(-case.nwater // last["segment_molecules"]))
    rows = worst(got, ref)
    print(case.name, {k: "%.2e / %.2e (%.2f)" % v for k, v in rows.items()})
    assert all(v[2] <= 1.0 for v in rows.values()), rows
    if case.M:
        assert got["rho"].shape == (case.nframes, case.nboxes, case.M) and got["fkt"].shape == (case.nboxes, case.nlags, case.M)
        assert np.all(got["fkt"][:, 0].real > 0.0)
        if case.M >= 2:                                                    # vectors 0 and 1 are n and -n
            assert _same(got["fkt"][:, :, 1], np.conj(got["fkt"][:, :, 0])) and _same(got["rho"][:, :, 1], np.conj(got["rho"][:, :, 0]))
        if case.M >= 4:
            assert _same(got["fkt"][:, :, 3], np.conj(got["fkt"][:, :, 2]))
    else:
        assert got["rho"] is None and got["fkt"] is None
    if case.nbins:
        assert got["gd"].dtype == np.int64 and np.array_equal(got["gd"], ref["gd"])
    else:
        assert got["gd"] is None
    if case.a:
        assert np.array_equal(got["qsum"], ref["qsum"]) and np.array_equal(got["q2sum"], ref["q2sum"])
        assert np.all(got["qsum"][:, 0] == coll_ref.n_origins(case.nframes, 0, min(case.every, case.nframes)) * case.nwater)
    else:
        assert got["qsum"] is None and got["q2sum"] is None
    cells, f, nvec, r_max = make_input(case)
    dev = collective_correlations_torch(cells, torch.tensor(f).cuda(), case.nlags, case.every, nvec, r_max, case.nbins, case.hist_lags, case.a)
    assert _all_same([None if t is None else t.cpu().numpy() for t in dev], out)


# -- 2. the static limits in the other libraries ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("nwater_63", "nwater_64", "nwater_65", "nwater_1025", "nwater_8193"))
def test_the_modes_are_byte_for_byte_the_structure_factor_library(name):
    from mc_water_ls_mw_amd.structure import structure_factor
    case = BY_NAME[name]
    cells, f, nvec, _ = make_input(case)
    from mc_water_ls_mw_amd.collective import coll_last
    rho = _compute(case, outputs=("rho",))[0]
    assert coll_last()["scratch_bytes_per_box"] == 0                      # rho alone keeps no transposed copy of the modes
    assert _same(rho, _compute(case)[0])
    for t in range(case.nframes):
        _, want = structure_factor(cells, f[t], nvec, want_rho=True)
        assert _same(rho[t], want), (name, t)
    one = structure_factor(cells[:1], f[0, :1], nvec, want_rho=True)[1]   # and a single box of a single frame
    assert _same(rho[0, :1], one)


@pytest.mark.parametrize("name,r_ang", (("ih48", 7.0), ("ih48", 3.1), ("ic96", 7.5)))
def test_lag_zero_of_one_origin_is_the_engines_pair_histogram(name, r_ang):
    from mc_water_ls_mw_amd.collective import collective_correlations
    from mc_water_ls_mw_amd.energy import load_boxes
    z = load_golden(name)
    h, xyz = np.asarray(z["h"], dtype=np.float64), np.asarray(z["xyz"], dtype=np.float64)
    r_max = float(r_ang) / 0.5291772108                                    # the engine's Angstrom -> bohr
    w = coll_ref.pair_cell(h, 1e-3)[1]
    if r_ang == 7.0:
        assert r_max > 0.5 * w.min()                                       # beyond half the smallest width: images are counted
    em = load_boxes([h], [xyz])
    try:
        want = em.rdf_counts(1, r_ang, 200)
    finally:
        em.energy_deinit()
    rng = np.random.default_rng(3)
    frames = np.stack([xyz, xyz + rng.normal(0.0, 0.2, xyz.shape)])        # the second frame is never an origin
    gd = collective_correlations(h, frames, nlags=2, origin_every=2, r_max=r_max, nbins=200, hist_lags=(0,))[2]
    assert gd.shape == (1, 200) and np.array_equal(gd[0], want) and want.sum() > 0


@pytest.mark.parametrize("name", ("every3", "nwater_65", "nlags_block+1"))
def test_the_overlap_sum_is_the_first_bin_of_the_self_histogram(name):
    from mc_water_ls_mw_amd.timecorr import time_correlations
    case = BY_NAME[name]
    _, f, _, _ = make_input(case)
    got = _named(_compute(case, outputs=("qsum", "q2sum")))
    lags = tuple(range(min(case.nlags, 64)))
    hist = time_correlations(f, None, case.nlags, case.every, None, [case.a, 1e6], lags)[4]
    assert np.array_equal(got["qsum"][:, :len(lags)], hist[:, :, 0])


# -- 3. byte equalities and exact identities -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("every3", "nwater_65", "nwater_tile+1"))
def test_a_frozen_trajectory_counts_one_frame_per_origin(name):
    case = BY_NAME[name]
    _, f, _, _ = make_input(case)
    frozen = np.ascontiguousarray(np.broadcast_to(f[:1], f.shape))
    got = _named(_compute(case, frames=frozen))
    single = _named(_compute(case._replace(nframes=1, nlags=1, hist_lags=(0,), every=1), frames=frozen[:1]))
    e = min(case.every, case.nframes)
    for h, lag in enumerate(case.hist_lags):
        assert np.array_equal(got["gd"][:, h], coll_ref.n_origins(case.nframes, lag, e) * single["gd"][:, 0]), (name, lag)
    o = coll_ref.n_origins(case.nframes, np.arange(case.nlags), e)
    assert np.array_equal(got["qsum"], np.broadcast_to(o * case.nwater, got["qsum"].shape))
    assert np.array_equal(got["q2sum"], np.broadcast_to(o * case.nwater ** 2, got["q2sum"].shape))
    assert _same(got["rho"][3 % case.nframes], got["rho"][0]) and _same(got["rho"][:1], single["rho"])


@pytest.mark.parametrize("name", ("every3", "nwater_65"))
def test_a_batch_is_its_boxes_one_at_a_time_whatever_the_other_boxes_hold(name):
    case = BY_NAME[name]
    full = _compute(case)
    for b in range(case.nboxes):
        one = _compute(case, boxes=slice(b, b + 1))
        assert _all_same(one, [a[:, b:b + 1] if k == 0 else a[b:b + 1] for k, a in enumerate(full)]), (name, b)
    f = make_input(case)[1]
    other = np.array(f[:, ::-1] * 1.5 + 2.0)                                 # every other box is replaced, the last one stays
    last = case.nboxes - 1
    other[:, last] = f[:, last]
    changed = _compute(case, frames=other)
    assert _all_same([a[:, last] if k == 0 else a[last] for k, a in enumerate(changed)], [a[:, last] if k == 0 else a[last] for k, a in enumerate(full)])
    assert not _same(changed[1][0], full[1][0])


def test_a_null_output_does_not_change_the_others():
    case = BY_NAME["every3"]
    full = _named(_compute(case))
    for keep in (("rho",), ("fkt",), ("gd",), ("qsum",), ("q2sum",), ("fkt", "q2sum"), ("rho", "gd")):
        part = _named(_compute(case, outputs=keep))
        for k in NAMES:
            assert _same(part[k], full[k]) if k in keep else part[k] is None, (keep, k)
    # prefilled buffers behind the C entry: what is NULL is not written, what is not asked for stays as it was
    from mc_water_ls_mw_amd.collective import load_coll_library
    L = load_coll_library()
    cells, f, nvec, r_max = make_input(case)
    hl = np.asarray(case.hist_lags, dtype=np.int32)
    bufs = {k: np.full(a.shape + ((2,) if k in ("rho", "fkt") else ()), -7, dtype=np.float64 if k in ("rho", "fkt") else np.int64) for k, a in full.items()}
    rc_ = L.mw_coll_compute(case.nframes, case.nboxes, case.nwater, cells.ctypes.data, f.ctypes.data, case.nlags, case.every, len(nvec), nvec.ctypes.data,
                            r_max, case.nbins, len(hl), hl.ctypes.data, case.a, None, bufs["fkt"].ctypes.data, None, bufs["qsum"].ctypes.data, None)
    assert rc_ == 0, L.mw_coll_last_error().decode()
    assert np.all(bufs["rho"] == -7) and np.all(bufs["gd"] == -7) and np.all(bufs["q2sum"] == -7)
    assert _same(bufs["fkt"][..., 0] + 1j * bufs["fkt"][..., 1], full["fkt"]) and _same(bufs["qsum"], full["qsum"])


def _chunk_run():
    from mc_water_ls_mw_amd.collective import coll_last
    out = _compute(BY_NAME["farm600"])
    return out, coll_last()


def test_the_scratch_budget_does_not_change_a_byte(tmp_path):
    """A fresh process with 1 MiB of scratch takes the 600 boxes in several chunks, the last one ragged, and the mode pass in
    several launches, and returns the bytes of this process, which takes them in one."""
    out, last = _chunk_run()
    assert last["chunks"] == 1 and last["boxes_per_chunk"] == 600
    path = tmp_path / "chunks.npz"
    res = subprocess.run([sys.executable, os.path.abspath(__file__), str(path)], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, MW_COLL_SCRATCH_MB="1"))
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-3000:])
    z = np.load(path)
    fit = int(z["boxes_per_chunk"])
    assert 1 < fit < 600 and 600 % fit != 0 and int(z["chunks"]) == -(-600 // fit) >= 2
    assert fit == ((1 << 20) - (1 << 18)) // last["scratch_bytes_per_box"]    # the mode pass keeps a quarter of the budget
    assert 1 <= int(z["mode_units"]) < fit * 16                              # and takes a chunk's (frame, box) units in several launches
    assert _all_same([z[f"out{j}"] for j in range(5)], out)


# -- 4. with molecular dynamics ------------------------------------------------------------------------------------------------------
def test_the_engine_and_the_farm_give_what_the_arrays_give():
    import torch
    from mc_water_ls_mw_amd import lattice as lat
    from mc_water_ls_mw_amd.collective import collective_correlations_torch
    from mc_water_ls_mw_amd.dynamics import trajectory
    from mc_water_ls_mw_amd.energy import load_boxes
    from mc_water_ls_mw_amd.sweep import MuGrid, WalkerFarm
    z1, z2 = load_golden("ic48"), load_golden("ih48_t020")                 # two walkers of two lattices
    boxes = []
    for w in range(2):
        boxes += [(z1["h"], lat.thermalise(z1["xyz"], 0.06, 760 + w)), (z2["h"], lat.thermalise(z2["xyz"], 0.06, 780 + w))]
    em = load_boxes([b[0] for b in boxes], [b[1] for b in boxes])
    try:
        farm = WalkerFarm(em, 2, 200.0, 1.1, grid=MuGrid(101, -400.0, 400.0), weight=np.zeros(101), pressure_au=1.0 / 2.90363081e8)
        for w in range(1, 3):
            farm.set_state(w, 1 + (w % 2), farm.initial_mu(w))
        nb = em.num_lattices
        pos = np.array([farm.positions(b + 1) for b in range(nb)])
        e0 = em.model_energy_batch(1, nb).copy()
        vel = md_ref.maxwell_boltzmann(nb, 48, BAR_KT, seed=9)
        hs = farm.sync_cells()
        r_max = 0.45 * min(float(coll_ref.pair_cell(h, 1e-3)[1].min()) for h in hs)
        nvec = np.array(coll_ref.VECTORS[:4], dtype=np.int32)
        kw = dict(kT=BAR_KT, gamma=BAR_GAMMA, vel=vel, seed=13, nvec=nvec, r_max=r_max, nbins=40, hist_lags=(0, 1, 5), origin_every=2, overlap_a=0.05)
        fkt, gd, qsum, q2sum, status = farm.collective_correlations(6, 4, BAR_DT, first_global_walker=6, **kw)
        assert fkt.shape == (2, 6, 4) and gd.shape == (2, 3, 40) and qsum.shape == q2sum.shape == (2, 6) and np.all(status == (20, 0))
        per = []
        for w in range(2):
            kw_w = dict(kw, vel=vel[2 * w:2 * w + 2], streams=[(6 + w) * 2, (6 + w) * 2 + 1])
            curves, st = em.collective_correlations(1 + 2 * w, 2, 6, 4, BAR_DT, outputs=NAMES, **kw_w)
            assert np.all(st == (20, 0))
            per.append(curves)
            up = lambda a, dtype=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()   # noqa: E731
            frames, _, _, _ = trajectory(up(hs[2 * w:2 * w + 2]), up(pos[2 * w:2 * w + 2]), 6, 4, BAR_DT, kT=BAR_KT, gamma=BAR_GAMMA, seed=13,
                                         vel_t=up(vel[2 * w:2 * w + 2]), streams_t=up(kw_w["streams"], torch.int64))
            arrays = collective_correlations_torch(hs[2 * w:2 * w + 2], frames, None, 2, nvec, r_max, 40, (0, 1, 5), 0.05)
            assert _all_same([t.cpu().numpy() for t in arrays], curves)
        assert _same(fkt, np.stack([per[0][1], per[1][1]]).mean(axis=0))
        for k, got in ((2, gd), (3, qsum), (4, q2sum)):
            assert _same(got, per[0][k] + per[1][k]), k
        assert np.all(qsum[:, 0] == 2 * 3 * 48) and np.all(q2sum[:, 0] == 2 * 3 * 48 * 48) and gd[:, 0].sum() > 0
        assert not _same(per[0][1], per[1][1])
        assert np.array_equal(em.model_energy_batch(1, nb), e0) and np.array_equal(np.array([farm.positions(b + 1) for b in range(nb)]), pos)
    finally:
        em.energy_deinit()


if __name__ == "__main__":
    # the child of test_the_scratch_budget_does_not_change_a_byte: MW_COLL_SCRATCH_MB is set, mw_coll_init reads it
    from mc_water_ls_mw_amd.collective import coll_finalize
    res, last_ = _chunk_run()
    coll_finalize()
    np.savez(sys.argv[1], chunks=last_["chunks"], boxes_per_chunk=last_["boxes_per_chunk"], mode_units=last_["mode_units"], **{f"out{j}": res[j] for j in range(5)})
