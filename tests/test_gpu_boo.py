"""GPU: the bond-order parameters of libmw_boo.so (bondorder.bond_order / _torch, EnergyModule.bond_order,
WalkerFarm.bond_order) against the long-double reference of tests/boo_ref.py -- 1e-12 absolute on q4^2, q6^2, qbar4^2,
qbar6^2, Q4^2, Q6^2 and the two means (all <= 1; ten times the noise floor of a plain-double evaluation that
tests/test_boo_ref.py asserts), neighbour and connection counts exactly (the preconditions are asserted there too) -- and
the bit rules of include/mw_boo.h: the bytes of a box's results depend on the box, rc and the threshold alone."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from conftest import load_golden
from boo_ref import ANG_TO_BOHR, BATCHES, batch_set, boo_exact, case_exact, cases, gaps, load_case, scaled_set

pytestmark = pytest.mark.gpu

TOL = 1e-12
BOHR_TO_ANG = 0.5291772108
CASES = cases()
LD = np.longdouble
_REF = {}


@pytest.fixture(scope="module", autouse=True)
def _library_lifetime():
    """The library is initialised by its first call here and finalised when this file is done."""
    yield
    from mc_water_ls_mw_amd import bondorder
    bondorder.boo_finalize()


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _all_same(a, b):
    return all(_same(x, y) for x, y in zip(a, b))


def _against(ref, q, nn, summary, what):
    """The device's results of one box against a boo_exact dict; prints every figure before it asserts."""
    dq = np.abs((q.astype(LD) ** 2 - ref["q2"]).astype(np.float64)).max(axis=0)
    ds = np.abs(np.array([summary[0].astype(LD) ** 2 - ref["summary"][0], summary[1].astype(LD) ** 2 - ref["summary"][1],
                          summary[2] - ref["summary"][2], summary[3] - ref["summary"][3]]).astype(np.float64))
    wrong_n = int(np.count_nonzero(nn[:, 0] != ref["n"])), int(np.count_nonzero(nn[:, 1] != ref["conn"]))
    print(what, "max |d q^2| (q4, q6, qbar4, qbar6)", " ".join("%.2e" % v for v in dq), " |d summary|", " ".join("%.2e" % v for v in ds),
          " wrong (n, conn)", wrong_n)
    assert nn.dtype == np.int32 and np.array_equal(nn[:, 0], ref["n"]), what
    assert np.array_equal(nn[:, 1], ref["conn"]), what
    assert dq.max() <= TOL and ds.max() <= TOL, what
    assert np.all(q >= 0.0) and np.all(q <= 1.0 + 1e-12)


# -- against boo_exact ------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_input_matches_the_reference(case):
    from mc_water_ls_mw_amd.bondorder import bond_order, boo_last, boo_plan
    h, xyz, rc, thr, _ = load_case(case)
    if case[0] not in _REF:
        _REF[case[0]] = case_exact(case)
    q, nn, summary = bond_order(h, xyz, rc * BOHR_TO_ANG, thr)
    assert q.shape == (len(xyz), 4) and nn.shape == (len(xyz), 2) and summary.shape == (4,)
    _against(_REF[case[0]], q, nn, summary, case[0])
    last = boo_last()
    assert last == boo_plan(len(xyz), h, rc * BOHR_TO_ANG, 1) and last["small"] == (len(xyz) <= 64) and last["chunks"] == 1, last
    if "one cell" in case[0]:
        assert not last["small"] and sorted((last["g1"], last["g2"], last["g3"])) == [1, 1, 2], last
    if case[0] == "ih8_small at its width":
        assert (last["g1"], last["g2"], last["g3"]) == (1, 1, 1)
    if case[0] == "gas N = 65":
        assert min(last["g1"], last["g2"], last["g3"]) == 2, last
    # the same call again: the same bytes
    assert _all_same(bond_order(h, xyz, rc * BOHR_TO_ANG, thr), (q, nn, summary))


def test_positions_beyond_one_cell_and_null_outputs():
    """Molecules moved by lattice vectors keep their neighbours; any output may be left out."""
    from mc_water_ls_mw_amd.bondorder import bond_order, load_boo_library
    for name in ("ic64_sheared", "ih1536_t012"):
        z = load_golden(name)
        h, xyz = z["h"], z["xyz"]
        rng = np.random.default_rng(3)
        moved = xyz + rng.integers(-3, 4, xyz.shape).astype(np.float64) @ h
        if name not in _REF:
            _REF[name] = boo_exact(h, xyz, 3.5 * ANG_TO_BOHR, 0.5, grid=len(xyz) > 256)
        q, nn, summary = bond_order(h, moved, 3.5, 0.5)
        _against(_REF[name], q, nn, summary, name + " displaced")
        L = load_boo_library()
        cells, pos = np.ascontiguousarray(h), np.ascontiguousarray(moved)
        for keep in range(3):
            outs = [np.zeros_like(q), np.zeros_like(nn), np.zeros_like(summary)]
            ptrs = [o.ctypes.data if k == keep else None for k, o in enumerate(outs)]
            assert L.mw_boo_compute(1, len(xyz), cells.ctypes.data, pos.ctypes.data, 3.5 / BOHR_TO_ANG, 0.5, *ptrs) == 0
            assert _same(outs[keep], (q, nn, summary)[keep]), (name, keep)


def test_the_threshold_moves_only_the_connections():
    z = load_golden("ih48_t020")
    from mc_water_ls_mw_amd.bondorder import bond_order
    q, nn, summary = bond_order(z["h"], z["xyz"], 3.5, 0.5)
    lo, hi = bond_order(z["h"], z["xyz"], 3.5, -1.0), bond_order(z["h"], z["xyz"], 3.5, 1.0)
    for o in (lo, hi):
        assert _same(o[0], q) and _same(o[2], summary) and np.array_equal(o[1][:, 0], nn[:, 0])
    assert np.array_equal(lo[1][:, 1], nn[:, 0]) and not np.any(hi[1][:, 1])       # s_ij > -1 for every bond here; none > 1


# -- bit rules --------------------------------------------------------------------------------
_scaled_set = scaled_set


@pytest.mark.parametrize("name,n", BATCHES)
def test_a_batch_equals_the_single_calls_bit_for_bit(name, n):
    from mc_water_ls_mw_amd.bondorder import bond_order
    hs, xs = batch_set(name, n)                                            # (preconditions of its last box: tests/test_boo_ref.py)
    q, nn, summary = bond_order(hs, xs, 3.5, 0.5)
    assert q.shape == (n, xs.shape[1], 4) and nn.shape == (n, xs.shape[1], 2) and summary.shape == (n, 4)
    for b in range(n):
        assert _all_same(bond_order(hs[b], xs[b], 3.5, 0.5), (q[b], nn[b], summary[b])), b
    assert len({summary[b].tobytes() for b in range(n)}) == n
    assert _all_same(bond_order(hs[1:], xs[1:], 3.5, 0.5), (q[1:], nn[1:], summary[1:]))
    ref = boo_exact(hs[n - 1], xs[n - 1], 3.5 * ANG_TO_BOHR, 0.5, sums=False, grid=xs.shape[1] > 256)
    _against(ref, q[n - 1], nn[n - 1], summary[n - 1], f"{name} box {n}")


def _chunk_case():
    return _scaled_set("ic96", 80, 0.12, 300)


def test_chunks_give_the_bits_of_one_chunk(tmp_path):
    """A fresh process whose scratch budget is 1 MiB takes the 80 boxes in several chunks, the last one ragged; here they fit one."""
    from mc_water_ls_mw_amd.bondorder import bond_order, boo_last, boo_plan
    hs, xs = _chunk_case()
    q, nn, summary = bond_order(hs, xs, 3.5, 0.5)
    last = boo_last()
    assert last["chunks"] == 1 and last["boxes_per_chunk"] == 80 and not last["small"]
    out = tmp_path / "chunks.npz"
    env = dict(os.environ, MW_BOO_SCRATCH_MB="1")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-3000:])
    z = np.load(out)
    fit = (1 << 20) // last["scratch_bytes_per_box"]
    assert 1 < fit < 40 and 80 % fit != 0
    assert int(z["boxes_per_chunk"]) == fit and int(z["chunks"]) == -(-80 // fit) >= 3
    assert _same(z["q"], q) and _same(z["nn"], nn) and _same(z["summary"], summary)
    assert boo_plan(96, hs[0], 3.5, 80)["chunks"] == 1                       # this process kept its own budget


def test_device_tensors_give_the_bits_of_the_host_entry():
    import torch
    from mc_water_ls_mw_amd.bondorder import bond_order, bond_order_torch
    dev = torch.device("cuda:0")
    for name, n in (("ic96", 3), ("ih48_t020", 6)):
        hs, xs = _scaled_set(name, n, 0.1, 70)
        q, nn, summary = bond_order(hs, xs, 3.5, 0.5)
        qt, nt, st = bond_order_torch(torch.from_numpy(hs).to(dev), torch.from_numpy(xs).to(dev), 3.5, 0.5)
        assert qt.is_cuda and nt.is_cuda and st.is_cuda and qt.dtype == st.dtype == torch.float64 and nt.dtype == torch.int32
        assert _same(qt.cpu().numpy(), q) and _same(nt.cpu().numpy(), nn) and _same(st.cpu().numpy(), summary)


# -- rejected calls ---------------------------------------------------------------------------
def test_rejected_calls_name_the_argument_and_write_nothing():
    import torch
    from mc_water_ls_mw_amd.bondorder import MwError, bond_order, boo_elapsed_ms, boo_last, load_boo_library
    z = load_golden("ic48")
    h, xyz = z["h"], z["xyz"]
    bond_order(h, xyz)                                                     # the library is live and has launched
    L = load_boo_library()
    before = boo_last()
    cells = np.ascontiguousarray(np.array([h, h, h]).reshape(3, 9))
    pos = np.ascontiguousarray(np.array([xyz, xyz, xyz]))
    flat = cells.copy()
    flat[2, 6:9] = 0.0
    narrow = cells.copy()
    narrow[1] *= 0.3                                                       # box 1 is narrower than 3.5 Angstrom
    rc = 3.5 / BOHR_TO_ANG
    dev = torch.device("cuda:0")
    for c, r, t, pattern in ((flat, rc, 0.5, r"cells.*box 2\b"), (narrow, rc, 0.5, r"\brc\b.*box 1\b"), (cells, float("nan"), 0.5, r"\brc\b"),
                             (cells, 30.0, 0.5, r"\brc\b.*box 0\b"), (cells, rc, 1.25, "threshold")):
        q, nn, summary = np.full((3, 48, 4), -7.0), np.full((3, 48, 2), -7, dtype=np.int32), np.full((3, 4), -7.0)
        assert L.mw_boo_compute(3, 48, c.ctypes.data, pos.ctypes.data, r, t, q.ctypes.data, nn.ctypes.data, summary.ctypes.data) != 0
        msg = L.mw_boo_last_error().decode()
        assert "mw_boo_compute" in msg and re.search(pattern, msg), msg
        assert np.all(q == -7.0) and np.all(nn == -7) and np.all(summary == -7.0)
        ct, pt = torch.from_numpy(c).to(dev), torch.from_numpy(pos).to(dev)
        qt = torch.full((3, 48, 4), -7.0, dtype=torch.float64, device=dev)
        nt = torch.full((3, 48, 2), -7, dtype=torch.int32, device=dev)
        st = torch.full((3, 4), -7.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        assert L.mw_boo_compute_device(3, 48, ct.data_ptr(), pt.data_ptr(), r, t, qt.data_ptr(), nt.data_ptr(), st.data_ptr()) != 0
        msg = L.mw_boo_last_error().decode()
        assert "mw_boo_compute_device" in msg and re.search(pattern, msg), msg
        assert bool((qt == -7.0).all()) and bool((nt == -7).all()) and bool((st == -7.0).all())
    assert boo_last() == before                                            # nothing launched
    assert all(t >= 0.0 for t in boo_elapsed_ms()) and len(boo_elapsed_ms()) == 4
    with pytest.raises(MwError, match="expected"):
        bond_order(h, xyz[:, :2])


# -- with the engine in the same process ------------------------------------------------------
def _npt_farm(nw=4):
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


def test_engine_boxes_give_what_the_arrays_give():
    from mc_water_ls_mw_amd.bondorder import bond_order
    from mc_water_ls_mw_amd.energy import load_boxes
    names = ("ic96", "ih1536_t012")
    for name in names:
        hs, xs = _scaled_set(name, 3, 0.08, 900)
        em = load_boxes(list(hs), list(xs))
        try:
            got = em.bond_order()
            assert _all_same(got, bond_order(hs, xs, 3.5, 0.5))
            assert _all_same(em.bond_order(2, 2, rc_ang=3.4, threshold=0.4), bond_order(hs[1:], xs[1:], 3.4, 0.4))
        finally:
            em.energy_deinit()


def test_npt_farm_bond_order_after_device_sweeps():
    em, farm = _npt_farm()
    try:
        h0 = np.array(em.hmatrix)
        farm.sweep(288, seed=51)
        summary, solid = farm.bond_order(rc_ang=3.5, threshold=0.5)
        hs = farm.sync_cells()
        assert not np.array_equal(hs, h0)                                  # some volume move was accepted (and synced)
        assert summary.shape == (4, 2, 4) and solid.shape == (4, 2)
        pos = np.array([farm.positions(b + 1) for b in range(em.num_lattices)])
        _, nn_all, s2 = em.bond_order(1, em.num_lattices)
        for b in range(em.num_lattices):
            ref = boo_exact(hs[b], pos[b], 3.5 * ANG_TO_BOHR, 0.5)
            got = summary[b // 2, b % 2]
            err = np.abs(np.array([got[0].astype(LD) ** 2 - ref["summary"][0], got[1].astype(LD) ** 2 - ref["summary"][1],
                                   got[2] - ref["summary"][2], got[3] - ref["summary"][3]]).astype(np.float64))
            gap, near = gaps(hs[b], pos[b], 3.5 * ANG_TO_BOHR, 0.5, ref)
            print("box", b, "|d summary|", " ".join("%.2e" % v for v in err), "solid", solid[b // 2, b % 2], "nearest |d| - rc (rel) %.1e" % gap, "nearest s - thr %.1e" % near)
            assert err.max() <= TOL
            assert gap > 1e-9 and near > 1e-6                              # (the preconditions of exact counts)
            assert np.array_equal(nn_all[b, :, 0], ref["n"]) and np.array_equal(nn_all[b, :, 1], ref["conn"])
            assert solid[b // 2, b % 2] == np.count_nonzero(ref["conn"] >= 3) / 48.0
        assert _same(s2, summary.reshape(8, 4)) and np.array_equal((nn_all[:, :, 1] >= 3).sum(axis=1) / 48.0, solid.reshape(8))
        assert np.all(summary[:, :, 3] > 0.3)                              # both lattices are still crystals
    finally:
        em.energy_deinit()


def test_engine_state_is_untouched_by_a_bond_order_call():
    def run(with_boo):
        em, farm = _npt_farm()
        try:
            farm.sweep(96, seed=41)
            nb = em.num_lattices
            z = load_golden("ic48")
            e0 = em.model_energy_batch(1, nb).copy()
            eo0, en0 = em.delta_energy_batch(1, z["trial_imol"][:64], z["trial_xyz"][:64])
            if with_boo:
                farm.bond_order()
                em.bond_order(1, nb, rc_ang=3.2, threshold=0.7)
            assert np.array_equal(em.model_energy_batch(1, nb), e0)
            eo, en = em.delta_energy_batch(1, z["trial_imol"][:64], z["trial_xyz"][:64])
            assert np.array_equal(eo, eo0) and np.array_equal(en, en0)
            farm.sweep(96, seed=41, move0=96)
            return ([farm.state(w + 1) for w in range(farm.nwalkers)],
                    [farm.tables(w + 1) for w in range(farm.nwalkers)],
                    em.model_energy_batch(1, nb).copy(),
                    [farm.positions(b + 1) for b in range(nb)],
                    farm.sync_cells().copy())
        finally:
            em.energy_deinit()

    a, b = run(False), run(True)
    assert a[0] == b[0]
    for ta, tb in zip(a[1], b[1]):
        assert all(np.array_equal(x, y) for x, y in zip(ta, tb))
    assert np.array_equal(a[2], b[2])
    assert all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))
    assert np.array_equal(a[4], b[4])


if __name__ == "__main__":
    # the child of test_chunks_give_the_bits_of_one_chunk: MW_BOO_SCRATCH_MB is set, so mw_boo_init takes the small budget
    from mc_water_ls_mw_amd.bondorder import bond_order, boo_finalize, boo_last
    hs, xs = _chunk_case()
    q, nn, summary = bond_order(hs, xs, 3.5, 0.5)
    last = boo_last()
    boo_finalize()
    np.savez(sys.argv[1], q=q, nn=nn, summary=summary, chunks=last["chunks"], boxes_per_chunk=last["boxes_per_chunk"])
