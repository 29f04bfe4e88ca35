"""GPU: the nearest-neighbour order parameters of libmw_tet.so (tetrahedral.tetrahedral_order / _torch,
EnergyModule.tetrahedral_order, WalkerFarm.tetrahedral_order) against the long-double reference of tests/tet_ref.py -- counts
exactly, the four nearest as sets, NaN exactly where a value is not defined, (q, s_k, d5, lsi) and the box means within 1e-12
absolute (tests/test_gpu_boo.py's TOL: a distance carries about 1e-14 bohr of rounding from the fractional reduction at
|r| <= 100 bohr and every output is a short sum of such terms; the preconditions of the exact comparisons are asserted in
tests/test_tet_ref.py) -- and the bit rules of include/mw_tet.h: the bytes of a box's results depend on the box and the two
radii alone."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from conftest import load_golden
from boo_ref import batch_set, scaled_set
from tet_ref import BATCHES, MARGIN, batch_radii, case_exact, cases, load_case, preconditions, tet_exact

pytestmark = pytest.mark.gpu

TOL = 1e-12
BOHR_TO_ANG = 0.5291772108
CASES = cases()
LD = np.longdouble
NAN_BITS = 0x7ff8000000000000
_REF = {}


@pytest.fixture(scope="module", autouse=True)
def _library_lifetime():
    """The library is initialised by its first call here and finalised when this file is done."""
    yield
    from mc_water_ls_mw_amd import tetrahedral
    tetrahedral.tet_finalize()


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _all_same(a, b):
    return all(_same(x, y) for x, y in zip(a, b))


def _ref(case):
    if case[0] not in _REF:
        _REF[case[0]] = case_exact(case)
    return _REF[case[0]]


def _against(ref, order, near, counts, summary, what):
    """The device's results of one box against a tet_exact dict; prints every figure before it asserts."""
    nan_ref = np.isnan(ref["order"].astype(np.float64))
    bits = order.view(np.uint64)
    err = np.abs((order.astype(LD) - ref["order"]).astype(np.float64))
    worst = [float(np.max(err[~nan_ref[:, k], k], initial=0.0)) for k in range(4)]
    snan = np.isnan(ref["summary"][:4].astype(np.float64))
    serr = np.abs((summary[:4].astype(LD) - ref["summary"][:4]).astype(np.float64))
    sworst = float(np.max(serr[~snan], initial=0.0))
    wrong = (int(np.count_nonzero(counts != ref["counts"])), int(np.count_nonzero(np.sort(near, axis=1) != np.sort(ref["near"], axis=1))))
    print(what, "max |d| (q, s_k, d5, lsi)", " ".join("%.2e" % v for v in worst), " means %.2e" % sworst, " wrong (counts, near)", wrong)
    assert counts.dtype == np.int32 and near.dtype == np.int32
    assert np.array_equal(counts, ref["counts"]), what
    assert np.array_equal(np.sort(near, axis=1), np.sort(ref["near"], axis=1)), what
    assert np.array_equal(np.isnan(order), nan_ref) and np.all(bits[nan_ref] == NAN_BITS), what
    assert max(worst) <= TOL, what
    assert np.array_equal(np.isnan(summary[:4]), snan) and np.all(summary[:4].view(np.uint64)[snan] == NAN_BITS), what
    assert sworst <= TOL and np.array_equal(summary[4:], ref["summary"][4:].astype(np.float64)), what


# -- against tet_exact ------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_input_matches_the_reference(case):
    from mc_water_ls_mw_amd.tetrahedral import tet_last, tet_plan, tetrahedral_order
    h, xyz, rs, rl = load_case(case)
    got = tetrahedral_order(h, xyz, rs * BOHR_TO_ANG, rl * BOHR_TO_ANG)
    order, near, counts, summary = got
    n = len(xyz)
    assert order.shape == (n, 4) and near.shape == (n, 4) and counts.shape == (n, 2) and summary.shape == (8,)
    _against(_ref(case), order, near, counts, summary, case[0])
    last = tet_last()
    assert last == tet_plan(n, h, rs * BOHR_TO_ANG, 1) and last["small"] == (n <= 64) and last["chunks"] == 1, last
    if "one cell" in case[0]:
        assert not last["small"] and sorted((last["g1"], last["g2"], last["g3"])) == [1, 1, 2], last
    if case[0] == "ih8_small":
        assert (last["g1"], last["g2"], last["g3"]) == (1, 1, 1)
    # the same call again: the same bytes
    assert _all_same(tetrahedral_order(h, xyz, rs * BOHR_TO_ANG, rl * BOHR_TO_ANG), got)


def test_positions_beyond_one_cell_and_null_outputs():
    """Molecules moved by whole cell vectors keep their neighbours; any output may be left out."""
    from mc_water_ls_mw_amd.tetrahedral import load_tet_library, tetrahedral_order
    for label in ("ic64_sheared", "ih1536_t012"):
        case = next(c for c in CASES if c[0] == label)
        h, xyz, rs, rl = load_case(case)
        rng = np.random.default_rng(3)
        moved = xyz + rng.integers(-2, 3, xyz.shape).astype(np.float64) @ h
        got = tetrahedral_order(h, moved, rs * BOHR_TO_ANG, rl * BOHR_TO_ANG)
        _against(_ref(case), *got, label + " displaced")
        L = load_tet_library()
        cells, pos = np.ascontiguousarray(h), np.ascontiguousarray(moved)
        rs_lib, rl_lib = (rs * BOHR_TO_ANG) / BOHR_TO_ANG, (rl * BOHR_TO_ANG) / BOHR_TO_ANG      # as the wrapper converts them
        for keep in range(4):
            outs = [np.zeros_like(o) for o in got]
            ptrs = [o.ctypes.data if k == keep else None for k, o in enumerate(outs)]
            assert L.mw_tet_compute(1, len(xyz), cells.ctypes.data, pos.ctypes.data, rs_lib, rl_lib, *ptrs) == 0
            assert _same(outs[keep], got[keep]), (label, keep)
        assert L.mw_tet_compute(1, len(xyz), cells.ctypes.data, pos.ctypes.data, rs_lib, rl_lib, None, None, None, None) == 0


def test_r_lsi_moves_only_the_lsi():
    z = load_golden("ih48_t020")
    from mc_water_ls_mw_amd.tetrahedral import tetrahedral_order
    a = tetrahedral_order(z["h"], z["xyz"], 5.5, 3.7)
    b = tetrahedral_order(z["h"], z["xyz"], 5.5, 3.3)
    assert _same(a[0][:, :3].copy(), b[0][:, :3].copy()) and _same(a[1], b[1]) and np.array_equal(a[2][:, 0], b[2][:, 0])
    assert np.all(b[2][:, 1] <= a[2][:, 1]) and _same(a[3][:3].copy(), b[3][:3].copy())


# -- bit rules --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", BATCHES)
def test_a_batch_equals_the_single_calls_bit_for_bit(name, n):
    from mc_water_ls_mw_amd.tetrahedral import tetrahedral_order
    hs, xs = batch_set(name, n)                                            # (preconditions of every box: tests/test_tet_ref.py)
    rs, rl = (r * BOHR_TO_ANG for r in batch_radii(hs))
    got = tetrahedral_order(hs, xs, rs, rl)
    nw = xs.shape[1]
    assert got[0].shape == (n, nw, 4) and got[1].shape == (n, nw, 4) and got[2].shape == (n, nw, 2) and got[3].shape == (n, 8)
    for b in range(n):
        assert _all_same(tetrahedral_order(hs[b], xs[b], rs, rl), [o[b] for o in got]), b
    assert len({got[3][b].tobytes() for b in range(n)}) == n
    assert _all_same(tetrahedral_order(hs[1:], xs[1:], rs, rl), [o[1:] for o in got])
    ref = tet_exact(hs[n - 1], xs[n - 1], rs / BOHR_TO_ANG, rl / BOHR_TO_ANG)
    assert min(preconditions(ref)) > MARGIN
    _against(ref, *[o[n - 1] for o in got], f"{name} box {n}")


def _chunk_case():
    return scaled_set("ic96", 250, 0.12, 300)


def test_chunks_give_the_bits_of_one_chunk(tmp_path):
    """A fresh process whose scratch budget is 1 MiB takes the 250 boxes in several chunks, the last one ragged; here they fit one."""
    from mc_water_ls_mw_amd.tetrahedral import tet_last, tet_plan, tetrahedral_order
    hs, xs = _chunk_case()
    got = tetrahedral_order(hs, xs, 5.5, 3.7)
    last = tet_last()
    assert last["chunks"] == 1 and last["boxes_per_chunk"] == 250 and not last["small"]
    out = tmp_path / "chunks.npz"
    env = dict(os.environ, MW_TET_SCRATCH_MB="1")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-3000:])
    z = np.load(out)
    fit = (1 << 20) // last["scratch_bytes_per_box"]
    assert 1 < fit < 250 and 250 % fit != 0
    assert int(z["boxes_per_chunk"]) == fit and int(z["chunks"]) == -(-250 // fit) >= 3
    assert _all_same([z["order"], z["near"], z["counts"], z["summary"]], got)
    assert tet_plan(96, hs[0], 5.5, 250)["chunks"] == 1                     # this process kept its own budget


def test_device_tensors_give_the_bits_of_the_host_entry():
    import torch
    from mc_water_ls_mw_amd.tetrahedral import tetrahedral_order, tetrahedral_order_torch
    dev = torch.device("cuda:0")
    for name, n in (("ic96", 3), ("ih48_t020", 6)):
        hs, xs = scaled_set(name, n, 0.1, 70)
        got = tetrahedral_order(hs, xs, 5.5, 3.7)
        t = tetrahedral_order_torch(torch.from_numpy(hs).to(dev), torch.from_numpy(xs).to(dev), 5.5, 3.7)
        assert all(v.is_cuda for v in t) and t[0].dtype == t[3].dtype == torch.float64 and t[1].dtype == t[2].dtype == torch.int32
        assert _all_same([v.cpu().numpy() for v in t], got)


# -- rejected calls ---------------------------------------------------------------------------
def test_rejected_calls_name_the_argument_and_write_nothing():
    import torch
    from mc_water_ls_mw_amd.tetrahedral import MwError, load_tet_library, tet_elapsed_ms, tet_last, tetrahedral_order
    z = load_golden("ic48")
    h, xyz = z["h"], z["xyz"]
    tetrahedral_order(h, xyz)                                              # the library is live and has launched
    L = load_tet_library()
    before = tet_last()
    cells = np.ascontiguousarray(np.array([h, h, h]).reshape(3, 9))
    pos = np.ascontiguousarray(np.array([xyz, xyz, xyz]))
    flat = cells.copy()
    flat[2, 6:9] = 0.0
    narrow = cells.copy()
    narrow[1] *= 0.3                                                       # box 1 is narrower than 5.5 Angstrom
    rs, rl = 5.5 / BOHR_TO_ANG, 3.7 / BOHR_TO_ANG
    dev = torch.device("cuda:0")
    for c, r, l, pattern in ((flat, rs, rl, r"cells.*box 2\b"), (narrow, rs, rl, r"r_search.*box 1\b"), (cells, float("nan"), rl, "r_search"),
                             (cells, 60.0, rl, r"r_search.*box 0\b"), (cells, rs, float("inf"), "r_lsi"), (cells, rs, 1.01 * rs, r"r_lsi.*r_search")):
        order, near = np.full((3, 48, 4), -7.0), np.full((3, 48, 4), -7, dtype=np.int32)
        counts, summary = np.full((3, 48, 2), -7, dtype=np.int32), np.full((3, 8), -7.0)
        assert L.mw_tet_compute(3, 48, c.ctypes.data, pos.ctypes.data, r, l, order.ctypes.data, near.ctypes.data, counts.ctypes.data,
                                summary.ctypes.data) != 0
        msg = L.mw_tet_last_error().decode()
        assert "mw_tet_compute" in msg and re.search(pattern, msg), msg
        assert np.all(order == -7.0) and np.all(near == -7) and np.all(counts == -7) and np.all(summary == -7.0)
        ct, pt = torch.from_numpy(c).to(dev), torch.from_numpy(pos).to(dev)
        ot = torch.full((3, 48, 4), -7.0, dtype=torch.float64, device=dev)
        nt = torch.full((3, 48, 4), -7, dtype=torch.int32, device=dev)
        kt = torch.full((3, 48, 2), -7, dtype=torch.int32, device=dev)
        st = torch.full((3, 8), -7.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        assert L.mw_tet_compute_device(3, 48, ct.data_ptr(), pt.data_ptr(), r, l, ot.data_ptr(), nt.data_ptr(), kt.data_ptr(), st.data_ptr()) != 0
        msg = L.mw_tet_last_error().decode()
        assert "mw_tet_compute_device" in msg and re.search(pattern, msg), msg
        assert bool((ot == -7.0).all()) and bool((nt == -7).all()) and bool((kt == -7).all()) and bool((st == -7.0).all())
    assert tet_last() == before                                            # nothing launched
    assert all(t >= 0.0 for t in tet_elapsed_ms()) and len(tet_elapsed_ms()) == 3
    with pytest.raises(MwError, match="expected"):
        tetrahedral_order(h, xyz[:, :2])


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
    from mc_water_ls_mw_amd.energy import load_boxes
    from mc_water_ls_mw_amd.tetrahedral import tetrahedral_order
    for name in ("ic96", "ih1536_t012"):
        hs, xs = scaled_set(name, 3, 0.08, 900)
        em = load_boxes(list(hs), list(xs))
        try:
            e0 = em.model_energy_batch(1, 3).copy()
            assert _all_same(em.tetrahedral_order(), tetrahedral_order(hs, xs, 5.5, 3.7))
            assert _all_same(em.tetrahedral_order(2, 2, r_search_ang=5.2, r_lsi_ang=3.5), tetrahedral_order(hs[1:], xs[1:], 5.2, 3.5))
            assert np.array_equal(em.model_energy_batch(1, 3), e0)
        finally:
            em.energy_deinit()


def test_npt_farm_tetrahedral_order_after_device_sweeps():
    em, farm = _npt_farm()
    try:
        h0 = np.array(em.hmatrix)
        farm.sweep(288, seed=51)
        summary, tetra = farm.tetrahedral_order()
        hs = farm.sync_cells()
        assert not np.array_equal(hs, h0)                                  # some volume move was accepted (and synced)
        assert summary.shape == (4, 2, 8) and tetra.shape == (4, 2)
        pos = np.array([farm.positions(b + 1) for b in range(em.num_lattices)])
        order, near, counts, s2 = em.tetrahedral_order(1, em.num_lattices)
        for b in range(em.num_lattices):
            ref = tet_exact(hs[b], pos[b], 5.5 / BOHR_TO_ANG, 3.7 / BOHR_TO_ANG)
            print("box", b, "preconditions", " ".join("%.1e" % v for v in preconditions(ref)), "q > 0.9:", tetra[b // 2, b % 2])
            assert min(preconditions(ref)) > MARGIN                        # (the preconditions of the exact comparisons)
            _against(ref, order[b], near[b], counts[b], summary[b // 2, b % 2], f"farm box {b}")
            assert tetra[b // 2, b % 2] == np.count_nonzero(order[b, :, 0] > 0.9) / 48.0
        assert _same(s2, summary.reshape(8, 8))
        assert np.all(summary[:, :, 0] > 0.8) and np.all(summary[:, :, 4] == 48)   # both lattices are still four-coordinated crystals
    finally:
        em.energy_deinit()


def test_engine_state_is_untouched_by_a_tetrahedral_order_call():
    def run(with_tet):
        em, farm = _npt_farm()
        try:
            farm.sweep(96, seed=41)
            nb = em.num_lattices
            z = load_golden("ic48")
            e0 = em.model_energy_batch(1, nb).copy()
            eo0, en0 = em.delta_energy_batch(1, z["trial_imol"][:64], z["trial_xyz"][:64])
            if with_tet:
                farm.tetrahedral_order()
                em.tetrahedral_order(1, nb, r_search_ang=5.0, r_lsi_ang=3.5)
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
    # the child of test_chunks_give_the_bits_of_one_chunk: MW_TET_SCRATCH_MB is set, so mw_tet_init takes the small budget
    from mc_water_ls_mw_amd.tetrahedral import tet_finalize, tet_last, tetrahedral_order
    hs, xs = _chunk_case()
    order, near, counts, summary = tetrahedral_order(hs, xs, 5.5, 3.7)
    last = tet_last()
    tet_finalize()
    np.savez(sys.argv[1], order=order, near=near, counts=counts, summary=summary, chunks=last["chunks"], boxes_per_chunk=last["boxes_per_chunk"])
