"""GPU: the ring statistics of libmw_rings.so (rings.ring_statistics / _torch, EnergyModule.ring_statistics,
WalkerFarm.ring_statistics) against the depth-first search of tests/rings_ref.py.  Every output is an integer and every
comparison here is exact (np.array_equal on hist, closed, member, counts, summary and list): the one precondition -- no r^2
within 1e-9 of r_cut^2 -- is asserted for every input in tests/test_rings_ref.py.  Then the bit rules of include/mw_rings.h:
the bytes of a box's results depend on the box and r_cut alone."""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from conftest import load_golden
from boo_ref import batch_set, scaled_set
from rings_ref import AT_THE_CAP, BATCHES, HOT, ICE, PARTLY_CAPPED, case_exact, cases, lib_radius, outputs, rings_exact

pytestmark = pytest.mark.gpu

BOHR_TO_ANG = 0.5291772108
CASES = cases()
NAMES = ("hist", "closed", "member", "counts", "summary", "list")


@pytest.fixture(scope="module", autouse=True)
def _library_lifetime():
    """The library is initialised by its first call here and finalised when this file is done."""
    yield
    from mc_water_ls_mw_amd import rings
    rings.rings_finalize()


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _all_same(a, b):
    return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))


def _case(label):
    return next(c for c in CASES if c[0] == label)


def _run(h, xyz, rc, list_cap=0):
    """ring_statistics at the radius rc (bohr): the wrapper takes Angstrom and divides by the same constant again."""
    from mc_water_ls_mw_amd.rings import ring_statistics
    return ring_statistics(h, xyz, rc * BOHR_TO_ANG, list_cap)


def _against(ref, got, list_cap, what):
    want = outputs(ref, list_cap)
    print(what, "hist", got[0].tolist(), "closed", got[1].tolist(), "summary", got[4].tolist(), "largest count", ref["max_count"],
          "wrong", [name for name, g, w in zip(NAMES, got, want) if not np.array_equal(g, w)])
    assert [g.dtype for g in got] == [np.int64, np.int64, np.int32, np.int32, np.int64, np.int32]
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (what, name)
    assert np.array_equal(got[2].sum(axis=0), np.arange(3, 8) * got[0]) and got[4][3] == got[0].sum(), what


# -- against rings_exact ------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_input_matches_the_reference(case):
    from mc_water_ls_mw_amd.rings import rings_last, rings_plan
    h, xyz, rc, ref = case_exact(case)
    n = len(xyz)
    cap = len(ref["rings"]) + 3                                            # ample: every ring and three rows left at -1
    got = _run(h, xyz, rc, cap)
    _against(ref, got, cap, case[0])
    last = rings_last()
    assert last == rings_plan(n, h, rc * BOHR_TO_ANG, 1) and last["small"] == (n <= 64) and last["chunks"] == 1, last
    assert _all_same(_run(h, xyz, rc, cap), got)                           # the same call again: the same bytes
    if case[0].split(" 3.5")[0] in ICE:
        assert got[0].tolist() == got[1].tolist() == [0, 0, 0, 2 * n, 0] and np.all(got[2][:, 3] == 12)
    if case[0] == AT_THE_CAP:
        assert 8 in got[3] and 9 in got[3] and got[4][0] == int((got[3] > 8).sum()) > 0
    if case[0] in PARTLY_CAPPED:
        assert got[4][0] > 0 and got[4][3] > 0
    if case[0] == "ih1536_t012 4.8":
        assert got[4].tolist() == [n, 0, 0, 0] and not got[0].any() and not got[1].any() and not got[2].any()


def test_list_cap_none_short_and_ample():
    key = ("ih", (3, 2, 2), 0.5, 2)
    h, xyz, rc, ref = case_exact(_case(f"{key[0]}{key[1]} sigma {key[2]} seed {key[3]}"))
    total = int(ref["summary"][3])
    assert total == sum(HOT[key][0]) == len(ref["rings"]) > 50
    full = _run(h, xyz, rc, total)
    _against(ref, full, total, "exactly enough rows")
    for cap in (0, 1, 50, total + 40):
        got = _run(h, xyz, rc, cap)
        _against(ref, got, cap, f"list_cap {cap}")
        k = min(cap, total)
        assert got[5].shape == (cap, 8) and np.array_equal(got[5][:k], full[5][:k]) and np.all(got[5][k:] == -1)
        assert _all_same(got[:5], full[:5])                                # the list changes nothing else
    roots = full[5][:, 1]
    assert np.all(np.diff(roots) >= 0) and np.all(full[5][:, 1:].max(axis=1) >= roots)


def test_positions_beyond_one_cell_and_null_outputs():
    """Molecules moved by whole cell vectors keep their rings; any output may be left out, and all of them."""
    from mc_water_ls_mw_amd.rings import load_rings_library
    for label in ("ic64_sheared 3.5", "ih(4, 3, 3) sigma 0.6 seed 4"):
        h, xyz, rc, ref = case_exact(_case(label))
        cap = len(ref["rings"])
        rng = np.random.default_rng(3)
        moved = xyz + rng.integers(-2, 3, xyz.shape).astype(np.float64) @ h
        got = _run(h, moved, rc, cap)
        _against(ref, got, cap, label + " displaced")
        L = load_rings_library()
        cells, pos = np.ascontiguousarray(h), np.ascontiguousarray(moved)
        for keep in range(6):
            outs = [np.full_like(o, -7) for o in got]
            ptrs = [o.ctypes.data if k == keep else None for k, o in enumerate(outs)]
            assert L.mw_rings_compute(1, len(xyz), cells.ctypes.data, pos.ctypes.data, lib_radius(rc), cap, *ptrs) == 0
            assert _same(outs[keep], got[keep]), (label, NAMES[keep])
        assert L.mw_rings_compute(1, len(xyz), cells.ctypes.data, pos.ctypes.data, lib_radius(rc), cap, None, None, None, None, None, None) == 0


# -- bit rules --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", BATCHES)
def test_a_batch_equals_the_single_calls_bit_for_bit(name, n):
    from mc_water_ls_mw_amd.rings import ring_statistics, rings_last, rings_plan
    hs, xs = batch_set(name, n)                                            # (preconditions of every box: tests/test_rings_ref.py)
    nw = xs.shape[1]
    cap = 2 * nw + 8
    got = ring_statistics(hs, xs, 3.5, cap)
    assert [g.shape for g in got] == [(n, 5), (n, 5), (n, nw, 5), (n, nw), (n, 4), (n, cap, 8)]
    assert rings_last() == rings_plan(nw, hs[0], 3.5, n)
    for b in range(n):
        assert _all_same(ring_statistics(hs[b], xs[b], 3.5, cap), [o[b] for o in got]), b
    assert _all_same(ring_statistics(hs[1:], xs[1:], 3.5, cap), [o[1:] for o in got])
    _against(rings_exact(hs[n - 1], xs[n - 1], lib_radius(3.5 / BOHR_TO_ANG)), [o[n - 1] for o in got], cap, f"{name} box {n}")


def _chunk_case():
    return scaled_set("ih48_t020", 250, 0.3, 500)


def test_chunks_give_the_bits_of_one_chunk(tmp_path):
    """A fresh process whose scratch budget is 1 MiB takes the 250 boxes in several chunks, the last one ragged; here they fit one."""
    from mc_water_ls_mw_amd.rings import ring_statistics, rings_last, rings_plan
    hs, xs = _chunk_case()
    got = ring_statistics(hs, xs, 3.5, 120)
    last = rings_last()
    assert last["chunks"] == 1 and last["boxes_per_chunk"] == 250 and last["small"]
    assert len({got[0][b].tobytes() for b in range(250)}) > 20             # hot boxes: not 250 times the ice answer
    out = tmp_path / "chunks.npz"
    env = dict(os.environ, MW_RINGS_SCRATCH_MB="1")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-3000:])
    z = np.load(out)
    fit = (1 << 20) // last["scratch_bytes_per_box"]
    assert 1 < fit < 250 and 250 % fit != 0
    assert int(z["boxes_per_chunk"]) == fit and int(z["chunks"]) == -(-250 // fit) >= 2
    assert _all_same([z[k] for k in NAMES], got)
    assert rings_plan(48, hs[0], 3.5, 250)["chunks"] == 1                   # this process kept its own budget


def test_device_tensors_give_the_bits_of_the_host_entry():
    import torch
    from mc_water_ls_mw_amd.rings import ring_statistics, ring_statistics_torch
    dev = torch.device("cuda:0")
    for name, n in (("ic96", 3), ("ih48_t020", 6)):
        hs, xs = scaled_set(name, n, 0.3, 70)
        for cap in (0, 150):
            got = ring_statistics(hs, xs, 3.5, cap)
            t = ring_statistics_torch(torch.from_numpy(hs).to(dev), torch.from_numpy(xs).to(dev), 3.5, cap)
            assert all(v.is_cuda for v in t) and [v.dtype for v in t] == [torch.int64, torch.int64, torch.int32, torch.int32, torch.int64, torch.int32]
            assert _all_same([v.cpu().numpy() for v in t], got)
    from mc_water_ls_mw_amd.rings import MwError
    with pytest.raises(MwError, match=r"mw_rings_compute_device.*r_cut.*box 1\b"):
        narrow = hs.copy()
        narrow[1] *= 0.2
        ring_statistics_torch(torch.from_numpy(narrow).to(dev), torch.from_numpy(xs).to(dev), 3.5)


# -- with the engine in the same process ------------------------------------------------------
def test_engine_boxes_give_what_the_arrays_give():
    from mc_water_ls_mw_amd.rings import ring_statistics
    from mc_water_ls_mw_amd.energy import load_boxes
    from mc_water_ls_mw_amd import lattice as lat
    z1, z2 = load_golden("ic48"), load_golden("ih48")                      # a two-lattice pair of 48 molecules
    hs = np.array([z1["h"], z2["h"]])
    xs = np.array([lat.thermalise(z1["xyz"], 0.3, 900), lat.thermalise(z2["xyz"], 0.3, 901)])
    em = load_boxes(list(hs), list(xs))
    try:
        e0 = em.model_energy_batch(1, 2).copy()
        assert _all_same(em.ring_statistics(), ring_statistics(hs, xs))
        got = em.ring_statistics(2, 1, r_cut_ang=3.4, list_cap=100)
        assert _all_same(got, ring_statistics(hs[1:], xs[1:], 3.4, 100)) and got[5].shape == (1, 100, 8) and got[4][0, 3] > 0
        assert np.array_equal(em.model_energy_batch(1, 2), e0)
    finally:
        em.energy_deinit()


def test_farm_of_ideal_lattices_reports_2n_six_rings_per_walker():
    from mc_water_ls_mw_amd.energy import load_boxes
    from mc_water_ls_mw_amd.sweep import MuGrid, WalkerFarm
    z1, z2 = load_golden("ic48"), load_golden("ih48")                      # ideal cubic and hexagonal ice
    nw = 3
    em = load_boxes([z1["h"], z2["h"]] * nw, [z1["xyz"], z2["xyz"]] * nw)
    try:
        farm = WalkerFarm(em, 2, 200.0, 1.1, grid=MuGrid(101, -400.0, 400.0), weight=np.zeros(101), pressure_au=1.0 / 2.90363081e8)
        farm.options(record=True, samplerun=False, always_switch=True, npt=True, wl_factor=0.05)
        farm.moves(trans_prob=0.5, vol_prob=0.2, dv_max_ang=0.924)
        for w in range(1, nw + 1):
            farm.set_state(w, 1 + (w % 2), farm.initial_mu(w))
        hist, six, capped = farm.ring_statistics()
        assert hist.shape == (nw, 2, 5) and six.shape == capped.shape == (nw, 2) and not capped.any()
        assert np.all(hist == np.array([0, 0, 0, 96, 0])) and np.all(six == 12.0)
    finally:
        em.energy_deinit()


if __name__ == "__main__":
    # the child of test_chunks_give_the_bits_of_one_chunk: MW_RINGS_SCRATCH_MB is set, so mw_rings_init takes the small budget
    from mc_water_ls_mw_amd.rings import ring_statistics, rings_finalize, rings_last
    hs, xs = _chunk_case()
    got = ring_statistics(hs, xs, 3.5, 120)
    last = rings_last()
    rings_finalize()
    np.savez(sys.argv[1], chunks=last["chunks"], boxes_per_chunk=last["boxes_per_chunk"], **dict(zip(NAMES, got)))
