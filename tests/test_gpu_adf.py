"""GPU: the O-O-O angle histograms of libmw_adf.so (angles.angle_counts / _torch, EnergyModule.angle_counts,
WalkerFarm.angle_distribution) against the long-double reference of tests/adf_ref.py.  Every output is an integer and every
comparison here is exact (np.array_equal on hist, counts and summary): the preconditions -- no r^2 within 1e-9 of r_cut^2, no
cos(theta) within 1e-9 of a bin edge, no molecule of a box over the cap within 1e-9 of changing the walk order -- are asserted
for every input in tests/test_adf_ref.py.  Then the bit rules of include/mw_adf.h: the bytes of a box's results depend on the
box, its groups, r_cut and the edges alone."""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from conftest import load_golden
from boo_ref import batch_set, gas_box, scaled_set
from adf_ref import BATCHES, EDGE_SETS, MARGIN, adf_exact, batch_radius, cap_radius, cases, cell_grid, load_case, preconditions

pytestmark = pytest.mark.gpu

BOHR_TO_ANG = 0.5291772108
CASES = cases()
CAP_BOXES = {"small": ((40, 2040), (56, 2056), (64, 2064)), "general": ((65, 2065), (100, 2100), (130, 2130))}
_REF = {}


@pytest.fixture(scope="module", autouse=True)
def _library_lifetime():
    """The library is initialised by its first call here and finalised when this file is done."""
    yield
    from mc_water_ls_mw_amd import angles
    angles.adf_finalize()


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _all_same(a, b):
    return all(_same(x, y) for x, y in zip(a, b))


def _ref(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _run(h, xyz, rc, edges, group=None, ngroups=1):
    """angle_counts at the radius rc (bohr): the wrapper takes Angstrom and divides by the same constant again."""
    from mc_water_ls_mw_amd.angles import angle_counts
    return angle_counts(h, xyz, rc * BOHR_TO_ANG, edges, group, ngroups)


def _lib_radius(rc):
    return (rc * BOHR_TO_ANG) / BOHR_TO_ANG                                # what the library sees of rc


def _against(ref, got, what):
    hist, counts, summary = got
    print(what, "pairs", int(ref["summary"][:, 1].sum()), "binned", int(ref["summary"][:, 2].sum()), "largest count", ref["max_count"],
          "wrong bins", int(np.count_nonzero(hist != ref["hist"])), "wrong counts", int(np.count_nonzero(counts != ref["counts"])))
    assert hist.dtype == np.int64 and counts.dtype == np.int32 and summary.dtype == np.int64
    assert np.array_equal(counts, ref["counts"]), what
    assert np.array_equal(hist, ref["hist"]), what
    assert np.array_equal(summary, ref["summary"]), what
    assert np.array_equal(summary[:, 2], hist.sum(axis=1)), what


# -- against adf_exact --------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_every_input_matches_the_reference(case):
    from mc_water_ls_mw_amd.angles import adf_edges, adf_last, adf_plan
    h, xyz, rc = load_case(case)
    n = len(xyz)
    assert np.array_equal(adf_edges(97, "cos"), EDGE_SETS["cos97"]) and np.array_equal(adf_edges(90, "theta"), EDGE_SETS["theta90"])
    for name in case[4]:
        edges = EDGE_SETS[name]
        ref = _ref((case[0], name), lambda: adf_exact(h, xyz, _lib_radius(rc), edges))
        got = _run(h, xyz, rc, edges)
        assert got[0].shape == (1, len(edges) - 1) and got[1].shape == (n,) and got[2].shape == (1, 4)
        _against(ref, got, f"{case[0]} {name}")
        last = adf_last()
        assert last == adf_plan(n, h, rc * BOHR_TO_ANG, len(edges) - 1, 1, 1) and last["small"] == (n <= 64) and last["chunks"] == 1, last
        assert (last["g1"], last["g2"], last["g3"]) == cell_grid(h, _lib_radius(rc), n)
        if "one cell" in case[0]:
            assert not last["small"] and sorted((last["g1"], last["g2"], last["g3"])) == [1, 1, 2] and got[2][0, 3] >= 1, last
        assert _all_same(_run(h, xyz, rc, edges), got)                     # the same call again: the same bytes


@pytest.mark.parametrize("geometry", ("small", "general"))
def test_the_cap_keeps_the_first_32_of_the_walk(geometry):
    """Three boxes whose largest count is 31, 32 and 33: only the last has centres over the cap, and its histogram is that of
    the first 32 entries of the walk -- not of the 32 nearest, which the reference shows to differ."""
    e = EDGE_SETS["cos97"]
    for (n, seed), want in zip(CAP_BOXES[geometry], (31, 32, 33)):
        h, xyz = gas_box(n, seed)
        rc = _lib_radius(cap_radius(h, xyz, want))
        ref = adf_exact(h, xyz, rc, e)
        assert ref["max_count"] == want and min(preconditions(ref)) > MARGIN
        got = _run(h, xyz, rc, e)
        _against(ref, got, f"cap {geometry} N = {n} largest count {want}")
        assert int(got[1].max()) == want and (got[2][0, 3] >= 1) == (want == 33) and (got[2][0, 3] == 0) == (want < 33)
        if want == 33:
            nearest = adf_exact(h, xyz, rc, e, keep="nearest")
            assert not np.array_equal(nearest["hist"], got[0]) and np.array_equal(nearest["summary"], got[2])


def test_bins_one_two_many_restricted_and_clamped():
    h, xyz, rc = load_case(next(c for c in CASES if c[0] == "ih1536_t012 4.8"))
    h2, xyz2, rc2 = load_case(next(c for c in CASES if c[0] == "gas N = 63"))
    rc, rc2 = _lib_radius(rc), _lib_radius(rc2)
    from mc_water_ls_mw_amd.angles import adf_edges
    for edges in (adf_edges(1, "cos"), adf_edges(2, "cos"), adf_edges(1024, "cos"), adf_edges(1024, "theta"), np.array([-0.6, 0.2]),
                  np.linspace(-0.6, 0.2, 12), np.array([-1.0, -0.999, 0.3])):
        for hh, xx, rr, what in ((h, xyz, rc, "ih1536_t012"), (h2, xyz2, rc2, "gas 63")):
            ref = adf_exact(hh, xx, rr, edges)
            assert min(preconditions(ref)) > MARGIN, (what, len(edges), preconditions(ref))
            _against(ref, _run(hh, xx, rr, edges), f"{what} with {len(edges) - 1} bins in [{edges[0]}, {edges[-1]}]")
            if edges[0] > -1.0:
                assert 0 < ref["summary"][0, 2] < ref["summary"][0, 1]     # binned < enumerated
    # A clamped c: no golden has one (the dimer has a single entry per molecule), so two molecules half a cell vector apart in
    # a sheared cell: each sees the other's two images in exactly opposite directions, and fma(ux, -ux, ...) of a unit vector
    # rounded off the axes is not exactly -1.  Every pair must land in the first bin, whose lower edge is -1.
    cell = np.array([[9.0, 0.0, 0.0], [2.7, 11.0, 0.0], [-1.9, 3.1, 12.5]])
    clamped = 0
    for k in range(8):
        rng = np.random.default_rng(70 + k)
        a = rng.random(3) @ cell
        pair = np.array([a, a + 0.5 * cell[2]])
        ref = adf_exact(cell, pair, 8.0, EDGE_SETS["cos97"])
        assert ref["counts"].tolist() == [2, 2] and ref["hist"][0, 0] == 2 and ref["hist"].sum() == 2
        _against(ref, _run(cell, pair, 8.0, EDGE_SETS["cos97"]), f"collinear images {k}")
        d = 0.5 * cell[2]
        u = d * (1.0 / np.sqrt(d @ d))
        clamped += int(-(u @ u) < -1.0)
    print("pairs whose double dot product is below -1:", clamped)


def test_groups():
    h, xyz, rc = load_case(next(c for c in CASES if c[0] == "ih1536_t012 4.8"))
    hs, xs, rs = load_case(next(c for c in CASES if c[0] == "gas N = 64"))
    e = EDGE_SETS["theta90"]
    for hh, xx, rr, what in ((h, xyz, _lib_radius(rc), "ih1536_t012"), (hs, xs, _lib_radius(rs), "gas 64")):
        n = len(xx)
        rng = np.random.default_rng(17)
        group = rng.integers(-1, 8, n).astype(np.int32)
        whole = _run(hh, xx, rr, e)
        _against(adf_exact(hh, xx, rr, e, group=group, ngroups=8), _run(hh, xx, rr, e, group, 8), f"{what} in 8 groups")
        every = _run(hh, xx, rr, e, np.where(group < 0, 7, group).astype(np.int32), 8)
        assert np.array_equal(every[0].sum(axis=0), whole[0][0]) and np.array_equal(every[2].sum(axis=0), whole[2][0])
        none = _run(hh, xx, rr, e, np.full(n, -1, dtype=np.int32), 3)
        assert none[0].shape == (3, 90) and not none[0].any() and not none[2].any() and np.array_equal(none[1], whole[1])
        assert np.array_equal(every[1], whole[1])
    from mc_water_ls_mw_amd.angles import MwError
    with pytest.raises(MwError, match=r"group = 8 of molecule 5 of box 0\b"):
        bad = np.zeros(len(xs), dtype=np.int32)
        bad[5] = 8
        _run(hs, xs, rs, e, bad, 8)


def test_positions_beyond_one_cell_and_null_outputs():
    """Molecules moved by whole cell vectors keep their angles; any output may be left out."""
    from mc_water_ls_mw_amd.angles import load_adf_library
    e = EDGE_SETS["cos97"]
    for label in ("ic64_sheared 4.8", "ih1536_t012 4.8"):
        case = next(c for c in CASES if c[0] == label)
        h, xyz, rc = load_case(case)
        ref = _ref((label, "cos97"), lambda: adf_exact(h, xyz, _lib_radius(rc), e))
        rng = np.random.default_rng(3)
        moved = xyz + rng.integers(-2, 3, xyz.shape).astype(np.float64) @ h
        got = _run(h, moved, rc, e)
        _against(ref, got, label + " displaced")
        L = load_adf_library()
        cells, pos = np.ascontiguousarray(h), np.ascontiguousarray(moved)
        for keep in range(3):
            outs = [np.full_like(o, -7) for o in got]
            ptrs = [o.ctypes.data if k == keep else None for k, o in enumerate(outs)]
            assert L.mw_adf_compute(1, len(xyz), cells.ctypes.data, pos.ctypes.data, _lib_radius(rc), 97, e.ctypes.data, 1, None, *ptrs) == 0
            assert _same(outs[keep], got[keep]), (label, keep)
        assert L.mw_adf_compute(1, len(xyz), cells.ctypes.data, pos.ctypes.data, _lib_radius(rc), 97, e.ctypes.data, 1, None, None, None, None) == 0


# -- bit rules --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", BATCHES)
def test_a_batch_equals_the_single_calls_bit_for_bit(name, n):
    from mc_water_ls_mw_amd.angles import adf_last, adf_plan, angle_counts
    hs, xs = batch_set(name, n)                                            # (preconditions of every box: tests/test_adf_ref.py)
    rc = batch_radius(hs)
    e = EDGE_SETS["theta90"]
    rng = np.random.default_rng(23)
    group = rng.integers(-1, 3, xs.shape[:2]).astype(np.int32)
    for grp, ng in ((None, 1), (group, 3)):
        got = angle_counts(hs, xs, rc * BOHR_TO_ANG, e, grp, ng)
        nw = xs.shape[1]
        assert got[0].shape == (n, ng, 90) and got[1].shape == (n, nw) and got[2].shape == (n, ng, 4)
        assert adf_last() == adf_plan(nw, hs[0], rc * BOHR_TO_ANG, 90, ng, n)
        for b in range(n):
            one = angle_counts(hs[b], xs[b], rc * BOHR_TO_ANG, e, None if grp is None else grp[b], ng)
            assert _all_same(one, [o[b] for o in got]), b
        assert len({got[0][b].tobytes() for b in range(n)}) == n
        tail = angle_counts(hs[1:], xs[1:], rc * BOHR_TO_ANG, e, None if grp is None else grp[1:], ng)
        assert _all_same(tail, [o[1:] for o in got])
        ref = adf_exact(hs[n - 1], xs[n - 1], _lib_radius(rc), e, group=None if grp is None else grp[n - 1], ngroups=ng)
        _against(ref, [o[n - 1] for o in got], f"{name} box {n} in {ng} groups")


def _chunk_case():
    hs, xs = scaled_set("ic96", 250, 0.12, 300)
    return hs, xs, np.random.default_rng(29).integers(-1, 2, xs.shape[:2]).astype(np.int32)


def test_chunks_give_the_bits_of_one_chunk(tmp_path):
    """A fresh process whose scratch budget is 1 MiB takes the 250 boxes in several chunks, the last one ragged; here they fit one."""
    from mc_water_ls_mw_amd.angles import adf_last, adf_plan, angle_counts
    hs, xs, group = _chunk_case()
    got = angle_counts(hs, xs, 3.5, EDGE_SETS["theta90"], group, 2)
    last = adf_last()
    assert last["chunks"] == 1 and last["boxes_per_chunk"] == 250 and not last["small"]
    out = tmp_path / "chunks.npz"
    env = dict(os.environ, MW_ADF_SCRATCH_MB="1")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-3000:])
    z = np.load(out)
    fit = (1 << 20) // last["scratch_bytes_per_box"]
    assert 1 < fit < 250 and 250 % fit != 0
    assert int(z["boxes_per_chunk"]) == fit and int(z["chunks"]) == -(-250 // fit) >= 3
    assert _all_same([z["hist"], z["counts"], z["summary"]], got)
    assert adf_plan(96, hs[0], 3.5, 90, 2, 250)["chunks"] == 1               # this process kept its own budget


def test_device_tensors_give_the_bits_of_the_host_entry():
    import torch
    from mc_water_ls_mw_amd.angles import angle_counts, angle_counts_torch
    dev = torch.device("cuda:0")
    e = EDGE_SETS["theta90"]
    for name, n in (("ic96", 3), ("ih48_t020", 6)):
        hs, xs = scaled_set(name, n, 0.1, 70)
        group = np.random.default_rng(31).integers(-1, 4, xs.shape[:2]).astype(np.int32)
        for grp, ng in ((None, 1), (group, 4)):
            got = angle_counts(hs, xs, 4.8 if name == "ic96" else 3.5, e, grp, ng)
            t = angle_counts_torch(torch.from_numpy(hs).to(dev), torch.from_numpy(xs).to(dev), 4.8 if name == "ic96" else 3.5, e,
                                   None if grp is None else torch.from_numpy(grp).to(dev), ng)
            assert all(v.is_cuda for v in t) and t[0].dtype == t[2].dtype == torch.int64 and t[1].dtype == torch.int32
            assert _all_same([v.cpu().numpy() for v in t], got)
    from mc_water_ls_mw_amd.angles import MwError
    bad = torch.full(xs.shape[:2], 4, dtype=torch.int32, device=dev)
    with pytest.raises(MwError, match=r"mw_adf_compute_device.*group = 4 of molecule 0 of box 0\b"):
        angle_counts_torch(torch.from_numpy(hs).to(dev), torch.from_numpy(xs).to(dev), 3.5, e, bad, 4)


# -- with the engine in the same process ------------------------------------------------------
def test_engine_boxes_give_what_the_arrays_give():
    from mc_water_ls_mw_amd.angles import angle_counts
    from mc_water_ls_mw_amd.energy import load_boxes
    z1, z2 = load_golden("ic48"), load_golden("ih48")                      # a two-lattice pair of 48 molecules
    from mc_water_ls_mw_amd import lattice as lat
    hs = np.array([z1["h"], z2["h"]])
    xs = np.array([lat.thermalise(z1["xyz"], 0.08, 900), lat.thermalise(z2["xyz"], 0.08, 901)])
    em = load_boxes(list(hs), list(xs))
    try:
        e0 = em.model_energy_batch(1, 2).copy()
        assert _all_same(em.angle_counts(), angle_counts(hs, xs))
        group = np.random.default_rng(37).integers(-1, 2, (1, 48)).astype(np.int32)
        got = em.angle_counts(2, 1, r_cut_ang=4.8, edges=EDGE_SETS["cos97"], group=group, ngroups=2)
        assert _all_same(got, angle_counts(hs[1:], xs[1:], 4.8, EDGE_SETS["cos97"], group, 2)) and got[0].shape == (1, 2, 97)
        assert np.array_equal(em.model_energy_batch(1, 2), e0)
    finally:
        em.energy_deinit()


def test_farm_angle_distribution_by_ice_class_on_ideal_lattices():
    from mc_water_ls_mw_amd.energy import ICE_CLASS_NAMES, load_boxes
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
        theta, p, capped = farm.angle_distribution(by="ice_class")
        assert theta.shape == (90,) and p.shape == (2, 6, 90) and capped.shape == (nw, 2) and not capped.any()
        cubic, hexagonal = ICE_CLASS_NAMES.index("cubic ice"), ICE_CLASS_NAMES.index("hexagonal ice")
        peak = int(np.argmin(np.abs(theta - 109.47)))
        assert abs(theta[peak] - 109.0) < 1e-9                             # the bin from 108 to 110 degrees
        for lattice, own in ((0, cubic), (1, hexagonal)):
            for g in range(6):
                if g == own:
                    assert int(np.argmax(p[lattice, g])) == peak and abs(p[lattice, g].sum() * 2.0 - 1.0) < 1e-12
                else:
                    assert not p[lattice, g].any(), (lattice, ICE_CLASS_NAMES[g])
        theta1, p1, capped1 = farm.angle_distribution()
        assert p1.shape == (2, 1, 90) and np.array_equal(theta1, theta) and not capped1.any()
        assert np.array_equal(p1[0, 0], p[0, cubic]) and np.array_equal(p1[1, 0], p[1, hexagonal])
        with pytest.raises(ValueError):
            farm.angle_distribution(by="colour")
    finally:
        em.energy_deinit()


if __name__ == "__main__":
    # the child of test_chunks_give_the_bits_of_one_chunk: MW_ADF_SCRATCH_MB is set, so mw_adf_init takes the small budget
    from mc_water_ls_mw_amd.angles import adf_finalize, adf_last, angle_counts
    hs, xs, group = _chunk_case()
    hist, counts, summary = angle_counts(hs, xs, 3.5, EDGE_SETS["theta90"], group, 2)
    last = adf_last()
    adf_finalize()
    np.savez(sys.argv[1], hist=hist, counts=counts, summary=summary, chunks=last["chunks"], boxes_per_chunk=last["boxes_per_chunk"])
