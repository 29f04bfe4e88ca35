"""GPU: the inherent-structure quenches of libmw_quench.so (quench.inherent_structures / _torch,
EnergyModule.inherent_structures, WalkerFarm.inherent_structures) against the numpy mirror of tests/quench_ref.py and against
the engine, and the bit rules of include/mw_quench.h: the bytes of a box's results depend on its cell, its positions, ftol,
max_iter and fire alone.

Bars.  Energies: conftest.RTOL = 1e-10 relative.  Forces of a single point: quench_ref.F_ATOL = 1e-10 Hartree / bohr absolute.
Positions after a quench: quench_ref.POS_TOL = 4.3e-7 bohr, ten times the largest spread max |x(ftol 1e-10) - x(ftol 1e-12)|
= 4.3e-8 bohr the mirror shows over its five bar cases on the CPU (1.8e-8 ... 4.3e-8; the 65-molecule box, 2.2e-7, is held
to the bar and is not part of it) -- the softest mode sets it, and the device's rounding may move the stopping iteration by one
or two.  The centre of mass: quench_ref.COM_TOL = 1e-12 bohr.  The preconditions (the mirror and L-BFGS-B reach the same
minimum for every case compared here) are asserted in tests/test_quench_ref.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from conftest import RTOL, load_golden
from boo_ref import scaled_set
from quench_ref import COM_TOL, F_ATOL, FTOL, POINT_CASES, POS_TOL, QUENCH_CASES, energy_forces, load_case, reference

pytestmark = pytest.mark.gpu

MAX_ITER = 5000


@pytest.fixture(scope="module", autouse=True)
def _library_lifetime():
    """The library is initialised by its first call here and finalised when this file is done."""
    yield
    from mc_water_ls_mw_amd import quench
    quench.quench_finalize()


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _all_same(a, b):
    return all(_same(x, y) for x, y in zip(a, b))


def _engine(h, xyz):
    """(E, F) of one box from the engine's two passes over its own lists."""
    from mc_water_ls_mw_amd.energy import load_boxes
    em = load_boxes([h], [xyz])
    try:
        e, f, _ = em.forces_batch()
        return float(e[0]), f[0].copy()
    finally:
        em.energy_deinit()


def _consistent(pos, pos_out, forces, stats, iters, what):
    """stats against the other outputs of the same box."""
    disp = np.sqrt(((pos_out - pos) ** 2).sum(axis=1))
    print(what, "stats", " ".join("%.17g" % v for v in stats), "iters", tuple(iters))
    assert stats[3] == np.abs(forces).max(), what                          # the largest component of the forces returned, bit for bit
    assert abs(stats[4] - disp.max()) <= 1e-14 * max(1.0, disp.max()) and abs(stats[5] - np.sqrt((disp * disp).mean())) <= 1e-14 * max(1.0, disp.max()), what
    assert iters.dtype == np.int32 and iters[1] == (1 if stats[3] <= FTOL else 0), what


# -- single points ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", POINT_CASES)
def test_a_single_point_is_the_energy_and_the_forces_of_the_engine_and_of_the_reference(name):
    from mc_water_ls_mw_amd.quench import inherent_structures, quench_last
    h, xyz = load_case(name)
    pos_out, forces, stats, iters = inherent_structures(h, xyz, FTOL, 0)
    n = len(xyz)
    assert pos_out.shape == (n, 3) and forces.shape == (n, 3) and stats.shape == (6,) and iters.shape == (2,)
    assert quench_last()["small"] == (n <= 64) and quench_last()["chunks"] == 1
    e_ref, f_ref = energy_forces(h, xyz)
    e_eng, f_eng = _engine(h, xyz)
    print(name, n, "E %.15g" % stats[0], "dE/E (reference, engine) %.1e %.1e" % (abs(stats[0] - e_ref) / max(abs(e_ref), 1e-300), abs(stats[0] - e_eng) / max(abs(e_eng), 1e-300)),
          "max |dF| (reference, engine) %.1e %.1e" % (np.abs(forces - f_ref).max(), np.abs(forces - f_eng).max()), "max |F| %.3g" % np.abs(f_ref).max())
    assert abs(stats[0] - e_ref) <= RTOL * abs(e_ref) and abs(stats[0] - e_eng) <= RTOL * abs(e_eng)
    assert np.abs(forces - f_ref).max() <= F_ATOL and np.abs(forces - f_eng).max() <= F_ATOL
    assert _same(pos_out, np.ascontiguousarray(xyz))                       # bit for bit
    assert stats[0] == stats[1] and stats[2] == stats[3] and stats[4] == 0.0 and stats[5] == 0.0
    assert tuple(iters) == (0, 1 if stats[2] <= FTOL else 0) and (iters[1] == 1) == (name == "single_atom")
    _consistent(xyz, pos_out, forces, stats, iters, name)


# -- quenches against the mirror --------------------------------------------------------------
@pytest.mark.parametrize("name", QUENCH_CASES)
def test_a_quench_lands_where_the_mirror_lands(name):
    from mc_water_ls_mw_amd.quench import inherent_structures
    h, xyz = load_case(name)
    ref = reference(name)                                                  # (computed once per process, read-only)
    got = inherent_structures(h, xyz, FTOL, MAX_ITER)
    pos_out, forces, stats, iters = got
    de = abs(stats[1] - ref["stats"][1]) / abs(ref["stats"][1])
    dx = float(np.abs(pos_out - ref["pos"]).max())
    com = float(np.abs(pos_out.mean(axis=0) - xyz.mean(axis=0)).max())
    print(name, len(xyz), "iterations", int(iters[0]), "mirror", int(ref["iters"][0]), "dE/E %.1e" % de, "max |dx| %.2e" % dx, "fmax %.2e" % stats[3],
          "centre of mass %.1e" % com)
    assert iters[1] == 1 and 0 < iters[0] <= MAX_ITER
    assert stats[3] <= FTOL
    assert de <= RTOL
    assert dx <= POS_TOL
    assert com <= COM_TOL
    assert abs(stats[0] - ref["stats"][0]) <= RTOL * abs(ref["stats"][0]) and abs(stats[2] - ref["stats"][2]) <= F_ATOL
    assert abs(stats[4] - ref["stats"][4]) <= POS_TOL and abs(stats[5] - ref["stats"][5]) <= POS_TOL
    _consistent(xyz, pos_out, forces, stats, iters, name)
    assert _all_same(inherent_structures(h, xyz, FTOL, MAX_ITER), got)     # the same call again: the same bytes


def test_a_box_of_several_workgroups_converges_to_the_energy_the_engine_sees():
    from mc_water_ls_mw_amd.quench import inherent_structures, quench_last
    h, xyz = load_case("ih1536_t012")
    pos_out, forces, stats, iters = inherent_structures(h, xyz, FTOL, MAX_ITER)
    last = quench_last()
    assert not last["small"] and last["chunks"] == 1
    e_eng, f_eng = _engine(h, pos_out)
    print("ih1536_t012 iterations", tuple(iters), "E %.15g engine %.15g" % (stats[1], e_eng), "fmax %.3e engine %.3e" % (stats[3], np.abs(f_eng).max()))
    assert iters[1] == 1 and stats[3] <= FTOL
    assert abs(stats[1] - e_eng) <= RTOL * abs(e_eng)
    assert np.abs(f_eng).max() <= FTOL * (1.0 + 1e-3)
    _consistent(xyz, pos_out, forces, stats, iters, "ih1536_t012")
    h0, xyz0 = load_case("ih1536")                                         # the same ice without the thermal noise
    assert np.array_equal(h0, h)
    _, _, stats0, iters0 = inherent_structures(h0, xyz0, FTOL, MAX_ITER)
    print("ih1536 iterations", tuple(iters0), "E %.15g" % stats0[1], "dE %.1e" % abs(stats0[1] - stats[1]))
    assert iters0[1] == 1 and abs(stats0[1] - stats[1]) <= RTOL * abs(stats[1])


def test_max_iter_stops_a_box_unconverged_with_the_energy_of_where_it_is():
    from mc_water_ls_mw_amd.quench import inherent_structures
    for name in ("ih48_t020", "ic96"):                                     # one box of each geometry
        h, xyz = load_case(name)
        pos_out, forces, stats, iters = inherent_structures(h, xyz, FTOL, 10)
        e_eng, f_eng = _engine(h, pos_out)
        print(name, "E %.15g engine %.15g" % (stats[1], e_eng), "fmax %.3e" % stats[3])
        assert tuple(iters) == (10, 0)
        assert abs(stats[1] - e_eng) <= RTOL * abs(e_eng) and np.abs(forces - f_eng).max() <= F_ATOL
        assert stats[1] < stats[0] and not np.array_equal(pos_out, xyz)
        _consistent(xyz, pos_out, forces, stats, iters, name)


# -- bit rules --------------------------------------------------------------------------------
def _batches():
    """One batch per geometry whose boxes stop at different iterations: (cells, positions)."""
    return [scaled_set("ih48_t020", 6, 0.1, 40), scaled_set("ic96", 5, 0.1, 40)]


@pytest.mark.parametrize("k", (0, 1), ids=("small", "general"))
def test_a_batch_equals_the_single_calls_bit_for_bit(k):
    from mc_water_ls_mw_amd.quench import inherent_structures
    hs, xs = _batches()[k]
    got = inherent_structures(hs, xs, FTOL, MAX_ITER)
    n, nw = xs.shape[0], xs.shape[1]
    assert got[0].shape == (n, nw, 3) and got[1].shape == (n, nw, 3) and got[2].shape == (n, 6) and got[3].shape == (n, 2)
    print("iterations", got[3][:, 0])
    assert np.all(got[3][:, 1] == 1) and len(set(got[3][:, 0])) > 1         # they stop at different iterations
    for b in range(n):
        assert _all_same(inherent_structures(hs[b], xs[b], FTOL, MAX_ITER), [o[b] for o in got]), b
    assert _all_same(inherent_structures(hs[1:], xs[1:], FTOL, MAX_ITER), [o[1:] for o in got])
    # ... and a box that stops early does not depend on max_iter cutting the others short
    short = int(got[3][:, 0].min())
    cut = inherent_structures(hs, xs, FTOL, short)
    b = int(got[3][:, 0].argmin())
    assert _all_same([o[b] for o in cut], [o[b] for o in got]) and np.count_nonzero(cut[3][:, 1]) < n


def test_device_tensors_and_null_outputs_give_the_bits_of_the_host_entry():
    import torch
    from mc_water_ls_mw_amd.quench import inherent_structures, inherent_structures_torch, load_quench_library
    dev = torch.device("cuda:0")
    for hs, xs in _batches():
        got = inherent_structures(hs, xs, FTOL, MAX_ITER)
        t = inherent_structures_torch(torch.from_numpy(hs).to(dev), torch.from_numpy(xs).to(dev), FTOL, MAX_ITER)
        assert all(v.is_cuda for v in t) and t[0].dtype == t[2].dtype == torch.float64 and t[3].dtype == torch.int32
        assert _all_same([v.cpu().numpy() for v in t], got)
        L = load_quench_library()
        cells, pos = np.ascontiguousarray(hs), np.ascontiguousarray(xs)
        for keep in range(4):
            outs = [np.zeros_like(o) for o in got]
            ptrs = [o.ctypes.data if j == keep else None for j, o in enumerate(outs)]
            assert L.mw_quench_compute(len(xs), xs.shape[1], cells.ctypes.data, pos.ctypes.data, FTOL, MAX_ITER, None, *ptrs) == 0
            assert _same(outs[keep], got[keep]), keep
        assert L.mw_quench_compute(len(xs), xs.shape[1], cells.ctypes.data, pos.ctypes.data, FTOL, MAX_ITER, None, None, None, None, None) == 0
        # fire = the defaults spelled out: the same bytes; another dt0: another trajectory
        from mc_water_ls_mw_amd.quench import FIRE_DEFAULTS
        assert _all_same(inherent_structures(hs, xs, FTOL, MAX_ITER, fire=FIRE_DEFAULTS), got)
        other = inherent_structures(hs, xs, FTOL, MAX_ITER, fire=dict(dt0=10.0))
        assert np.all(other[3][:, 1] == 1) and not _same(other[0], got[0])
        assert np.abs(other[2][:, 1] - got[2][:, 1]).max() <= RTOL * np.abs(got[2][:, 1]).max()


def _chunk_cases():
    """More boxes of each geometry than 1 MiB of scratch holds."""
    return [scaled_set("ic48_t015", 320, 0.05, 300), scaled_set("ic96", 50, 0.05, 300)]


def test_chunks_looks_and_slices_do_not_change_a_byte(tmp_path):
    """A fresh process with 1 MiB of scratch (several chunks, the last one ragged), a look of the host every 3 iterations
    instead of 32 and 5 iterations per launch of the small geometry instead of 64 returns the bytes of this process; a second
    one with a look every 7 iterations and 2 per launch does too."""
    from mc_water_ls_mw_amd.quench import inherent_structures, quench_last, quench_plan
    got, fits = [], []
    for hs, xs in _chunk_cases():
        got.append(inherent_structures(hs, xs, 1e-8, MAX_ITER))
        last = quench_last()
        assert last["chunks"] == 1 and last["boxes_per_chunk"] == len(xs)
        fits.append((1 << 20) // last["scratch_bytes_per_box"])
        assert 1 < fits[-1] < len(xs) and len(xs) % fits[-1] != 0
        assert np.all(got[-1][3][:, 1] == 1)
    for mb, look, piece in (("1", "3", "5"), ("", "7", "2")):
        out = tmp_path / f"chunks_{look}.npz"
        env = dict(os.environ, MW_QUENCH_SCRATCH_MB=mb, MW_QUENCH_LOOK=look, MW_QUENCH_SLICE=piece)
        res = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], capture_output=True, text=True, timeout=300, env=env)
        assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-3000:])
        z = np.load(out)
        for k in range(2):
            if mb:
                assert int(z[f"boxes_per_chunk{k}"]) == fits[k] and int(z[f"chunks{k}"]) == -(-len(got[k][0]) // fits[k]) >= 2
            else:
                assert int(z[f"chunks{k}"]) == 1
            assert _all_same([z[f"pos_out{k}"], z[f"forces{k}"], z[f"stats{k}"], z[f"iters{k}"]], got[k]), (mb, look, piece, k)
    assert quench_plan(96, _chunk_cases()[1][0][0], 50)["chunks"] == 1     # this process kept its own budget


# -- rejected calls ---------------------------------------------------------------------------
def test_rejected_calls_name_the_argument_and_write_nothing():
    import torch
    from mc_water_ls_mw_amd.quench import MwError, inherent_structures, load_quench_library, quench_elapsed_ms, quench_last
    z = load_golden("ic48")
    h, xyz = z["h"], z["xyz"]
    inherent_structures(h, xyz, FTOL, 5)                                   # the library is live and has launched
    L = load_quench_library()
    before = quench_last()
    cells = np.ascontiguousarray(np.array([h, h, h]).reshape(3, 9))
    pos = np.ascontiguousarray(np.array([xyz, xyz, xyz]))
    flat = cells.copy()
    flat[2, 6:9] = 0.0
    narrow = cells.copy()
    narrow[1] *= 0.3                                                       # box 1 is narrower than a sigma
    bad_fire = np.array([20.0, 200.0, 0.2, 0.1, 0.99, 1.1, float("nan"), 5.0])
    dev = torch.device("cuda:0")
    for c, ftol, mi, fire, pattern in ((flat, FTOL, 5, None, r"cells.*box 2\b"), (narrow, FTOL, 5, None, r"a_sigma.*box 1\b"), (cells, float("nan"), 5, None, "ftol"),
                                       (cells, FTOL, -1, None, "max_iter"), (cells, FTOL, 5, bad_fire, r"fire\[6\] \(f_dec\)")):
        fp = None if fire is None else fire.ctypes.data
        po, fo = np.full((3, 48, 3), -7.0), np.full((3, 48, 3), -7.0)
        st, it = np.full((3, 6), -7.0), np.full((3, 2), -7, dtype=np.int32)
        assert L.mw_quench_compute(3, 48, c.ctypes.data, pos.ctypes.data, ftol, mi, fp, po.ctypes.data, fo.ctypes.data, st.ctypes.data, it.ctypes.data) != 0
        msg = L.mw_quench_last_error().decode()
        assert "mw_quench_compute" in msg and re.search(pattern, msg), msg
        assert np.all(po == -7.0) and np.all(fo == -7.0) and np.all(st == -7.0) and np.all(it == -7)
        ct, pt = torch.from_numpy(c).to(dev), torch.from_numpy(pos).to(dev)
        pot = torch.full((3, 48, 3), -7.0, dtype=torch.float64, device=dev)
        fot = torch.full((3, 48, 3), -7.0, dtype=torch.float64, device=dev)
        stt = torch.full((3, 6), -7.0, dtype=torch.float64, device=dev)
        itt = torch.full((3, 2), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        assert L.mw_quench_compute_device(3, 48, ct.data_ptr(), pt.data_ptr(), ftol, mi, fp, pot.data_ptr(), fot.data_ptr(), stt.data_ptr(), itt.data_ptr()) != 0
        msg = L.mw_quench_last_error().decode()
        assert "mw_quench_compute_device" in msg and re.search(pattern, msg), msg
        assert bool((pot == -7.0).all()) and bool((fot == -7.0).all()) and bool((stt == -7.0).all()) and bool((itt == -7).all())
    assert quench_last() == before                                         # nothing launched
    assert all(t >= 0.0 for t in quench_elapsed_ms()) and len(quench_elapsed_ms()) == 4
    with pytest.raises(MwError, match="expected"):
        inherent_structures(h, xyz[:, :2])
    with pytest.raises(MwError, match="unknown parameters"):
        inherent_structures(h, xyz, fire=dict(timestep=1.0))


# -- with the engine in the same process ------------------------------------------------------
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


def test_the_engine_and_the_farm_give_what_the_arrays_give():
    from mc_water_ls_mw_amd.quench import inherent_structures
    em, farm = _farm()
    try:
        farm.sweep(96, seed=41)
        nb = em.num_lattices
        e0 = em.model_energy_batch(1, nb).copy()
        pos_f, stats_f, iters_f = farm.inherent_structures(ftol=FTOL, max_iter=MAX_ITER)
        hs = farm.sync_cells()
        pos = np.array([farm.positions(b + 1) for b in range(nb)])
        want = inherent_structures(hs, pos, FTOL, MAX_ITER)
        assert pos_f.shape == (2, 2, 48, 3) and stats_f.shape == (2, 2, 6) and iters_f.shape == (2, 2, 2)
        assert _same(pos_f.reshape(nb, 48, 3), want[0]) and _same(stats_f.reshape(nb, 6), want[2]) and _same(iters_f.reshape(nb, 2), want[3])
        assert np.all(iters_f[:, :, 1] == 1) and np.all(stats_f[:, :, 1] < stats_f[:, :, 0])
        assert _all_same(em.inherent_structures(ftol=FTOL, max_iter=MAX_ITER), want)
        assert _all_same(em.inherent_structures(2, 2, ftol=1e-6, max_iter=50, fire=dict(dtmax=100.0)),
                         inherent_structures(hs[1:3], pos[1:3], 1e-6, 50, fire=dict(dtmax=100.0)))
        # the engine's own boxes are where they were
        assert np.array_equal(em.model_energy_batch(1, nb), e0) and np.array_equal(np.array([farm.positions(b + 1) for b in range(nb)]), pos)
        # the pairing of the docstring: the quenched positions go straight into another library
        from mc_water_ls_mw_amd import tetrahedral
        try:
            order, _, _, summary = tetrahedral.tetrahedral_order(hs, pos_f.reshape(nb, 48, 3))
            assert order.shape == (nb, 48, 4) and np.all(summary[:, 4] == 48) and np.all(summary[:, 0] > 0.9)      # four-coordinated minima
        finally:
            tetrahedral.tet_finalize()
    finally:
        em.energy_deinit()


if __name__ == "__main__":
    # the child of test_chunks_looks_and_slices_do_not_change_a_byte: the switches are set, mw_quench_init reads them
    from mc_water_ls_mw_amd.quench import inherent_structures, quench_finalize, quench_last
    out = {}
    for k, (hs, xs) in enumerate(_chunk_cases()):
        r = inherent_structures(hs, xs, 1e-8, MAX_ITER)
        last = quench_last()
        out.update({f"pos_out{k}": r[0], f"forces{k}": r[1], f"stats{k}": r[2], f"iters{k}": r[3], f"chunks{k}": last["chunks"],
                    f"boxes_per_chunk{k}": last["boxes_per_chunk"]})
    quench_finalize()
    np.savez(sys.argv[1], **out)
