"""GPU: the structure factor of libmw_sk.so (structure.structure_factor / _mean / _torch, EnergyModule.structure_factor,
WalkerFarm.structure_factor) against the long-double reference of tests/sk_ref.py within its derived bound delta(n), at the
sizes where the kernels change path, and the bit rules of include/mw_sk.h: rho(-n) = conj rho(n), and the bits of rho_b(n)
depend on the box and n alone."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from conftest import golden_names, load_golden
from sk_ref import assert_within, s_max, sk_exact, vectors_for

pytestmark = pytest.mark.gpu

SMALL = [n for n in golden_names() if not any(t in n for t in ("4096", "32768"))]
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)


@pytest.fixture(scope="module", autouse=True)
def _library_lifetime():
    """The library is initialised by its first call here and finalised when this file is done."""
    yield
    from mc_water_ls_mw_amd import structure
    structure.sk_finalize()


def _sf(h, xyz, nvec):
    """(rho complex [M], S [M]) of one box."""
    from mc_water_ls_mw_amd.structure import structure_factor
    S, rho = structure_factor(h, xyz, nvec, want_rho=True)
    return rho[0], S[0]


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _check(h, xyz, nvec, what):
    rho, S = _sf(h, xyz, nvec)
    assert_within(rho, S, sk_exact(h, xyz, nvec), nvec, len(xyz), s_max(h, xyz), what)
    return rho, S


def _nmax(nvec):
    return tuple(int(v) for v in np.abs(nvec).max(axis=0))


# -- against sk_exact within delta -------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_every_small_golden_box_matches_the_reference(name):
    from mc_water_ls_mw_amd.structure import sk_last, sk_plan
    z = load_golden(name)
    h, xyz = z["h"], z["xyz"]
    nvec = vectors_for(h)
    assert 1 <= len(nvec) <= 4096
    _check(h, xyz, nvec, name)
    last = sk_last()
    assert last == sk_plan(len(xyz), _nmax(nvec), len(nvec), 1) and last["small"] == (len(xyz) <= 64) and last["chunks"] == 1, last


def _drawn_vectors(h, reps, bragg, count, seed):
    """``count`` triples drawn from the half space up to 3 / Angstrom, among them the one of largest |n|_1, a Bragg vector of
    the ideal lattice and n = 0."""
    from mc_water_ls_mw_amd.structure import kvectors
    full = kvectors(h, 3.0, half=True)
    rng = np.random.default_rng(seed)
    pick = full[rng.choice(len(full), count - 3, replace=False)]
    l1 = np.abs(full).sum(axis=1)
    fixed = np.array([full[int(np.argmax(l1))], np.array(bragg) * np.array(reps), [0, 0, 0]], dtype=np.int32)
    nvec = np.ascontiguousarray(np.concatenate([pick, fixed]), dtype=np.int32)
    assert np.abs(nvec).sum(axis=1).max() == l1.max()
    return nvec


@pytest.mark.parametrize("name,reps,count", [("ih4096_t015", (8, 8, 8), 512), ("ih32768_t015", (16, 16, 16), 256)])
def test_large_boxes_match_the_reference(name, reps, count):
    from mc_water_ls_mw_amd.structure import sk_last
    z = load_golden(name)
    h, xyz = z["h"], z["xyz"]
    nvec = _drawn_vectors(h, reps, (0, 0, 2), count, 77)
    assert len(nvec) == count and len(xyz) * count <= 10 ** 7
    rho, S = _check(h, xyz, nvec, name)
    assert rho[-1] == len(xyz) and S[-1] == len(xyz)                     # n = 0: rho = N exactly
    assert S[-2] > 0.05 * len(xyz)                                       # the (002) reflection of the thermal crystal
    last = sk_last()
    assert last["segments"] == -(-len(xyz) // last["segment_length"]) > 1 and not last["small"]


@pytest.mark.parametrize("name", ["ic64_sheared", "ih8_small"])
def test_positions_beyond_one_cell(name):
    z = load_golden(name)
    h, xyz = z["h"], z["xyz"]
    rng = np.random.default_rng(3)
    moved = xyz + rng.integers(-3, 4, xyz.shape).astype(np.float64) @ h
    assert s_max(h, moved) > 2.0
    nvec = vectors_for(h, m_target=600)
    rho, S = _check(h, moved, nvec, name + " displaced")
    assert_within(rho, S, sk_exact(h, xyz, nvec), nvec, len(xyz), s_max(h, moved), name + " against the cell's own images")


# -- boundaries -------------------------------------------------------------------------------
def _random_box(n, seed):
    rng = np.random.default_rng(seed)
    h = np.array([[31.0, 0.0, 0.0], [4.5, 28.0, 0.0], [-3.0, 5.0, 35.0]])
    return h, np.ascontiguousarray((rng.random((n, 3)) * 1.6 - 0.3) @ h)


ODD_VECTORS = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 2, -3], [5, -4, 3], [7, 7, 7], [-7, -7, -7], [12, 0, -9],
                        [0, -11, 2], [3, 3, -13], [13, 12, 11], [-13, 12, -11], [2, -1, 0], [9, 9, 0], [0, 6, 6], [4, 0, 4],
                        [1, 1, 1], [-1, -1, -1], [10, -10, 10], [6, 5, -4], [-2, 13, 1], [8, -3, 12], [0, 0, -12],
                        [0, 13, 0], [-12, 0, 0], [11, 1, -1], [3, -8, 5], [-5, 8, -3], [1, 12, 13], [13, 1, 12], [12, 13, 1],
                        [-6, 0, 7], [2, 2, -2], [4, -9, 9], [9, 4, -9], [-9, 9, 4]], dtype=np.int32)


def test_molecule_counts_around_every_threshold():
    """One molecule below, at and above the small-box limit, the LDS tile and the segment length that mw_sk_plan reports, and
    a box of more than two segments with a ragged tail."""
    from mc_water_ls_mw_amd.structure import sk_last, sk_plan
    plan = sk_plan(5000, _nmax(ODD_VECTORS), len(ODD_VECTORS), 1)
    tile, seg = plan["tile"], plan["segment_length"]
    assert (tile, seg) == (32, 1024)
    sizes = sorted({tile - 1, tile, tile + 1, 63, 64, 65, 2 * tile + 1, seg - 1, seg, seg + 1, 2 * seg + tile + 1})
    for n in sizes:
        h, xyz = _random_box(n, 100 + n)
        _check(h, xyz, ODD_VECTORS, f"N = {n}")
        last = sk_last()
        assert last["small"] == (n <= 64) and last["segments"] == (1 if n <= 64 else -(-n // seg)), (n, last)


def test_vector_counts_around_one_workgroup():
    """M = 1 and one vector below, at and above what one workgroup takes: each call must give the bits of the longest one."""
    from mc_water_ls_mw_amd.structure import sk_plan
    for name in ("ic48_t015", "ic96"):
        z = load_golden(name)
        h, xyz = z["h"], z["xyz"]
        nvec = vectors_for(h, m_target=1300)
        vpw = sk_plan(len(xyz), _nmax(nvec), len(nvec), 1)["kvec_per_workgroup"]
        assert vpw == 512 and len(nvec) > 2 * vpw + 1
        rho, S = _check(h, xyz, nvec[:2 * vpw + 1], name)
        for m in (1, vpw - 1, vpw, vpw + 1, 2 * vpw):
            r, s = _sf(h, xyz, nvec[:m])
            assert _same(r, rho[:m]) and _same(s, S[:m]), (name, m)


def test_components_of_255_next_to_empty_axes():
    for h, xyz, what in [(load_golden("ic48_t015")["h"], load_golden("ic48_t015")["xyz"], "ic48_t015"), _random_box(65, 9) + ("N = 65",)]:
        for nvec in ([[255, 0, 0]], [[0, -255, 0]], [[0, 0, 255], [0, 0, -255]], [[255, -255, 255], [-255, 255, -255], [0, 0, 0]]):
            nvec = np.array(nvec, dtype=np.int32)
            rho, S = _check(h, xyz, nvec, f"{what} {nvec[0].tolist()}")
            if len(nvec) > 1:
                assert rho[1] == np.conj(rho[0]) and S[1] == S[0]


def test_duplicates_get_the_same_bits():
    z = load_golden("ih48_t020")
    base = vectors_for(z["h"], m_target=200)
    nvec = np.ascontiguousarray(np.concatenate([base, base[::3], base[:5], base[:5]]), dtype=np.int32)
    rho, S = _check(z["h"], z["xyz"], nvec, "duplicates")
    m = len(base)
    assert _same(rho[m:m + len(base[::3])], rho[:m:3]) and _same(S[-5:], S[:5]) and _same(S[-10:-5], S[:5])


# -- bit rules --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ic48_t015", "ic96", "ih1536_t012"])
def test_minus_n_is_the_conjugate_bit_for_bit(name):
    z = load_golden(name)
    half = vectors_for(z["h"], m_target=700)
    rho, S = _sf(z["h"], z["xyz"], np.ascontiguousarray(np.concatenate([half, -half]), dtype=np.int32))
    m = len(half)
    assert np.array_equal(rho[m:].real, rho[:m].real) and np.array_equal(rho[m:].imag, -rho[:m].imag)
    assert _same(S[m:], S[:m])
    assert np.count_nonzero(rho[:m].imag) > m // 2


@pytest.mark.parametrize("name", ["ic48_t015", "ih1536_t012"])
def test_the_list_decides_nothing(name):
    """A permuted list gives the same bits, permuted; and a list that drives the small boxes out of the small-box geometry
    (a component of 255 makes the tables too tall for LDS) leaves the bits of the other vectors alone."""
    from mc_water_ls_mw_amd.structure import sk_last
    z = load_golden(name)
    nvec = vectors_for(z["h"], m_target=900)
    rho, S = _sf(z["h"], z["xyz"], nvec)
    small = sk_last()["small"]
    perm = np.random.default_rng(8).permutation(len(nvec))
    r, s = _sf(z["h"], z["xyz"], np.ascontiguousarray(nvec[perm]))
    assert _same(r, rho[perm]) and _same(s, S[perm])
    tall = np.ascontiguousarray(np.concatenate([[[0, 255, -1]], nvec]), dtype=np.int32)
    r, s = _sf(z["h"], z["xyz"], tall)
    assert not sk_last()["small"] and small == (len(z["xyz"]) <= 64)
    assert _same(r[1:], rho) and _same(s[1:], S)


def _scaled_set(name, n, sigma, seed):
    from mc_water_ls_mw_amd import lattice as lat
    z = load_golden(name)
    hs, xs = [], []
    for k in range(n):
        f = 1.0 + 0.013 * (k % 5 - 2)
        hs.append(z["h"] * f)
        xs.append(lat.thermalise(z["xyz"], sigma, seed + k) * f)
    return np.array(hs), np.array(xs)


@pytest.mark.parametrize("name,n", [("ih48_t020", 5), ("ic96", 4), ("ih1536_t012", 3)])
def test_a_batch_equals_the_single_calls_bit_for_bit(name, n):
    from mc_water_ls_mw_amd.structure import structure_factor
    hs, xs = _scaled_set(name, n, 0.1, 40)
    nvec = vectors_for(hs[0], m_target=700)
    S, rho = structure_factor(hs, xs, nvec, want_rho=True)
    assert S.shape == (n, len(nvec)) and rho.shape == (n, len(nvec))
    for b in range(n):
        r1, s1 = _sf(hs[b], xs[b], nvec)
        assert _same(r1, rho[b]) and _same(s1, S[b]), b
    assert len({S[b].tobytes() for b in range(n)}) == n
    only_s = structure_factor(hs[1:], xs[1:], nvec)
    assert _same(only_s, S[1:])
    assert_within(rho[n - 1], S[n - 1], sk_exact(hs[n - 1], xs[n - 1], nvec), nvec, xs.shape[1], s_max(hs[n - 1], xs[n - 1]),
                  f"{name} box {n}")


def _chunk_case():
    hs, xs = _scaled_set("ic96", 80, 0.12, 300)
    return hs, xs, vectors_for(hs[0], m_target=500)


def test_chunks_give_the_bits_of_one_chunk(tmp_path):
    """A fresh process whose scratch budget is 1 MiB takes the 80 boxes in several chunks, the last one ragged; here they fit one."""
    from mc_water_ls_mw_amd.structure import sk_last, sk_plan, structure_factor
    hs, xs, nvec = _chunk_case()
    S, rho = structure_factor(hs, xs, nvec, want_rho=True)
    last = sk_last()
    assert last["chunks"] == 1 and last["boxes_per_chunk"] == 80
    out = tmp_path / "chunks.npz"
    env = dict(os.environ, MW_SK_SCRATCH_MB="1")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-3000:])
    z = np.load(out)
    per_box = 96 * (sum(_nmax(nvec)) + 3) * 16 + len(nvec) * 16
    fit = (1 << 20) // per_box
    assert 1 < fit < 40 and 80 % fit != 0
    assert int(z["boxes_per_chunk"]) == fit and int(z["chunks"]) == -(-80 // fit) >= 3
    assert _same(z["S"], S) and _same(z["rho_re"], rho.real) and _same(z["rho_im"], rho.imag)
    want = np.zeros((2, len(nvec)))
    for w in range(40):
        want = want + S[2 * w:2 * w + 2]
    assert _same(z["mean"], want / 40.0)
    assert sk_plan(96, _nmax(nvec), len(nvec), 80)["chunks"] == 1            # this process kept its own budget


def test_device_tensors_give_the_bits_of_the_host_entry():
    import torch
    from mc_water_ls_mw_amd.structure import structure_factor, structure_factor_torch
    hs, xs = _scaled_set("ic96", 3, 0.1, 70)
    nvec = vectors_for(hs[0], m_target=600)
    S, rho = structure_factor(hs, xs, nvec, want_rho=True)
    dev = torch.device("cuda:0")
    St, rt = structure_factor_torch(torch.from_numpy(hs).to(dev), torch.from_numpy(xs).to(dev), torch.from_numpy(nvec).to(dev))
    assert St.is_cuda and rt.is_cuda and St.dtype == rt.dtype == torch.float64
    St, rt = St.cpu().numpy(), rt.cpu().numpy()
    assert _same(St, S) and _same(rt[..., 0], rho.real) and _same(rt[..., 1], rho.imag)


@pytest.mark.parametrize("name,walkers,groups", [("ih48_t020", 7, 2), ("ic96", 3, 1), ("ih1536_t012", 2, 2)])
def test_the_mean_is_the_sequential_mean_in_walker_order(name, walkers, groups):
    from mc_water_ls_mw_amd.structure import structure_factor, structure_factor_mean
    hs, xs = _scaled_set(name, walkers * groups, 0.1, 500)
    nvec = vectors_for(hs[0], m_target=400)
    S = structure_factor(hs, xs, nvec)
    mean = structure_factor_mean(hs, xs, nvec, groups)
    want = np.zeros((groups, len(nvec)))
    for w in range(walkers):
        want = want + S[w * groups:(w + 1) * groups]
    want = want / float(walkers)
    assert _same(mean, want)


# -- rejected calls ---------------------------------------------------------------------------
def test_rejected_calls_name_the_argument_and_write_nothing():
    import torch
    from mc_water_ls_mw_amd.structure import load_sk_library, sk_elapsed_ms, sk_last
    z = load_golden("ic48")
    h, xyz = z["h"], z["xyz"]
    nvec = vectors_for(h, m_target=50)
    _sf(h, xyz, nvec)                                                      # the library is live and has launched
    L = load_sk_library()
    before = sk_last()
    cells = np.ascontiguousarray(np.array([h, h, h]).reshape(3, 9))
    pos = np.ascontiguousarray(np.array([xyz, xyz, xyz]))
    big = nvec.copy()
    big[3, 2] = 256
    flat = cells.copy()
    flat[2, 6:9] = 0.0                                                     # a cell vector of length 0: the determinant is exactly 0
    inf = cells.copy()
    inf[1, 0] = np.inf
    M = len(nvec)
    dev = torch.device("cuda:0")
    for kw, pattern in ((dict(nvec=big), r"nvec.*vector 3\b"), (dict(cells=flat), r"cells.*box 2\b"), (dict(cells=inf), r"cells.*box 1\b"),
                        (dict(ngroups=2), "ngroups")):
        c, v, g = kw.get("cells", cells), kw.get("nvec", nvec), kw.get("ngroups", 1)
        rho, S, mean = np.full((3, M, 2), -7.0), np.full((3, M), -7.0), np.full((3, M), -7.0)
        args = (3, 48, c.ctypes.data_as(_dp), pos.ctypes.data_as(_dp), M, v.ctypes.data_as(_ip))
        if "ngroups" not in kw:
            assert L.mw_sk_compute(*args, rho.ctypes.data_as(_dp), S.ctypes.data_as(_dp)) != 0
            msg = L.mw_sk_last_error().decode()
            assert "mw_sk_compute" in msg and re.search(pattern, msg), msg
            ct, pt, vt = torch.from_numpy(c).to(dev), torch.from_numpy(pos).to(dev), torch.from_numpy(v).to(dev)
            rt, st = torch.full((3, M, 2), -7.0, dtype=torch.float64, device=dev), torch.full((3, M), -7.0, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            assert L.mw_sk_compute_device(3, 48, ctypes.c_void_p(ct.data_ptr()), ctypes.c_void_p(pt.data_ptr()), M,
                                          ctypes.c_void_p(vt.data_ptr()), ctypes.c_void_p(rt.data_ptr()), ctypes.c_void_p(st.data_ptr())) != 0
            msg = L.mw_sk_last_error().decode()
            assert "mw_sk_compute_device" in msg and re.search(pattern, msg), msg
            assert bool((rt == -7.0).all()) and bool((st == -7.0).all())
        assert L.mw_sk_mean(*args, g, mean.ctypes.data_as(_dp)) != 0
        msg = L.mw_sk_last_error().decode()
        assert "mw_sk_mean" in msg and re.search(pattern, msg), msg
        assert np.all(rho == -7.0) and np.all(S == -7.0) and np.all(mean == -7.0)
    assert sk_last() == before                                             # nothing launched
    assert all(t >= 0.0 for t in sk_elapsed_ms())


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


def test_npt_farm_structure_factor_after_device_sweeps():
    from mc_water_ls_mw_amd.structure import k_lengths, structure_factor
    em, farm = _npt_farm()
    try:
        h0 = np.array(em.hmatrix)
        farm.sweep(288, seed=51)
        nvec, smean, klen = farm.structure_factor(k_max_ang=4.0)
        hs = farm.sync_cells()
        assert not np.array_equal(hs, h0)                                  # some volume move was accepted (and synced)
        m = len(nvec)
        assert nvec.dtype == np.int32 and smean.shape == klen.shape == (2, m) and m > 300
        pos = np.array([farm.positions(b + 1) for b in range(em.num_lattices)])
        hmean = hs.reshape(4, 2, 3, 3).mean(axis=0)
        for g in range(2):
            assert np.array_equal(klen[g], k_lengths(hmean[g], nvec))
        assert np.all(klen[0] <= 4.0) and np.all(np.diff(klen[0]) >= 0)
        # the reference: sk_exact of every box as read back, averaged over the walkers; the bound is the boxes' mean bound
        ex = [sk_exact(hs[b], pos[b], nvec) for b in range(em.num_lattices)]
        from sk_ref import delta
        for g in range(2):
            want = sum(ex[w * 2 + g][2] for w in range(4)) / np.longdouble(4)
            bound = np.zeros(m)
            for w in range(4):
                re, im, _ = ex[w * 2 + g]
                d = delta(nvec, 48, s_max(hs[w * 2 + g], pos[w * 2 + g]))
                bound += (2.0 * np.sqrt((re * re + im * im).astype(np.float64)) * d + d * d) / 48.0
            err = np.abs((smean[g].astype(np.longdouble) - want).astype(np.float64))
            print("lattice", g + 1, "max |dS_mean| / bound %.4f" % float((err / (bound / 4.0)).max()))
            assert np.all(err <= bound / 4.0 + 2.0 ** -52 * np.abs(smean[g]))       # (+ the rounding of the mean itself)
        # EnergyModule.structure_factor is structure_factor on the downloaded arrays, bit for bit
        S, rho = em.structure_factor(1, em.num_lattices, nvec, want_rho=True)
        S2, rho2 = structure_factor(hs, pos, nvec, want_rho=True)
        assert _same(S, S2) and _same(rho, rho2)
        assert _same(em.structure_factor(3, 2, nvec), S[2:4])
        # Ic and Ih differ where it matters
        assert np.abs(smean[0] - smean[1]).max() > 5.0
    finally:
        em.energy_deinit()


def test_engine_state_is_untouched_by_a_structure_factor_call():
    from mc_water_ls_mw_amd.structure import kvectors

    def run(with_sk):
        em, farm = _npt_farm()
        try:
            farm.sweep(96, seed=41)
            nb = em.num_lattices
            if with_sk:
                e0 = em.model_energy_batch(1, nb).copy()
                z = load_golden("ic48")
                eo0, en0 = em.delta_energy_batch(1, z["trial_imol"][:64], z["trial_xyz"][:64])
                nvec, smean, klen = farm.structure_factor(k_max_ang=3.0)
                em.structure_factor(1, nb, kvectors(em.hmatrix[1], 2.0))
                assert np.array_equal(em.model_energy_batch(1, nb), e0)
                eo, en = em.delta_energy_batch(1, z["trial_imol"][:64], z["trial_xyz"][:64])
                assert np.array_equal(eo, eo0) and np.array_equal(en, en0)
            else:
                em.model_energy_batch(1, nb)
                z = load_golden("ic48")
                em.delta_energy_batch(1, z["trial_imol"][:64], z["trial_xyz"][:64])
                em.delta_energy_batch(1, z["trial_imol"][:64], z["trial_xyz"][:64])
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
    # the child of test_chunks_give_the_bits_of_one_chunk: MW_SK_SCRATCH_MB is set, so mw_sk_init takes the small budget
    from mc_water_ls_mw_amd.structure import sk_finalize, sk_last, structure_factor, structure_factor_mean
    hs, xs, nvec = _chunk_case()
    S, rho = structure_factor(hs, xs, nvec, want_rho=True)
    last = sk_last()
    mean = structure_factor_mean(hs, xs, nvec, 2)
    assert sk_last() == last
    sk_finalize()
    np.savez(sys.argv[1], S=S, rho_re=rho.real, rho_im=rho.imag, mean=mean, chunks=last["chunks"], boxes_per_chunk=last["boxes_per_chunk"])
