"""GPU: the second derivatives of libmw_hess.so (phonons.hessian / hessian_matvec and their _torch forms, EnergyModule.hessian,
WalkerFarm.harmonic_free_energies) against the autograd reference of tests/hess_ref.py, and the bit rules of include/mw_hess.h:
the bytes of a box's products depend on its cell, its positions and the vector alone, those of its matrix and of its energy and
largest force on the cell and the positions alone.

Bars.  Elements of H: H_ATOL = conftest.RTOL * max |H_ref| of the case -- the project's 1e-10 relative bar for energies and
forces applied to the next derivative.  Products: RTOL * max |H_ref v| over the vectors of the case; a uniform translation: |H v|
<= RTOL * max |H_ref| (for the 1536-molecule box, which has no dense reference, max |H_ref| is replaced by the largest element of
one reference column, which is no larger).  Eigenvalues: eps = 3 N H_ATOL (Weyl: the 2-norm of the difference of two matrices is
at most 3 N times its largest element).  E against the single-point evaluation of libmw_quench.so: RTOL relative; the largest
|F| component: quench_ref.F_ATOL absolute.  The preconditions (what the reference itself is good for) are asserted in
tests/test_hess_ref.py.  Every test prints the gaps it measures.

Measured on the MI355X (profiles/hess_summary.md): the largest gap of an element is 9e-15 of max |H_ref| (ic96), of a product 3e-15 of
max |H_ref v|; a uniform translation gives exactly zero."""
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
from quench_ref import F_ATOL
import hess_ref

pytestmark = pytest.mark.gpu

KT_200K = 200.0 / 3.1577465e5                                        # Hartree


@pytest.fixture(scope="module", autouse=True)
def _library_lifetime():
    """The libraries are initialised by their first calls here and finalised when this file is done."""
    yield
    from mc_water_ls_mw_amd import phonons, quench
    phonons.hess_finalize()
    quench.quench_finalize()


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _h_atol(name):
    return RTOL * float(np.abs(hess_ref.dense_reference(name)).max())


# -- against the reference --------------------------------------------------------------------
@pytest.mark.parametrize("name", hess_ref.DENSE_CASES)
def test_the_dense_matrix_is_the_reference(name):
    from mc_water_ls_mw_amd.phonons import hessian
    from mc_water_ls_mw_amd.quench import inherent_structures
    h, xyz = hess_ref.load_case(name)
    n = len(xyz)
    H, ef = hessian(h, xyz)
    ref, bar = hess_ref.dense_reference(name), _h_atol(name)
    rows = H.reshape(3 * n, n, 3).sum(axis=1)
    _, forces, stats, _ = inherent_structures(h, xyz, 1e-10, 0)
    print(name, "max |H_ref|", bar / RTOL, "max |H - H_ref|", np.abs(H - ref).max(), "asymmetry", np.abs(H - H.T).max(), "sum rule", np.abs(rows).max(),
          "|E - E_quench|", abs(ef[0] - stats[1]), "|fmax - fmax_quench|", abs(ef[1] - stats[3]))
    assert H.shape == (3 * n, 3 * n) and ef.shape == (2,) and np.all(np.isfinite(H))
    assert np.abs(H - ref).max() <= bar
    assert np.abs(H - H.T).max() <= bar
    assert np.abs(rows).max() <= bar
    assert abs(ef[0] - stats[1]) <= RTOL * abs(stats[1]) and abs(ef[1] - stats[3]) <= F_ATOL
    assert abs(ef[1] - np.abs(forces).max()) <= F_ATOL


@pytest.mark.parametrize("name", hess_ref.MATVEC_CASES)
def test_products_are_the_reference(name):
    from mc_water_ls_mw_amd.phonons import hessian_matvec
    from mc_water_ls_mw_amd.quench import inherent_structures
    h, xyz = hess_ref.load_case(name)
    n = len(xyz)
    vecs = hess_ref.test_vectors(name)
    ref = hess_ref.matvec_reference(name)
    out, ef = hessian_matvec(h, xyz, vecs)
    bar = RTOL * float(np.abs(ref[:-1]).max())
    if name == hess_ref.LARGE_CASE:
        unit = np.zeros((1, n, 3))
        unit[0, 0, 0] = 1.0
        scale = float(np.abs(hess_ref.energy(name).matvec(unit)).max())            # one column of H_ref: no larger than max |H_ref|
    else:
        scale = float(np.abs(hess_ref.dense_reference(name)).max())
    _, _, stats, _ = inherent_structures(h, xyz, 1e-10, 0)
    print(name, "max |H_ref v|", bar / RTOL, "max |H v - H_ref v|", np.abs(out[:-1] - ref[:-1]).max(), "translation: max |H v|", np.abs(out[-1]).max(),
          "against", RTOL * scale, "|E - E_quench|", abs(ef[0] - stats[1]), "|fmax - fmax_quench|", abs(ef[1] - stats[3]))
    assert out.shape == vecs.shape and ef.shape == (2,)
    assert np.abs(out[:-1] - ref[:-1]).max() <= bar
    assert np.abs(out[-1]).max() <= RTOL * scale
    assert abs(ef[0] - stats[1]) <= RTOL * abs(stats[1]) and abs(ef[1] - stats[3]) <= F_ATOL


@pytest.mark.parametrize("name", hess_ref.DENSE_CASES)
def test_products_with_the_unit_vectors_are_the_columns_of_the_dense_matrix(name):
    from mc_water_ls_mw_amd.phonons import hess_last, hessian, hessian_matvec
    h, xyz = hess_ref.load_case(name)
    n = len(xyz)
    H, ef_d = hessian(h, xyz)
    out, ef_m = hessian_matvec(h, xyz, np.eye(3 * n).reshape(3 * n, n, 3))
    cols = out.reshape(3 * n, 3 * n).T                                 # out[c] = H e_c = column c
    print(name, "max |H e_c - H[:, c]|", np.abs(cols - H).max(), "vectors per group", hess_last()["vectors_per_group"])
    assert np.abs(cols - H).max() <= _h_atol(name)
    assert _same(ef_d, ef_m)                                           # the same passes, whatever follows them


@pytest.mark.parametrize("name", hess_ref.DENSE_CASES)
def test_spectra_lie_within_weyl_of_the_reference(name):
    from mc_water_ls_mw_amd.phonons import harmonic_free_energy, hessian, normal_modes
    h, xyz = hess_ref.load_case(name)
    n = len(xyz)
    H, _ = hessian(h, xyz)
    ref = hess_ref.dense_reference(name)
    eps = 3 * n * _h_atol(name)
    lam, lam_ref = np.linalg.eigvalsh(0.5 * (H + H.T)), np.linalg.eigvalsh(ref)
    print(name, "eps", eps, "max |lambda - lambda_ref|", np.abs(lam - lam_ref).max())
    assert np.abs(lam - lam_ref).max() <= eps
    if name == "ic96":
        assert int((np.abs(lam) <= eps).sum()) == 3 and lam.min() >= -eps
        f_dev, f_ref = harmonic_free_energy(normal_modes(H), KT_200K), harmonic_free_energy(normal_modes(ref), KT_200K)
        kept = np.sort(np.abs(lam_ref))[3:]
        bound = KT_200K * float(np.sum(eps / (2.0 * kept)))
        print("ic96: F_vib(200 K)", f_dev, "reference", f_ref, "gap", abs(f_dev - f_ref), "bound", bound)
        assert np.isfinite(f_dev) and abs(f_dev - f_ref) <= bound


def test_a_quenched_box_is_a_minimum_with_three_zero_modes():
    from mc_water_ls_mw_amd.phonons import harmonic_free_energy, hessian, mode_dos, normal_modes, participation_ratio
    from mc_water_ls_mw_amd.quench import inherent_structures
    h, xyz = hess_ref.load_case("ih48_t020")
    pos, _, stats, iters = inherent_structures(h, xyz, 1e-10, 10000)
    assert iters[1] == 1
    H, ef = hessian(h, pos)
    omega, vec = normal_modes(H, vectors=True)
    keep = omega[np.argsort(np.abs(omega))[3:]]
    f_cl, f_q = harmonic_free_energy(omega, KT_200K), harmonic_free_energy(omega, KT_200K, quantum=True)
    print("ih48_t020 quenched: fmax", ef[1], "three smallest |omega|", np.sort(np.abs(omega))[:3], "lowest kept", keep.min(), "highest", keep.max(),
          "F_vib classical", f_cl, "quantum", f_q)
    assert ef[1] <= 1e-10 and abs(ef[0] - stats[1]) <= RTOL * abs(stats[1])
    assert len(keep) == 3 * 48 - 3 and keep.min() > 0.0
    assert np.isfinite(f_cl) and np.isfinite(f_q)
    assert mode_dos(omega, np.linspace(omega.min(), omega.max(), 11)).sum() == 3 * 48
    p = participation_ratio(vec)
    assert p.shape == (3 * 48,) and np.all(p > 0.0) and np.all(p <= 1.0 + 1e-12)


# -- the bit rules ----------------------------------------------------------------------------
def _mixed_boxes():
    """Seven boxes of 96 molecules: thermal Ic boxes of five sizes, the disordered Ih box and the perfect lattice."""
    hs, xs = scaled_set("ic96", 5, 0.05, 300)
    h1, x1 = hess_ref.load_case("ih96_disordered")
    h2, x2 = hess_ref.load_case("ic96")
    return np.concatenate([hs, [h1, h2]]), np.concatenate([xs, [x1, x2]])


def _vectors(nb, nvec, n, seed=9):
    return np.random.default_rng(seed).standard_normal((nb, nvec, n, 3))


def test_a_batch_equals_the_single_calls_bit_for_bit():
    from mc_water_ls_mw_amd.phonons import hessian, hessian_matvec
    hs, xs = _mixed_boxes()
    vecs = _vectors(len(xs), 5, 96)
    H, ef = hessian(hs, xs)
    out, ef_m = hessian_matvec(hs, xs, vecs)
    assert _same(ef, ef_m)
    for b in range(len(xs)):
        H1, ef1 = hessian(hs[b], xs[b])
        out1, ef2 = hessian_matvec(hs[b], xs[b], vecs[b])
        assert _same(H1, H[b]) and _same(ef1, ef[b]) and _same(out1, out[b]) and _same(ef2, ef[b]), b
    # every vector on its own, and the vectors in another order
    for v in (0, 3):
        alone, _ = hessian_matvec(hs, xs, vecs[:, v:v + 1])
        assert _same(alone[:, 0], out[:, v]), v
    back, _ = hessian_matvec(hs, xs, vecs[:, ::-1])
    assert _same(np.ascontiguousarray(back[:, ::-1]), out)
    # the boxes in another order, and the same call again
    perm = np.array([4, 0, 6, 2, 5, 1, 3])
    Hp, efp = hessian(hs[perm], xs[perm])
    outp, _ = hessian_matvec(hs[perm], xs[perm], vecs[perm])
    assert _same(Hp, H[perm]) and _same(efp, ef[perm]) and _same(outp, out[perm])
    H2, ef2 = hessian(hs, xs)
    out2, _ = hessian_matvec(hs, xs, vecs)
    assert _same(H2, H) and _same(ef2, ef) and _same(out2, out)


def test_device_tensors_give_the_bits_of_the_host_entries():
    import torch
    from mc_water_ls_mw_amd.phonons import hessian, hessian_matvec, hessian_matvec_torch, hessian_torch, load_hess_library
    hs, xs = _mixed_boxes()
    vecs = _vectors(len(xs), 35, 96)                                   # more than one group of vectors
    H, ef = hessian(hs, xs)
    out, _ = hessian_matvec(hs, xs, vecs)
    dev = torch.device("cuda:0")
    ct, pt, vt = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (hs, xs, vecs))
    Ht, eft = hessian_torch(ct, pt)
    outt, eft2 = hessian_matvec_torch(ct, pt, vt)
    assert _same(Ht.cpu().numpy(), H) and _same(eft.cpu().numpy(), ef) and _same(outt.cpu().numpy(), out) and _same(eft2.cpu().numpy(), ef)
    # ef is optional
    L = load_hess_library()
    H0 = np.full_like(H, -7.0)
    assert L.mw_hess_dense(len(xs), 96, hs.ctypes.data, xs.ctypes.data, H0.ctypes.data, None) == 0 and _same(H0, H)
    out0 = torch.full_like(vt, -7.0)
    torch.cuda.synchronize()
    assert L.mw_hess_matvec_device(len(xs), 96, ct.data_ptr(), pt.data_ptr(), 35, vt.data_ptr(), out0.data_ptr(), None) == 0
    assert _same(out0.cpu().numpy(), out)
    # the large box through both entries, several workgroups per box
    h, xyz = hess_ref.load_case(hess_ref.LARGE_CASE)
    big = hess_ref.test_vectors(hess_ref.LARGE_CASE)
    o1, e1 = hessian_matvec(h, xyz, big)
    o2, e2 = hessian_matvec_torch(*(torch.from_numpy(np.array(a)).to(dev) for a in (h[None], xyz[None], big[None])))
    assert _same(o2.cpu().numpy()[0], o1) and _same(e2.cpu().numpy()[0], e1)


def _chunk_cases():
    hs, xs = _mixed_boxes()
    h, xyz = hess_ref.load_case(hess_ref.LARGE_CASE)
    return (hs, xs, _vectors(len(xs), 40, 96, 21)), (np.array([h, h * 1.01]), np.array([xyz, xyz * 1.01]), _vectors(2, 6, len(xyz), 22))


def test_chunks_and_vector_groups_do_not_change_a_byte(tmp_path):
    """A fresh process with 1 MiB of scratch -- three boxes of 96 molecules per chunk with 32 vectors in a group and one box per
    chunk of the dense matrix; one box of 1536 molecules per chunk with four vectors in a group -- returns the bytes of this
    process, where every call is one chunk."""
    from mc_water_ls_mw_amd.phonons import hess_last, hess_plan, hessian, hessian_matvec
    (hs, xs, vs), (hb, xb, vb) = _chunk_cases()
    H, ef = hessian(hs, xs)
    assert hess_last()["chunks"] == 1
    out, _ = hessian_matvec(hs, xs, vs)
    last = hess_last()
    assert last["chunks"] == 1 and last["vectors_per_group"] == 32
    outb, efb = hessian_matvec(hb, xb, vb)
    last = hess_last()
    assert last["chunks"] == 1 and last["vectors_per_group"] == 6
    path = tmp_path / "chunks.npz"
    env = dict(os.environ, MW_HESS_SCRATCH_MB="1")
    res = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), str(path)], capture_output=True, text=True, env=env)
    assert res.returncode == 0, (res.returncode, res.stdout[-1000:], res.stderr[-3000:])
    z = np.load(path)
    assert (int(z["dense_chunks"]), int(z["dense_bpc"])) == (7, 1)
    assert (int(z["mv_chunks"]), int(z["mv_bpc"]), int(z["mv_group"])) == (3, 3, 32)
    assert (int(z["big_chunks"]), int(z["big_bpc"]), int(z["big_group"])) == (2, 1, 4)
    assert _same(z["H"], H) and _same(z["ef"], ef) and _same(z["out"], out) and _same(z["outb"], outb) and _same(z["efb"], efb)
    assert hess_plan(96, hs[0], 7, 40)["chunks"] == 1                  # this process kept its own budget


# -- rejected calls ---------------------------------------------------------------------------
def test_rejected_calls_name_the_argument_and_write_nothing():
    import torch
    from mc_water_ls_mw_amd.phonons import MwError, hess_elapsed_ms, hess_last, hessian, hessian_matvec, load_hess_library
    z = load_golden("ic48")
    h, xyz = z["h"], z["xyz"]
    hessian(h, xyz)                                                    # the library is live and has launched
    L = load_hess_library()
    before = hess_last()
    cells = np.ascontiguousarray(np.array([h, h, h]).reshape(3, 9))
    pos = np.ascontiguousarray(np.array([xyz, xyz, xyz]))
    vecs = np.ones((3, 2, 48, 3))
    flat = cells.copy()
    flat[2, 6:9] = 0.0
    narrow = cells.copy()
    narrow[1] *= 0.3                                                   # box 1 is narrower than a sigma
    nan = cells.copy()
    nan[0, 4] = float("nan")
    dev = torch.device("cuda:0")
    pt, vt = torch.from_numpy(pos).to(dev), torch.from_numpy(vecs).to(dev)
    for c, nvec, pattern in ((flat, 2, r"cells.*box 2\b"), (narrow, 2, r"a_sigma.*box 1\b"), (nan, 2, r"cells.*box 0\b"), (cells, 0, "nvec"), (cells, 1025, "nvec")):
        Hb, ob, eb = np.full((3, 144, 144), -7.0), np.full((3, 2, 48, 3), -7.0), np.full((3, 2), -7.0)
        ct = torch.from_numpy(c).to(dev)
        Ht, ot, et = (torch.full(a.shape, -7.0, dtype=torch.float64, device=dev) for a in (Hb, ob, eb))
        torch.cuda.synchronize()
        calls = [("mw_hess_matvec", lambda: L.mw_hess_matvec(3, 48, c.ctypes.data, pos.ctypes.data, nvec, vecs.ctypes.data, ob.ctypes.data, eb.ctypes.data)),
                 ("mw_hess_matvec_device", lambda: L.mw_hess_matvec_device(3, 48, ct.data_ptr(), pt.data_ptr(), nvec, vt.data_ptr(), ot.data_ptr(), et.data_ptr()))]
        if pattern != "nvec":
            calls += [("mw_hess_dense", lambda: L.mw_hess_dense(3, 48, c.ctypes.data, pos.ctypes.data, Hb.ctypes.data, eb.ctypes.data)),
                      ("mw_hess_dense_device", lambda: L.mw_hess_dense_device(3, 48, ct.data_ptr(), pt.data_ptr(), Ht.data_ptr(), et.data_ptr()))]
        for entry, call in calls:
            assert call() != 0, (entry, pattern)
            msg = L.mw_hess_last_error().decode()
            assert msg.startswith(entry + ":") and re.search(pattern, msg), msg
        torch.cuda.synchronize()
        assert np.all(Hb == -7.0) and np.all(ob == -7.0) and np.all(eb == -7.0)
        assert bool((Ht == -7.0).all()) and bool((ot == -7.0).all()) and bool((et == -7.0).all())
    assert hess_last() == before                                       # nothing launched
    t = hess_elapsed_ms()
    assert len(t) == 4 and all(v >= 0.0 for v in t) and t[3] > 0.0 and t[2] == 0.0      # the last call that launched was a dense one
    hessian_matvec(h, xyz, vecs[0])
    t = hess_elapsed_ms()
    assert t[2] > 0.0 and t[3] == 0.0
    with pytest.raises(MwError, match="expected"):
        hessian(h, xyz[:, :2])
    with pytest.raises(MwError, match="vecs"):
        hessian_matvec(h, xyz, np.ones((2, 47, 3)))


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


def test_the_farm_gives_the_harmonic_free_energies_of_its_minima():
    from mc_water_ls_mw_amd.phonons import harmonic_free_energy, hessian, normal_modes
    em, farm = _farm()
    try:
        farm.sweep(96, seed=41)
        nb = em.num_lattices
        e0 = em.model_energy_batch(1, nb).copy()
        e_min, f_vib, negative, converged, f_harm = farm.harmonic_free_energies(KT_200K)
        assert e_min.shape == f_vib.shape == negative.shape == converged.shape == (2, 2) and f_harm.shape == (2,)
        assert converged.dtype == bool and np.all(converged) and np.all(negative == 0) and np.all(np.isfinite(f_vib))
        pos_f, stats_f, _ = farm.inherent_structures(ftol=1e-10, max_iter=10000)
        hs = farm.sync_cells()
        H, ef = hessian(hs, pos_f.reshape(nb, 48, 3))
        want = np.array([harmonic_free_energy(normal_modes(H[b]), KT_200K) for b in range(nb)]).reshape(2, 2)
        print("farm: e_min", e_min.ravel(), "f_vib", f_vib.ravel(), "f_harm", f_harm, "fmax at the minima", ef[:, 1])
        assert _same(f_vib, want) and _same(e_min, np.ascontiguousarray(stats_f[:, :, 1])) and _same(f_harm, (stats_f[:, :, 1] + want).mean(axis=0))
        assert np.all(np.abs(ef[:, 0] - e_min.ravel()) <= RTOL * np.abs(e_min.ravel())) and np.all(ef[:, 1] <= 1e-10 + F_ATOL)
        # the engine's view of one box: the Hessian where the walker is, not at its minimum
        pos = np.array([farm.positions(b + 1) for b in range(nb)])
        H2, ef2 = em.hessian(2)
        Hw, efw = hessian(hs[1], pos[1])
        assert _same(H2, Hw) and _same(ef2, efw) and abs(ef2[0] - e0[1]) <= RTOL * abs(e0[1])
        omega = em.normal_modes(2)
        assert omega.shape == (144,) and _same(omega, normal_modes(Hw))
        assert np.array_equal(em.model_energy_batch(1, nb), e0)            # the engine's own boxes are where they were
    finally:
        em.energy_deinit()


if __name__ == "__main__":
    # the child of test_chunks_and_vector_groups_do_not_change_a_byte: MW_HESS_SCRATCH_MB is set, mw_hess_init reads it
    from mc_water_ls_mw_amd.phonons import hess_finalize, hess_last, hessian, hessian_matvec
    (hs, xs, vs), (hb, xb, vb) = _chunk_cases()
    res = {}
    res["H"], res["ef"] = hessian(hs, xs)
    last = hess_last()
    res.update(dense_chunks=last["chunks"], dense_bpc=last["boxes_per_chunk"])
    res["out"], _ = hessian_matvec(hs, xs, vs)
    last = hess_last()
    res.update(mv_chunks=last["chunks"], mv_bpc=last["boxes_per_chunk"], mv_group=last["vectors_per_group"])
    res["outb"], res["efb"] = hessian_matvec(hb, xb, vb)
    last = hess_last()
    res.update(big_chunks=last["chunks"], big_bpc=last["boxes_per_chunk"], big_group=last["vectors_per_group"])
    hess_finalize()
    np.savez(sys.argv[1], **res)
