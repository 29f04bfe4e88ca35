"""GPU: forces and virial of the full-box energy (mw_model_forces*, EnergyModule.compute_forces / forces_batch,
WalkerFarm.virial_pressures) against the numpy reference of tests/forces_ref.py, which tests/test_forces_ref.py pins to
central differences of the C oracle's energy."""
import numpy as np
import pytest

from conftest import DE_ATOL, RTOL, golden_names, load_golden
from forces_ref import model_forces

pytestmark = pytest.mark.gpu


def _check(f, w, f_ref, w_ref):
    # per component 1e-10 relative, with a floor of 1e-10 max|F| -- and of 1e-14 Hartree/bohr: in an ideal lattice every force
    # is zero by symmetry and what either side returns is rounding, O(1e-17)
    fmax = np.abs(f_ref).max()
    tol = 1e-10 * np.maximum(np.abs(f_ref), fmax) + 1e-14
    assert np.all(np.abs(f - f_ref) <= tol), np.abs(f - f_ref).max() / max(fmax, 1e-300)
    wmax = np.abs(w_ref).max()
    assert np.all(np.abs(w - w_ref) <= 1e-10 * np.maximum(np.abs(w_ref), wmax)), (w, w_ref)


@pytest.mark.parametrize("name", golden_names())
def test_forces_and_virial_match_the_reference(name):
    from mc_water_ls_mw_amd.energy import load_boxes
    z = load_golden(name)
    em = load_boxes([z["h"]], [z["xyz"]])
    try:
        e, f, w = em.compute_forces(1)
        e_plain = ctypes_energy(em, 1)
        assert e == e_plain                                  # the energy of the same pass, bit for bit
        nn, jn, vn = em.neighbours(1)
        iv = em.ivect(1)
        e_ref, f_ref, w_ref = model_forces(z["xyz"], iv, nn, jn, vn)
        assert abs(e - e_ref) <= RTOL * abs(e_ref) + 1e-14
        assert f.shape == (len(z["xyz"]), 3) and w.shape == (3, 3)
        if len(z["xyz"]) == 1:
            assert np.array_equal(f, np.zeros((1, 3)))
        _check(f, w, f_ref, w_ref)
        assert np.abs(w - w.T).max() <= 1e-10 * max(np.abs(w).max(), 1e-300)
    finally:
        em.energy_deinit()


def ctypes_energy(em, ils):
    import ctypes
    v = ctypes.c_double(0.0)
    em._chk(em.L.mw_model_energy(ils, ctypes.byref(v)))
    return v.value


def test_single_molecule_has_exactly_zero_force():
    from mc_water_ls_mw_amd.energy import load_boxes
    z = load_golden("single_atom")
    em = load_boxes([z["h"]], [z["xyz"]])
    try:
        _, f, _ = em.compute_forces(1)
        assert np.array_equal(f, np.zeros((1, 3)))
    finally:
        em.energy_deinit()


@pytest.mark.parametrize("gap", [1e-4, 1e-9])
def test_dimer_at_the_cutoff_has_finite_forces(gap):
    from mc_water_ls_mw_amd.energy import load_boxes
    from forces_ref import constants
    sigma, a = float(constants()[0]), float(constants()[6])
    rc = sigma * a
    h = np.eye(3) * 40.0
    xyz = np.array([[10.0, 10.0, 10.0], [10.0 + rc - gap, 10.0, 10.0]])
    em = load_boxes([h], [xyz])
    try:
        e, f, w = em.compute_forces(1)
        assert np.all(np.isfinite(f)) and np.all(np.isfinite(w)) and np.isfinite(e)
        assert np.array_equal(f[0], -f[1])
        nn, jn, vn = em.neighbours(1)
        _, f_ref, _ = model_forces(xyz, em.ivect(1), nn, jn, vn)
        assert np.all(np.abs(f - f_ref) <= 1e-10 * np.abs(f_ref).max() + 1e-300)
    finally:
        em.energy_deinit()


def _thermal_set(name, n, sigma, seed):
    from mc_water_ls_mw_amd import lattice as lat
    z = load_golden(name)
    return [z["h"]] * n, [lat.thermalise(z["xyz"], sigma, seed + k) for k in range(n)]


@pytest.mark.parametrize("name,n", [("ih48_t020", 6), ("ih4096_t015", 3)])
def test_batch_equals_the_single_calls_bit_for_bit(name, n):
    from mc_water_ls_mw_amd.energy import load_boxes
    hs, xs = _thermal_set(name, n, 0.05, 70)
    em = load_boxes(hs, xs)
    try:
        e, f, w = em.forces_batch()
        e2, f2, w2 = em.forces_batch()
        assert np.array_equal(e, e2) and np.array_equal(f, f2) and np.array_equal(w, w2)
        for b in range(n):
            eb, fb, wb = em.compute_forces(b + 1)
            assert eb == e[b] and np.array_equal(fb, f[b]) and np.array_equal(wb, w[b])
            assert eb == ctypes_energy(em, b + 1)
        e3, f3, w3 = em.forces_batch(2, n - 1)
        assert np.array_equal(e3, e[1:]) and np.array_equal(f3, f[1:]) and np.array_equal(w3, w[1:])
    finally:
        em.energy_deinit()


def test_forces_are_differences_of_the_engine_energy():
    """Central differences on the GPU itself: mw_model_energy_of on displaced copies of the box, same list."""
    import ctypes
    from mc_water_ls_mw_amd.energy import load_boxes
    z = load_golden("ih48_t020")
    xyz = z["xyz"]
    em = load_boxes([z["h"]], [xyz])
    try:
        _, f, _ = em.compute_forces(1)
        step = 1e-5
        e = ctypes.c_double(0.0)

        def energy(x):
            x = np.ascontiguousarray(x)
            em._chk(em.L.mw_model_energy_of(1, x.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(e)))
            return e.value

        for i in (0, 7, 30, 47):
            for c in range(3):
                xp, xm = xyz.copy(), xyz.copy()
                xp[i, c] += step
                xm[i, c] -= step
                fd = -(energy(xp) - energy(xm)) / (2 * step)
                assert abs(fd - f[i, c]) <= 1e-7 * np.abs(f).max(), (i, c, fd, f[i, c])
    finally:
        em.energy_deinit()


def test_move_energies_are_unchanged_by_a_forces_call():
    """The forces call writes every molecule's moments; the trial-move kernels' moment path must still see current ones."""
    from mc_water_ls_mw_amd.energy import load_boxes
    z = load_golden("ih4096_t015")
    em = load_boxes([z["h"]], [z["xyz"]])
    try:
        imol, trial = z["trial_imol"], z["trial_xyz"]
        eo0, en0 = em.delta_energy_batch(1, imol, trial)
        em.compute_forces(1)
        eo, en = em.delta_energy_batch(1, imol, trial)
        assert np.array_equal(eo, eo0) and np.array_equal(en, en0)
        assert np.all(np.abs((en - eo) - (z["trial_new"] - z["trial_old"])) <= DE_ATOL)
        assert np.all(np.abs(eo - z["trial_old"]) <= RTOL * np.abs(z["trial_old"]))
        em.forces_batch()
        eo2, en2 = em.delta_energy_batch(1, imol, trial)
        assert np.array_equal(eo2, eo0) and np.array_equal(en2, en0)
    finally:
        em.energy_deinit()


def test_npt_farm_forces_and_virial_pressures_after_device_sweeps(c_oracle):
    """After NPT sweeps with volume moves the device's positions and cells are the authoritative ones: forces_batch and
    virial_pressures must match the reference on the downloaded positions and the synced cells."""
    from mc_water_ls_mw_amd import lattice as lat
    from mc_water_ls_mw_amd.energy import load_boxes
    from mc_water_ls_mw_amd.sweep import KB, MuGrid, WalkerFarm
    z1, z2 = load_golden("ic48"), load_golden("ih48")
    nw, temp, p_au = 3, 200.0, 1.0 / 2.90363081e8
    boxes = []
    for w in range(nw):
        boxes += [(z1["h"], lat.thermalise(z1["xyz"], 0.06, 560 + w)), (z2["h"], lat.thermalise(z2["xyz"], 0.06, 580 + w))]
    em = load_boxes([b[0] for b in boxes], [b[1] for b in boxes])
    farm = WalkerFarm(em, 2, temp, 1.1, grid=MuGrid(101, -400.0, 400.0), weight=np.zeros(101), pressure_au=p_au)
    try:
        farm.options(record=True, samplerun=False, always_switch=True, npt=True, wl_factor=0.05)
        farm.moves(trans_prob=0.5, vol_prob=0.2, dv_max_ang=0.924)
        for w in range(1, nw + 1):
            farm.set_state(w, 1 + (w % 2), farm.initial_mu(w))
        h0 = np.array(em.hmatrix)
        farm.sweep(192, seed=33)
        p, p_atm = farm.virial_pressures()
        hdev = np.array(em.hmatrix)
        assert not np.array_equal(hdev, h0)                  # some volume move was accepted
        e, f, wv = em.forces_batch()
        for b in range(2 * nw):
            x = farm.positions(b + 1)
            nn, jn, vn = em.neighbours(b + 1)
            iv = em.ivect(b + 1)
            e_ref, f_ref, w_ref = model_forces(x, iv, nn, jn, vn)
            assert abs(e[b] - c_oracle.model_energy(x, iv, nn, jn, vn)) <= RTOL * abs(e_ref)
            _check(f[b], wv[b], f_ref, w_ref)
        for w in range(nw):
            b = 2 * w + farm.state(w + 1)["ls"] - 1
            vol = abs(np.linalg.det(hdev[b]))
            x = farm.positions(b + 1)
            nn, jn, vn = em.neighbours(b + 1)
            _, _, w_ref = model_forces(x, em.ivect(b + 1), nn, jn, vn)
            p_ref = (em.nwater * KB * temp + np.trace(w_ref) / 3.0) / vol
            assert abs(p[w] - p_ref) <= 1e-9 * abs(p_ref), (p[w], p_ref)
            assert p_atm[w] == p[w] * 2.90363081e8
        p2, _ = farm.virial_pressures(temperature=300.0)
        assert np.all(p2 > p)
    finally:
        em.energy_deinit()
