"""GPU: CHILL+ ice structure classes (mw_ice_*, EnergyModule.ice_classes / ice_classes_batch / ice_bonds,
WalkerFarm.ice_fractions) against the numpy reference of tests/ice_ref.py on the engine's own neighbour list."""
import ctypes

import numpy as np
import pytest

from conftest import DE_ATOL, golden_names, load_golden
from ice_ref import ANG_TO_BOHR, RC_ANG, ice_classes, stacking_counts

pytestmark = pytest.mark.gpu

RC = RC_ANG * ANG_TO_BOHR

#: boxes that are one phase throughout
ONE_PHASE = {"ih48": 2, "ih48_t020": 2, "ih8_small": 2, "ih1536_t012": 2, "ih4096_ideal": 2,
             "ic48": 1, "ic48_t015": 1, "ic96": 1, "ic64_sheared": 1, "ic4096_ideal": 1, "gas20": 0}


def _reference(em, ils, xyz):
    nn, jn, vn = em.neighbours(ils)
    return ice_classes(xyz, em.ivect(ils), nn, jn, vn, RC)


def _check(cls, counts, c, ref):
    cls_ref, c_ref, counts_ref = ref
    assert cls.dtype == np.uint8 and np.array_equal(cls, cls_ref), np.bincount(cls, minlength=6)
    assert np.array_equal(counts, counts_ref) and np.array_equal(counts, np.bincount(cls, minlength=6))
    if c is None:
        return
    assert c.shape == c_ref.shape
    assert np.array_equal(c == 2.0, c_ref == 2.0)                          # the same entries are bonds
    assert np.array_equal(np.isnan(c), np.isnan(c_ref))                    # ... and the same ones degenerate
    live = (c_ref != 2.0) & ~np.isnan(c_ref)
    assert np.all(np.abs(c[live] - c_ref[live]) <= 1e-12), np.abs(c[live] - c_ref[live]).max()


@pytest.mark.parametrize("name", golden_names())
def test_classes_and_bonds_match_the_reference(name):
    from mc_water_ls_mw_amd.energy import load_boxes
    z = load_golden(name)
    em = load_boxes([z["h"]], [z["xyz"]])
    try:
        cls, counts = em.ice_classes(1)
        c = em.ice_bonds(1)
        ref = _reference(em, 1, z["xyz"])
        _check(cls, counts, c, ref)
        if name in ONE_PHASE:
            assert np.all(cls == ONE_PHASE[name])
    finally:
        em.energy_deinit()


@pytest.mark.parametrize("seq,reps", [("ABAB", (2, 1)), ("ABC", (2, 1)), ("ABCB", (2, 1)), ("ABCACB", (2, 1)),
                                      ("ABCACB", (3, 2)), ("ABCBACAB", (4, 3))])
def test_stacked_boxes(seq, reps):
    from mc_water_ls_mw_amd import lattice as lat
    from mc_water_ls_mw_amd.energy import load_boxes
    h, xyz = lat.stacked_ice_box(seq, reps)
    _, xt = lat.stacked_ice_box(seq, reps, sigma_ang=0.1, seed=17)
    em = load_boxes([h, h], [xyz, xt])
    try:
        cls, counts = em.ice_classes_batch()
        n_cubic, n_hex = stacking_counts(seq, reps)
        assert counts[0, 1] == n_cubic and counts[0, 2] == n_hex and counts[0].sum() == len(xyz), counts[0]
        for b, x in ((0, xyz), (1, xt)):
            _check(cls[b], counts[b], em.ice_bonds(b + 1), _reference(em, b + 1, x))
    finally:
        em.energy_deinit()


def _thermal_set(name, n, sigma, seed):
    from mc_water_ls_mw_amd import lattice as lat
    z = load_golden(name)
    return [z["h"]] * n, [lat.thermalise(z["xyz"], sigma, seed + k) for k in range(n)]


@pytest.mark.parametrize("name,n,sigma", [("ih48_t020", 6, 0.3), ("ih4096_t015", 3, 0.25), ("ih32768_t015", 2, 0.2)])
def test_batch_equals_the_single_calls_bit_for_bit(name, n, sigma):
    from mc_water_ls_mw_amd.energy import load_boxes
    hs, xs = _thermal_set(name, n, sigma, 90)
    em = load_boxes(hs, xs)
    try:
        cls, counts = em.ice_classes_batch()
        assert cls.shape == (n, len(xs[0])) and counts.shape == (n, 6)
        cls2, counts2 = em.ice_classes_batch()
        assert np.array_equal(cls, cls2) and np.array_equal(counts, counts2)
        for b in range(n):
            cb, nb = em.ice_classes(b + 1)
            assert np.array_equal(cb, cls[b]) and np.array_equal(nb, counts[b])
        cls3, counts3 = em.ice_classes_batch(2, n - 1)
        assert np.array_equal(cls3, cls[1:]) and np.array_equal(counts3, counts[1:])
        _check(cls[-1], counts[-1], None, _reference(em, n, xs[-1]))
    finally:
        em.energy_deinit()


def test_cutoff_outside_its_range_fails_with_a_message():
    from mc_water_ls_mw_amd.energy import MwError, load_boxes
    z = load_golden("ih48")
    em = load_boxes([z["h"]], [z["xyz"]])
    try:
        for rc_ang in (0.0, -1.0, 4.31, 10.0, float("nan")):
            with pytest.raises(MwError, match="r_c"):
                em.ice_classes(1, rc_ang=rc_ang)
            with pytest.raises(MwError, match="r_c"):
                em.ice_classes_batch(rc_ang=rc_ang)
            with pytest.raises(MwError, match="r_c"):
                em.ice_bonds(1, rc_ang=rc_ang)
            with pytest.raises(MwError, match="r_c"):
                em.ice_classes_launch(1, 1, rc_ang=rc_ang)
        cls, _ = em.ice_classes(1, rc_ang=4.3)                              # just inside a sigma = 4.3065 A
        nn, jn, vn = em.neighbours(1)
        assert np.array_equal(cls, ice_classes(z["xyz"], em.ivect(1), nn, jn, vn, 4.3 * ANG_TO_BOHR)[0])
    finally:
        em.energy_deinit()


def test_energies_are_unchanged_by_a_classification():
    from mc_water_ls_mw_amd.energy import load_boxes
    z = load_golden("ih4096_t015")
    em = load_boxes([z["h"]], [z["xyz"]])
    try:
        e = ctypes.c_double(0.0)
        em._chk(em.L.mw_model_energy(1, ctypes.byref(e)))
        e0 = e.value
        imol, trial = z["trial_imol"], z["trial_xyz"]
        eo0, en0 = em.delta_energy_batch(1, imol, trial)
        em.ice_classes(1)
        eo, en = em.delta_energy_batch(1, imol, trial)
        assert np.array_equal(eo, eo0) and np.array_equal(en, en0)
        em.ice_classes_batch()
        em.ice_bonds(1)
        eo2, en2 = em.delta_energy_batch(1, imol, trial)
        assert np.array_equal(eo2, eo0) and np.array_equal(en2, en0)
        assert np.all(np.abs((en - eo) - (z["trial_new"] - z["trial_old"])) <= DE_ATOL)
        em._chk(em.L.mw_model_energy(1, ctypes.byref(e)))
        assert e.value == e0
    finally:
        em.energy_deinit()


def _npt_farm(nw=3):
    from mc_water_ls_mw_amd import lattice as lat
    from mc_water_ls_mw_amd.energy import load_boxes
    from mc_water_ls_mw_amd.sweep import MuGrid, WalkerFarm
    z1, z2 = load_golden("ic48"), load_golden("ih48")
    boxes = []
    for w in range(nw):
        boxes += [(z1["h"], lat.thermalise(z1["xyz"], 0.06, 560 + w)), (z2["h"], lat.thermalise(z2["xyz"], 0.06, 580 + w))]
    em = load_boxes([b[0] for b in boxes], [b[1] for b in boxes])
    farm = WalkerFarm(em, 2, 200.0, 1.1, grid=MuGrid(101, -400.0, 400.0), weight=np.zeros(101), pressure_au=1.0 / 2.90363081e8)
    farm.options(record=True, samplerun=False, always_switch=True, npt=True, wl_factor=0.05)
    farm.moves(trans_prob=0.5, vol_prob=0.2, dv_max_ang=0.924)
    for w in range(1, nw + 1):
        farm.set_state(w, 1 + (w % 2), farm.initial_mu(w))
    return em, farm


def test_a_farm_sweep_is_unchanged_by_ice_fractions():
    def run(classify):
        em, farm = _npt_farm()
        try:
            farm.sweep(96, seed=41)
            if classify:
                f = farm.ice_fractions()
                assert f.shape == (farm.nwalkers, 2, 6)
            farm.sweep(96, seed=41, move0=96)
            nb = em.num_lattices
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


def test_npt_farm_ice_fractions_after_device_sweeps():
    """After NPT sweeps with volume moves the device's positions and cells are the authoritative ones: ice_fractions must
    match the reference on the downloaded positions, the synced cells' image vectors and the engine's list."""
    em, farm = _npt_farm()
    try:
        h0 = np.array(em.hmatrix)
        farm.sweep(192, seed=33)
        frac = farm.ice_fractions()
        assert not np.array_equal(np.array(em.hmatrix), h0)                 # some volume move was accepted (and synced)
        assert frac.shape == (3, 2, 6) and np.allclose(frac.sum(axis=2), 1.0)
        for b in range(em.num_lattices):
            cls_ref, _, counts_ref = _reference(em, b + 1, farm.positions(b + 1))
            assert np.array_equal(frac[b // 2, b % 2], counts_ref / float(em.nwater)), (b, frac[b // 2, b % 2], counts_ref)
        cls, counts = em.ice_classes_batch()
        for b in range(em.num_lattices):
            assert np.array_equal(counts[b], np.bincount(cls[b], minlength=6))
    finally:
        em.energy_deinit()
