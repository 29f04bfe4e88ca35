"""GPU: pair-distance histograms (mw_rdf*, EnergyModule.rdf_counts / rdf_counts_batch / rdf_launch / rdf, WalkerFarm.rdf)
against the numpy reference of tests/rdf_ref.py, under its comparison rule: cumulative counts may differ at a bin edge by
no more than the pairs the reference finds within 1e-9 bohr of that edge, and at most one edge of an input has any.
Odd N, an odd number of tiles, ragged last tiles and 1 / 7 / 4096 bins on both kernels: tests/test_gpu_derived_shapes.py."""
import ctypes

import numpy as np
import pytest

from conftest import golden_names, load_golden
from rdf_ref import ANG_TO_BOHR, assert_cap, assert_same, image_range, rdf_brute, rdf_fast, widths

pytestmark = pytest.mark.gpu

NBINS = 200
BOHR_TO_ANG = 0.5291772108


def _r_max_ang(h, r_ang=10.0):
    return min(r_ang, 1.5 * widths(h).min() * (1.0 - 1e-6) * BOHR_TO_ANG)


def _bohr(r_ang):
    return float(r_ang) / 0.5291772108                     # as the module converts it


def _reference(h, xyz, r_ang, nbins=NBINS):
    if len(xyz) <= 96:
        return rdf_brute(h, xyz, _bohr(r_ang), nbins)
    return rdf_fast(h, xyz, _bohr(r_ang), nbins, chunk=128 if len(xyz) > 8192 else 256, workers=8)


def _images(h, r_ang):
    return int(np.prod([2 * image_range(_bohr(r_ang), w) + 1 for w in widths(h)]))


@pytest.mark.parametrize("name", golden_names())
def test_every_golden_box_matches_the_reference(name):
    from mc_water_ls_mw_amd.energy import load_boxes, rdf_from_counts
    z = load_golden(name)
    r_ang = _r_max_ang(z["h"])
    ref, edge = _reference(z["h"], z["xyz"], r_ang)
    assert_cap(edge, name)
    em = load_boxes([z["h"]], [z["xyz"]])
    try:
        hist = em.rdf_counts(1, r_ang, NBINS)
        assert hist.dtype == np.int64 and hist.shape == (NBINS,)
        print(name, "N", len(z["xyz"]), "r_max", r_ang, "pairs", int(hist.sum()), "ref", int(ref.sum()), "near an edge", int(edge.sum()))
        assert_same(hist, ref, edge, name)
        d = em.last_dispatch("rdf")
        assert d["boxes"] == 1 and d["small"] == (len(z["xyz"]) <= 64) and d["images"] == _images(z["h"], r_ang), d
        assert d["workgroups_per_box"] == (1 if d["small"] else -(-len(z["xyz"]) // 256))
        r, g, n = em.rdf(1, r_ang, NBINS)
        r2, g2, n2 = rdf_from_counts(hist, len(z["xyz"]), abs(np.linalg.det(z["h"])), r_ang)
        assert np.array_equal(r, r2) and np.allclose(g, g2, rtol=1e-13, atol=0) and np.array_equal(n, n2)
    finally:
        em.energy_deinit()


@pytest.mark.parametrize("name,r_of_wmin,r_ang,images,small", [
    ("ih48", 0.45, None, 1, True), ("ih48", 0.9, None, 9, True), ("ih48", 1.49, None, 27, True),
    ("ic96", None, 5.0, 3, False), ("ih1536_t012", None, 10.0, None, False)])
def test_image_branches_and_geometry(name, r_of_wmin, r_ang, images, small):
    from mc_water_ls_mw_amd.energy import load_boxes
    z = load_golden(name)
    if r_ang is None:
        r_ang = r_of_wmin * widths(z["h"]).min() * BOHR_TO_ANG
    if images is not None:
        assert _images(z["h"], r_ang) == images                    # the rule itself, on the reference's side
    ref, edge = _reference(z["h"], z["xyz"], r_ang)
    assert_cap(edge, name)
    em = load_boxes([z["h"]], [z["xyz"]])
    try:
        hist = em.rdf_counts(1, r_ang, NBINS)
        assert_same(hist, ref, edge, (name, r_ang))
        d = em.last_dispatch("rdf")
        assert d["images"] == _images(z["h"], r_ang) and bool(d["small"]) == small, d
        assert d["lds_bytes"] > 0
    finally:
        em.energy_deinit()


def test_unwrapped_positions_give_the_same_histogram():
    from mc_water_ls_mw_amd.energy import load_boxes
    z = load_golden("ih4096_t015")
    h, xyz = z["h"], z["xyz"]
    ref, edge = _reference(h, xyz, 10.0)
    assert_cap(edge)
    rng = np.random.default_rng(11)
    moved = xyz.copy()
    pick = rng.permutation(len(xyz))[:len(xyz) // 3]
    moved[pick] += rng.integers(-2, 3, (len(pick), 3)).astype(np.float64) @ h
    assert not np.array_equal(moved, xyz)
    em = load_boxes([h, h], [xyz, moved])
    try:
        hist = em.rdf_counts_batch(1, 2, 10.0, NBINS)
        assert_same(hist[0], ref, edge, "as stored")
        assert_same(hist[1], ref, edge, "displaced by lattice translations")
    finally:
        em.energy_deinit()


def _thermal_set(name, n, sigma, seed):
    from mc_water_ls_mw_amd import lattice as lat
    z = load_golden(name)
    return [z["h"]] * n, [lat.thermalise(z["xyz"], sigma, seed + k) for k in range(n)]


@pytest.mark.parametrize("name,n,sigma,r_of_w", [("ih48_t020", 6, 0.3, 0.5), ("ih4096_t015", 3, 0.25, 0.5),
                                                 ("ih32768_t015", 2, 0.2, None)])
def test_batch_equals_the_single_calls_bit_for_bit(name, n, sigma, r_of_w):
    """Boxes of different cells in one launch: box 2 is scaled by 0.97 and box 3 by 1.03 where there are three, and r_max is
    half a width of the unscaled cell, so the image sets of the boxes of one launch differ."""
    from mc_water_ls_mw_amd.energy import load_boxes
    hs, xs = _thermal_set(name, n, sigma, 90)
    hs = [np.array(h) for h in hs]
    r_ang = 10.0
    if r_of_w is not None:
        for b, f in ((1, 0.97), (2, 1.03)):
            hs[b], xs[b] = hs[b] * f, xs[b] * f
        r_ang = r_of_w * widths(hs[0])[2] * BOHR_TO_ANG
        assert len({_images(h, r_ang) for h in hs}) > 1
    em = load_boxes(hs, xs)
    try:
        hist = em.rdf_counts_batch(1, n, r_ang, NBINS)
        assert hist.shape == (n, NBINS) and hist.dtype == np.int64
        assert em.last_dispatch("rdf")["images"] == max(_images(h, r_ang) for h in hs)
        assert np.array_equal(hist, em.rdf_counts_batch(1, n, r_ang, NBINS))
        for b in range(n):
            assert np.array_equal(em.rdf_counts(b + 1, r_ang, NBINS), hist[b]), b
        assert np.array_equal(em.rdf_counts_batch(2, n - 1, r_ang, NBINS), hist[1:])
        em.rdf_launch(1, n, r_ang, NBINS, timer_slot=7)
        em.sync()
        assert em.timer_ms(7) > 0.0
        if len(xs[0]) <= 4096:
            for b in range(n):
                ref, edge = _reference(hs[b], xs[b], r_ang)
                assert_cap(edge, (name, b))
                assert_same(hist[b], ref, edge, (name, b))
    finally:
        em.energy_deinit()


def test_bin_counts_and_argument_errors():
    from mc_water_ls_mw_amd.energy import MwError, load_boxes
    z = load_golden("ih48")
    small = z["h"] * 0.9
    em = load_boxes([z["h"], z["h"], small], [z["xyz"], z["xyz"], z["xyz"] * 0.9])
    try:
        r_ang = _r_max_ang(z["h"])
        total = None
        for nbins in (1, 7, 4096):
            ref, edge = _reference(z["h"], z["xyz"], r_ang, nbins)
            assert_cap(edge, nbins)
            hist = em.rdf_counts(1, r_ang, nbins)
            assert hist.shape == (nbins,)
            assert_same(hist, ref, edge, nbins)
            batch = em.rdf_counts_batch(1, 2, r_ang, nbins)
            assert np.array_equal(batch[0], hist) and np.array_equal(batch[1], hist)
            total = int(hist.sum()) if total is None else total
            assert abs(int(hist.sum()) - total) <= int(edge[-1])          # only a pair at r_max itself may come or go
        wmin_ang = widths(z["h"]).min() * BOHR_TO_ANG
        before = em.rdf_counts(1, 5.0, 50)
        for bad in (0.0, -1.0, float("nan"), 1.51 * wmin_ang):
            with pytest.raises(MwError, match="r_max"):
                em.rdf_counts(1, bad, NBINS)
            with pytest.raises(MwError, match="r_max"):
                em.rdf_counts_batch(1, 2, bad, NBINS)
            with pytest.raises(MwError, match="r_max"):
                em.rdf_launch(1, 2, bad, NBINS)
        for bad in (0, 4097):
            with pytest.raises(MwError, match="nbins"):
                em.rdf_counts(1, 5.0, bad)
            with pytest.raises(MwError, match="nbins"):
                em.rdf_counts_batch(1, 2, 5.0, bad)
            with pytest.raises(MwError, match="nbins"):
                em.rdf_launch(1, 2, 5.0, bad)
        # only the LAST box of the batch is too small for this r_max: the message names it
        r_edge = 1.45 * wmin_ang
        assert r_edge > 1.5 * widths(small).min() * BOHR_TO_ANG
        em.rdf_counts_batch(1, 2, r_edge, NBINS)
        with pytest.raises(MwError, match=r"r_max.*box 3"):
            em.rdf_counts_batch(1, 3, r_edge, NBINS)
        with pytest.raises(MwError, match=r"r_max.*box 3"):
            em.rdf_launch(2, 2, r_edge, NBINS)
        assert np.array_equal(em.rdf_counts(1, 5.0, 50), before)
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


def test_npt_farm_rdf_after_device_sweeps():
    """After NPT sweeps with volume moves the device's positions and cells are the authoritative ones: farm.rdf() must be
    rdf_from_counts of the reference histograms of the downloaded positions and the synced cells, box by box, averaged."""
    from mc_water_ls_mw_amd.energy import rdf_from_counts
    em, farm = _npt_farm()
    try:
        h0 = np.array(em.hmatrix)
        farm.sweep(192, seed=33)
        r, g, n = farm.rdf()
        assert r.shape == (NBINS,) and g.shape == n.shape == (2, NBINS)
        assert not np.array_equal(np.array(em.hmatrix), h0)                # some volume move was accepted (and synced)
        hs = farm.sync_cells()
        gs, ns = [], []
        clear = np.ones(NBINS, dtype=bool)                                  # bins that no pair near an edge can move between
        counts = em.rdf_counts_batch(1, em.num_lattices, 10.0, NBINS)
        for b in range(em.num_lattices):
            ref, edge = rdf_brute(hs[b], farm.positions(b + 1), _bohr(10.0), NBINS)
            assert_cap(edge, b)
            assert_same(counts[b], ref, edge, b)
            for k in np.nonzero(edge[1:])[0] + 1:
                clear[k - 1:k + 1] = False
            _, gb, nb = rdf_from_counts(ref, em.nwater, abs(np.linalg.det(hs[b])), 10.0)
            gs.append(gb), ns.append(nb)
        g_ref = np.array(gs).reshape(3, 2, NBINS).mean(axis=0)
        n_ref = np.array(ns).reshape(3, 2, NBINS).mean(axis=0)
        assert clear.sum() >= NBINS - 2 * em.num_lattices
        assert np.allclose(g[:, clear], g_ref[:, clear], rtol=1e-12, atol=0)
        assert np.allclose(n[:, clear], n_ref[:, clear], rtol=1e-12, atol=0)
        k35 = int(round(3.5 / 10.0 * NBINS)) - 1                            # the bin whose upper edge is 3.5 Angstrom
        print("n(3.5 A) per lattice", n[:, k35], "reference", n_ref[:, k35])
        assert np.all(np.abs(n[:, k35] - 4.0) <= 0.2), n[:, k35]
        beyond = r > 4.0                                                    # Ih and Ic part beyond the second shell
        assert np.abs(g[0, beyond] - g[1, beyond]).max() > 0.5
    finally:
        em.energy_deinit()


def test_a_farm_sweep_is_unchanged_by_rdf():
    def run(with_rdf):
        em, farm = _npt_farm()
        try:
            farm.sweep(96, seed=41)
            if with_rdf:
                r, g, n = farm.rdf()
                assert g.shape == (2, NBINS)
                em.rdf_launch(1, em.num_lattices, 6.0, 64)
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


def test_energies_classes_and_the_server_are_unchanged_by_rdf():
    from mc_water_ls_mw_amd.energy import load_boxes
    z = load_golden("ih4096_t015")
    em = load_boxes([z["h"]], [z["xyz"]])
    try:
        e = ctypes.c_double(0.0)
        em._chk(em.L.mw_model_energy(1, ctypes.byref(e)))
        e0 = e.value
        imol, trial = z["trial_imol"], z["trial_xyz"]
        eo0, en0 = em.delta_energy_batch(1, imol, trial)
        cls0, cnt0 = em.ice_classes_batch()
        loc0 = [em.compute_local_real_energy(m, 1) for m in (1, 17, 4096)]
        pos0 = np.zeros((4096, 3))
        em._chk(em.L.mw_download_positions(1, pos0.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        em.rdf_counts(1, 10.0, NBINS)
        em.rdf_counts_batch(1, 1, 7.0, 33)
        em.rdf_launch(1, 1, 10.0, 4096)
        loc = [em.compute_local_real_energy(m, 1) for m in (1, 17, 4096)]
        assert loc == loc0
        eo, en = em.delta_energy_batch(1, imol, trial)
        assert np.array_equal(eo, eo0) and np.array_equal(en, en0)
        cls, cnt = em.ice_classes_batch()
        assert np.array_equal(cls, cls0) and np.array_equal(cnt, cnt0)
        em._chk(em.L.mw_model_energy(1, ctypes.byref(e)))
        assert e.value == e0
        pos = np.zeros((4096, 3))
        em._chk(em.L.mw_download_positions(1, pos.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        assert np.array_equal(pos, pos0)
    finally:
        em.energy_deinit()
