"""GPU: the engine's derived kernels -- forces and virial, CHILL+ classes and bonds, ice clusters, the pair-distance histogram --
on the inputs of tests/derived_cases.py, the shapes the golden boxes and the stacked ice boxes do not have: odd N in k_rdf_small;
an odd number of tiles, a ragged last tile next to full ones in k_rdf_tiles; 1, 7 and 4096 bins; every per-axis image set on an
oblique cell against a reference that uses no image rule; a degenerate CHILL+ bond and a molecule with no neighbour; the 36 random
systems tests/test_gpu_fuzz.py holds the energy paths to; five boxes of different cells and image tables in one context.

The bars and comparison rules are the existing ones, imported: test_gpu_forces._check (1e-10 relative with its floors),
test_gpu_ice._check (classes and counts exact, bonds 1e-12, the same NaN and non-bond entries), == for cluster labels and
summaries, rdf_ref.assert_same after assert_cap.  tests/test_derived_cases.py shows on the CPU that the inputs are what they claim
and that those rules cannot hide a failure on them.  Every test prints what it measured over its bar before it asserts."""
import numpy as np
import pytest

import cluster_ref as cr
import derived_cases as dc
from conftest import RTOL
from forces_ref import model_forces
from ice_ref import ANG_TO_BOHR, RC_ANG, ice_classes
from rdf_ref import assert_cap, assert_same, rdf_brute
from test_gpu_forces import _check as check_forces, ctypes_energy
from test_gpu_ice import _check as check_ice

pytestmark = pytest.mark.gpu

RC = RC_ANG * ANG_TO_BOHR
NBINS = 200
MASK_ALL = 0b111110
FUZZ = {seed: (kind, h, x) for seed, kind, h, x in dc.fuzz_systems()}


def _forces_against_the_mirror(what, f, w, x, iv, nn, jn, vn):
    """test_gpu_forces._check against forces_ref.model_forces, the sum rule that follows from it and the virial's symmetry;
    prints the largest deviation in units of the bar first.  Returns the mirror's (e, f, w)."""
    e_ref, f_ref, w_ref = model_forces(x, iv, nn, jn, vn)
    fmax, wmax = np.abs(f_ref).max(), np.abs(w_ref).max()
    f_over = (np.abs(f - f_ref) / (1e-10 * np.maximum(np.abs(f_ref), fmax) + 1e-14)).max()
    w_over = (np.abs(w - w_ref) / np.maximum(1e-10 * np.maximum(np.abs(w_ref), wmax), 1e-300)).max()
    print(what, "N", len(x), "max|F|", fmax, "F over bar", f_over, "W over bar", w_over, "|sum F|", np.abs(f.sum(axis=0)).max())
    check_forces(f, w, f_ref, w_ref)
    assert np.all(np.abs(f.sum(axis=0)) <= 1e-10 * len(x) * fmax), f.sum(axis=0)
    assert np.abs(w - w.T).max() <= 1e-10 * max(np.abs(w).max(), 1e-300)
    return e_ref, f_ref, w_ref


def _ice_against_the_mirror(what, cls, counts, c, x, iv, nn, jn, vn):
    ref = ice_classes(x, iv, nn, jn, vn, RC)
    if c is not None:
        live = (ref[1] != 2.0) & ~np.isnan(ref[1]) & (c != 2.0) & ~np.isnan(c)
        print(what, "classes", np.bincount(cls, minlength=6), "bonds", int(live.sum()), "degenerate", int(np.isnan(ref[1]).sum()),
              "bond value over bar", (np.abs(c - ref[1])[live] / 1e-12).max() if live.any() else 0.0)
    check_ice(cls, counts, c, ref)
    return ref


def _cluster_masks(cls):
    return [MASK_ALL] + [1 << k for k in range(1, 6) if np.any(cls == k)]


# -- g(r): every row of the table -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(dc.RDF_CASES))
def test_rdf_case_matches_its_reference(name):
    from mc_water_ls_mw_amd.energy import load_boxes
    c = dc.RDF_CASES[name]
    ref, edge = dc.rdf_reference(name)
    assert_cap(edge, name)
    em = load_boxes([c.h], [c.xyz])
    try:
        hist = em.rdf_counts(1, c.r_max_ang, c.nbins)
        d = em.last_dispatch("rdf")
        print(name, "N", c.n, "r_max", c.r_max_ang, "bins", c.nbins, "pairs", int(hist.sum()), "ref", int(ref.sum()),
              "near an edge", int(edge.sum()), d)
        assert hist.dtype == np.int64 and hist.shape == (c.nbins,)
        assert_same(hist, ref, edge, name)
        if edge[c.nbins] == 0:
            assert int(hist.sum()) == int(ref.sum())
        small = c.n <= dc.SMALL_MAX
        assert d["boxes"] == 1 and bool(d["small"]) == small and d["images"] == dc.image_count(c.h, c.r_max_ang), d
        assert d["images"] == int(np.prod([2 * m + 1 for m in c.images]))
        assert d["workgroups_per_box"] == (1 if small else -(-c.n // dc.TILE)), d
        assert d["lds_bytes"] == (4 * (3 * 64 * 8 + 4 * c.nbins) if small else 4 * c.nbins + 3 * dc.TILE * 8), d
    finally:
        em.energy_deinit()


# -- the fuzz systems: everything derived, on the oracle's list -----------------------------------------------------------------------
def _skip_reason(c_oracle, h, x):
    """The skip rules of tests/test_gpu_fuzz.py: (None, image vectors, list) where neither fires."""
    iv = c_oracle.ivects(h)
    if len(iv) > 1000:
        return "cell too thin for the image table", iv, None
    lists = c_oracle.neighbours(x, iv, 64)
    if lists[0].max() > 64:
        return "denser than maxneigh = 64", iv, None
    return None, iv, lists


def test_at_most_two_fuzz_systems_are_skipped(c_oracle):
    skipped = {seed: why for seed, (kind, h, x) in FUZZ.items() for why in [_skip_reason(c_oracle, h, x)[0]] if why}
    print("skipped", skipped)
    assert len(skipped) <= 2, skipped


@pytest.mark.parametrize("seed", range(36))
def test_derived_quantities_on_a_fuzz_system(seed, c_oracle):
    from mc_water_ls_mw_amd.energy import load_boxes
    kind, h, x = FUZZ[seed]
    n = len(x)
    why, iv, lists = _skip_reason(c_oracle, h, x)
    if why:
        pytest.skip(why)
    nn, jn, vn = lists
    what = (seed, kind)
    em = load_boxes([h], [x], maxneigh=64)
    try:
        assert np.array_equal(em.ivect(1), iv)
        gnn, gjn, gvn = em.neighbours(1)
        assert np.array_equal(gnn, nn) and np.array_equal(gjn, jn) and np.array_equal(gvn, vn), what
        everyone = np.arange(1, n + 1)
        e0 = em.compute_model_energy(1)
        loc0 = em.local_energy_batch(1, everyone)
        e_oracle = c_oracle.model_energy(x, iv, nn, jn, vn)
        assert abs(e0 - e_oracle) <= RTOL * abs(e_oracle) + 1e-14, what

        e, f, w = em.compute_forces(1)
        assert e == e0 and e == ctypes_energy(em, 1)                    # the energy of the same pass, bit for bit
        e_ref, _, _ = _forces_against_the_mirror(what, f, w, x, iv, nn, jn, vn)
        assert abs(e - e_ref) <= RTOL * abs(e_ref) + 1e-14

        cls, counts = em.ice_classes(1)
        ref = _ice_against_the_mirror(what, cls, counts, em.ice_bonds(1), x, iv, nn, jn, vn)
        for mask in _cluster_masks(ref[0]):
            label, summary = em.ice_clusters(1, mask)
            label_ref, summary_ref = cr.clusters(ref[0], x, iv, nn, jn, vn, RC, mask)
            assert np.array_equal(label, label_ref) and np.array_equal(summary, summary_ref), (what, bin(mask), summary, summary_ref)

        r_ang = dc.r_max_ang(h)
        hist_ref, edge = rdf_brute(h, x, dc.bohr(r_ang), NBINS)
        assert_cap(edge, what)
        hist = em.rdf_counts(1, r_ang, NBINS)
        d = em.last_dispatch("rdf")
        print(what, "r_max", r_ang, "pairs", int(hist.sum()), "near an edge", int(edge.sum()), d)
        assert_same(hist, hist_ref, edge, what)
        assert bool(d["small"]) == (n <= dc.SMALL_MAX) and d["images"] == dc.image_count(h, r_ang), d

        # the derived passes wrote nothing the energy paths read
        assert em.compute_model_energy(1) == e0 and em.model_energy[0] == e0
        assert np.array_equal(em.local_energy_batch(1, everyone), loc0)
    finally:
        em.energy_deinit()


# -- the degenerate box ---------------------------------------------------------------------------------------------------------------
def test_degenerate_bonds_and_an_isolated_molecule():
    from mc_water_ls_mw_amd.energy import load_boxes
    h, x = dc.DEGENERATE
    mid, alone, centre = dc.DEGENERATE_MIDDLE, dc.DEGENERATE_ALONE, dc.DEGENERATE_CENTRE
    em = load_boxes([h], [x])
    try:
        nn, jn, vn = em.neighbours(1)
        iv = em.ivect(1)
        cls, counts = em.ice_classes(1)
        c = em.ice_bonds(1)
        ref = _ice_against_the_mirror("degenerate", cls, counts, c, x, iv, nn, jn, vn)
        bonds = c != 2.0
        assert bonds[mid].sum() == 2 and np.isnan(c[mid][bonds[mid]]).all() and cls[mid] == 0
        assert np.isnan(c[0][bonds[0]]).all() and np.isnan(c[2][bonds[2]]).all()
        assert bonds[alone].sum() == 0 and cls[alone] == 0
        assert bonds[centre].sum() == 4 and not np.isnan(c[centre]).any()
        for mask in (MASK_ALL, 0b1110) + tuple(1 << k for k in range(1, 6)):
            label, summary = em.ice_clusters(1, mask)
            label_ref, summary_ref = cr.clusters(ref[0], x, iv, nn, jn, vn, RC, mask)
            assert np.array_equal(label, label_ref) and np.array_equal(summary, summary_ref), (bin(mask), summary, summary_ref)
            assert label[mid] == 0 and label[alone] == 0
        e, f, w = em.compute_forces(1)
        assert e == ctypes_energy(em, 1)
        e_ref, _, _ = _forces_against_the_mirror("degenerate", f, w, x, iv, nn, jn, vn)
        assert abs(e - e_ref) <= RTOL * abs(e_ref) + 1e-14
        assert np.array_equal(f[alone], np.zeros(3))
        assert np.abs(f[mid]).max() > 0.0 or np.abs(f[0]).max() > 0.0
    finally:
        em.energy_deinit()


# -- five different boxes in one context ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", list(dc.BATCHES))
def test_batches_of_different_cells_equal_the_single_calls_and_their_mirrors(n, c_oracle):
    from mc_water_ls_mw_amd.energy import load_boxes
    boxes = dc.BATCHES[n]
    nb = len(boxes)
    r_ang = dc.batch_r_max_ang(boxes)
    em = load_boxes([h for h, _ in boxes], [x for _, x in boxes], maxneigh=64)
    try:
        ivs = [em.ivect(b + 1) for b in range(nb)]
        for b, (h, _) in enumerate(boxes):
            assert np.array_equal(ivs[b], c_oracle.ivects(h)), b
        assert len({len(iv) for iv in ivs}) > 1, [len(iv) for iv in ivs]
        energies = em.model_energy_batch(1, nb).copy()

        e, f, w = em.forces_batch()
        cls, counts = em.ice_classes_batch()
        clusters = {mask: em.ice_clusters_batch(1, nb, mask) for mask in (MASK_ALL, 0b1110)}
        hist = em.rdf_counts_batch(1, nb, r_ang, NBINS)
        d = em.last_dispatch("rdf")
        images = [dc.image_count(h, r_ang) for h, _ in boxes]
        print(n, "image vectors", [len(iv) for iv in ivs], "r_max", r_ang, "g(r) images", images, d)
        assert d["boxes"] == nb and d["images"] == max(images) and len(set(images)) > 1, d
        assert bool(d["small"]) == (n <= dc.SMALL_MAX) and d["workgroups_per_box"] == (1 if n <= dc.SMALL_MAX else -(-n // dc.TILE))

        # the sub-range (2, 3)
        e3, f3, w3 = em.forces_batch(2, 3)
        assert np.array_equal(e3, e[1:4]) and np.array_equal(f3, f[1:4]) and np.array_equal(w3, w[1:4])
        cls3, counts3 = em.ice_classes_batch(2, 3)
        assert np.array_equal(cls3, cls[1:4]) and np.array_equal(counts3, counts[1:4])
        for mask, (label, summary) in clusters.items():
            label3, summary3 = em.ice_clusters_batch(2, 3, mask)
            assert np.array_equal(label3, label[1:4]) and np.array_equal(summary3, summary[1:4]), bin(mask)
        assert np.array_equal(em.rdf_counts_batch(2, 3, r_ang, NBINS), hist[1:4])

        for b, (h, x) in enumerate(boxes):
            what = (n, b)
            nn, jn, vn = em.neighbours(b + 1)
            # the single calls, bit for bit
            eb, fb, wb = em.compute_forces(b + 1)
            assert eb == e[b] and np.array_equal(fb, f[b]) and np.array_equal(wb, w[b]), what
            assert eb == ctypes_energy(em, b + 1)
            cb, cntb = em.ice_classes(b + 1)
            assert np.array_equal(cb, cls[b]) and np.array_equal(cntb, counts[b]), what
            for mask, (label, summary) in clusters.items():
                lb, sb = em.ice_clusters(b + 1, mask)
                assert np.array_equal(lb, label[b]) and np.array_equal(sb, summary[b]), (what, bin(mask))
            assert np.array_equal(em.rdf_counts(b + 1, r_ang, NBINS), hist[b]), what
            # the mirrors
            e_ref, _, _ = _forces_against_the_mirror(what, f[b], w[b], x, ivs[b], nn, jn, vn)
            assert abs(e[b] - e_ref) <= RTOL * abs(e_ref) + 1e-14, what
            ref = _ice_against_the_mirror(what, cls[b], counts[b], em.ice_bonds(b + 1), x, ivs[b], nn, jn, vn)
            for mask, (label, summary) in clusters.items():
                label_ref, summary_ref = cr.clusters(ref[0], x, ivs[b], nn, jn, vn, RC, mask)
                assert np.array_equal(label[b], label_ref) and np.array_equal(summary[b], summary_ref), (what, bin(mask))
            hist_ref, edge = rdf_brute(h, x, dc.bohr(r_ang), NBINS)
            assert_cap(edge, what)
            assert_same(hist[b], hist_ref, edge, what)
        assert len({tuple(c) for c in counts}) > 1                                # the boxes do differ
        assert np.array_equal(em.model_energy_batch(1, nb), energies)
    finally:
        em.energy_deinit()
