"""GPU: clusters of ice-like molecules (mw_ice_clusters*, EnergyModule.ice_clusters / ice_clusters_batch,
WalkerFarm.largest_ice_clusters) against the union-find reference of tests/cluster_ref.py on the engine's own neighbour list
and classes.  The results are integers in a canonical form: every comparison is ==.

Run as a script (`python tests/test_gpu_ice_clusters.py OUT.npz`) it evaluates the reference and shuffled-order cases and
saves what the engine returned: the LDS-variant test does that in a fresh child process with MW_ICE_CLUSTERS_LDS=0."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden
import cluster_ref as cr
from ice_ref import ANG_TO_BOHR, RC_ANG

pytestmark = pytest.mark.gpu

RC = RC_ANG * ANG_TO_BOHR
MASKS = (0b10, 0b100, 0b110, 0b1110, 0b111110)
SEQ160 = "ABCABCABABABCABCBCBC"
#: cluster sizes known in closed form (tests/test_cluster_ref.py pins them on brute-force neighbours): box -> mask -> sizes
CLOSED_FORM = {"abcb32": {0b10: [2] * 8, 0b100: [2] * 8, 0b110: [32]},
               "sd160": {0b10: [64, 32], 0b100: [32, 32], 0b110: [160], 0b1110: [160], 0b111110: [160]},
               "sd160_thermal": {0b10: [64, 32], 0b100: [32, 32], 0b110: [160], 0b1110: [160], 0b111110: [160]},
               "ih512": {0b100: [512], 0b10: [], 0b110: [512], 0b1110: [512], 0b111110: [512]},
               "ih512_reversed": {0b100: [512]}, "ih512_permuted": {0b100: [512]}}


@functools.lru_cache(maxsize=None)
def _case_boxes():
    from mc_water_ls_mw_amd import lattice as lat
    h512, x512 = lat.stacked_ice_box("AB" * 32, (2, 1))
    return {"abcb32": lat.stacked_ice_box("ABCB", (2, 1)),
            "sd160": lat.stacked_ice_box(SEQ160, (2, 1)),
            "sd160_thermal": lat.stacked_ice_box(SEQ160, (2, 1), sigma_ang=0.08),
            "ih512": (h512, x512),
            "defect": cr.defect_box(),
            "ih512_reversed": (h512, np.ascontiguousarray(x512[::-1])),
            "ih512_permuted": (h512, np.ascontiguousarray(x512[np.random.default_rng(64).permutation(len(x512))]))}


@functools.lru_cache(maxsize=None)
def _engine_results():
    """{box: what the engine says of it}: labels and summaries for every mask, what mw_ice_clusters_last reported, and the
    engine's own list and classes (for the reference)."""
    from mc_water_ls_mw_amd.energy import load_boxes
    out = {}
    for name, (h, xyz) in _case_boxes().items():
        em = load_boxes([h], [xyz])
        try:
            labels, summaries, last = [], [], []
            for mask in MASKS:
                label, summary = em.ice_clusters(1, mask)
                assert label.dtype == np.int32 and summary.dtype == np.int32 and label.shape == (len(xyz),)
                labels.append(label), summaries.append(summary), last.append(em.ice_clusters_last())
            nn, jn, vn = em.neighbours(1)
            out[name] = {"label": np.array(labels), "summary": np.array(summaries), "last": last, "list": (nn, jn, vn),
                         "ivect": em.ivect(1), "cls": em.ice_classes(1)[0], "xyz": xyz}
        finally:
            em.energy_deinit()
    return out


def _reference(res, mask):
    nn, jn, vn = res["list"]
    return cr.clusters(res["cls"], res["xyz"], res["ivect"], nn, jn, vn, RC, mask)


@pytest.mark.parametrize("name", ["abcb32", "sd160", "sd160_thermal", "ih512", "defect"])
def test_labels_and_summaries_equal_the_reference_and_the_closed_form(name):
    res = _engine_results()[name]
    for k, mask in enumerate(MASKS):
        label, summary = res["label"][k], res["summary"][k]
        label_ref, summary_ref = _reference(res, mask)
        assert np.array_equal(label, label_ref), (name, bin(mask), cr.sizes(label), cr.sizes(label_ref))
        assert np.array_equal(summary, summary_ref), (name, bin(mask), summary, summary_ref)
        if mask in CLOSED_FORM.get(name, {}):
            assert cr.sizes(label) == CLOSED_FORM[name][mask], (name, bin(mask))
        from mc_water_ls_mw_amd.energy import cluster_sizes
        assert list(cluster_sizes(label)) == cr.sizes(label)
        assert res["last"][k]["boxes"] == 1 and res["last"][k]["rounds"] >= 1
    if name == "defect":
        sz = cr.sizes(res["label"][MASKS.index(0b1110)])
        assert len(sz) >= 3 and len(set(sz)) >= 2 and sz[-1] == 1, sz


@pytest.mark.parametrize("name", ["ih512_reversed", "ih512_permuted"])
def test_a_long_cluster_in_shuffled_molecule_order_is_one_cluster(name):
    """64 bilayers of hexagonal ice with the molecule order reversed / randomly permuted before upload: labels have to travel
    the length of the box against the molecule order, which an iteration cap would cut short."""
    res = _engine_results()[name]
    k = MASKS.index(0b100)
    rounds = res["last"][k]["rounds"]
    assert np.array_equal(res["summary"][k], [512, 1, 512, 1]), (res["summary"][k], f"{rounds} rounds")
    assert np.all(res["label"][k] == 1), (cr.sizes(res["label"][k]), f"{rounds} rounds")
    assert rounds >= 1, f"{rounds} rounds"
    for j, mask in enumerate(MASKS):
        label_ref, summary_ref = _reference(res, mask)
        assert np.array_equal(res["label"][j], label_ref) and np.array_equal(res["summary"][j], summary_ref), bin(mask)


@pytest.mark.parametrize("name,mask", [("ih4096_t015", 0b100), ("ic48", 0b10), ("gas20", 0b111110)])
def test_golden_boxes(name, mask):
    from mc_water_ls_mw_amd.energy import load_boxes
    z = load_golden(name)
    em = load_boxes([z["h"]], [z["xyz"]])
    try:
        label, summary = em.ice_clusters(1, mask)
        nn, jn, vn = em.neighbours(1)
        cls = em.ice_classes(1)[0]
        label_ref, summary_ref = cr.clusters(cls, z["xyz"], em.ivect(1), nn, jn, vn, RC, mask)
        assert np.array_equal(label, label_ref) and np.array_equal(summary, summary_ref), (summary, summary_ref)
        if name == "gas20":
            assert not label.any() and not summary.any()
        elif name == "ic48":
            assert np.array_equal(summary, [48, 1, 48, 1]) and np.all(label == 1)
        else:
            assert summary[0] == (cls == 2).sum() and summary[2] == cr.sizes(label_ref)[0]
    finally:
        em.energy_deinit()


def _stacking(n, seed):
    """A random cyclic stacking sequence of n bilayers: no two neighbours equal, the last and the first included."""
    rng = np.random.default_rng(seed)
    while True:
        seq = ["ABC"[rng.integers(3)]]
        while len(seq) < n:
            seq.append([c for c in "ABC" if c != seq[-1]][rng.integers(2)])
        if seq[-1] != seq[0]:
            return "".join(seq)


def test_batch_equals_the_single_calls_and_does_not_depend_on_the_range():
    """Different boxes of one N in one context: the defect box and three differently permuted, differently stacked boxes."""
    from mc_water_ls_mw_amd import lattice as lat
    from mc_water_ls_mw_amd.energy import load_boxes
    hd, xd = cr.defect_box()
    nb = len(cr.DEFECT["sequence"])
    rng = np.random.default_rng(12)
    boxes = [(hd, xd)]
    for k in range(3):
        h, x = lat.stacked_ice_box(_stacking(nb, 40 + k), cr.DEFECT["reps_xy"], sigma_ang=0.05, seed=300 + k)
        assert len(x) == len(xd)
        boxes.append((h, np.ascontiguousarray(x[rng.permutation(len(x))])))
    em = load_boxes([b[0] for b in boxes], [b[1] for b in boxes])
    n = len(boxes)
    try:
        for mask in (0b1110, 0b10):
            label, summary = em.ice_clusters_batch(1, n, mask)
            assert label.shape == (n, len(xd)) and summary.shape == (n, 4) and em.ice_clusters_last()["boxes"] == n
            assert len({tuple(s) for s in summary}) > 1                                   # the boxes do differ
            for b in range(n):
                single = em.ice_clusters(b + 1, mask)
                alone = em.ice_clusters_batch(b + 1, 1, mask)
                first = em.ice_clusters_batch(b + 1, n - b, mask)
                last = em.ice_clusters_batch(1, b + 1, mask)
                for lab, summ in (single, (alone[0][0], alone[1][0]), (first[0][0], first[1][0]), (last[0][-1], last[1][-1])):
                    assert np.array_equal(lab, label[b]) and np.array_equal(summ, summary[b]), (b, bin(mask))
                nn, jn, vn = em.neighbours(b + 1)
                ref = cr.clusters(em.ice_classes(b + 1)[0], boxes[b][1], em.ivect(b + 1), nn, jn, vn, RC, mask)
                assert np.array_equal(label[b], ref[0]) and np.array_equal(summary[b], ref[1]), (b, bin(mask))
    finally:
        em.energy_deinit()


def test_the_global_variant_forced_in_a_fresh_process_gives_identical_results(tmp_path):
    out = tmp_path / "global.npz"
    res = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, MW_ICE_CLUSTERS_LDS="0"))
    assert res.returncode == 0, res.stderr[-2000:]
    child = np.load(out)
    mine = _engine_results()
    assert sorted(k[6:] for k in child.files if k.startswith("label:")) == sorted(mine)
    for name, res in mine.items():
        assert np.array_equal(child["label:" + name], res["label"]), name
        assert np.array_equal(child["summary:" + name], res["summary"]), name
        assert not child["lds:" + name].any() and all(v["lds"] for v in res["last"]), name
        assert np.all(child["rounds:" + name] >= 1)


def _thresholds():
    from mc_water_ls_mw_amd.energy import ice_clusters_plan
    return ice_clusters_plan(48)["lds_max_nwater"]


def test_a_box_above_the_lds_limit_takes_the_global_variant_unforced():
    from mc_water_ls_mw_amd.energy import ice_clusters_plan, load_boxes
    z = load_golden("ih32768_t015")
    assert len(z["xyz"]) > _thresholds() and not ice_clusters_plan(len(z["xyz"]))["lds"]
    em = load_boxes([z["h"]], [z["xyz"]])
    try:
        label, summary = em.ice_clusters(1, 0b1110)
        last = em.ice_clusters_last()
        assert not last["lds"] and last["threads"] == 1024 and last["rounds"] >= 1, last
        nn, jn, vn = em.neighbours(1)
        label_ref, summary_ref = cr.clusters(em.ice_classes(1)[0], z["xyz"], em.ivect(1), nn, jn, vn, RC, 0b1110)
        assert np.array_equal(label, label_ref) and np.array_equal(summary, summary_ref), (summary, summary_ref)
    finally:
        em.energy_deinit()


def test_a_box_just_below_the_lds_limit_takes_the_lds_variant():
    """Ih of 14 x 13 x 14 cells, 20384 molecules: the largest such box under the limit of 8 B per molecule."""
    from mc_water_ls_mw_amd import lattice as lat
    from mc_water_ls_mw_amd.energy import ice_clusters_plan, load_boxes
    h, xyz = lat.ice_box("ih", (14, 13, 14), 0.15, seed=7)
    limit = _thresholds()
    assert limit - 64 <= len(xyz) <= limit and ice_clusters_plan(len(xyz))["lds"]
    em = load_boxes([h], [xyz])
    try:
        label, summary = em.ice_clusters(1, 0b1110)
        last = em.ice_clusters_last()
        assert last["lds"] and last["threads"] == 1024, last
        nn, jn, vn = em.neighbours(1)
        label_ref, summary_ref = cr.clusters(em.ice_classes(1)[0], xyz, em.ivect(1), nn, jn, vn, RC, 0b1110)
        assert np.array_equal(label, label_ref) and np.array_equal(summary, summary_ref), (summary, summary_ref)
    finally:
        em.energy_deinit()


def test_bad_arguments_fail_with_a_message_and_leave_the_engine_usable():
    from mc_water_ls_mw_amd.energy import MwError, load_boxes
    h, xyz = _case_boxes()["sd160_thermal"]
    em = load_boxes([h], [xyz])
    try:
        good = em.ice_clusters(1, 0b10)
        for mask in (0, 0b1, 0b1111, 64, 0b1000010, -2):
            with pytest.raises(MwError, match="mask"):
                em.ice_clusters(1, mask)
            with pytest.raises(MwError, match="mask"):
                em.ice_clusters_batch(1, 1, mask)
            with pytest.raises(MwError, match="mask"):
                em.ice_clusters_launch(1, 1, mask)
        with pytest.raises(MwError, match="other"):
            em.ice_clusters(1, 0b111)
        for rc_ang in (0.0, -1.0, 4.31, float("nan")):
            with pytest.raises(MwError, match="r_c"):
                em.ice_clusters(1, 0b10, rc_ang=rc_ang)
            with pytest.raises(MwError, match="r_c"):
                em.ice_clusters_launch(1, 1, 0b10, rc_ang=rc_ang)
        label, summary = np.full(160, -7, dtype=np.int32), np.full(4, -7, dtype=np.int32)
        lp, sp = label.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), summary.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        for ils, count in ((0, 1), (2, 1), (1, 2), (1, 0)):
            assert em.L.mw_ice_clusters_batch(ils, count, ctypes.c_double(RC), 0b10, lp, sp) != 0
            assert b"outside" in em.L.mw_last_error()
        assert em.L.mw_ice_clusters(2, ctypes.c_double(RC), 0b10, lp, sp) != 0 and b"outside" in em.L.mw_last_error()
        assert em.L.mw_ice_clusters_launch(1, 1, ctypes.c_double(RC), 0b10, 4095) != 0 and b"timer" in em.L.mw_last_error()
        assert np.all(label == -7) and np.all(summary == -7)
        again = em.ice_clusters(1, 0b10)
        assert np.array_equal(again[0], good[0]) and np.array_equal(again[1], good[1])
        assert cr.sizes(again[0]) == [64, 32]
    finally:
        em.energy_deinit()


def test_energies_and_classes_are_unchanged_by_a_cluster_call():
    from conftest import DE_ATOL
    from mc_water_ls_mw_amd.energy import load_boxes
    z = load_golden("ih4096_t015")
    em = load_boxes([z["h"]], [z["xyz"]])
    try:
        e = ctypes.c_double(0.0)
        em._chk(em.L.mw_model_energy(1, ctypes.byref(e)))
        e0 = e.value
        imol, trial = z["trial_imol"], z["trial_xyz"]
        eo0, en0 = em.delta_energy_batch(1, imol, trial)
        cls0, counts0 = em.ice_classes(1)
        em.ice_clusters(1)
        eo, en = em.delta_energy_batch(1, imol, trial)
        assert np.array_equal(eo, eo0) and np.array_equal(en, en0)
        em.ice_clusters_batch(1, 1, 0b111110)
        em.ice_clusters_launch(1, 1, timer_slot=0)
        em.sync()
        assert all(em.timer_ms(s) >= 0.0 for s in (0, 1, 2))
        eo2, en2 = em.delta_energy_batch(1, imol, trial)
        assert np.array_equal(eo2, eo0) and np.array_equal(en2, en0)
        assert np.all(np.abs((en - eo) - (z["trial_new"] - z["trial_old"])) <= DE_ATOL)
        em._chk(em.L.mw_model_energy(1, ctypes.byref(e)))
        assert e.value == e0
        cls1, counts1 = em.ice_classes(1)
        assert np.array_equal(cls1, cls0) and np.array_equal(counts1, counts0)
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


def test_a_farm_sweep_is_unchanged_by_largest_ice_clusters():
    def run(clusters):
        em, farm = _npt_farm()
        try:
            farm.sweep(96, seed=41)
            if clusters:
                assert farm.largest_ice_clusters().shape == (farm.nwalkers, 2)
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


def test_npt_farm_largest_clusters_after_device_sweeps():
    """After NPT sweeps with volume moves the device's positions and cells are the authoritative ones: the largest clusters
    must match the reference on the downloaded positions, the synced cells' image vectors and the engine's list."""
    em, farm = _npt_farm()
    try:
        h0 = np.array(em.hmatrix)
        farm.sweep(192, seed=33)
        for classes in (None, ("cubic",), 0b100):
            big = farm.largest_ice_clusters() if classes is None else farm.largest_ice_clusters(classes)
            mask = {None: 0b1110, ("cubic",): 0b10, 0b100: 0b100}[classes]
            assert big.shape == (3, 2)
            cls, _ = em.ice_classes_batch()
            for b in range(em.num_lattices):
                nn, jn, vn = em.neighbours(b + 1)
                ref = cr.clusters(cls[b], farm.positions(b + 1), em.ivect(b + 1), nn, jn, vn, RC, mask)
                assert big[b // 2, b % 2] == ref[1][2], (b, classes, big, ref[1])
        assert not np.array_equal(np.array(em.hmatrix), h0)                 # some volume move was accepted (and synced)
    finally:
        em.energy_deinit()


if __name__ == "__main__":
    results = _engine_results()
    arrays = {}
    for box, r in results.items():
        arrays["label:" + box], arrays["summary:" + box] = r["label"], r["summary"]
        arrays["lds:" + box] = np.array([v["lds"] for v in r["last"]])
        arrays["rounds:" + box] = np.array([v["rounds"] for v in r["last"]])
    np.savez(sys.argv[1], **arrays)
