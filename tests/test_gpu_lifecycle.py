"""GPU: what the context keeps across mw_finalize, and the last event-timer slots of the timed launches.

The context's device buffers are allocated through one helper that records them (release_all frees whatever exists), and the
kernels whose dynamic LDS limit is raised on first use have one flag each in the context.  Both are state that a finalize has
to reset: a stale capacity, pointer or flag left behind would show as a fault, a failed launch or different numbers in a later
context of another shape.  The life-cycle test runs every lazily allocating path in a context of 96 molecules x 2 boxes, then in
one of 48 molecules x 3 boxes, then in the first again, and holds the third run to the first bit for bit.

Run as a script (`python tests/test_gpu_lifecycle.py OUT.npz`) it runs the three cycles and saves their results: the test does
that in a fresh child process, because MW_ICE_CLUSTERS_LDS is read at mw_init."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RDF_RMAX_ANG = 6.0          # within 1.5 x the smallest cell width of both boxes (the 48-molecule cell is 7.28 A thick)


def _boxes(which):
    from mc_water_ls_mw_amd import lattice as lat
    if which == "A":        # the smoke box: Ih (3, 2, 2), 96 molecules, twice
        return [lat.ice_box("ih", (3, 2, 2), 0.15, seed=11 + k) for k in range(2)]
    return [lat.ice_box("ih", (3, 2, 1), 0.15, seed=21 + k) for k in range(3)]      # 48 molecules, three boxes


def _cycle(which):
    """Every lazily allocating path once, in two contexts: the second has MW_ICE_CLUSTERS_LDS=0 and runs the cluster pass's
    global variant.  Returns {name: array}."""
    from mc_water_ls_mw_amd import lattice as lat
    from mc_water_ls_mw_amd.energy import load_boxes
    boxes = _boxes(which)
    n = len(boxes)
    out = {}
    os.environ.pop("MW_ICE_CLUSTERS_LDS", None)
    em = load_boxes([b[0] for b in boxes], [b[1] for b in boxes])
    try:
        out["e"], out["f"], out["w"] = em.forces_batch(1, n)
        out["cls"], out["cls_counts"] = em.ice_classes_batch(1, n)
        out["bonds"] = em.ice_bonds(n)
        out["label"], out["summary"] = em.ice_clusters_batch(1, n)
        assert em.ice_clusters_last()["lds"]
        out["rdf50"] = em.rdf_counts_batch(1, n, RDF_RMAX_ANG, 50)
        out["rdf200"] = em.rdf_counts_batch(1, n, RDF_RMAX_ANG, 200)          # the histogram regrows
        assert out["rdf50"].sum() == out["rdf200"].sum() > 0
        imol, trial = lat.trial_moves(boxes[0][1], 256, seed=4)
        out["e_old"], out["e_new"] = em.delta_energy_batch(1, imol, trial)
        zero = ctypes.c_double(0.0)
        for _ in range(2):                                                      # the second call replaces the first one's tables
            em._chk(em.L.mw_sweep_configure(1, ctypes.c_double(1.0), ctypes.c_double(0.5), 0, 0, 0, 0, zero, zero, zero, zero,
                                            zero, zero, None, None, None))
        ls, mu, acc = ctypes.c_int(0), ctypes.c_double(-1.0), ctypes.c_longlong(-1)
        e2 = (ctypes.c_double * 2)()
        em._chk(em.L.mw_sweep_get_state(n, ctypes.byref(ls), ctypes.byref(mu), e2, ctypes.byref(acc)))
        out["walker"] = np.array([ls.value, mu.value, acc.value, e2[0]])
    finally:
        em.energy_deinit()
    os.environ["MW_ICE_CLUSTERS_LDS"] = "0"
    try:
        em = load_boxes([b[0] for b in boxes], [b[1] for b in boxes])
        try:
            out["label_global"], out["summary_global"] = em.ice_clusters_batch(1, n)
            assert not em.ice_clusters_last()["lds"]
        finally:
            em.energy_deinit()
    finally:
        os.environ.pop("MW_ICE_CLUSTERS_LDS", None)
    return out


def _main(path):
    saved = {}
    for k, which in enumerate("ABA"):
        for name, a in _cycle(which).items():
            saved[f"{k}:{name}"] = a
    np.savez(path, **saved)


def test_a_context_after_finalize_repeats_the_first_one_bit_for_bit(tmp_path):
    out = tmp_path / "cycles.npz"
    env = {k: v for k, v in os.environ.items() if k != "MW_ICE_CLUSTERS_LDS"}
    res = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-3000:])
    z = np.load(out)
    names = sorted(k[2:] for k in z.files if k.startswith("0:"))
    assert len(names) == 15 and sorted(k[2:] for k in z.files if k.startswith("2:")) == names
    for name in names:
        first, third = z["0:" + name], z["2:" + name]
        assert first.dtype == third.dtype and first.shape == third.shape, name
        assert first.tobytes() == third.tobytes(), name                       # bit for bit (NaN bonds included)
    assert z["0:f"].shape == (2, 96, 3) and z["1:f"].shape == (3, 48, 3)
    assert np.array_equal(z["0:label"], z["0:label_global"]) and np.array_equal(z["1:summary"], z["1:summary_global"])
    assert np.abs(z["0:f"]).max() > 0 and z["0:cls_counts"].sum() == 2 * 96 and z["1:cls_counts"].sum() == 3 * 48


#: entry point -> (timer slots it takes, the dispatch family its launch records)
TIMED = {"mw_model_forces_launch": (2, "forces"), "mw_ice_classes_launch": (2, "ice"),
         "mw_ice_clusters_launch": (3, "ice"), "mw_rdf_launch": (1, "rdf")}


@pytest.mark.parametrize("entry", sorted(TIMED))
def test_the_last_timer_slots_are_admitted_and_the_next_one_refused(entry):
    from mc_water_ls_mw_amd.energy import _rc, load_boxes
    boxes = _boxes("A")
    em = load_boxes([b[0] for b in boxes], [b[1] for b in boxes])
    nslots, family = TIMED[entry]
    last = 4096 - nslots
    assert last == {"mw_model_forces_launch": 4094, "mw_ice_classes_launch": 4094, "mw_ice_clusters_launch": 4093,
                    "mw_rdf_launch": 4095}[entry]

    def call(slot, count, nbins=50, mask=0b110):
        if entry == "mw_model_forces_launch":
            return em.L.mw_model_forces_launch(1, count, slot)
        if entry == "mw_ice_classes_launch":
            return em.L.mw_ice_classes_launch(1, count, _rc(3.5), slot)
        if entry == "mw_ice_clusters_launch":
            return em.L.mw_ice_clusters_launch(1, count, _rc(3.5), mask, slot)
        return em.L.mw_rdf_launch(1, count, _rc(RDF_RMAX_ANG), nbins, slot)

    def state():
        s = [em.last_dispatch(family)]
        if entry == "mw_ice_clusters_launch":
            s.append(em.ice_clusters_last())
        return s
    try:
        assert call(last, 2) == 0, em.L.mw_last_error()
        em.sync()
        for slot in range(last, last + nslots):
            ms = em.timer_ms(slot)
            assert math.isfinite(ms) and ms >= 0.0, (slot, ms)
        before = state()
        # (other arguments than the admitted call's: a launch behind a late slot check would rewrite the records)
        assert call(last + 1, 1, nbins=200, mask=0b100) != 0
        msg = em.L.mw_last_error().decode()
        assert "timer" in msg and entry in msg and str(last + 1) in msg and f"0..{last}" in msg, msg
        assert state() == before and before[0]["boxes"] == 2
    finally:
        em.energy_deinit()


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _main(sys.argv[1])
