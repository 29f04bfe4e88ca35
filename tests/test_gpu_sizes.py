"""GPU: every kernel family on both sides of its LDS thresholds.

Each hot kernel has a build that stages the box in LDS and one that gathers positions through L2; the host picks one by box
size (mw_lds_plan gives the rules: the full-box energy, forces, ice pass 1 and the whole-box list order share one limit, the
move kernel has a lower one, the fused list sort a fixed cap).  Here boxes sit AT each limit and one molecule past it -- a
thermal Ic or Ih lattice with random vacancies, so N is no multiple of 64 -- and every result is held to the C oracle and the
numpy references at the suite's bars: image vectors and lists exact, counts exact, energies 1e-10 relative, move energy
changes 1e-10 Ha.  mw_last_dispatch says which build each launch took, so a threshold that moves makes these tests fail
instead of testing the same side twice."""
import numpy as np
import pytest

from conftest import DE_ATOL, RTOL, list_digest
from forces_ref import model_forces
from ice_ref import ANG_TO_BOHR, RC_ANG, ice_classes

pytestmark = pytest.mark.gpu

RC = RC_ANG * ANG_TO_BOHR


def _limit(build, ivcap=32):
    """Largest N at which LDS build `build` is admitted (the engine's own rule, mw_lds_plan)."""
    from mc_water_ls_mw_amd.energy import lds_plan
    lo, hi = 1, 1 << 16
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if lds_plan(mid, ivcap)[build][0] else (lo, mid)
    return lo


E32, M32, S32, E48 = _limit("energy"), _limit("move"), _limit("sort"), _limit("energy", 48)
#: N at each limit and one past it, plus one odd size between 4096 and the move kernel's limit
SIZES = sorted({(4096 + M32) // 2 | 1, M32, M32 + 1, E32, E32 + 1, S32, S32 + 1})


def _box(n, seed):
    """A thermal Ic (odd seeds) or Ih lattice of more than n molecules with random vacancies down to exactly n."""
    from mc_water_ls_mw_amd import lattice as lat
    h, x = lat.ice_box("ic", (9, 9, 9)) if seed % 2 else lat.ice_box("ih", (8, 8, 11))
    x = lat.thermalise(x, 0.1, 1000 + seed)
    keep = np.sort(np.random.default_rng(seed).choice(len(x), n, replace=False))
    return h, np.ascontiguousarray(x[keep])


_REF = {}


def _ref(key, h, x, c_oracle):
    """Oracle image vectors, list, energy and counts, local energies of one box (built once per module run)."""
    if key not in _REF:
        iv = c_oracle.ivects(h)
        nn, jn, vn = c_oracle.neighbours(x, iv)
        e, counts = c_oracle.model_energy(x, iv, nn, jn, vn, counts=True)
        _REF[key] = dict(iv=iv, lists=(nn, jn, vn), e=e, counts=(int(counts[0]), int(counts[1])),
                         local=c_oracle.local_energy_all(x, iv, nn, jn, vn))
    return _REF[key]


def _load(h_list, x_list, monkeypatch, **env):
    """load_boxes with the engine's init-time switches set as given (and every other one unset)."""
    from mc_water_ls_mw_amd.energy import load_boxes
    for k in ("MW_MOVE_MOMENTS", "MW_MODEL_PERSIST", "MW_MOVE_CHUNK", "MW_FORCE_BRUTE_NEIGHBOURS", "MW_CELL_SORT", "MW_ORDER_SEG"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    em = load_boxes(h_list, x_list)
    for k in env:
        monkeypatch.delenv(k)
    return em


def _check_moves(em, ils, x, ref, imol, trial, c_oracle, chunk, monkeypatch):
    """delta_energy_batch against c_oracle.trial_moves; returns what the move launch did."""
    if chunk:
        monkeypatch.setenv("MW_MOVE_CHUNK", str(chunk))
    eo, en = em.delta_energy_batch(ils, imol, trial)
    monkeypatch.delenv("MW_MOVE_CHUNK", raising=False)
    d = em.last_dispatch("moves")
    ro, rn = c_oracle.trial_moves(imol, trial, x, ref["iv"], *ref["lists"])
    assert np.all(np.abs(eo - ro) <= RTOL * np.abs(ro)), np.abs(eo - ro).max()
    assert np.all(np.abs(en - rn) <= RTOL * np.abs(rn)), np.abs(en - rn).max()
    assert np.all(np.abs((en - eo) - (rn - ro)) <= DE_ATOL)
    return d


def _check_box(em, ils, h, x, ref):
    """Image vectors, list, counts, full-box and every local energy, forces and virial, ice classes and bonds of box ils."""
    n = len(x)
    assert np.array_equal(em.ivect(ils), ref["iv"])
    nn, jn, vn = em.neighbours(ils)
    assert np.array_equal(nn, ref["lists"][0])
    assert list_digest(nn, jn, vn) == list_digest(*ref["lists"])
    e = em.model_energy_batch(ils, 1)[0]
    assert abs(e - ref["e"]) <= RTOL * abs(ref["e"])
    assert em.model_energy_counts(ils) == ref["counts"]
    energy = em.last_dispatch("energy")
    loc = em.local_energy_batch(ils, np.arange(1, n + 1))
    assert np.all(np.abs(loc - ref["local"]) <= RTOL * np.abs(ref["local"])), np.abs(loc - ref["local"]).max()
    ef, f, w = em.compute_forces(ils)
    forces = em.last_dispatch("forces")
    e_ref, f_ref, w_ref = model_forces(x, ref["iv"], *ref["lists"])
    assert abs(ef - e_ref) <= RTOL * abs(e_ref)
    fmax, wmax = np.abs(f_ref).max(), np.abs(w_ref).max()
    assert np.all(np.abs(f - f_ref) <= 1e-10 * np.maximum(np.abs(f_ref), fmax) + 1e-14)
    assert np.all(np.abs(w - w_ref) <= 1e-10 * np.maximum(np.abs(w_ref), wmax))
    cls, counts = em.ice_classes(ils)
    ice = em.last_dispatch("ice")
    c = em.ice_bonds(ils)
    cls_ref, c_ref, counts_ref = ice_classes(x, ref["iv"], *ref["lists"], RC)
    assert np.array_equal(cls, cls_ref) and np.array_equal(counts, counts_ref)
    assert np.array_equal(c == 2.0, c_ref == 2.0) and np.array_equal(np.isnan(c), np.isnan(c_ref))
    live = (c_ref != 2.0) & ~np.isnan(c_ref)
    assert np.all(np.abs(c[live] - c_ref[live]) <= 1e-12)
    return energy, forces, ice


def test_threshold_sizes_are_the_pinned_ones():
    """The sizes below come from mw_lds_plan; tests/test_code_object.py pins the same limits on the CPU."""
    assert (E32, M32, S32, E48) == (4490, 4372, 5120, 4474)


@pytest.mark.parametrize("n", SIZES)
def test_box_on_each_side_of_the_thresholds(n, c_oracle, monkeypatch):
    from mc_water_ls_mw_amd import lattice as lat
    from mc_water_ls_mw_amd.energy import lds_plan
    h, x = _box(n, n)
    ref = _ref(n, h, x, c_oracle)
    plan = lds_plan(n, 32)
    em = _load([h], [x], monkeypatch)
    try:
        build = em.last_dispatch("build")
        assert build["ivcap"] == 32 and build["grid_boxes"] == 1 and build["brute_boxes"] == 0
        assert build["fused_sort"] == (n <= S32) and not build["legacy_search"]
        assert build["order_seg"] == ((n + 63) & ~63 if n <= E32 else 64)
        energy, forces, ice = _check_box(em, 1, h, x, ref)
        assert energy["lds"] == forces["lds"] == ice["lds"] == (n <= E32)
        if n <= E32:
            assert energy["lds_bytes"] == plan["energy"][1]
        assert forces["nsplit"] == (1 if n <= E32 else (n + 255) // 256)
        # trial moves: many requests in items of the largest size (the most dynamic LDS the budget allows), then a handful
        imol, trial = lat.trial_moves(x, 4096, seed=n)
        d = _check_moves(em, 1, x, ref, imol, trial, c_oracle, 2048, monkeypatch)
        assert d["mlds"] == (n <= M32) and d["noself"] == 1
        if n <= M32:
            assert d["mchunk"] == 2048 and d["items"] == 2 and d["lds_bytes"] == plan["move"][1]
            assert d["build"] == 3                        # 4096 requests per box: the moment path by the count rule
        else:
            assert d["build"] == 0
        few = _check_moves(em, 1, x, ref, imol[:5], trial[:5], c_oracle, None, monkeypatch)
        assert few["build"] == 0 and few["mlds"] == 0
        # the step of the bench (full-box pass + moves in one call): the moments of the pass go to the move kernel where admitted
        em.moves_upload(np.ones(len(imol), dtype=np.int32), imol, trial)
        em.step_launch(1, 1)
        eo, en = em.moves_fetch()
        e = em.model_energy_fetch(1, 1)[0]
        step = em.last_dispatch("moves")
        ro, rn = c_oracle.trial_moves(imol, trial, x, ref["iv"], *ref["lists"])
        assert abs(e - ref["e"]) <= RTOL * abs(ref["e"])
        assert np.all(np.abs((en - eo) - (rn - ro)) <= DE_ATOL) and np.all(np.abs(eo - ro) <= RTOL * np.abs(ro))
        assert step["use_mom"] == step["fresh"] == (n <= M32)
        print(f"\nN={n}: build {build}\n  energy {energy}\n  forces {forces}\n  ice {ice}\n  moves {d}\n  few moves {few}\n  step {step}")
    finally:
        em.energy_deinit()
    if n > M32:
        return
    # the two overrides of the move kernel's path, on requests the count rule would serve the other way
    em = _load([h], [x], monkeypatch, MW_MOVE_MOMENTS="0")
    try:
        d = _check_moves(em, 1, x, ref, imol, trial, c_oracle, 2048, monkeypatch)
        assert d["build"] == 2 and d["use_mom"] == 0 and d["mlds"] == 1
    finally:
        em.energy_deinit()
    em = _load([h], [x], monkeypatch, MW_MOVE_MOMENTS="1")
    try:
        d = _check_moves(em, 1, x, ref, imol[:600], trial[:600], c_oracle, None, monkeypatch)
        assert d["build"] == 3 and d["use_mom"] == 1 and d["fresh"] == 0
    finally:
        em.energy_deinit()


@pytest.mark.parametrize("n", [E48, E48 + 1])
def test_npt_farm_at_48_image_vectors(n, c_oracle, monkeypatch):
    """A farm with volume moves keeps room for 48 image vectors per box: every limit moves down (mw_sweep_moves)."""
    from mc_water_ls_mw_amd import lattice as lat
    from mc_water_ls_mw_amd.sweep import WalkerFarm
    h, x = _box(n, n)
    ref = _ref(n, h, x, c_oracle)
    em = _load([h], [x], monkeypatch)
    try:
        WalkerFarm(em, 1, 200.0).moves(trans_prob=0.5, vol_prob=0.1)
        em.build_neighbours_batch(1, 1)
        assert em.last_dispatch("build")["ivcap"] == 48
        energy, forces, ice = _check_box(em, 1, h, x, ref)
        assert energy["ivcap"] == forces["ivcap"] == ice["ivcap"] == 48
        assert energy["lds"] == forces["lds"] == ice["lds"] == (n <= E48)
        imol, trial = lat.trial_moves(x, 1024, seed=n)
        d = _check_moves(em, 1, x, ref, imol, trial, c_oracle, None, monkeypatch)
        assert d["ivcap"] == 48 and d["build"] == 0
        print(f"\nN={n} ivcap 48: energy {energy} forces {forces} ice {ice} moves {d}")
    finally:
        em.energy_deinit()


def test_thin_slab_with_self_images(c_oracle, monkeypatch):
    """A compressed Ih slab one cell thick (|h1| < the cutoff): 45 image vectors, so the table grows past 32 and every limit
    moves down; no cell grid (brute-force list builder), and molecules meet images of themselves (the move kernel's SELFIMG
    build).  N sits at the move kernel's limit for that capacity."""
    from mc_water_ls_mw_amd import lattice as lat
    from mc_water_ls_mw_amd.energy import lds_plan
    h, x = lat.ice_ih_cell(2.6)
    h, x = lat.replicate(h, x, (1, 22, 25))
    iv = c_oracle.ivects(h)
    assert len(iv) == 45
    ivcap = 48
    n = _limit("move", ivcap)
    x = lat.thermalise(x, 0.08, 5)
    x = np.ascontiguousarray(x[np.sort(np.random.default_rng(5).choice(len(x), n, replace=False))])
    ref = _ref("slab", h, x, c_oracle)
    em = _load([h], [x], monkeypatch)
    try:
        build = em.last_dispatch("build")
        assert build["ivcap"] == ivcap and build["brute_boxes"] == 1 and build["grid_boxes"] == 0
        energy, forces, ice = _check_box(em, 1, h, x, ref)
        assert energy["lds"] == forces["lds"] == ice["lds"] == 1 and energy["ivcap"] == ivcap
        imol, trial = lat.trial_moves(x, 4096, seed=6)
        d = _check_moves(em, 1, x, ref, imol, trial, c_oracle, 2048, monkeypatch)
        assert d["build"] == 1 and d["noself"] == 0 and d["lds_bytes"] == lds_plan(n, ivcap)["move"][1]
        d5 = _check_moves(em, 1, x, ref, imol[:5], trial[:5], c_oracle, None, monkeypatch)
        assert d5["build"] == 0
        print(f"\nslab N={n}: build {build}\n  energy {energy}\n  moves {d}")
    finally:
        em.energy_deinit()


def test_split_and_persistent_geometries_at_the_energy_limit(c_oracle, monkeypatch):
    """N at the full-box kernel's LDS limit over 1, 150, 200, 300 and 520 boxes: 5, 4, 3, 2 and 1 workgroups per box, each with
    a shorter last chunk, and persistent workgroups at 520.  Every box equals its single-box launch, a sample equals the
    oracle, and one workgroup per box (MW_MODEL_PERSIST=0) gives the same bits."""
    from mc_water_ls_mw_amd import lattice as lat
    n, nb = E32, 520
    h, x0 = _box(n, 7)
    xs = [lat.thermalise(x0, 0.05, 3000 + w) for w in range(nb)]
    em = _load([h] * nb, xs, monkeypatch)
    try:
        _, cu, _ = em.device_info()
        assert cu == 256
        single = np.array([em.model_energy_batch(w + 1, 1)[0] for w in range(nb)])
        assert em.last_dispatch("energy")["nsplit"] == 5
        sample = (0, 149, 199, 299, 519)
        refs = {w: _ref(("multi", w), h, xs[w], c_oracle) for w in sample}
        for w in sample:
            assert list_digest(*em.neighbours(w + 1)) == list_digest(*refs[w]["lists"])
        want = {1: (5, 650), 150: (4, 1034), 200: (3, 1418), 300: (2, 2186), 520: (1, n)}
        for count, (nsplit, last) in want.items():
            e = em.model_energy_batch(1, count)
            d = em.last_dispatch("energy")
            assert d["lds"] == 1 and d["nsplit"] == nsplit and n - (nsplit - 1) * d["chunk"] == last, (count, d)
            assert d["grid_y"] == (cu if nsplit == 1 and count > cu else count)      # persistent workgroups: unsplit boxes only
            assert np.all(np.abs(e - single[:count]) <= 1e-13 * np.abs(single[:count]))
            for w in sample:
                if w < count:
                    assert abs(e[w] - refs[w]["e"]) <= RTOL * abs(refs[w]["e"])
                    assert em.model_energy_counts(w + 1) == refs[w]["counts"]
            print(f"\n{count} boxes: {d}")
        e_persist = em.model_energy_batch(1, nb).copy()
        c_persist = [em.model_energy_counts(w + 1) for w in range(nb)]
    finally:
        em.energy_deinit()
    em = _load([h] * nb, xs, monkeypatch, MW_MODEL_PERSIST="0")
    try:
        e = em.model_energy_batch(1, nb)
        assert em.last_dispatch("energy")["grid_y"] == nb
        assert np.array_equal(e, e_persist)
        assert [em.model_energy_counts(w + 1) for w in range(nb)] == c_persist
    finally:
        em.energy_deinit()


def test_driver_past_the_energy_limit(c_oracle, monkeypatch):
    """The translation driver at N = energy limit + 1: one lattice, two walkers, translations only -- walkers in global memory
    without the moment path -- move for move against the oracle's restatement."""
    from mc_water_ls_mw_amd import lattice as lat
    from mc_water_ls_mw_amd.sweep import WalkerFarm
    from oracle import SweepOracle
    from test_sweep import _compare
    n = E32 + 1
    h, x = _box(n, n)
    xs = [x, lat.thermalise(x, 0.03, 41)]
    refs = [_ref(n, h, xs[0], c_oracle), _ref(("driver", n), h, xs[1], c_oracle)]
    em = _load([h, h], xs, monkeypatch)
    so = SweepOracle()
    try:
        farm = WalkerFarm(em, 1, 220.0, 1.1)
        for w in (1, 2):
            farm.set_state(w, 1, 0.0)
        log = farm.sweep(200, seed=31, move0=0, log=True)
        what = farm.last_launch()
        assert what["residency"] == 0 and em.last_dispatch("energy")["lds"] == 0
        for w in range(2):
            ref = so.sweep(200, 31, w, 0, [h], [xs[w]], farm.beta, farm.max_trans, lists=[refs[w]["lists"]],
                           model_energy=[em.model_energy[w]])
            _compare(log[w], ref, farm.state(w + 1), [farm.positions(w + 1)])
        print(f"\ndriver N={n}: {what}")
    finally:
        em.energy_deinit()
