"""GPU: the per-molecule moments the full-box pass leaves behind (k_model_energy's MOMOUT builds), which a wavefront stores
cooperatively -- the records of 64 molecules re-dealt through the wavefront's queue segment in LDS and written as whole 80-byte
runs (store_moments_wave, mw_full_energy.hip.h).  Every reader of the records is held to the C oracle here, on the shapes where
that store can go wrong: a last group with inactive lanes, a persistent workgroup that stores the moments of several boxes in turn,
the force pass as an independent reader, and the pass mw_moves_launch makes on its own.  Energies to 1e-10 relative, move energy
changes to 1e-10 Ha, counts exact -- the bars of tests/test_gpu_parity.py."""
import numpy as np
import pytest

from conftest import DE_ATOL, RTOL

pytestmark = pytest.mark.gpu


class _Boxes:
    """`nbox` thermal copies of an ice Ih box and what the C oracle makes of each (computed once, never changed)."""

    def __init__(self, c_oracle, reps, nbox, seed):
        from mc_water_ls_mw_amd import lattice as lat
        self.oracle = c_oracle
        self.h, x0 = lat.ice_box("ih", reps)
        self.iv = c_oracle.ivects(self.h)
        self.xs = [lat.thermalise(x0, 0.1, seed + b) for b in range(nbox)]
        self.lists = [c_oracle.neighbours(x, self.iv) for x in self.xs]
        self.n = len(x0)
        full = [c_oracle.model_energy(x, self.iv, *l, counts=True) for x, l in zip(self.xs, self.lists)]
        self.e_full = np.array([e for e, _ in full])
        self.c_full = [(int(c[0]), int(c[1])) for _, c in full]

    def engine(self):
        from mc_water_ls_mw_amd.energy import load_boxes
        return load_boxes([self.h] * len(self.xs), self.xs)

    def moves(self, per_molecule, seed):
        """`per_molecule` trial moves of every molecule of every box: (ils, imol, trial) and the oracle's (e_old, e_new)."""
        rng = np.random.default_rng(seed)
        ils, imol, trial, eo, en = [], [], [], [], []
        for b, (x, l) in enumerate(zip(self.xs, self.lists)):
            i = np.tile(np.arange(1, self.n + 1, dtype=np.int32), per_molecule)
            t = x[i - 1] + rng.normal(0.0, 0.4, (len(i), 3))
            o, n = self.oracle.trial_moves(i, t, x, self.iv, *l)
            ils.append(np.full(len(i), b + 1, dtype=np.int32)); imol.append(i); trial.append(t); eo.append(o); en.append(n)
        return tuple(np.concatenate(a) for a in (ils, imol, trial, eo, en))


@pytest.fixture(scope="module")
def odd_boxes(c_oracle):
    """Ice Ih 4 x 3 x 3 = 288 molecules = 4 groups of 64 + 32 lanes: the smallest ice Ih box whose cells are wide enough for the
    cell-grid builder (3 x 4 x 4 grid cells), so it takes the LDS-staged, no-self-image moment path."""
    return _Boxes(c_oracle, (4, 3, 3), 3, 4100)


def _check_moves(eo, en, ro, rn):
    print("max rel err e_old", np.max(np.abs(eo - ro) / np.abs(ro)), "max |d(dE)|", np.max(np.abs((en - eo) - (rn - ro))))
    assert np.all(np.abs(eo - ro) <= RTOL * np.abs(ro))
    assert np.all(np.abs(en - rn) <= RTOL * np.abs(rn) + 1e-14)
    assert np.all(np.abs((en - eo) - (rn - ro)) <= DE_ATOL)


def _step_and_check(boxes, monkeypatch, seed):
    """One step (full-box pass that also writes the moments, then one trial move of every molecule on the moment path) against
    the oracle: the boxes' energies and counts, every move's old and new energy, the interactions of the unmoved molecules."""
    monkeypatch.setenv("MW_MOVE_MOMENTS", "1")
    nbox = len(boxes.xs)
    ils, imol, trial, ro, rn = boxes.moves(1, seed)
    em = boxes.engine()
    try:
        em.moves_upload(ils, imol, trial)
        em.step_launch(1, nbox)
        e = em.model_energy_fetch(1, nbox)
        eo, en = em.moves_fetch()
        de, dm = em.last_dispatch("energy"), em.last_dispatch("moves")
        assert de["lds"] == 1 and de["moments"] == 1 and de["nsplit"] == 1 and de["boxes"] == nbox
        assert dm["mlds"] == 1 and dm["noself"] == 1 and dm["use_mom"] == 1 and dm["fresh"] == 1 and dm["build"] == 3
        print("max rel err E", np.max(np.abs(e - boxes.e_full) / np.abs(boxes.e_full)))
        assert np.all(np.abs(e - boxes.e_full) <= RTOL * np.abs(boxes.e_full))
        assert [em.model_energy_counts(b + 1) for b in range(nbox)] == boxes.c_full
        _check_moves(eo, en, ro, rn)
        # unmoved molecules of the first box: old = new, the interactions of both sides counted exactly
        x, l = boxes.xs[0], boxes.lists[0]
        every = np.arange(1, boxes.n + 1, dtype=np.int32)
        ref_i = sum(int(boxes.oracle.local_energy(int(i), x, boxes.iv, *l, counts=True)[1].sum()) for i in every)
        em.moves_upload(1, every, x)
        em.step_launch(1, nbox)
        eo1, en1 = em.moves_fetch()
        assert em.last_dispatch("moves")["use_mom"] == 1
        c = em.moves_counts()
        assert c[0] == ref_i and c[2] == ref_i
        assert np.all(np.abs(eo1 - ro[:boxes.n]) <= RTOL * np.abs(ro[:boxes.n])) and np.all(np.abs(en1 - eo1) <= DE_ATOL)
        return de
    finally:
        em.energy_deinit()


def test_partial_last_group_writes_the_active_lanes_only(odd_boxes, monkeypatch):
    """288 molecules: the last group of a box has 32 inactive lanes, whose records must not be stored -- and the 32 active ones must.
    One trial move of every molecule consumes every record."""
    assert odd_boxes.n == 288 and odd_boxes.n % 64 == 32
    _step_and_check(odd_boxes, monkeypatch, 11)


def test_persistent_workgroups_store_the_moments_of_several_boxes(c_oracle, monkeypatch):
    """300 boxes of 512 molecules (ice Ih 4 x 4 x 4: whole groups only) in one launch -- more boxes than compute units, so a
    persistent workgroup stores the moments of two boxes in turn through the same staging area."""
    boxes = _Boxes(c_oracle, (4, 4, 4), 300, 5200)
    assert boxes.n == 512
    de = _step_and_check(boxes, monkeypatch, 12)
    assert de["grid_y"] < de["boxes"]


def test_forces_read_the_same_records(odd_boxes):
    """mw_model_forces* makes the moments with the same full-box pass and reads them with a kernel of its own."""
    from forces_ref import model_forces
    em = odd_boxes.engine()
    try:
        e, f, w = em.forces_batch()
        for b, x in enumerate(odd_boxes.xs):
            e_ref, f_ref, w_ref = model_forces(x, em.ivect(b + 1), *em.neighbours(b + 1))
            assert abs(e[b] - odd_boxes.e_full[b]) <= RTOL * abs(odd_boxes.e_full[b]) and abs(e[b] - e_ref) <= RTOL * abs(e_ref)
            # per component 1e-10 relative with a floor of 1e-10 max|F| (tests/test_gpu_forces.py)
            fmax, wmax = np.abs(f_ref).max(), np.abs(w_ref).max()
            print("box", b, "max |dF| / max|F|", np.abs(f[b] - f_ref).max() / fmax, "max |dW| / max|W|", np.abs(w[b] - w_ref).max() / wmax)
            assert np.all(np.abs(f[b] - f_ref) <= 1e-10 * np.maximum(np.abs(f_ref), fmax) + 1e-14)
            assert np.all(np.abs(w[b] - w_ref) <= 1e-10 * np.maximum(np.abs(w_ref), wmax))
    finally:
        em.energy_deinit()


def test_moments_made_by_the_move_launch_itself(odd_boxes):
    """No step before the launch and 1440 requests per box (>= 1280): mw_moves_launch makes the moments with a full-box pass of
    its own, one that leaves the boxes' energies alone."""
    ils, imol, trial, ro, rn = odd_boxes.moves(5, 13)
    em = odd_boxes.engine()
    try:
        e0 = em.model_energy_fetch(1, len(odd_boxes.xs))
        eo, en = em.delta_energy_batch(ils, imol, trial)
        dm, de = em.last_dispatch("moves"), em.last_dispatch("energy")
        assert dm["use_mom"] == 1 and dm["fresh"] == 0 and dm["build"] == 3 and de["moments"] == 1
        _check_moves(eo, en, ro, rn)
        assert np.array_equal(em.model_energy_fetch(1, len(odd_boxes.xs)), e0)
    finally:
        em.energy_deinit()
