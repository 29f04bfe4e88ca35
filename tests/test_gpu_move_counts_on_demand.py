"""GPU: the move kernel's moment path counts ON DEMAND (mw_moves_counts, include/mw_energy.h).  The launch computes energies only;
the first mw_moves_counts after it runs the same kernel once more over the same work items (mode bits 3 "count" and 4 "no energy
output") and later calls launch nothing; MW_MOVE_COUNTS=eager counts inside the launch as before.  Held to the C oracle on two
288-molecule ice Ih boxes (the smallest the moment path takes) with 600 requests each in work items of 256 (MW_MOVE_CHUNK), so a
box has several items: counts exact (tests/move_counts_ref.py), energies 1e-10 relative, and bit-identical between the ways of
asking."""
import numpy as np
import pytest

from conftest import DE_ATOL, RTOL
from move_counts_ref import request_counts
from test_gpu_moment_store import _Boxes

pytestmark = pytest.mark.gpu

NREQ = 600            # per box: three work items of 200 with MW_MOVE_CHUNK=256


class _Case:
    """Two boxes, their requests and what the oracle makes of them (computed once, never changed)."""

    def __init__(self, oracle, xs=None, first=(), seed=31):
        self.boxes = _Boxes(oracle, (4, 3, 3), 2, 6100)
        if xs is not None:
            self.boxes.xs = xs
            self.boxes.lists = [oracle.neighbours(x, self.boxes.iv) for x in xs]
        b, rng = self.boxes, np.random.default_rng(seed)
        ils, imol, trial, ref, eo, en = [], [], [], [], [], []
        for k, (x, l) in enumerate(zip(b.xs, b.lists)):
            i = rng.integers(1, b.n + 1, NREQ).astype(np.int32)
            t = x[i - 1] + rng.normal(0.0, 0.4, (NREQ, 3))
            if k == 0 and len(first):
                i[:len(first)] = first
                t[:len(first)] = x[i[:len(first)] - 1]                      # (unmoved: old == new)
            o, n = oracle.trial_moves(i, t, x, b.iv, *l)
            ils.append(np.full(NREQ, k + 1, dtype=np.int32)); imol.append(i); trial.append(t); eo.append(o); en.append(n)
            ref.append(request_counts(oracle, x, b.iv, *l, i, t)[0])
        self.ils, self.imol, self.trial, self.eo, self.en = (np.concatenate(a) for a in (ils, imol, trial, eo, en))
        self.ref = np.concatenate(ref)
        self.totals = tuple(int(v) for v in self.ref.sum(axis=0))

    def engine(self, monkeypatch, counts=None):
        monkeypatch.setenv("MW_MOVE_MOMENTS", "1")
        monkeypatch.setenv("MW_MOVE_CHUNK", "256")
        if counts is None:
            monkeypatch.delenv("MW_MOVE_COUNTS", raising=False)
        else:
            monkeypatch.setenv("MW_MOVE_COUNTS", counts)
        return self.boxes.engine()

    def check_energies(self, eo, en):
        print("max rel err e_old", np.max(np.abs(eo - self.eo) / np.abs(self.eo)), "max |d(dE)|", np.max(np.abs((en - eo) - (self.en - self.eo))))
        assert np.all(np.abs(eo - self.eo) <= RTOL * np.abs(self.eo)) and np.all(np.abs(en - self.en) <= RTOL * np.abs(self.en) + 1e-14)
        assert np.all(np.abs((en - eo) - (self.en - self.eo)) <= DE_ATOL)


@pytest.fixture(scope="module")
def case(c_oracle):
    return _Case(c_oracle)


def _on_moment_path(em, items_at_least=4):
    d = em.last_dispatch("moves")
    assert d["use_mom"] == 1 and d["build"] == 3 and d["mchunk"] == 256 and d["items"] >= items_at_least
    return d


def test_counts_after_a_step_and_after_a_move_launch_alone(case, monkeypatch):
    em = case.engine(monkeypatch)
    try:
        em.moves_upload(case.ils, case.imol, case.trial)
        for launch in (lambda: em.step_launch(1, 2), em.moves_launch):
            launch()
            d = _on_moment_path(em)
            assert d["counts"] == 1                                         # pending: the launch did not count
            c = em.moves_counts()
            print("counts", c, "oracle", case.totals)
            assert c == case.totals
            d1 = em.last_dispatch("moves")
            assert d1["counts"] == 0 and d1["count_passes"] == d["count_passes"] + 1 and d1["declined"] == 0
            assert em.moves_counts() == case.totals                         # a second call: the same values, no launch
            assert em.last_dispatch("moves")["count_passes"] == d1["count_passes"]
            case.check_energies(*em.moves_fetch())
    finally:
        em.energy_deinit()


def test_energies_do_not_depend_on_when_or_whether_the_counts_are_made(case, monkeypatch):
    got = {}
    for how in (None, "eager"):
        em = case.engine(monkeypatch, how)
        try:
            em.moves_upload(case.ils, case.imol, case.trial)
            em.step_launch(1, 2)
            d = _on_moment_path(em)
            assert d["counts"] == (0 if how else 1)
            before = em.moves_fetch()
            counts = em.moves_counts()
            assert em.last_dispatch("moves")["count_passes"] == (0 if how else 1)
            after = em.moves_fetch()
            got[how] = (before, after, counts)
        finally:
            em.energy_deinit()
    case.check_energies(*got[None][0])
    for k in (0, 1):
        assert np.array_equal(got[None][0][k], got[None][1][k])             # fetched before and after asking for the counts
        assert np.array_equal(got[None][0][k], got["eager"][0][k]) and np.array_equal(got[None][0][k], got["eager"][1][k])
    assert got[None][2] == got["eager"][2] == case.totals


def test_declined_requests_are_counted_by_the_fallback_alone(c_oracle, monkeypatch):
    """One molecule pushed almost behind a neighbour's neighbour (the construction of tests/test_gpu_parity.py's
    test_moment_path_of_the_move_kernel_and_the_triplets_it_must_decline): the requests that meet a triplet with cos(theta) >= 0.99
    are declined to k_move_fallback, which counts them at the launch; the count pass adds the served ones and neither counts the
    declined ones again nor appends them to the list a second time."""
    base = _Boxes(c_oracle, (4, 3, 3), 2, 6100)
    x = base.xs[0].copy()
    nn, jn, vn = base.lists[0]
    a = 100
    dab, b = min((np.linalg.norm(x[jn[a, s] - 1] - x[a]), jn[a, s] - 1) for s in range(nn[a]) if vn[a, s] == 1)
    c = next(k for k in range(len(x)) if k not in (a, b) and np.linalg.norm(x[k] - x[a]) > 15.0)
    x[c] = x[a] + 1.45 * (x[b] - x[a]) + np.array([0.02, -0.01, 0.015])
    case = _Case(c_oracle, xs=[x, base.xs[1]], first=[a + 1, b + 1, c + 1] * 3, seed=32)
    em = case.engine(monkeypatch)
    try:
        em.moves_upload(case.ils, case.imol, case.trial)
        runs = []
        for _ in range(2):
            em.step_launch(1, 2)
            _on_moment_path(em)
            eo, en = em.moves_fetch()
            counts = em.moves_counts()
            runs.append((eo, en, counts, em.last_dispatch("moves")["declined"]))
        print("declined", runs[0][3], "counts", runs[0][2], "oracle", case.totals)
        assert 1 <= runs[0][3] < len(case.imol)
        case.check_energies(runs[0][0], runs[0][1])
        assert runs[0][2] == case.totals
        assert runs[1][3] == runs[0][3] and runs[1][2] == runs[0][2]
        assert np.array_equal(runs[1][0], runs[0][0]) and np.array_equal(runs[1][1], runs[0][1])
    finally:
        em.energy_deinit()


def test_one_sided_launches_fill_their_own_two_totals(case, monkeypatch):
    em = case.engine(monkeypatch)
    try:
        e1 = em.local_energy_batch(case.ils, case.imol)                     # mode 1: mirrored positions
        _on_moment_path(em)
        assert np.all(np.abs(e1 - case.eo) <= RTOL * np.abs(case.eo))
        assert em.moves_counts() == (case.totals[0], case.totals[1], 0, 0)
        e2 = em.local_energy_batch(case.ils, case.imol, case.trial)         # mode 2: trial positions
        _on_moment_path(em)
        assert np.all(np.abs(e2 - case.en) <= RTOL * np.abs(case.en) + 1e-14)
        assert em.moves_counts() == (0, 0, case.totals[2], case.totals[3])
    finally:
        em.energy_deinit()


def test_counts_never_made_are_dropped_by_what_changes_their_inputs(case, monkeypatch):
    from mc_water_ls_mw_amd.energy import MwError
    em = case.engine(monkeypatch)
    try:
        em.moves_upload(case.ils, case.imol, case.trial)
        em.step_launch(1, 2)
        em.moves_upload(case.ils, case.imol, case.trial)                    # new requests, no launch
        with pytest.raises(MwError, match="changed since"):
            em.moves_counts()
        em.moves_launch()
        assert em.moves_counts() == case.totals
        em.moves_launch()
        em.sync_positions(1)                                                # a position upload
        with pytest.raises(MwError, match="changed since"):
            em.moves_counts()
        assert em.last_dispatch("moves")["count_passes"] == 1
        em.step_launch(1, 2)
        assert em.moves_counts() == case.totals
        em.sync_positions(1)                                                # counts already made stay readable
        assert em.moves_counts() == case.totals
    finally:
        em.energy_deinit()
