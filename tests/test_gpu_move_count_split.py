"""GPU: the count pass of the move kernel's moment path splits the four slots of a row load between the two lanes of a pair --
lane `side` gathers slots side and 2 + side, tests each against both positions, and one exchange per load brings the two lanes
the same nibble of the row-slot mask, the same count and the same self bit (lanes_scan<false>, mw_move_lanes.hip.h).  What can go
wrong there that a full scan per lane could not: a slot past the row's end in one lane only (rows of odd length), a row that ends
inside the first load (1, 2, 3 slots), at its end (4) and one slot into the second (5), a bit in the other lane's place of the
nibble, and the last load of a 32-slot row.  The mask decides what the main pass queues, so a wrong bit shows in the energies and
the counts; with MW_MOVE_MASKS=0 the main pass scans the rows itself (the STORE scan, a full scan per lane as before) and must
give the same bytes.  Energies against the C oracle at RTOL / DE_ATOL of conftest.py, counts exact (tests/move_counts_ref.py), the
declined requests predicted on the host (tests/move_lanes_ref.py); every launch must be build 3."""
import numpy as np
import pytest

from move_counts_ref import request_counts
from move_lanes_ref import predict
from test_gpu_move_masks import _Bcc, _env, _row_classes
from test_gpu_move_sorted import _ask, _check, _same, _want

pytestmark = pytest.mark.gpu


class _Sparse:
    """A jittered simple cubic box of 6 x 6 x 8 molecules 1.2 cutoffs apart (sigma 0.12 cutoffs): rows of 0 to 6 slots, of which a
    request has up to three in range of its old or its trial position.  140 requests of molecules whose row is not empty."""

    def __init__(self, oracle):
        from mc_water_ls_mw_amd import lattice as lat
        rc = oracle.constants()[0] * oracle.constants()[6]
        a = 1.2 * rc
        grid = np.array([[i, j, k] for i in range(6) for j in range(6) for k in range(8)], dtype=np.float64) * a
        self.h = np.diag([6 * a, 6 * a, 8 * a])
        self.x = grid + np.random.default_rng(5).normal(0.0, 0.1 * a, grid.shape)
        self.iv = oracle.ivects(self.h)
        self.lists = oracle.neighbours(self.x, self.iv, 64)
        imol, trial = lat.trial_moves(self.x, 400, max_trans_ang=1.1, seed=3)
        keep = self.lists[0][imol - 1] >= 1                                     # (the host's prediction wants a row to look at)
        self.imol, self.trial = imol[keep][:140].astype(np.int32), trial[keep][:140]
        self.p = predict(oracle, self.x, self.iv, *self.lists, self.imol, self.trial)
        self.ro, self.rn = oracle.trial_moves(self.imol, self.trial, self.x, self.iv, *self.lists)
        self.ref = request_counts(oracle, self.x, self.iv, *self.lists, self.imol, self.trial)[0]


@pytest.fixture(scope="module")
def sparse(c_oracle):
    return _Sparse(c_oracle)


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_rows_of_one_to_five_slots(sparse, monkeypatch, mode):
    from mc_water_ls_mw_amd.energy import load_boxes
    p = sparse.p
    print("requests by row length", np.bincount(p["row"]), "by union", np.bincount(p["union"]), "declined", p["declined"].sum(), "margin", p["margin"].min())
    assert len(sparse.imol) == 140 and p["margin"].min() > 1e-6
    for n in (1, 2, 3, 4, 5):                                                   # (each with a request that has an entry in range)
        assert np.sum((p["row"] == n) & (p["union"] >= 1)) >= 1, n
    assert p["union"].max() >= 2 and np.sum(p["union"] == 0) >= 10
    got = {}
    for masks in (True, False):
        _env(monkeypatch, 64, masks)
        em = load_boxes([sparse.h], [sparse.x], maxneigh=64)
        try:
            nn, jn, vn = em.neighbours(1)
            assert np.array_equal(nn, sparse.lists[0])                          # (the rows the prediction looked at)
            got[masks] = _ask(em, mode, 1, sparse.imol, sparse.trial, 64)
        finally:
            em.energy_deinit()
    assert _same(got[True][0], got[False][0]) and _same(got[True][1], got[False][1])
    assert got[True][2] == got[False][2] and got[True][3] == got[False][3]
    for masks in (True, False):
        _check(got[masks][0], got[masks][1], sparse.ro, sparse.rn, mode)
        assert got[masks][2] == _want(sparse.ref, mode)
        if mode != 1:
            assert got[masks][3] == int(p["declined"].sum())


def test_slot_edges_and_rows_on_both_sides_of_32_slots(c_oracle, monkeypatch):
    """The box of test_gpu_move_masks.py's test_slot_edges and test_rows_on_both_sides_of_32_slots_in_one_item (rows of 27 to 38
    slots, odd and even lengths, rows of exactly 32): what the count pass marks is held to the prediction's union through the
    number declined -- every request over the cap and no other -- the counts and the energies."""
    bcc = _Bcc(c_oracle, 2.70, 0.10, 400, 0.05, 3)
    p = bcc.p
    served = ~p["declined"]
    print("rows", np.bincount(p["row"])[27:], "served by row class", _row_classes(p), "union", np.bincount(p["union"]))
    assert p["margin"].min() > 1e-6 and np.array_equal(p["declined"], p["cap"]) and min(_row_classes(p)) >= 25
    assert np.sum(served & (p["row"] % 2 == 0) & (p["row"] < 32)) >= 10 and np.sum(served & (p["row"] % 2 == 1) & (p["row"] < 32)) >= 10
    assert np.sum(p["union"] == 16) >= 1 and np.sum(p["union"] == 17) >= 1        # (the count on both sides of the cap)
    bcc.on_and_off(monkeypatch, 64)
