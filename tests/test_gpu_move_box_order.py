"""GPU: a step's trial moves served NEWEST BOXES FIRST (mw_moves_upload builds the work list with the boxes in descending order, the
opposite of the order in which the persistent full-box pass hands them out; MW_MOVE_BOX_ORDER=asc: the ascending order, for A/B
runs) and the full-box pass's list stream read with the non-temporal policy (list_load, mw_full_energy.hip.h).  Neither may change
a bit: a request's result is its own, a box's energy is summed in group order.  Three thermalised ice Ih boxes to an engine -- 288,
640 and 512 molecules: a last group of 32, of 0 and of 0 lanes, staged in LDS, no self-image (checked here on the oracle's lists)
-- 600 requests in each, interleaved on upload, among them molecule 1, the last molecules and every molecule of their rows.  One
step (mw_step_launch) against the C oracle: energies to 1e-10 relative (RTOL of conftest.py), energy changes to DE_ATOL, counts
exact, with MW_MOVE_MOMENTS=1 and =0; then default, `asc` and `desc` byte for byte, in items of 64 requests so that the thirty
work items go through the XCD dealing in either order."""
import numpy as np
import pytest

from conftest import DE_ATOL, RTOL
from move_counts_ref import request_counts
from test_gpu_moment_store import _Boxes

pytestmark = pytest.mark.gpu

NREQ = 600
REPS = {0: (4, 3, 3), 1: (4, 4, 5), 2: (4, 4, 4)}            # ice Ih cells of 288, 640 and 512 molecules
NBOX = 3


class _Case:
    """Three thermal boxes, NREQ requests in each and what the oracle makes of them (computed once, never changed)."""

    def __init__(self, oracle, rem):
        from mc_water_ls_mw_amd import lattice as lat
        self.boxes = bx = _Boxes(oracle, REPS[rem], NBOX, 7300 + rem)
        n = bx.n
        assert n % 3 == rem
        per = []
        for b in range(NBOX):
            nn, jn, vn = bx.lists[b]
            assert all(i + 1 not in jn[i, :nn[i]] for i in range(n))               # no molecule lists an image of itself
            ends = [1, n, n - 1, n - 2]                                            # molecule 1 and the last ones
            rows = [int(j) for i in (1, n) for j in jn[i - 1, :nn[i - 1]]]          # ... and the molecules that have them as neighbours
            i_rand, _ = lat.trial_moves(bx.xs[b], NREQ, seed=60 + 10 * rem + b)
            imol = np.array((ends + rows + list(i_rand))[:NREQ], dtype=np.int32)
            rng = np.random.default_rng(900 + 10 * rem + b)
            trial = bx.xs[b][imol - 1] + rng.normal(0.0, 0.4, (NREQ, 3))
            ro, rn = oracle.trial_moves(imol, trial, bx.xs[b], bx.iv, *bx.lists[b])
            ref = request_counts(oracle, bx.xs[b], bx.iv, *bx.lists[b], imol, trial)[0]
            per.append((imol, trial, ro, rn, ref))
        order = sorted((k, b) for b in range(NBOX) for k in range(NREQ))            # interleaved on upload: the output slots are no identity
        self.ils = np.array([b + 1 for _, b in order], dtype=np.int32)
        pick = lambda c: np.array([per[b][c][k] for k, b in order])               # noqa: E731
        self.imol, self.trial, self.ro, self.rn, self.ref = pick(0).astype(np.int32), pick(1), pick(2), pick(3), pick(4)


@pytest.fixture(scope="module", params=[0, 1, 2], ids=["n288", "n640", "n512"])
def case(request, c_oracle):
    return _Case(c_oracle, request.param)


def _step(case, monkeypatch, moments, order=None, chunk=None):
    """One step on a fresh engine: (box energies, box counts, e_old, e_new, move counts, dispatch of the moves)."""
    monkeypatch.setenv("MW_MOVE_MOMENTS", moments)
    for name, v in (("MW_MOVE_BOX_ORDER", order), ("MW_MOVE_CHUNK", chunk)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)
    em = case.boxes.engine()
    try:
        em.moves_upload(case.ils, case.imol, case.trial)
        em.step_launch(1, NBOX)
        e = em.model_energy_fetch(1, NBOX)
        eo, en = em.moves_fetch()
        c = em.moves_counts()
        return e, [em.model_energy_counts(b + 1) for b in range(NBOX)], eo, en, tuple(int(v) for v in c), em.last_dispatch("moves"), em.last_dispatch("energy")
    finally:
        em.energy_deinit()


@pytest.mark.parametrize("moments", ["1", "0"])
def test_a_step_against_the_oracle(case, monkeypatch, moments):
    bx = case.boxes
    e, cfull, eo, en, c, dm, de = _step(case, monkeypatch, moments)
    assert dm["mlds"] == 1 and dm["noself"] == 1 and de["lds"] == 1 and de["nsplit"] == 1
    assert dm["use_mom"] == int(moments) and de["moments"] == int(moments) and dm["build"] == (3 if moments == "1" else 2), (dm, de)
    print("N", bx.n, "moments", moments, "declined", dm["declined"],
          "max rel err E", np.max(np.abs(e - bx.e_full) / np.abs(bx.e_full)),
          "e_old", np.max(np.abs(eo - case.ro) / np.abs(case.ro)), "e_new", np.max(np.abs(en - case.rn) / np.abs(case.rn)),
          "max |d(dE)|", np.max(np.abs((en - eo) - (case.rn - case.ro))))
    assert np.all(np.abs(e - bx.e_full) <= RTOL * np.abs(bx.e_full))
    assert cfull == bx.c_full
    assert np.all(np.abs(eo - case.ro) <= RTOL * np.abs(case.ro))
    assert np.all(np.abs(en - case.rn) <= RTOL * np.abs(case.rn))
    assert np.all(np.abs((en - eo) - (case.rn - case.ro)) <= DE_ATOL)
    assert c == tuple(int(v) for v in case.ref.sum(axis=0))


def test_the_box_order_changes_no_byte(case, monkeypatch):
    """Items of 64 requests: 30 work items, dealt to the eight XCD sequences in either order."""
    got = {o: _step(case, monkeypatch, "1", order=o, chunk="64") for o in (None, "asc", "desc")}
    for o in ("asc", "desc"):
        assert got[o][5]["items"] == got[None][5]["items"] >= 16 and got[o][5]["mchunk"] == 64
        assert got[o][0].tobytes() == got[None][0].tobytes() and got[o][1] == got[None][1]
        assert got[o][2].tobytes() == got[None][2].tobytes() and got[o][3].tobytes() == got[None][3].tobytes()
        assert got[o][4] == got[None][4] and got[o][5]["declined"] == got[None][5]["declined"]
    assert np.all(np.abs(got[None][2] - case.ro) <= RTOL * np.abs(case.ro))
    # the switch works: the work list starts from the highest box by default and with `desc`, from the lowest with `asc`
    assert got[None][5]["first_box"] == NBOX - 1 and got["desc"][5]["first_box"] == NBOX - 1 and got["asc"][5]["first_box"] == 0
