"""GPU: the count pass of the move kernel's moment path leaves every request a ROW-SLOT MASK -- bit s set when slot s of its
molecule's row is in range of the old or the trial position -- and the main pass walks the masks instead of scanning the rows again
(k_move_energy's mode bit 6, lanes_entries / lanes_park of mw_move_lanes.hip.h; MW_MOVE_MASKS=0 keeps the second scan).  The queue
a mask decodes to is word for word the one the scan parks, so the switch may change nothing: energies byte-identical with it off,
counts and the number declined equal, and both held to the C oracle at RTOL / DE_ATOL of conftest.py, counts exact
(tests/move_counts_ref.py), the declined requests predicted on the host (tests/move_lanes_ref.py).  What the masks add that can go
wrong: a mask in another request's slot of the table, slots 0 and 31, rows longer than the mask is wide (the "scan me" word) beside
rows that fit in one group, a launch without a count pass reading a table nobody wrote, the lanes past the end of the last group,
and the pass that counts on demand walking the same masks.  Every launch must be build 3."""
import numpy as np
import pytest

from move_counts_ref import request_counts
from move_lanes_ref import predict
from test_gpu_move_lanes import _dense_case
from test_gpu_move_sorted import FILL, _Fill, _ask, _check, _same, _want

pytestmark = pytest.mark.gpu


def _env(monkeypatch, chunk, masks, sort=True, counts=None):
    monkeypatch.setenv("MW_MOVE_MOMENTS", "1")
    monkeypatch.setenv("MW_MOVE_CHUNK", str(chunk))
    for name, on in (("MW_MOVE_MASKS", masks), ("MW_MOVE_SORT", sort)):
        if on:
            monkeypatch.delenv(name, raising=False)                            # (the default is on)
        else:
            monkeypatch.setenv(name, "0")
    if counts is None:
        monkeypatch.delenv("MW_MOVE_COUNTS", raising=False)
    else:
        monkeypatch.setenv("MW_MOVE_COUNTS", counts)


@pytest.fixture(scope="module")
def fill(c_oracle):
    return _Fill(c_oracle)


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("chunk", [64, 256, 1024])
def test_same_bits_with_and_without_the_masks(fill, monkeypatch, chunk, mode):
    """Masks on, masks off, and masks on without the sort (no count pass: nothing may read a mask).  Mode 1 has no trial position --
    its mask is the old position's alone -- and mode 2 must still mark what the even lane finds at the old position: both show in
    the counts and in the energies."""
    assert not np.array_equal(fill.ils, np.sort(fill.ils))
    got = {}
    for name, masks, sort in (("on", True, True), ("off", False, True), ("unsorted", True, False)):
        _env(monkeypatch, chunk, masks, sort)
        em = fill.boxes.engine()
        try:
            got[name] = _ask(em, mode, fill.ils, fill.imol, fill.trial, chunk)
        finally:
            em.energy_deinit()
    print("chunk", chunk, "mode", mode, "declined", [g[3] for g in got.values()], "counts", got["on"][2])
    for name, g in got.items():
        assert _same(g[0], got["on"][0]) and _same(g[1], got["on"][1]), name
        assert g[2] == got["on"][2] and g[3] == got["on"][3], name
        _check(g[0], g[1], fill.ro, fill.rn, mode)
        assert g[2] == _want(fill.ref, mode), name
    assert fill.declined == 0 and got["on"][3] == fill.declined


class _Bcc:
    """A body-centred cubic box of 6 x 6 x 6 cells (432 molecules), nearest neighbours `d_ang` apart, thermalised, its requests and
    what the oracle and the host's prediction make of them (computed once, never changed)."""

    def __init__(self, oracle, d_ang, sigma, nreq, max_trans, seed):
        from mc_water_ls_mw_amd import lattice as lat
        a = 2.0 * d_ang / np.sqrt(3.0) * lat.ANG_TO_BOHR
        h, x = lat.replicate(np.eye(3) * a, np.array([[0.0, 0.0, 0.0], [0.5, 0.5, 0.5]]) * a, (6, 6, 6))
        self.h, self.x, self.iv, self.lists, self.imol, self.trial = _dense_case(oracle, h, x, sigma, nreq, max_trans, seed)
        self.p = predict(oracle, self.x, self.iv, *self.lists, self.imol, self.trial)
        self.ro, self.rn = oracle.trial_moves(self.imol, self.trial, self.x, self.iv, *self.lists)
        self.ref = request_counts(oracle, self.x, self.iv, *self.lists, self.imol, self.trial)[0]
        self.rc = oracle.constants()[0] * oracle.constants()[6]               # the cutoff, as move_lanes_ref.py takes it

    def engine(self):
        from mc_water_ls_mw_amd.energy import load_boxes
        return load_boxes([self.h], [self.x], maxneigh=64)

    def on_and_off(self, monkeypatch, chunk):
        """One launch (old + trial) with the masks and one without: byte-identical, and each held to the oracle and the prediction."""
        got = {}
        for masks in (True, False):
            _env(monkeypatch, chunk, masks)
            em = self.engine()
            try:
                got[masks] = _ask(em, 3, 1, self.imol, self.trial, chunk)
            finally:
                em.energy_deinit()
        print("chunk", chunk, "declined", got[True][3], got[False][3], "predicted", int(self.p["declined"].sum()), "counts", got[True][2])
        assert _same(got[True][0], got[False][0]) and _same(got[True][1], got[False][1])
        assert got[True][2] == got[False][2] and got[True][3] == got[False][3]
        for masks in (True, False):
            assert got[masks][3] == int(self.p["declined"].sum())
            _check(got[masks][0], got[masks][1], self.ro, self.rn, 3)
            assert got[masks][2] == _want(self.ref, 3)


@pytest.fixture(scope="module")
def bcc270(c_oracle):
    """Nearest neighbours 2.70 A apart, sigma 0.10 A: rows of 27 to 38 slots, so one item holds requests the masks serve and
    requests that carry the "scan me" word."""
    return _Bcc(c_oracle, 2.70, 0.10, 400, 0.05, 3)


def _row_classes(p):
    served = ~p["declined"]
    return [int(np.sum(served & sel)) for sel in (p["row"] <= 31, p["row"] == 32, p["row"] == 33, p["row"] > 33)]


@pytest.mark.parametrize("chunk", [64, 256])
def test_rows_on_both_sides_of_32_slots_in_one_item(bcc270, monkeypatch, chunk):
    """Items of about 57 requests (two groups each) and two items of 200: after the sort a group holds only requests with masks,
    only requests of long rows, or both -- and a group with one long row scans all of its requests."""
    p = bcc270.p
    print("rows", p["row"].min(), p["row"].max(), "served by row class <=31 / 32 / 33 / >33", _row_classes(p), "union of the served",
          p["union"][~p["declined"]].min(), p["union"][~p["declined"]].max(), "declined", p["declined"].sum(), "margin", p["margin"].min())
    assert min(_row_classes(p)) >= 25
    assert p["margin"].min() > 1e-6                                              # (the prediction is exact: nothing sits on a threshold)
    assert np.array_equal(p["declined"], p["cap"])
    bcc270.on_and_off(monkeypatch, chunk)


def test_slot_edges(bcc270, monkeypatch):
    """The first and the last bit of a mask, from the ENGINE's own rows (the device orders a row its own way): among the served
    requests of the case above, one whose row of exactly 32 slots has slot 31 in range of the old or the trial position, and one
    with slot 0 in range.  (test_rows_on_both_sides_of_32_slots_in_one_item holds those requests to the oracle.)"""
    _env(monkeypatch, 64, True)
    em = bcc270.engine()
    try:
        nn, jn, vn = em.neighbours(1)
        iv = em.ivect(1)
    finally:
        em.energy_deinit()
    rc = bcc270.rc
    last32 = first = 0
    for r in np.flatnonzero(~bcc270.p["declined"]):
        i = int(bcc270.imol[r]) - 1
        n = int(nn[i])
        assert n == int(bcc270.p["row"][r])                                     # (the same row, whatever its order)
        q = bcc270.x[jn[i, :n] - 1] + iv[vn[i, :n] - 1]
        inr = (np.linalg.norm(q - bcc270.x[i], axis=1) < rc) | (np.linalg.norm(q - bcc270.trial[r], axis=1) < rc)
        assert int(inr.sum()) == int(bcc270.p["union"][r])
        first += bool(inr[0])
        last32 += n == 32 and bool(inr[31])
    print("served requests with slot 0 in range", first, "with a row of 32 and slot 31 in range", last32)
    assert first >= 1 and last32 >= 1


def test_rows_that_are_all_long(c_oracle, monkeypatch):
    """Nearest neighbours 2.65 A apart (test_rows_longer_than_32_entries of test_gpu_move_lanes.py): rows of 43 to 50 slots, every
    mask the "scan me" word, every group scanned."""
    case = _Bcc(c_oracle, 2.65, 0.004, 160, 0.03, 3)
    assert case.p["row"].min() >= 33 and case.p["margin"].min() > 1e-6
    assert np.sum(~case.p["declined"]) >= 100
    case.on_and_off(monkeypatch, 64)


@pytest.mark.parametrize("n", [33, 65])
def test_a_partial_last_group_with_masks(fill, monkeypatch, n):
    """33 and 65 requests in one item of 1024: the last group holds one request, and the lanes past the end decode the last
    request's mask again and serve nothing -- the output slots beyond the launch's range keep what an earlier launch left there."""
    sel = np.flatnonzero(fill.ils == 10)                                        # the box with 600 requests
    first, second = sel[:200], sel[200:200 + n]
    _env(monkeypatch, 1024, True)
    em = fill.boxes.engine()
    try:
        em.moves_upload(fill.ils[first], fill.imol[first], fill.trial[first])
        em.moves_launch()
        eo1, en1 = em.moves_fetch()
        _check(eo1, en1, fill.ro[first], fill.rn[first], 3)
        em.moves_upload(fill.ils[second], fill.imol[second], fill.trial[second])
        em.moves_launch()
        d = em.last_dispatch("moves")
        assert d["build"] == 3 and d["use_mom"] == 1 and d["items"] == 1 and d["mchunk"] == 1024, d
        eo2, en2 = em.moves_fetch()
        assert len(eo2) == n
        _check(eo2, en2, fill.ro[second], fill.rn[second], 3)
        assert em.moves_counts() == _want(fill.ref[second], 3)
        em.moves_upload(fill.ils[first], fill.imol[first], fill.trial[first])   # (read back with no launch)
        eo3, en3 = em.moves_fetch()
        assert eo3[n:].tobytes() == eo1[n:].tobytes() and en3[n:].tobytes() == en1[n:].tobytes()
        assert eo3[:n].tobytes() == eo2.tobytes() and en3[:n].tobytes() == en2.tobytes()
    finally:
        em.energy_deinit()


def test_counts_on_demand_walk_the_masks(fill, monkeypatch):
    got = {}
    for how in (None, "eager"):
        _env(monkeypatch, 256, True, counts=how)
        em = fill.boxes.engine()
        try:
            em.moves_upload(fill.ils, fill.imol, fill.trial)
            em.step_launch(1, len(FILL))
            d = em.last_dispatch("moves")
            assert d["build"] == 3 and d["use_mom"] == 1 and d["counts"] == (0 if how else 1), d
            e = em.moves_fetch()
            got[how] = (e, em.moves_counts(), em.last_dispatch("moves")["count_passes"])
        finally:
            em.energy_deinit()
    assert got[None][2] == 1 and got["eager"][2] == 0
    assert got[None][1] == got["eager"][1] == _want(fill.ref, 3)
    assert _same(got[None][0][0], got["eager"][0][0]) and _same(got[None][0][1], got["eager"][0][1])
    _check(got[None][0][0], got[None][0][1], fill.ro, fill.rn, 3)
