"""GPU: the moment path of the move kernel SORTS an item's requests by their number of in-range neighbours before it evaluates
them (k_move_energy's count / sort / evaluate, mw_move_energy.hip.h; MW_MOVE_SORT=0 keeps the order of the upload).  A request's
bits are its own, so the sort may change nothing: energies byte-identical with the switch off, counts and the number declined
equal, and both held to the C oracle at RTOL / DE_ATOL of conftest.py, counts exact (tests/move_counts_ref.py), the declined
requests predicted on the host (tests/move_lanes_ref.py).  What the sort adds that can go wrong: requests landing in another
caller slot, the bin of requests over the queue's cap (left out of the groups, declined exactly once), an item with nothing left
to serve, the partial last group of the SORTED table, and the pass that counts on demand walking the same order.  Every launch must
be build 3."""
import numpy as np
import pytest

from conftest import DE_ATOL, RTOL
from move_counts_ref import request_counts
from move_lanes_ref import predict
from test_gpu_moment_store import _Boxes

pytestmark = pytest.mark.gpu

FILL = (1, 2, 31, 32, 33, 63, 64, 65, 200, 600)          # requests per box


def _env(monkeypatch, chunk, sort, counts=None):
    monkeypatch.setenv("MW_MOVE_MOMENTS", "1")
    monkeypatch.setenv("MW_MOVE_CHUNK", str(chunk))
    if sort:
        monkeypatch.delenv("MW_MOVE_SORT", raising=False)                  # (the default is on)
    else:
        monkeypatch.setenv("MW_MOVE_SORT", "0")
    if counts is None:
        monkeypatch.delenv("MW_MOVE_COUNTS", raising=False)
    else:
        monkeypatch.setenv("MW_MOVE_COUNTS", counts)


def _ask(em, mode, ils, imol, trial, chunk):
    """(e_old or None, e_new or None, counts, declined) of one launch in `mode` (1 old, 2 trial, 3 both)."""
    eo = en = None
    if mode == 1:
        eo = em.local_energy_batch(ils, imol)
    elif mode == 2:
        en = em.local_energy_batch(ils, imol, trial)
    else:
        eo, en = em.delta_energy_batch(ils, imol, trial)
    c = em.moves_counts()
    d = em.last_dispatch("moves")
    assert d["build"] == 3 and d["use_mom"] == 1 and d["mlds"] == 1 and d["noself"] == 1 and d["mchunk"] == chunk, d
    return eo, en, c, d["declined"]


def _want(ref, mode):
    t = ref.sum(axis=0)
    return (int(t[0]) if mode & 1 else 0, int(t[1]) if mode & 1 else 0, int(t[2]) if mode & 2 else 0, int(t[3]) if mode & 2 else 0)


def _check(eo, en, ro, rn, mode):
    if mode & 1:
        assert np.all(np.abs(eo - ro) <= RTOL * np.abs(ro))
    if mode & 2:
        assert np.all(np.abs(en - rn) <= RTOL * np.abs(rn))
    if mode == 3:
        assert np.all(np.abs((en - eo) - (rn - ro)) <= DE_ATOL)


def _same(a, b):
    return (a is None and b is None) or (a.tobytes() == b.tobytes())


class _Fill:
    """Ten 288-molecule boxes with FILL[b] requests in box b, interleaved on upload (the output slots are no identity), what the
    oracle makes of every request and the host's prediction of every request's queue (computed once, never changed)."""

    def __init__(self, oracle):
        from mc_water_ls_mw_amd import lattice as lat
        self.boxes = _Boxes(oracle, (4, 3, 3), len(FILL), 6100)
        bx = self.boxes
        per = []
        for b, n in enumerate(FILL):
            i, t = lat.trial_moves(bx.xs[b], n, seed=40 + b)
            ro, rn = oracle.trial_moves(i, t, bx.xs[b], bx.iv, *bx.lists[b])
            ref = request_counts(oracle, bx.xs[b], bx.iv, *bx.lists[b], i, t)[0]
            p = predict(oracle, bx.xs[b], bx.iv, *bx.lists[b], i, t)
            per.append((i.astype(np.int32), t, ro, rn, ref, p["union"], p["n_old"], p["n_new"], p["declined"]))
        order = sorted((k, b) for b, n in enumerate(FILL) for k in range(n))      # round robin over the boxes that still have requests
        self.ils = np.array([b + 1 for _, b in order], dtype=np.int32)
        pick = lambda c: np.array([per[b][c][k] for k, b in order])             # noqa: E731
        self.imol, self.trial, self.ro, self.rn, self.ref = pick(0).astype(np.int32), pick(1), pick(2), pick(3), pick(4)
        self.nq = {1: pick(6), 2: pick(5), 3: pick(5)}                          # what a request queues: mode 1 has no trial position
        self.declined = int(pick(8).sum())

    def widest_item(self, chunk, mode):
        """The largest number of different nq among the requests of one work item (equal shares of a box's requests, in the order
        of the upload within the box: mw_moves_upload)."""
        most = 0
        for b, n in enumerate(FILL):
            nq = self.nq[mode][self.ils == b + 1]
            nitems = (n + chunk - 1) // chunk
            for k in range(nitems):
                most = max(most, len(set(nq[n * k // nitems:n * (k + 1) // nitems])))
        return most


@pytest.fixture(scope="module")
def fill(c_oracle):
    return _Fill(c_oracle)


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("chunk", [64, 256, 1024])
def test_same_bits_with_and_without_the_sort(fill, monkeypatch, chunk, mode):
    assert not np.array_equal(fill.ils, np.sort(fill.ils))
    wide = fill.widest_item(chunk, mode)
    print("chunk", chunk, "mode", mode, "different nq in one item", wide)
    assert wide >= 6                                                            # (the sort really moves requests)
    got = {}
    for sort in (True, False):
        _env(monkeypatch, chunk, sort)
        em = fill.boxes.engine()
        try:
            got[sort] = _ask(em, mode, fill.ils, fill.imol, fill.trial, chunk)
        finally:
            em.energy_deinit()
    print("declined", got[True][3], got[False][3], "counts", got[True][2])
    assert _same(got[True][0], got[False][0]) and _same(got[True][1], got[False][1])
    assert got[True][2] == got[False][2] and got[True][3] == got[False][3]
    for sort in (True, False):
        _check(got[sort][0], got[sort][1], fill.ro, fill.rn, mode)
        assert got[sort][2] == _want(fill.ref, mode)
    # (mode 2 applies the same rules as mode 3 -- the even lane still scans and tests at the old position; mode 1 applies them at the
    #  old position alone, a subset; nothing of this fill is declined, so the prediction pins all three)
    assert fill.declined == 0 and got[True][3] == fill.declined


@pytest.mark.parametrize("moved", [False, True])
def test_all_keys_equal(c_oracle, monkeypatch, moved):
    """The ideal lattice, one item of 96 requests, every request unmoved: every key's nq is the same, the sort a stable no-op.
    `moved`: trial positions up to 0.05 A away instead -- still four entries in range of either position for every request, but
    trial energies that differ from request to request, so a result in the wrong caller slot misses the oracle."""
    from mc_water_ls_mw_amd import lattice as lat
    from mc_water_ls_mw_amd.energy import load_boxes
    h, x = lat.ice_box("ih", (4, 3, 3))
    iv = c_oracle.ivects(h)
    lists = c_oracle.neighbours(x, iv)
    imol = np.random.default_rng(5).permutation(len(x))[:96].astype(np.int32) + 1
    trial = x[imol - 1].copy()
    if moved:
        trial += np.random.default_rng(6).uniform(-0.05, 0.05, trial.shape) * lat.ANG_TO_BOHR
    p = predict(c_oracle, x, iv, *lists, imol, trial)
    assert len(set(p["union"])) == 1 and not p["declined"].any() and p["margin"].min() > 1e-6
    ro, rn = c_oracle.trial_moves(imol, trial, x, iv, *lists)
    ref = request_counts(c_oracle, x, iv, *lists, imol, trial)[0]
    got = {}
    for sort in (True, False):
        _env(monkeypatch, 256, sort)
        em = load_boxes([h], [x])
        try:
            got[sort] = _ask(em, 3, 1, imol, trial, 256)
            assert em.last_dispatch("moves")["items"] == 1
        finally:
            em.energy_deinit()
    assert _same(got[True][0], got[False][0]) and _same(got[True][1], got[False][1])
    assert got[True][2] == got[False][2] == _want(ref, 3) and got[True][3] == got[False][3] == 0
    _check(got[True][0], got[True][1], ro, rn, 3)
    if moved:                                                                   # (the slots can be told apart: neighbours' energies differ far beyond the tolerance)
        assert np.min(np.abs(np.diff(np.sort(rn)))) > 100.0 * RTOL * np.max(np.abs(rn))
    else:
        assert np.all(np.abs(got[True][1] - got[True][0]) <= DE_ATOL)


def test_the_cap_bin(c_oracle, monkeypatch):
    """Cubic ice compressed to d_OO = 2.5 A (216 molecules): unions of 16 to 20, more than half of the requests over the queue's cap
    of 16.  They sort behind all others, are declined once each and left out of the groups -- and a launch of those requests alone
    has items with nothing to serve."""
    from mc_water_ls_mw_amd import lattice as lat
    from mc_water_ls_mw_amd.energy import load_boxes
    h, x = lat.ice_ic_cell(2.5)
    h, x = lat.replicate(h, x, (3, 3, 3))
    x = lat.thermalise(x, 0.03, 1)
    iv = c_oracle.ivects(h)
    lists = c_oracle.neighbours(x, iv, 64)
    imol, trial = lat.trial_moves(x, 160, max_trans_ang=1.1, seed=8)
    imol = imol.astype(np.int32)
    p = predict(c_oracle, x, iv, *lists, imol, trial)
    print("union", np.bincount(p["union"]), "cap", p["cap"].sum(), "declined", p["declined"].sum(), "margin", p["margin"].min())
    assert p["margin"].min() > 1e-6
    over = np.flatnonzero(p["cap"])
    assert len(over) >= 64 and len(over) < 160
    ro, rn = c_oracle.trial_moves(imol, trial, x, iv, *lists)
    ref = request_counts(c_oracle, x, iv, *lists, imol, trial)[0]
    _env(monkeypatch, 64, True)
    em = load_boxes([h], [x], maxneigh=64)
    try:
        eo, en, c, declined = _ask(em, 3, 1, imol, trial, 64)
        assert declined == int(p["declined"].sum())
        _check(eo, en, ro, rn, 3)
        assert c == _want(ref, 3)
        # the requests over the cap alone: whole items with nothing to serve
        eo, en, c, declined = _ask(em, 3, 1, imol[over], trial[over], 64)
        assert declined == len(over)                                            # (each exactly once)
        _check(eo, en, ro[over], rn[over], 3)
        assert c == _want(ref[over], 3)
    finally:
        em.energy_deinit()


@pytest.mark.parametrize("n", [33, 65])
def test_a_partial_last_group_after_sorting(fill, monkeypatch, n):
    """33 and 65 requests in one item: the sorted table's last group holds one request.  The lanes past the end write nothing: the
    output slots beyond the launch's range keep what an earlier, larger launch left there."""
    bx = fill.boxes
    sel = np.flatnonzero(fill.ils == 10)                                        # the box with 600 requests
    first, second = sel[:200], sel[200:200 + n]
    _env(monkeypatch, 1024, True)
    em = bx.engine()
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
        # the slots past the second launch's range, read back with a third upload of the first size and no launch
        em.moves_upload(fill.ils[first], fill.imol[first], fill.trial[first])
        eo3, en3 = em.moves_fetch()
        assert eo3[n:].tobytes() == eo1[n:].tobytes() and en3[n:].tobytes() == en1[n:].tobytes()
        assert eo3[:n].tobytes() == eo2.tobytes() and en3[:n].tobytes() == en2.tobytes()
    finally:
        em.energy_deinit()


def test_counts_on_demand_after_a_sorted_launch(fill, monkeypatch):
    got = {}
    for how in (None, "eager"):
        _env(monkeypatch, 256, True, how)
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
