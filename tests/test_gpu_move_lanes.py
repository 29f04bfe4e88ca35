"""GPU: the moment path of the batched move kernel with a lane pair per request (move_energy_mom_lanes, mw_move_lanes.hip.h): a
wavefront serves groups of 32 requests, lanes 2r and 2r + 1 request r at the old and at the trial position.  What can go wrong
there that the older tests of the moment path do not reach: groups that are not full, wavefronts without a group and with several,
a request's bits depending on its companions, the 16-entry queue's cap, the j--i--k term the own-moments sum cannot drop, and rows
longer than the 32 entries the wavefront routine stopped at.  Energies against the C oracle at RTOL / DE_ATOL of conftest.py, counts
exact (tests/move_counts_ref.py), the declined requests predicted on the host (tests/move_lanes_ref.py); every launch must be build 3."""
import numpy as np
import pytest

from conftest import DE_ATOL, RTOL
from move_counts_ref import request_counts
from move_lanes_ref import predict
from test_gpu_moment_store import _Boxes

pytestmark = pytest.mark.gpu

FILL = (1, 2, 31, 32, 33, 63, 64, 65, 200, 600)          # requests per box (600 at chunk 1024: 19 groups for 16 wavefronts)


def _ask(em, mode, ils, imol, trial):
    """(e_old or None, e_new or None, counts, dispatch record) of one launch in `mode` (1 old, 2 trial, 3 both)."""
    eo = en = None
    if mode == 1:
        eo = em.local_energy_batch(ils, imol)
    elif mode == 2:
        en = em.local_energy_batch(ils, imol, trial)
    else:
        eo, en = em.delta_energy_batch(ils, imol, trial)
    c = em.moves_counts()
    d = em.last_dispatch("moves")
    assert d["build"] == 3 and d["use_mom"] == 1 and d["mlds"] == 1 and d["noself"] == 1, d
    return eo, en, c, d


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


class _Fill:
    """Ten 288-molecule boxes with FILL[b] requests in box b, interleaved on upload (the output slots are no identity), and what the
    oracle makes of every request (computed once)."""

    def __init__(self, oracle):
        from mc_water_ls_mw_amd import lattice as lat
        self.boxes = _Boxes(oracle, (4, 3, 3), len(FILL), 6100)
        bx = self.boxes
        per = []
        for b, n in enumerate(FILL):
            i, t = lat.trial_moves(bx.xs[b], n, seed=40 + b)
            ro, rn = oracle.trial_moves(i, t, bx.xs[b], bx.iv, *bx.lists[b])
            ref = request_counts(oracle, bx.xs[b], bx.iv, *bx.lists[b], i, t)[0]
            per.append((i.astype(np.int32), t, ro, rn, ref))
        order = sorted((k, b) for b, n in enumerate(FILL) for k in range(n))      # round robin over the boxes that still have requests
        self.ils = np.array([b + 1 for _, b in order], dtype=np.int32)
        pick = lambda c: np.array([per[b][c][k] for k, b in order])             # noqa: E731
        self.imol, self.trial, self.ro, self.rn, self.ref = pick(0).astype(np.int32), pick(1), pick(2), pick(3), pick(4)


@pytest.fixture(scope="module")
def fill(c_oracle):
    return _Fill(c_oracle)


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("chunk", [64, 256, 1024])
def test_group_fill(fill, monkeypatch, chunk, mode):
    """Lone lane pairs, a partial last group, wavefronts without a group, several groups per wavefront; items of 64, 256 and 1024."""
    monkeypatch.setenv("MW_MOVE_MOMENTS", "1")
    monkeypatch.setenv("MW_MOVE_CHUNK", str(chunk))
    assert not np.array_equal(fill.ils, np.sort(fill.ils))
    em = fill.boxes.engine()
    try:
        eo, en, c, d = _ask(em, mode, fill.ils, fill.imol, fill.trial)
        assert d["mchunk"] == chunk
        print("chunk", chunk, "mode", mode, "items", d["items"], "declined", d["declined"], "counts", c)
        _check(eo, en, fill.ro, fill.rn, mode)
        assert c == _want(fill.ref, mode)
    finally:
        em.energy_deinit()


def test_a_requests_bits_are_its_own(c_oracle, monkeypatch):
    """One moved and one unmoved request, each evaluated alone in its box, first in a full group, last in a full group and among
    other companions: the same bits every time.  (Another box carries the requests that make the launch large enough to stage.)"""
    monkeypatch.setenv("MW_MOVE_MOMENTS", "1")
    monkeypatch.setenv("MW_MOVE_CHUNK", "64")
    from mc_water_ls_mw_amd import lattice as lat
    bx = _Boxes(c_oracle, (4, 3, 3), 2, 6200)
    x = bx.xs[0]
    ci, ct = lat.trial_moves(x, 96, seed=3)
    pad_i, pad_t = lat.trial_moves(bx.xs[1], 40, seed=4)
    em = bx.engine()
    try:
        for who, (ri, rt) in {"moved": (ci[0], ct[0]), "unmoved": (ci[1], x[ci[1] - 1])}.items():
            ref_o, ref_n = c_oracle.trial_moves(np.array([ri], dtype=np.int32), rt[None, :], x, bx.iv, *bx.lists[0])
            got = []
            settings = {"alone": ([], []), "first": ([], list(range(2, 33))), "last": (list(range(2, 33)), []),
                        "others": (list(range(40, 57)), list(range(60, 90)))}
            for name, (before, after) in settings.items():
                i0 = np.concatenate([ci[before], [ri], ci[after]]).astype(np.int32)
                t0 = np.concatenate([ct[before].reshape(-1, 3), rt[None, :], ct[after].reshape(-1, 3)])
                ils = np.concatenate([np.full(len(i0), 1), np.full(len(pad_i), 2)]).astype(np.int32)
                eo, en, _, d = _ask(em, 3, ils, np.concatenate([i0, pad_i]).astype(np.int32), np.concatenate([t0, pad_t]))
                got.append((eo[len(before)], en[len(before)]))
                print(who, name, got[-1], "declined", d["declined"])
                assert d["declined"] == 0
            assert all(np.array_equal(g, got[0]) for g in got[1:]), (who, got)
            assert abs(got[0][0] - ref_o[0]) <= RTOL * abs(ref_o[0]) and abs(got[0][1] - ref_n[0]) <= RTOL * abs(ref_n[0])
            if who == "unmoved":
                assert abs(got[0][1] - got[0][0]) <= DE_ATOL
    finally:
        em.energy_deinit()


def _dense_case(oracle, h, x, sigma, nreq, max_trans, seed):
    from mc_water_ls_mw_amd import lattice as lat
    x = lat.thermalise(x, sigma, seed)
    iv = oracle.ivects(h)
    lists = oracle.neighbours(x, iv, 64)
    imol, trial = lat.trial_moves(x, nreq, max_trans_ang=max_trans, seed=seed + 7)
    return h, x, iv, lists, imol.astype(np.int32), trial


def _dense_check(oracle, case):
    """Launch the case's requests (old + trial) and hold energies, counts and the number declined to the oracle and the host's
    prediction; returns the prediction."""
    from mc_water_ls_mw_amd.energy import load_boxes
    h, x, iv, lists, imol, trial = case
    p = predict(oracle, x, iv, *lists, imol, trial)
    print("rows", lists[0].min(), lists[0].max(), "union", np.bincount(p["union"]), "declined", p["declined"].sum(), "margin", p["margin"].min())
    assert p["margin"].min() > 1e-6              # (the prediction is exact: nothing sits on a threshold)
    ro, rn = oracle.trial_moves(imol, trial, x, iv, *lists)
    ref = request_counts(oracle, x, iv, *lists, imol, trial)[0]
    em = load_boxes([h], [x], maxneigh=64)
    try:
        eo, en, c, d = _ask(em, 3, 1, imol, trial)
        assert d["declined"] == int(p["declined"].sum()), (d["declined"], int(p["declined"].sum()))
        _check(eo, en, ro, rn, 3)
        assert c == _want(ref, 3)
    finally:
        em.energy_deinit()
    return p


def test_queue_cap(c_oracle, monkeypatch):
    """Cubic ice compressed to d_OO = 2.6 A (216 molecules): the second shell, twelve molecules, sits just inside the cutoff, so a
    request has 13 to 18 neighbours in range of its old or its trial position.  16 are served, 17 are declined."""
    monkeypatch.setenv("MW_MOVE_MOMENTS", "1")
    monkeypatch.setenv("MW_MOVE_CHUNK", "64")
    from mc_water_ls_mw_amd import lattice as lat
    h, x = lat.ice_ic_cell(2.6)
    h, x = lat.replicate(h, x, (3, 3, 3))
    p = _dense_check(c_oracle, _dense_case(c_oracle, h, x, 0.03, 160, 1.1, 1))
    for u in (15, 16, 17):
        assert np.any(p["union"] == u)
    assert not np.any(p["declined"][p["union"] == 16]) and np.all(p["declined"][p["union"] == 17])
    assert np.array_equal(p["declined"], p["cap"])


def test_rows_longer_than_32_entries(c_oracle, monkeypatch):
    """A body-centred cubic box (432 molecules, nearest neighbours 2.65 A apart): fourteen neighbours inside the cutoff, the twelve of
    the third shell 0.02 A outside it and 24 more inside the list radius -- rows of 43 to 50 entries, which the wavefront routine
    declined for their length.  Requests whose union stays within 16 are served."""
    monkeypatch.setenv("MW_MOVE_MOMENTS", "1")
    monkeypatch.setenv("MW_MOVE_CHUNK", "64")
    from mc_water_ls_mw_amd import lattice as lat
    a = 2.0 * 2.65 / np.sqrt(3.0) * lat.ANG_TO_BOHR
    h, x = lat.replicate(np.eye(3) * a, np.array([[0.0, 0.0, 0.0], [0.5, 0.5, 0.5]]) * a, (6, 6, 6))
    case = _dense_case(c_oracle, h, x, 0.004, 160, 0.03, 3)
    assert case[3][0].min() >= 33 and case[3][0].max() <= 64
    p = _dense_check(c_oracle, case)
    assert np.sum((p["row"] > 32) & ~p["declined"]) >= 100 and np.all(p["union"][~p["declined"]] <= 16)


def test_the_dropped_jik_term(c_oracle, monkeypatch):
    """A molecule c placed next to a's nearest neighbour b: as seen from a the two are 4 degrees apart, at nearly equal distances, so
    the reference drops the triplet b--a--c (cos >= 0.99) while neither cos(theta_abc) nor cos(theta_acb) comes near 0.99 -- the one
    term only the own-moments sum is wrong about.  a's requests are declined, and everything matches the oracle."""
    monkeypatch.setenv("MW_MOVE_MOMENTS", "1")
    monkeypatch.setenv("MW_MOVE_CHUNK", "64")
    from mc_water_ls_mw_amd.energy import load_boxes
    bx = _Boxes(c_oracle, (4, 3, 3), 1, 6300)
    x, iv = bx.xs[0].copy(), bx.iv
    nn, jn, vn = bx.lists[0]
    a = 100
    dab, b = min((np.linalg.norm(x[jn[a, s] - 1] - x[a]), jn[a, s] - 1) for s in range(nn[a]) if vn[a, s] == 1)
    c = next(k for k in range(len(x)) if k not in (a, b) and np.linalg.norm(x[k] - x[a]) > 15.0)
    u = (x[b] - x[a]) / dab
    w = np.cross(u, [0.3, -0.5, 0.8]); w /= np.linalg.norm(w)
    th = np.deg2rad(4.0)
    x[c] = x[a] + 1.02 * dab * (np.cos(th) * u + np.sin(th) * w)
    lists = c_oracle.neighbours(x, iv)
    rng = np.random.default_rng(6)
    imol = np.concatenate([[a + 1, a + 1], rng.integers(1, len(x) + 1, 120)]).astype(np.int32)
    trial = x[imol - 1] + rng.normal(0.0, 0.4, (len(imol), 3))
    trial[0] = x[a]                                                      # (a unmoved, and a moved by less than the pair's width)
    trial[1] = x[a] + np.array([0.01, 0.02, -0.01])
    p = predict(c_oracle, x, iv, *lists, imol, trial)
    print("declined", np.flatnonzero(p["declined"]), "jik", np.flatnonzero(p["jik"]), "ijk", np.flatnonzero(p["ijk"]), "margin", p["margin"].min())
    assert p["jik"][0] and p["jik"][1] and not p["ijk"][0] and not p["ijk"][1] and not p["cap"].any()
    assert p["margin"].min() > 1e-6
    ro, rn = c_oracle.trial_moves(imol, trial, x, iv, *lists)
    ref = request_counts(c_oracle, x, iv, *lists, imol, trial)[0]
    em = load_boxes([bx.h], [x])
    try:
        eo, en, cnt, d = _ask(em, 3, 1, imol, trial)
        assert d["declined"] == int(p["declined"].sum()) and d["declined"] >= 2
        _check(eo, en, ro, rn, 3)
        assert cnt == _want(ref, 3)
        assert abs(en[0] - eo[0]) <= DE_ATOL
    finally:
        em.energy_deinit()
