"""GPU: the request loop of k_move_energy.  What a request brings from global memory (row entry, trial position, output slot) is
asked for one request ahead with vector loads and carried to that request's turn.  Held here, on 288-molecule ice Ih boxes (the
smallest the moment path takes): a wavefront that serves no request, one, two, three or many; output slots that are no identity;
requests that decline placed first, last and doubled in a box's list of requests; the two builds that share the loop without the moment path.  Energies to the C
oracle (RTOL, DE_ATOL of conftest), counts exact (tests/move_counts_ref.py)."""
import numpy as np
import pytest

from conftest import DE_ATOL, RTOL
from move_counts_ref import request_counts
from test_gpu_moment_store import _Boxes

pytestmark = pytest.mark.gpu

PER_BOX = (1, 15, 16, 17, 31, 32, 33, 47, 200)     # 16 wavefronts per item: none, one, two, three or many requests each


class _Mix:
    """Boxes, `per_box[b]` requests to box b uploaded in an order that interleaves the boxes, and what the oracle makes of them
    (computed once, never changed).  `first[b]`, `last[b]`: molecules (1-based) whose unmoved requests open and close box b's run."""

    def __init__(self, oracle, per_box, seed, xs=None, first=None, last=None):
        self.boxes = _Boxes(oracle, (4, 3, 3), len(per_box), 7300)
        b = self.boxes
        if xs is not None:
            b.xs = xs
            b.lists = [oracle.neighbours(x, b.iv) for x in xs]
        rng = np.random.default_rng(seed)
        ils, imol, trial, eo, en, ref = [], [], [], [], [], []
        for k, (x, l, n) in enumerate(zip(b.xs, b.lists, per_box)):
            i = rng.integers(1, b.n + 1, n).astype(np.int32)
            t = x[i - 1] + rng.normal(0.0, 0.4, (n, 3))
            if first is not None:
                m = np.asarray(first[k], dtype=np.int32)
                i[:len(m)] = m
                t[:len(m)] = x[m - 1]                                       # (unmoved: old == new)
            if last is not None:
                m = np.asarray(last[k], dtype=np.int32)
                i[n - len(m):] = m
                t[n - len(m):] = x[m - 1]
            o, nw = oracle.trial_moves(i, t, x, b.iv, *l)
            ils.append(np.full(n, k + 1, dtype=np.int32)); imol.append(i); trial.append(t); eo.append(o); en.append(nw)
            ref.append(request_counts(oracle, x, b.iv, *l, i, t)[0])
        cat = [np.concatenate(a) for a in (ils, imol, trial, eo, en, ref)]
        # the caller's order: the boxes interleaved by a fixed shuffle of their labels, so perm[] is no identity; each box's own
        # requests keep the order built above (the upload sorts by box, stably)
        labels = np.repeat(np.arange(len(per_box)), per_box)
        np.random.default_rng(seed + 1).shuffle(labels)
        nxt = np.concatenate(([0], np.cumsum(per_box)[:-1]))
        order = np.empty(len(labels), dtype=np.int64)
        for pos, lb in enumerate(labels):
            order[pos] = nxt[lb]
            nxt[lb] += 1
        self.ils, self.imol, self.trial, self.eo, self.en, self.ref = (a[order] for a in cat)
        assert np.any(np.diff(self.ils) < 0)
        self.totals = tuple(int(v) for v in self.ref.sum(axis=0))

    def engine(self, monkeypatch, chunk=None, moments="1"):
        monkeypatch.setenv("MW_MOVE_MOMENTS", moments)
        monkeypatch.delenv("MW_MOVE_COUNTS", raising=False)
        if chunk is None:
            monkeypatch.delenv("MW_MOVE_CHUNK", raising=False)
        else:
            monkeypatch.setenv("MW_MOVE_CHUNK", str(chunk))
        return self.boxes.engine()

    def check(self, eo=None, en=None):
        if eo is not None:
            print("max rel err e_old", np.max(np.abs(eo - self.eo) / np.abs(self.eo)))
            assert np.all(np.abs(eo - self.eo) <= RTOL * np.abs(self.eo))
        if en is not None:
            print("max rel err e_new", np.max(np.abs(en - self.en) / np.abs(self.en)))
            assert np.all(np.abs(en - self.en) <= RTOL * np.abs(self.en) + 1e-14)
        if eo is not None and en is not None:
            assert np.all(np.abs((en - eo) - (self.en - self.eo)) <= DE_ATOL)

    def four_ways(self, em, nbox, want_dispatch):
        """step_launch, moves_launch, local_energy_batch without and with a trial: energies and counts against the oracle."""
        em.moves_upload(self.ils, self.imol, self.trial)
        for launch in (lambda: em.step_launch(1, nbox), em.moves_launch):
            launch()
            want_dispatch(em.last_dispatch("moves"))
            eo, en = em.moves_fetch()
            self.check(eo, en)
            c = em.moves_counts()
            print("counts", c, "oracle", self.totals)
            assert c == self.totals
        e1 = em.local_energy_batch(self.ils, self.imol)
        want_dispatch(em.last_dispatch("moves"))
        self.check(eo=e1)
        assert em.moves_counts() == (self.totals[0], self.totals[1], 0, 0)
        e2 = em.local_energy_batch(self.ils, self.imol, self.trial)
        want_dispatch(em.last_dispatch("moves"))
        self.check(en=e2)
        assert em.moves_counts() == (0, 0, self.totals[2], self.totals[3])


@pytest.fixture(scope="module")
def mix(c_oracle):
    return _Mix(c_oracle, PER_BOX, 41)


@pytest.mark.parametrize("chunk", [64, 256])
def test_wavefronts_with_no_one_two_three_or_many_requests(mix, monkeypatch, chunk):
    assert sum(PER_BOX) * 2048 >= len(PER_BOX) * 24 * mix.boxes.n           # the LDS rule of mw_moves_upload
    def on_moment_path(d):
        assert d["use_mom"] == 1 and d["build"] == 3 and d["mchunk"] == chunk
        assert d["items"] == (len(PER_BOX) + 3 if chunk == 64 else len(PER_BOX))       # 200 requests: four items of 50
    em = mix.engine(monkeypatch, chunk)
    try:
        mix.four_ways(em, len(PER_BOX), on_moment_path)
    finally:
        em.energy_deinit()


def _declining_boxes(oracle):
    """Three copies of one box in which molecule c sits almost behind a's neighbour b as seen from a (the construction of
    test_declined_requests_are_counted_by_the_fallback_alone), and the molecules whose unmoved requests open and close each box's
    LIST of requests: a, b, c doubled, rotated from box to box, so that each of them is some box's first and some box's last request,
    follows itself, and stands next to requests that are served.  (Which wavefront draws which request is decided at run time: the
    first sixteen of an item go to its sixteen wavefronts, the rest to whoever is free -- where a declined request falls within a
    wavefront's own run is not pinned, only that declined and served requests meet in every order the list can give.)"""
    base = _Boxes(oracle, (4, 3, 3), 3, 7300)
    x = base.xs[0].copy()
    nn, jn, vn = base.lists[0]
    a = 100
    dab, b = min((np.linalg.norm(x[jn[a, s] - 1] - x[a]), jn[a, s] - 1) for s in range(nn[a]) if vn[a, s] == 1)
    c = next(k for k in range(len(x)) if k not in (a, b) and np.linalg.norm(x[k] - x[a]) > 15.0)
    x[c] = x[a] + 1.45 * (x[b] - x[a]) + np.array([0.02, -0.01, 0.015])
    abc = [a + 1, b + 1, c + 1]
    rot = [abc[k:] + abc[:k] for k in range(3)]
    first = [[m for m in r for _ in (0, 1)] for r in rot]
    last = [[m for m in r[::-1] for _ in (0, 1)] for r in rot]
    return [x, x.copy(), x.copy()], first, last


def test_requests_declined_first_last_and_doubled_in_a_box(c_oracle, monkeypatch):
    xs, first, last = _declining_boxes(c_oracle)
    case = _Mix(c_oracle, (40, 23, 64), 43, xs=xs, first=first, last=last)
    em = case.engine(monkeypatch, 64)
    try:
        em.moves_upload(case.ils, case.imol, case.trial)
        runs = []
        for _ in range(2):                                                  # the declined list's two count words in turn
            em.step_launch(1, 3)
            d = em.last_dispatch("moves")
            assert d["use_mom"] == 1 and d["build"] == 3
            eo, en = em.moves_fetch()
            counts = em.moves_counts()
            runs.append((eo, en, counts, em.last_dispatch("moves")["declined"]))
        print("declined", runs[0][3], "counts", runs[0][2], "oracle", case.totals)
        assert 1 <= runs[0][3] < len(case.imol)
        case.check(runs[0][0], runs[0][1])
        assert runs[0][2] == case.totals
        assert runs[1][3] == runs[0][3] and runs[1][2] == runs[0][2]
        assert np.array_equal(runs[1][0], runs[0][0]) and np.array_equal(runs[1][1], runs[0][1])
    finally:
        em.energy_deinit()


def test_the_scan_path_shares_the_loop(mix, monkeypatch):
    def on_scan_path(d):
        assert d["use_mom"] == 0 and d["build"] == 2 and d["mlds"] == 1
    em = mix.engine(monkeypatch, 64, moments="0")
    try:
        mix.four_ways(em, len(PER_BOX), on_scan_path)
    finally:
        em.energy_deinit()


def test_boxes_gathered_from_global_memory_share_the_loop(c_oracle, monkeypatch):
    """Two requests in each of four boxes fail the LDS rule: the build without staging, whose items hold one request per
    wavefront and hand out nothing."""
    case = _Mix(c_oracle, (2, 2, 2, 2), 47)
    assert 8 * 2048 < 4 * 24 * case.boxes.n

    def unstaged(d):
        assert d["mlds"] == 0 and d["use_mom"] == 0 and d["build"] == 0
    em = case.engine(monkeypatch)
    try:
        case.four_ways(em, 4, unstaged)
    finally:
        em.energy_deinit()
