"""GPU: THE F32 PAIR GATE in front of the 0.99 rule's pair pass (mode bit 8 of k_move_energy, lanes_pairs32 of mw_move_lanes.hip.h;
MW_MOVE_PAIRS32=0 sends every row of a walking group's queues through the float64 pair loop, as before).  The float32 pass only
chooses which rows that unchanged loop serves, and it names every row holding a pair the rule drops (tests/test_move_pairs32_ref.py),
so the switch may change nothing: energies byte-identical with it off, counts and the number declined equal.  What it adds that can
go wrong is a dropped triplet in a row it does not name, so every kind of dropped triplet is built here with the pass on -- the
triplets of test_gpu_move_gate.py, and in a dilute box queues of every shape the unrolled (a, c) triangle has an edge for: one
pair, odd and even lengths, all sixteen entries, a and b owned by either lane of the pair, empty and one-entry queues beside them,
a group of mixed lengths and a short last group -- one triplet's angle is swept across 0.99, and one pair's |ab| across the cutoff
within float32 rounding.  Energies against the C oracle at RTOL / DE_ATOL of conftest.py, counts exact, the declined requests
predicted on the host (tests/move_lanes_ref.py); every launch must be build 3."""
import numpy as np
import pytest

from move_counts_ref import request_counts
from move_lanes_ref import CAP, COS_MAX, predict
from test_gpu_move_gate import _Sweep, _Triplets, _hard_pairs, _queue, _unit
from test_gpu_move_sorted import _Fill, _ask, _check, _same, _want

pytestmark = pytest.mark.gpu


def _env(monkeypatch, chunk, pairs32):
    monkeypatch.setenv("MW_MOVE_MOMENTS", "1")
    monkeypatch.setenv("MW_MOVE_CHUNK", str(chunk))
    for name in ("MW_MOVE_SORT", "MW_MOVE_MASKS", "MW_MOVE_COUNTS", "MW_MOVE_GATE"):
        monkeypatch.delenv(name, raising=False)
    if pairs32:
        monkeypatch.delenv("MW_MOVE_PAIRS32", raising=False)                   # (the default is on)
    else:
        monkeypatch.setenv("MW_MOVE_PAIRS32", "0")


@pytest.fixture(scope="module")
def fill(c_oracle):
    return _Fill(c_oracle)


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("chunk", [64, 2048])
def test_same_bits_with_and_without_the_f32_pass(fill, monkeypatch, chunk, mode):
    """The ten-box fill of test_gpu_move_sorted.py in items of 64 (groups that scan, groups that walk the masks) and of 2048."""
    got = {}
    for on in (True, False):
        _env(monkeypatch, chunk, on)
        em = fill.boxes.engine()
        try:
            got[on] = _ask(em, mode, fill.ils, fill.imol, fill.trial, chunk)
        finally:
            em.energy_deinit()
    print("chunk", chunk, "mode", mode, "declined", got[True][3], got[False][3], "counts", got[True][2])
    assert _same(got[True][0], got[False][0]) and _same(got[True][1], got[False][1])
    assert got[True][2] == got[False][2] and got[True][3] == got[False][3]
    for on in (True, False):
        _check(got[on][0], got[on][1], fill.ro, fill.rn, mode)
        assert got[on][2] == _want(fill.ref, mode)
    assert fill.declined == 0 and got[True][3] == 0


# ---- the constructed triplets of the gate's test, with the new pass on --------------------------------------------------------------

@pytest.fixture(scope="module")
def triplets(c_oracle):
    return _Triplets(c_oracle)


def test_the_dropped_triplets_are_declined_with_the_f32_pass(triplets, monkeypatch):
    """KINDS x PROPS of test_gpu_move_gate.py (every one built: that module's own test holds it), box by box in items of 38 requests
    and all four boxes at once."""
    assert not triplets.left
    _env(monkeypatch, 64, True)
    em = triplets.engine()
    try:
        for b, (imol, trial, p, ro, rn, ref) in enumerate(triplets.req):
            assert p["margin"].min() > 1e-6
            eo, en, c, declined = _ask(em, 3, b + 1, imol, trial, 64)
            print("box", b, "declined", declined, "predicted", int(p["declined"].sum()), "built", len(triplets.cases[b]))
            assert declined == int(p["declined"].sum()) and declined >= len(triplets.cases[b])
            _check(eo, en, ro, rn, 3)
            assert c == _want(ref, 3)
        cat = lambda k: np.concatenate([r[k] for r in triplets.req])             # noqa: E731
        ils = np.concatenate([np.full(len(r[0]), b + 1, dtype=np.int32) for b, r in enumerate(triplets.req)])
        for mode in (1, 2, 3):
            eo, en, c, declined = _ask(em, mode, ils, cat(0), cat(1), 64)
            _check(eo, en, cat(3), cat(4), mode)
            assert c == _want(cat(5), mode)
            if mode != 1:
                assert declined == sum(int(r[2]["declined"].sum()) for r in triplets.req)
    finally:
        em.energy_deinit()


# ---- queues of every shape, in a dilute box ------------------------------------------------------------------------------------------

SCALE = 1.7                                  # of the ice cell: nearest neighbours at 8.5 to 9.1 bohr, between the cutoff (8.14) and the list's range (9.6)


def _apart(h, x, k, others):
    """The smallest minimum-image distance from molecule k to the molecules `others`."""
    if not len(others):
        return np.inf
    f = np.linalg.solve(np.asarray(h).reshape(3, 3).T, (x[others] - x[k]).T).T
    return float(np.min(np.linalg.norm((f - np.round(f)) @ np.asarray(h).reshape(3, 3), axis=1)))


def _sphere(n):
    """n directions spread over the sphere (a Fibonacci spiral): neighbours are more than 40 degrees apart for n <= 16."""
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    ph = np.pi * (1.0 + 5.0 ** 0.5) * k
    s = np.sqrt(1.0 - z * z)
    return np.stack([s * np.cos(ph), s * np.sin(ph), z], axis=1)


#: (queue length, the queue places (a, b) of the pair that forms a dropped triplet, or None): one pair; odd and even lengths; a and
#: b in the even lane's registers and in the odd lane's, in every combination; the last register of both lanes; a full queue served
SHAPES = [(0, None), (1, None), (2, (0, 1)), (2, None), (3, (1, 2)), (4, (1, 3)), (5, (0, 4)), (7, (2, 5)), (9, (3, 8)),
          (16, (14, 15)), (16, (0, 15)), (16, (13, 14)), (15, (12, 14)), (16, None), (15, None)]


class _Shapes:
    """One 288-molecule ice Ih cell blown up by SCALE -- every row has entries, none of them in range -- in which the centre of every
    shape of SHAPES gets its queue set down around it on a sphere of 0.7 to 0.8 rc, by molecules taken from elsewhere: rows are in the
    order of the molecules' numbers, so the molecules' numbers choose the places in the queue.  The dropped triplet is thin at the
    centre (4 degrees, the second arm 2 % longer: test_gpu_move_gate._place).  40 requests: the centres, then molecules that
    stayed alone (empty queues), so the one item sorts, walks its masks, and has a group of 32 of mixed lengths and a last group of 8.
    Computed once, never changed."""

    NREQ = 40

    def __init__(self, oracle):
        from mc_water_ls_mw_amd import lattice as lat
        c = oracle.constants()
        self.rc = rc = c[0] * c[6]
        h, x0 = lat.ice_box("ih", (4, 3, 3))
        self.h, x = SCALE * np.asarray(h), SCALE * lat.thermalise(x0, 0.02, 321)
        self.iv = oracle.ivects(self.h)
        n = len(x)
        rng = np.random.default_rng(5)
        centres = []                                                           # (no centre's queue in range of another centre)
        for k in rng.permutation(n):
            if len(centres) < len(SHAPES) and _apart(self.h, x, int(k), centres) > 2.2 * rc:
                centres.append(int(k))
        assert len(centres) == len(SHAPES)
        donors = [k for k in range(n) if _apart(self.h, x, k, centres) > 1.2 * rc]   # (a centre keeps its lattice neighbours: a row of four, none in range)
        # a centre's queue takes molecules whose numbers ascend with the place in the queue: the next free donors, in order
        free = iter(sorted(rng.choice(donors, sum(s[0] for s in SHAPES), replace=False).tolist()))
        self.moved = set()
        self.pairs = []
        for ctr, (nq, pair) in zip(centres, SHAPES):
            mine = [next(free) for _ in range(nq)]
            dirs = _sphere(max(nq, 1))[rng.permutation(nq)] if nq else np.zeros((0, 3))
            rad = rng.uniform(0.70, 0.80, nq) * rc
            for k, m in enumerate(mine):
                x[m] = x[ctr] + rad[k] * dirs[k]
            if pair is not None:
                a, b = pair
                u = dirs[a]
                w = _unit(np.cross(u, [0.3, -0.5, 0.8]))
                th = np.deg2rad(4.0)
                x[mine[b]] = x[ctr] + 1.02 * rad[a] * (np.cos(th) * u + np.sin(th) * w)
            self.moved |= set(mine)
            self.pairs.append(pair)
        # donors were drawn in ascending order over all centres: within one centre ascending too, which is what the places need
        self.x = x
        self.lists = oracle.neighbours(x, self.iv)
        alone = [k for k in donors if k not in self.moved and self.lists[0][k] > 0 and _apart(self.h, x, k, sorted(self.moved)) > 1.3 * rc][:self.NREQ - len(centres)]
        assert len(alone) == self.NREQ - len(centres)
        self.imol = np.array([k + 1 for k in centres + alone], dtype=np.int32)
        self.trial = x[self.imol - 1] + rng.normal(0.0, 0.02, (len(self.imol), 3))
        self.p = predict(oracle, x, self.iv, *self.lists, self.imol, self.trial)
        self.ro, self.rn = oracle.trial_moves(self.imol, self.trial, x, self.iv, *self.lists)
        self.ref = request_counts(oracle, x, self.iv, *self.lists, self.imol, self.trial)[0]
        self.centres = centres


@pytest.fixture(scope="module")
def shapes(c_oracle):
    return _Shapes(c_oracle)


def test_the_queue_shapes_are_built(shapes):
    """(No launch.)  Every centre queues what SHAPES says, its dropped pair sits at the places SHAPES names and is the only one, and
    the other requests queue nothing."""
    p = shapes.p
    assert p["margin"].min() > 1e-6 and not p["cap"].any() and not p["self"].any()
    assert list(p["union"][:len(SHAPES)]) == [s[0] for s in SHAPES] and not p["union"][len(SHAPES):].any()
    assert list(p["n_old"]) == list(p["union"]) and list(p["n_new"]) == list(p["union"])
    for k, (ctr, (nq, pair)) in enumerate(zip(shapes.centres, SHAPES)):
        j, v, q = _queue(shapes.x, shapes.iv, shapes.lists, ctr, shapes.x[ctr], shapes.trial[k], shapes.rc)
        assert len(j) == nq <= CAP
        hard = [_hard_pairs(q, pos, shapes.rc) for pos in (shapes.x[ctr], shapes.trial[k])]
        want = [] if pair is None else [(pair[0], pair[1], ("aPb",))]
        assert hard[0] == want and hard[1] == want, (k, hard)
        assert bool(p["declined"][k]) == (pair is not None)
    built = [s[1] for s in SHAPES if s[1] is not None]
    assert {(a % 2, b % 2) for a, b in built} == {(0, 0), (0, 1), (1, 0), (1, 1)}     # a and b in either lane's registers
    assert (2, (0, 1)) in SHAPES and (14, 15) in built and {s[0] % 2 for s in SHAPES} == {0, 1}


@pytest.mark.parametrize("on", [True, False])
def test_the_queue_shapes(shapes, monkeypatch, on):
    """The 40 requests as one item (a group of 32 of mixed lengths and a last group of 8), in modes 1, 2 and 3, then the centres of
    the two-entry queues alone beside empty ones (33 requests: a last group of one)."""
    from mc_water_ls_mw_amd.energy import load_boxes
    _env(monkeypatch, 64, on)
    em = load_boxes([shapes.h], [shapes.x])
    try:
        for mode in (3, 1, 2):
            eo, en, c, declined = _ask(em, mode, 1, shapes.imol, shapes.trial, 64)
            print("f32 pass", on, "mode", mode, "declined", declined, "predicted", int(shapes.p["declined"].sum()))
            assert declined == int(shapes.p["declined"].sum()) == sum(s[1] is not None for s in SHAPES)
            _check(eo, en, shapes.ro, shapes.rn, mode)
            assert c == _want(shapes.ref, mode)
        pick = np.array([2, 3] + list(range(len(SHAPES), len(SHAPES) + 25)) + [0, 1] + [2, 3] * 2)
        assert len(pick) == 33
        eo, en, c, declined = _ask(em, 3, 1, shapes.imol[pick], shapes.trial[pick], 64)
        assert declined == 3
        _check(eo, en, shapes.ro[pick], shapes.rn[pick], 3)
        assert c == _want(shapes.ref[pick], 3)
    finally:
        em.energy_deinit()


# ---- one angle across 0.99 -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sweep(c_oracle):
    return _Sweep(c_oracle)


def test_one_angle_swept_across_the_threshold_both_ways(sweep, monkeypatch):
    """test_gpu_move_gate._Sweep, upwards and downwards: the decline appears at the same copy with the float32 pass on and off."""
    from mc_water_ls_mw_amd.energy import load_boxes
    outcome = [bool(r[2]["declined"][0]) for r in sweep.req]
    assert outcome == [bool(c >= COS_MAX) for c in sweep.COS] and True in outcome and False in outcome
    seen = {}
    for on in (True, False):
        _env(monkeypatch, 64, on)
        em = load_boxes([sweep.h] * len(sweep.xs), sweep.xs)
        try:
            for order in (range(len(sweep.req)), reversed(range(len(sweep.req)))):
                for k in order:
                    imol, trial, p, ro, rn, ref = sweep.req[k]
                    assert p["margin"].min() > 1e-6
                    e1 = _ask(em, 3, k + 1, imol[:1].repeat(33), trial[:1].repeat(33, axis=0), 64)   # (33: an item that sorts and walks)
                    eo, en, c, declined = _ask(em, 3, k + 1, imol, trial, 64)
                    assert e1[3] == (33 if outcome[k] else 0) and declined == int(p["declined"].sum())
                    _check(eo, en, ro, rn, 3)
                    assert c == _want(ref, 3)
                    assert seen.setdefault(k, (eo.tobytes(), en.tobytes(), declined)) == (eo.tobytes(), en.tobytes(), declined)
        finally:
            em.energy_deinit()
    print("cos", sweep.COS, "declined", outcome)


# ---- |ab| across the cutoff ----------------------------------------------------------------------------------------------------------------

class _Cutoff:
    """Copies of the dilute box with ONE triplet: centre P, a at 0.6 rc, and b beyond P as seen from a, 4 degrees off the line a -> P
    at |ab| = rc (1 + d): thin at a, a term the reference drops while |ab| < rc and keeps once it is not.  d runs from -1e-4 over
    steps of 1e-15 around 0 -- a few units in the last place of |ab|^2, as fine as the coordinates' own rounding allows -- to 1e-4:
    past the 1e-5 the float32 pass allows |ab|^2 over rc^2."""

    FINE = [k * 1e-15 for k in range(-6, 7)]
    D = [-1e-4, -2e-6, -1e-7, -1e-9] + FINE + [1e-9, 1e-7, 2e-6, 8e-6, 1.2e-5, 1e-4]

    def __init__(self, oracle):
        from mc_water_ls_mw_amd import lattice as lat
        c = oracle.constants()
        self.rc = rc = c[0] * c[6]
        h, x0 = lat.ice_box("ih", (4, 3, 3))
        self.h, base = SCALE * np.asarray(h), SCALE * lat.thermalise(x0, 0.02, 322)
        self.iv = oracle.ivects(self.h)
        ctr = 140
        far = [k for k in range(len(base)) if _apart(self.h, base, k, [ctr]) > 3.0 * rc]
        ma, mb = far[0], far[-1]
        u = _unit(np.array([0.5, -0.4, 0.76]))
        w = _unit(np.cross(u, [0.3, -0.5, 0.8]))
        th = np.deg2rad(4.0)
        rng = np.random.default_rng(6)
        alone = far[1:33]                                                      # (their rows keep their lattice neighbours: only `far`'s two ends moved)
        self.imol = np.array([ctr + 1] + [k + 1 for k in alone], dtype=np.int32)
        self.xs, self.req = [], []
        for d in self.D:
            x = base.copy()
            x[ma] = x[ctr] + 0.6 * rc * u
            x[mb] = x[ma] - rc * (1.0 + d) * (np.cos(th) * u + np.sin(th) * w)
            lists = oracle.neighbours(x, self.iv)
            trial = x[self.imol - 1] + rng.normal(0.0, 0.02, (len(self.imol), 3))
            trial[0] = x[ctr] + np.array([0.001, 0.002, -0.001])
            p = predict(oracle, x, self.iv, *lists, self.imol, trial)
            ro, rn = oracle.trial_moves(self.imol, trial, x, self.iv, *lists)
            ref = request_counts(oracle, x, self.iv, *lists, self.imol, trial)[0]
            self.xs.append(x)
            self.req.append((trial, p, ro, rn, ref))


@pytest.fixture(scope="module")
def cutoff(c_oracle):
    return _Cutoff(c_oracle)


def test_ab_across_the_cutoff(cutoff, monkeypatch):
    """Declined while inside, served once outside, the same copy by copy with the float32 pass on and off.  Where |d| >= 1e-9 the
    host's float64 prediction decides the copy; on the thirteen fine steps the device's own rounding of |ab|^2 does, so there the
    two runs are held to each other, to one change from declined to served, and -- served -- to the oracle."""
    from mc_water_ls_mw_amd.energy import load_boxes
    got = {}
    for on in (True, False):
        _env(monkeypatch, 64, on)
        em = load_boxes([cutoff.h] * len(cutoff.xs), cutoff.xs)
        try:
            got[on] = [_ask(em, 3, k + 1, cutoff.imol, cutoff.req[k][0], 64) for k in range(len(cutoff.D))]
        finally:
            em.energy_deinit()
    decl = [g[3] for g in got[True]]
    print("d", cutoff.D, "declined", decl, "predicted", [int(r[1]["declined"].sum()) for r in cutoff.req])
    for k, d in enumerate(cutoff.D):
        trial, p, ro, rn, ref = cutoff.req[k]
        assert p["union"][0] == 2 and not p["jik"][0] and not p["cap"][0] and not p["union"][1:].any()
        a, b = got[True][k], got[False][k]
        assert _same(a[0], b[0]) and _same(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]
        assert a[3] in (0, 1)
        if abs(d) >= 1e-9:
            assert a[3] == int(p["declined"].sum()) == (1 if d < 0 else 0)
        if a[3] == int(p["declined"].sum()):                                    # (the oracle drops the term exactly where the host predicts)
            _check(a[0], a[1], ro, rn, 3)
            assert a[2] == _want(ref, 3)
    assert decl == sorted(decl, reverse=True) and decl[0] == 1 and decl[-1] == 0
