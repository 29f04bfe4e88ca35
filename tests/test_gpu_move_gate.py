"""GPU: THE GATE in front of the 0.99 rule of the move kernel's moment path (mode bit 7 of k_move_energy, mw_move_lanes.hip.h;
MW_MOVE_GATE=0 enters the angle block for every pair with |ab| < rc, as before).  The gate only chooses for which pairs the
unchanged angle tests run, and it passes every pair they can find hard (tests/test_move_gate_ref.py), so the switch may change
nothing: energies byte-identical with it off, counts and the number declined equal.  What the gate adds that can go wrong is a
dropped triplet it does not pass -- the request would be served with a term the reference drops -- so every kind of dropped triplet
is built here, hard at the old position only and at the trial position only (the gate tests both positions in either lane), in
the lane's own pair and in its partner's (b - a - 1 even and odd in the queue), with a the queue's first entry and its last but
one; and one triplet's angle is swept across the threshold.  Energies against the C oracle at RTOL / DE_ATOL of conftest.py,
counts exact (tests/move_counts_ref.py), the declined requests predicted on the host (tests/move_lanes_ref.py); every launch
must be build 3."""
import numpy as np
import pytest

from move_counts_ref import request_counts
from move_gate_ref import rule_drops
from move_lanes_ref import CAP, COS_MAX, predict
from test_gpu_moment_store import _Boxes
from test_gpu_move_sorted import _Fill, _ask, _check, _same, _want

pytestmark = pytest.mark.gpu

KINDS = ("aPb", "Pab", "Pba")                # the vertex of the small angle: the request's own position, the pair's first entry, its second
PROPS = [("where", "old"), ("where", "trial"), ("parity", 0), ("parity", 1), ("a", "first"), ("a", "last but one")]


def _env(monkeypatch, chunk, gate):
    monkeypatch.setenv("MW_MOVE_MOMENTS", "1")
    monkeypatch.setenv("MW_MOVE_CHUNK", str(chunk))
    for name in ("MW_MOVE_SORT", "MW_MOVE_MASKS", "MW_MOVE_COUNTS"):
        monkeypatch.delenv(name, raising=False)
    if gate:
        monkeypatch.delenv("MW_MOVE_GATE", raising=False)                      # (the default is on)
    else:
        monkeypatch.setenv("MW_MOVE_GATE", "0")


@pytest.fixture(scope="module")
def fill(c_oracle):
    return _Fill(c_oracle)


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("chunk", [64, 2048])
def test_same_bits_with_and_without_the_gate(fill, monkeypatch, chunk, mode):
    """The ten-box fill of test_gpu_move_sorted.py in items of 64 (groups that scan, groups that walk the masks) and of 2048.
    Nothing of it is declined -- the declined list is empty with the gate and without."""
    got = {}
    for gate in (True, False):
        _env(monkeypatch, chunk, gate)
        em = fill.boxes.engine()
        try:
            got[gate] = _ask(em, mode, fill.ils, fill.imol, fill.trial, chunk)
        finally:
            em.energy_deinit()
    print("chunk", chunk, "mode", mode, "declined", got[True][3], got[False][3], "counts", got[True][2])
    assert _same(got[True][0], got[False][0]) and _same(got[True][1], got[False][1])
    assert got[True][2] == got[False][2] and got[True][3] == got[False][3]
    for gate in (True, False):
        _check(got[gate][0], got[gate][1], fill.ro, fill.rn, mode)
        assert got[gate][2] == _want(fill.ref, mode)
    assert fill.declined == 0 and got[True][3] == 0


# ---- constructed triplets --------------------------------------------------------------------------------------------------------

RC = [0.0]                                   # the cutoff, set by _rc (bohr)


def _rc(oracle):
    c = oracle.constants()
    RC[0] = c[0] * c[6]
    return RC[0]


def _unit(v):
    return v / np.linalg.norm(v)


def _queue(x, iv, lists, i, p_old, p_new, rc):
    """(molecules, images, image positions) of what request (i, p_old, p_new) queues: the row's entries in range of either, in row order."""
    nn, jn, vn = lists
    n = int(nn[i])
    j, v = jn[i, :n] - 1, vn[i, :n] - 1
    q = x[j] + iv[v]
    inr = (np.linalg.norm(q - p_old, axis=1) < rc) | (np.linalg.norm(q - p_new, axis=1) < rc)
    return j[inr], v[inr], q[inr]


def _hard_pairs(q, p, rc):
    """The queue's pairs (a, b) the rule drops at position p, and for each the vertex of the small angle."""
    ia, ib = np.triu_indices(len(q), 1)
    out = []
    for a, b in zip(ia[rule_drops(p, q[ia], q[ib], rc)], ib[rule_drops(p, q[ia], q[ib], rc)]):
        A, B, D = q[a] - p, q[b] - p, q[b] - q[a]
        cos = {"aPb": A @ B / np.linalg.norm(A) / np.linalg.norm(B), "Pab": -(A @ D) / np.linalg.norm(A) / np.linalg.norm(D),
               "Pba": B @ D / np.linalg.norm(B) / np.linalg.norm(D)}
        out.append((int(a), int(b), tuple(k for k in KINDS if cos[k] >= COS_MAX)))
    return out


def _place(thin_at_p, p, qn, rc):
    """Where the third molecule goes, given the request's position p and a neighbour at qn.  thin_at_p: next to the neighbour as
    seen from p, 4 degrees off and 2 % farther (test_the_dropped_jik_term: only cos(theta_aPb) is near 1).  Else BEHIND p as seen
    from the neighbour, 5 degrees off the line and within the cutoff of the neighbour: the angle at the neighbour is 5 degrees,
    the one at p is obtuse and the one at the third molecule about 11 degrees.  (Set behind the NEIGHBOUR as seen from p it
    would stand 5 degrees from the neighbour at p as well: two small angles in one triangle, and no telling which test found it.)"""
    L = np.linalg.norm(qn - p)
    u = (qn - p) / L
    w = _unit(np.cross(u, [0.3, -0.5, 0.8]))
    if thin_at_p:
        th = np.deg2rad(4.0)
        return p + 1.02 * L * (np.cos(th) * u + np.sin(th) * w)
    al = np.deg2rad(5.0)
    return qn + min(1.45, 0.93 * rc / L) * L * (-np.cos(al) * u + np.sin(al) * w)


def _props_q(j, q, p_old, p_new, pair):
    """What a request with the queue (molecules j at q) and the two positions IS: (kind, where, parity, place of a) -- or None
    when it does not hold exactly one hard pair, at exactly one of its two positions, of exactly one kind, made of `pair`."""
    if len(j) > CAP:
        return None
    hard = {"old": _hard_pairs(q, p_old, RC[0]), "trial": _hard_pairs(q, p_new, RC[0])}
    where = [k for k in hard if hard[k]]
    if len(where) != 1 or len(hard[where[0]]) != 1:
        return None
    a, b, kinds = hard[where[0]][0]
    if len(kinds) != 1 or {int(j[a]), int(j[b])} != set(pair):
        return None
    return kinds[0], where[0], (b - a - 1) % 2, "first" if a == 0 else "last but one" if a == len(j) - 2 else "inside"


def _props_of(x, iv, lists, case, rc):
    """The same of a constructed case, from the lists of the final positions (every queue entry in the cell itself)."""
    i, trial = case["i"], case["trial"]
    j, v, q = _queue(x, iv, lists, i, x[i], trial, rc)
    if np.any(v != 0) or i in j:
        return None
    return _props_q(j, q, x[i], trial, (case["n"], case["c"]))


class _Triplets:
    """Four 288-molecule boxes, in each up to four molecules taken from elsewhere and set down beside a request's molecule so that
    the request owns ONE triplet the reference drops; found by a seeded search until every kind has been built hard at the old
    position only, at the trial position only, with b - a - 1 even and odd, with a the queue's first entry and its last but one.
    Every box carries 38 requests (the built ones, the rest random), so an item of 64 counts, sorts and walks its masks.  Computed
    once, never changed."""

    NBOX, PER_BOX, NREQ = 4, 4, 38

    def __init__(self, oracle):
        self.rc = rc = _rc(oracle)
        bx = _Boxes(oracle, (4, 3, 3), self.NBOX, 6400)
        self.h, self.iv = bx.h, bx.iv
        assert np.all(self.iv[0] == 0.0)                                       # (image 1 is the cell itself)
        xs = [x.copy() for x in bx.xs]
        lists = list(bx.lists)
        cases = [[] for _ in xs]
        taken = [set() for _ in xs]
        need = {(k, *p) for k in KINDS for p in PROPS}
        rng = np.random.default_rng(77)
        ang = 1.0 / 0.5291772108
        for attempt in range(4000):
            if not need:
                break
            b = attempt % self.NBOX
            if len(cases[b]) == self.PER_BOX:
                continue
            x = xs[b]
            i = int(rng.integers(len(x)))
            mine = [i] + [c["i"] for c in cases[b]]
            if i in taken[b] or np.any(lists[b][2][i, :lists[b][0][i]] != 1) or any(np.linalg.norm(x[i] - x[m]) < 16.0 for m in mine[1:]):
                continue
            thin_at_p = any(k[0] == "aPb" for k in need) and (rng.random() < 0.6 or all(k[0] == "aPb" for k in need))
            where = ("old", "trial")[int(rng.integers(2))]
            trial = x[i] + _unit(rng.normal(size=3)) * rng.uniform(0.6, 1.0) * ang
            p = x[i] if where == "old" else trial
            j, v, q = _queue(x, self.iv, lists[b], i, x[i], trial, rc)
            # the neighbour: in range of p; for a triplet thin at p one that the other position has out of range (two molecules 4
            # degrees apart at equal distances are 4 degrees apart from anywhere near), else one of the first shell
            dp, do = np.linalg.norm(q - p, axis=1), np.linalg.norm(q - (trial if where == "old" else x[i]), axis=1)
            ok = np.flatnonzero((dp < 0.975 * rc) & (do > 1.005 * rc) if thin_at_p else dp < 3.3 * ang)
            if len(ok) == 0:
                continue
            s = int(rng.choice(ok))
            if any(k[2] == "last but one" for k in need) and len(j) - 1 in ok and rng.random() < 0.5:
                s = len(j) - 1                                                  # (the pair is to be the queue's last two entries)
            far = np.flatnonzero(np.min([np.linalg.norm(x - x[m], axis=1) for m in mine], axis=0) > 15.0)
            far = [int(k) for k in far if k not in taken[b]]
            # (rows are in the order of the molecules' numbers: a low or a high number puts the third molecule at an end of the queue)
            c = int(rng.choice(far[:6] + far[-6:] + [int(k) for k in rng.choice(far, 6)] + [k for k in far if len(j) > 1 and j[-2] < k < j[-1]][:6]))
            at = _place(thin_at_p, p, q[s], rc)
            cand = {"i": i, "trial": trial, "n": int(j[s]), "c": c}
            # first on the queue as it will be -- the third molecule in its place by number -- and only then on rebuilt lists
            keep = j != c
            j2, q2 = np.append(j[keep], c), np.vstack([q[keep], at])
            order = np.argsort(j2, kind="stable")
            got = _props_q(j2[order], q2[order], x[i], trial, (cand["n"], c))
            if got is None or not {(got[0], "where", got[1]), (got[0], "parity", got[2]), (got[0], "a", got[3])} & need:
                continue
            x2 = x.copy()
            x2[c] = at
            l2 = oracle.neighbours(x2, self.iv)
            got = _props_of(x2, self.iv, l2, cand, rc)
            if got is None or any(_props_of(x2, self.iv, l2, e, rc) is None for e in cases[b]):
                continue
            new = {(got[0], "where", got[1]), (got[0], "parity", got[2]), (got[0], "a", got[3])} & need
            if not new:
                continue
            need -= new
            xs[b], lists[b] = x2, l2
            cases[b].append(cand)
            taken[b] |= {i, c, cand["n"]}
        self.left = need
        self.xs, self.lists, self.cases = xs, lists, cases
        self.props = [[_props_of(x, self.iv, l, c, rc) for c in cs] for x, l, cs in zip(xs, lists, cases)]
        self.req = []
        for b, (x, l, cs) in enumerate(zip(xs, lists, cases)):
            nf = self.NREQ - len(cs)
            imol = np.concatenate([[c["i"] + 1 for c in cs], rng.integers(1, len(x) + 1, nf)]).astype(np.int32)
            trial = x[imol - 1] + rng.normal(0.0, 0.4, (len(imol), 3))
            for k, c in enumerate(cs):
                trial[k] = c["trial"]
            p = predict(oracle, x, self.iv, *l, imol, trial)
            ro, rn = oracle.trial_moves(imol, trial, x, self.iv, *l)
            ref = request_counts(oracle, x, self.iv, *l, imol, trial)[0]
            self.req.append((imol, trial, p, ro, rn, ref))

    def engine(self):
        from mc_water_ls_mw_amd.energy import load_boxes
        return load_boxes([self.h] * len(self.xs), self.xs)


@pytest.fixture(scope="module")
def triplets(c_oracle):
    return _Triplets(c_oracle)


def test_every_kind_of_dropped_triplet_is_built(triplets):
    """(No launch: what the search found, on the final positions.)"""
    built = [p for ps in triplets.props for p in ps]
    for b, ps in enumerate(triplets.props):
        print("box", b, ps)
    assert not triplets.left and all(p is not None for p in built)
    for kind in KINDS:
        mine = [p for p in built if p[0] == kind]
        assert {p[1] for p in mine} == {"old", "trial"} and {p[2] for p in mine} == {0, 1}
        assert {"first", "last but one"} <= {p[3] for p in mine}
    for (imol, trial, p, ro, rn, ref), cs, ps in zip(triplets.req, triplets.cases, triplets.props):
        assert p["margin"].min() > 1e-6 and not p["cap"].any() and not p["self"].any()
        for k, got in enumerate(ps):                                            # (the request of a built case is declined for the built reason alone)
            assert p["declined"][k] and bool(p["jik"][k]) == (got[0] == "aPb") and bool(p["ijk"][k]) == (got[0] != "aPb")


@pytest.mark.parametrize("gate", [True, False])
def test_the_dropped_triplets_are_declined(triplets, monkeypatch, gate):
    """Box by box (an item of 38 requests), then all four at once: the number declined is the prediction's, and every energy and
    count the oracle's -- a request served with a dropped term would miss the oracle by that term."""
    _env(monkeypatch, 64, gate)
    em = triplets.engine()
    try:
        for b, (imol, trial, p, ro, rn, ref) in enumerate(triplets.req):
            assert p["margin"].min() > 1e-6
            eo, en, c, declined = _ask(em, 3, b + 1, imol, trial, 64)
            print("gate", gate, "box", b, "declined", declined, "predicted", int(p["declined"].sum()), "built", len(triplets.cases[b]))
            assert declined == int(p["declined"].sum()) and declined >= len(triplets.cases[b])
            _check(eo, en, ro, rn, 3)
            assert c == _want(ref, 3)
        cat = lambda k: np.concatenate([r[k] for r in triplets.req])             # noqa: E731
        ils = np.concatenate([np.full(len(r[0]), b + 1, dtype=np.int32) for b, r in enumerate(triplets.req)])
        assert 120 <= len(ils) <= 160
        for mode in (1, 2, 3):
            eo, en, c, declined = _ask(em, mode, ils, cat(0), cat(1), 64)
            _check(eo, en, cat(3), cat(4), mode)
            assert c == _want(cat(5), mode)
            if mode != 1:                                                       # (mode 1 applies the rule at the old position alone)
                assert declined == sum(int(r[2]["declined"].sum()) for r in triplets.req)
    finally:
        em.energy_deinit()


class _Sweep:
    """Ten copies of one box, in copy k a molecule set down beside a's nearest neighbour so that cos(theta) as seen from a is
    0.985 + k * 0.01 / 9 (arms of L and 1.02 L, as test_the_dropped_jik_term): below 0.99 - 1e-9 in copies 0 to 4, above it in
    5 to 9.  a's request comes with thirteen random ones per box."""

    COS = np.linspace(0.985, 0.995, 10)

    def __init__(self, oracle):
        bx = _Boxes(oracle, (4, 3, 3), 1, 6500)
        self.h, self.iv = bx.h, bx.iv
        x0 = bx.xs[0]
        nn, jn, vn = bx.lists[0]
        a = 100
        dab, b = min((np.linalg.norm(x0[jn[a, s] - 1] - x0[a]), jn[a, s] - 1) for s in range(nn[a]) if vn[a, s] == 1)
        c = next(k for k in range(len(x0)) if k not in (a, b) and np.linalg.norm(x0[k] - x0[a]) > 15.0)
        u = (x0[b] - x0[a]) / dab
        w = _unit(np.cross(u, [0.3, -0.5, 0.8]))
        rng = np.random.default_rng(9)
        self.xs, self.req = [], []
        for cos in self.COS:
            x = x0.copy()
            x[c] = x[a] + 1.02 * dab * (cos * u + np.sqrt(1.0 - cos * cos) * w)
            lists = oracle.neighbours(x, self.iv)
            imol = np.concatenate([[a + 1], rng.integers(1, len(x) + 1, 13)]).astype(np.int32)
            trial = x[imol - 1] + rng.normal(0.0, 0.4, (len(imol), 3))
            trial[0] = x[a] + np.array([0.01, 0.02, -0.01])                    # (moved by less than the pair's width: hard at both positions or at neither)
            p = predict(oracle, x, self.iv, *lists, imol, trial)
            ro, rn = oracle.trial_moves(imol, trial, x, self.iv, *lists)
            ref = request_counts(oracle, x, self.iv, *lists, imol, trial)[0]
            self.xs.append(x)
            self.req.append((imol, trial, p, ro, rn, ref))


@pytest.fixture(scope="module")
def sweep(c_oracle):
    return _Sweep(c_oracle)


@pytest.mark.parametrize("gate", [True, False])
def test_one_angle_swept_across_the_threshold(sweep, monkeypatch, gate):
    from mc_water_ls_mw_amd.energy import load_boxes
    _env(monkeypatch, 64, gate)
    outcome = [bool(r[2]["declined"][0]) for r in sweep.req]
    print("cos", sweep.COS, "a's request declined", outcome, "margins", [float(r[2]["margin"].min()) for r in sweep.req])
    assert outcome == [bool(c >= COS_MAX) for c in sweep.COS] and True in outcome and False in outcome
    assert 120 <= sum(len(r[0]) for r in sweep.req) <= 160
    em = load_boxes([sweep.h] * len(sweep.xs), sweep.xs)
    try:
        for k, (imol, trial, p, ro, rn, ref) in enumerate(sweep.req):
            assert p["margin"].min() > 1e-6
            assert bool(p["jik"][0]) == outcome[k] and not p["ijk"][0] and not p["cap"][0]
            eo, en, c, declined = _ask(em, 3, k + 1, imol, trial, 64)
            # a's request alone next: the launch declines one request or none, as predicted
            e1 = _ask(em, 3, k + 1, imol[:1].repeat(4), trial[:1].repeat(4, axis=0), 64)
            print("gate", gate, "cos %.6f" % sweep.COS[k], "declined", declined, "predicted", int(p["declined"].sum()), "a's request four times", e1[3])
            assert declined == int(p["declined"].sum())
            assert e1[3] == (4 if outcome[k] else 0)
            _check(eo, en, ro, rn, 3)
            assert c == _want(ref, 3)
            if not outcome[k]:                                                  # (served: a request's bits are its own)
                assert np.all(e1[0] == eo[0]) and np.all(e1[1] == en[0])
    finally:
        em.energy_deinit()
