"""The contract of the single local-energy call (include/mw_energy.h: mw_local_energy, mw_local_energy_patched,
mw_local_energy_post, mw_local_energy_collect) stated as a plain host ledger plus the C oracle, and seeded request scripts
that hold the engine to it.  Test infrastructure, not product code.

THE LEDGER.  One position array D[b] per box, starting as the uploaded positions.  A call (ils, i, r_i or None, p, r_p or None):
  1. o2 is present iff r_p is given, p >= 1 and p != i; if present D[p] = r_p;
  2. if r_i is given D[i] = r_i;
  3. the answer is COracle.local_energy(i, D[b], iv, nn, jn, vn) on the list made once from the uploaded positions
     (mw_build_neighbours rebuilds it from D on both sides).
`collect` returns the answer of the posted request as of its post; an exclusive entry point leaves D alone, and after it the
full-box energy is COracle.model_energy(D) and the downloaded positions are D bit for bit.

A SCRIPT is plain data: a list of dicts {"op": "patched" | "plain" | "post" | "collect" | "exclusive" | "sleep" | "counts", ...}
(molecules and boxes 1-based, positions as tuples of three floats).  Two replayers: `replay_ledger` (the contract) and
`replay_engine` (the raw ctypes library, em.L.mw_local_energy*).  `compare` holds one against the other.  Run as a program
(`python single_call_ref.py NAME`) this file replays script NAME on the engine and prints the records as JSON with energies
as hex floats: the GPU tests start it once per configuration, because the engine reads its switches once per process.
"""
import ctypes
import hashlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

NSLOTS_MAX = 8            # mail slots of the resident server: box ils goes to slot (ils - 1) % min(nboxes, 8)
#: Every energy a script asks for lies in E_FLOOR <= |E| < E_CEIL (Hartree), so that the plain relative bars apply to every call
#: and nothing needs a mask.  A local energy is a sum of a few thousand pair and triplet terms of either sign whose magnitudes add
#: up to some 0.1 Ha; two correct evaluations that add them in another order differ by a few ulp of THAT (ulp(0.1) = 1.4e-17:
#: some 1e-16 Ha), whatever is left after cancellation.  The tightest bar held here is 1e-12 relative (path against path), which
#: such a difference meets only where |E| >= 1e-4 Ha: the builders redraw a step whose answer falls below ten times that.
E_FLOOR, E_CEIL = 1e-3, 1.0
SINGLE = ("patched", "plain", "post")


# ------------------------------------------------------------------------------------------------------------------
# boxes
# ------------------------------------------------------------------------------------------------------------------
def boxes(name):
    """(h list, xyz list) of a box set: "ic1536" (one thermalised 1536-molecule Ic box: cells at least three list radii wide),
    "pair48" (ic48_t015 / ih48_t020: narrow cells, two-image records), "ten48" (ten 48-molecule boxes: slots shared by 1/9, 2/10)."""
    from conftest import load_golden
    from mc_water_ls_mw_amd import lattice as lat
    if name == "ic1536":
        z = load_golden("ic1536")
        return [np.array(z["h"])], [lat.thermalise(z["xyz"], 0.1, 77)]
    z1, z2 = load_golden("ic48_t015"), load_golden("ih48_t020")
    if name == "pair48":
        return [np.array(z1["h"]), np.array(z2["h"])], [np.array(z1["xyz"]), np.array(z2["xyz"])]
    if name == "ten48":
        hs, xs = [], []
        for k in range(10):
            z = (z1, z2)[k % 2]
            hs.append(np.array(z["h"]))
            xs.append(np.array(z["xyz"]) if k < 2 else lat.thermalise(z["xyz"], 0.03, 900 + k))
        return hs, xs
    raise KeyError(name)


class Geometry:
    """The uploaded boxes with the oracle's image vectors and lists (made once), and who is whose nearest neighbour."""

    def __init__(self, oracle, hs, xs):
        self.oracle = oracle
        self.hs = [np.ascontiguousarray(h, dtype=np.float64) for h in hs]
        self.xs = [np.ascontiguousarray(x, dtype=np.float64) for x in xs]
        self.iv = [oracle.ivects(h) for h in self.hs]
        self.lists = [oracle.neighbours(x, iv) for x, iv in zip(self.xs, self.iv)]
        self.n = len(self.xs[0])

    def nearest(self, b, i, D=None, exclude=()):
        """1-based nearest list neighbour of molecule i (1-based) of box b (0-based) at positions D (default: as uploaded)."""
        x = self.xs[b] if D is None else D
        nn, jn, vn = self.lists[b]
        best = None
        for s in range(nn[i - 1]):
            j = int(jn[i - 1, s])
            if j == i or j in exclude:
                continue
            d = float(np.linalg.norm(x[j - 1] + self.iv[b][vn[i - 1, s] - 1] - x[i - 1]))
            if best is None or d < best[0]:
                best = (d, j)
        return best[1]

    def is_neighbour(self, b, i, j):
        nn, jn, _ = self.lists[b]
        return j in jn[i - 1, :nn[i - 1]]


_GEO = {}


def geometry(name, oracle=None):
    if name not in _GEO:
        if oracle is None:
            from oracle import COracle
            oracle = COracle()
        _GEO[name] = Geometry(oracle, *boxes(name))
    return _GEO[name]


# ------------------------------------------------------------------------------------------------------------------
# the position ledger (no energies: the script builders and the shape counter use it too)
# ------------------------------------------------------------------------------------------------------------------
def overrides(op):
    """[(molecule, position)] a single call commits, in the order the contract applies them (o2, then o1)."""
    out = []
    if op["op"] == "plain":
        return out
    if op.get("rp") is not None and op.get("p", 0) >= 1 and op["p"] != op["i"]:
        out.append((op["p"], op["rp"]))
    if op.get("r") is not None:
        out.append((op["i"], op["r"]))
    return out


def commit(D, op):
    for m, r in overrides(op):
        D[op["ils"] - 1][m - 1] = r


# ------------------------------------------------------------------------------------------------------------------
# script builders
# ------------------------------------------------------------------------------------------------------------------
def _t(v):
    return tuple(float(c) for c in v)


class _Builder:
    """Host-side bookkeeping of a script under construction: D (the ledger's positions) and the molecule asked about last."""

    def __init__(self, geo, seed):
        self.geo, self.rng = geo, np.random.default_rng(seed)
        self.D = [x.copy() for x in geo.xs]
        self.last = [0] * len(geo.xs)
        self.ops = []
        self.old = {}               # box -> where the molecule asked about last was before its trial move (protocol_step)
        self.avoid = set()          # molecules the random picks leave alone
        self.es = []                # the answer of every single call so far
        self.lists = list(geo.lists)    # (mw_build_neighbours rebuilds a box's list from D)

    def pos(self, b, i):
        return _t(self.D[b][i - 1])

    def moved(self, b, i, firm=False):
        """A trial position of molecule i: N(0, 0.4) bohr a component; `firm`: a random direction, 0.3 .. 0.7 bohr long (the
        moves a stale copy of which must show: never a tiny one)."""
        if firm:
            d = self.rng.normal(0.0, 1.0, 3)
            d *= self.rng.uniform(0.3, 0.7) / np.linalg.norm(d)
        else:
            d = self.rng.normal(0.0, 0.4, 3)
        return _t(self.D[b][i - 1] + d)

    def other(self, b, *avoid):
        while True:
            i = int(self.rng.integers(1, self.geo.n + 1))
            if i not in avoid and i not in self.avoid:
                return i

    def with_nearest(self, b):
        """(a, n): a random molecule and its nearest neighbour at the current positions."""
        while True:
            a = self.other(b)
            n = self.geo.nearest(b, a, self.D[b])
            if n not in self.avoid:
                return a, n

    def emit(self, **op):
        self.ops.append(op)
        if op["op"] in SINGLE:
            b = op["ils"] - 1
            commit(self.D, op)
            self.last[b] = op["i"]
            self.es.append(self.geo.oracle.local_energy(op["i"], self.D[b], self.geo.iv[b], *self.lists[b]))
        if op["op"] == "exclusive" and op["kind"] == "build":
            b = op["ils"] - 1
            self.lists[b] = self.geo.oracle.neighbours(self.D[b], self.geo.iv[b])
        return op

    def attempt(self, step, *args, **kw):
        """Run one step of a script (a few ops); if an answer of it falls outside E_FLOOR <= |E| < E_CEIL, take the step back and
        draw it again."""
        for _ in range(200):
            keep = ([x.copy() for x in self.D], list(self.last), dict(self.old), len(self.ops), len(self.es))
            step(*args, **kw)
            if all(E_FLOOR * 1.01 <= abs(e) < E_CEIL * 0.99 for e in self.es[keep[4]:]):
                return
            self.D, self.last, self.old = keep[0], keep[1], keep[2]
            del self.ops[keep[3]:], self.es[keep[4]:]
        raise RuntimeError("no draw of this step gives comparable energies")

    def call(self, b, i, r=None, p=0, rp=None, op="patched", **extra):
        return self.emit(op=op, ils=b + 1, i=i, r=r, p=p, rp=rp, **extra)

    def plain(self, b, i, **extra):
        return self.emit(op="plain", ils=b + 1, i=i, **extra)

    # -- the shapes of the request stream (ISSUE: what the scripts must contain) ------------------------------------
    def protocol_step(self, b, accept):
        """The caller's own pattern (mc_moves.F90:1010-1190): old energy, trial energy, and the previous molecule travels along --
        at its trial position when the move was accepted, at its old one when it was silently reverted."""
        i = self.other(b)
        last = self.last[b]
        old_last = self.old.get(b)
        rp = None
        if last >= 1 and last != i:
            rp = self.pos(b, last) if (accept or old_last is None) else old_last
        self.old[b] = self.pos(b, i)
        self.call(b, i, self.moved(b, i), last if rp is not None else 0, rp)

    def noprev_then_neighbour(self, b, with_r):
        a, n = self.with_nearest(b)
        self.call(b, a, self.moved(b, a, firm=True))                       # no prev: nobody covers a from here on
        if with_r:
            self.call(b, n, self.moved(b, n), stale=a)
        else:
            self.plain(b, n, stale=a)
        self.old.pop(b, None)

    def wrong_prev(self, b):
        a, n = self.with_nearest(b)
        self.call(b, a, self.moved(b, a, firm=True))
        c = self.other(b, a, n)
        self.call(b, n, self.pos(b, n), c, self.moved(b, c), stale=a)      # prev names c; the molecule really asked about last is a
        self.old.pop(b, None)

    def prev_is_imol(self, b):
        i = self.other(b)
        self.call(b, i, self.moved(b, i), i, self.moved(b, i))             # o2 is absent by rule 1: only r_imol counts
        self.old.pop(b, None)

    def same_twice(self, b):
        i = self.other(b)
        last = self.last[b]
        self.call(b, i, self.moved(b, i), last if last not in (0, i) else 0, self.pos(b, last) if last not in (0, i) else None)
        self.call(b, i, self.moved(b, i))                                   # the same molecule again, moved again
        self.old.pop(b, None)

    def no_r_with_moved_prev(self, b):
        i = self.other(b)
        self.call(b, i, self.moved(b, i))
        j = self.other(b, i)
        self.call(b, j, None, i, self.moved(b, i))                          # r_imol == NULL, prev moved once more
        self.old.pop(b, None)

    def moved_prev_is_neighbour(self, b):
        i, n = self.with_nearest(b)
        self.call(b, i, self.moved(b, i))
        self.call(b, n, self.moved(b, n), i, self.moved(b, i, firm=True))
        self.old.pop(b, None)

    def exclusive(self, b, kind):
        self.emit(op="exclusive", kind=kind, ils=b + 1)
        self.old.pop(b, None)


def _mixed(bd, nboxes, rounds, exclusive_every):
    """`rounds` rounds of every shape on boxes chosen at random, an exclusive entry point every `exclusive_every` shapes."""
    k = 0
    kinds = ("model_energy", "download", "build")
    for _ in range(rounds):
        for shape in ("np_plain", "np_r", "wrong", "self", "twice", "nor", "nbr", "proto", "proto", "proto", "proto"):
            b = int(bd.rng.integers(0, nboxes))
            if shape == "np_plain":
                bd.attempt(bd.noprev_then_neighbour, b, False)
            elif shape == "np_r":
                bd.attempt(bd.noprev_then_neighbour, b, True)
            elif shape == "wrong":
                bd.attempt(bd.wrong_prev, b)
            elif shape == "self":
                bd.attempt(bd.prev_is_imol, b)
            elif shape == "twice":
                bd.attempt(bd.same_twice, b)
            elif shape == "nor":
                bd.attempt(bd.no_r_with_moved_prev, b)
            elif shape == "nbr":
                bd.attempt(bd.moved_prev_is_neighbour, b)
            else:
                for s in range(3):
                    bd.attempt(bd.protocol_step, b, accept=bool((k + s) % 3))
            k += 1
            if k % exclusive_every == 0:
                bd.exclusive(b, kinds[(k // exclusive_every) % 3])


def _post_collect_two(bd, moves):
    """post(2), patched(1), collect(2) over `moves` moves, the pattern of the Fortran module (energy_hip.F90:357-410), and the
    ways a posted reply is lost: nothing posted, another single call on the lattice, an exclusive entry point."""
    bd.emit(op="collect", ils=2)                                            # nothing posted: 2
    back = {}                                                               # lattice -> where a rejected move's molecule goes back to
    def move(m):
        i = bd.other(0)
        for trial in (False, True):                                         # old energies of both lattices, then the trial ones
            reqs = []
            for b in (1, 0):
                last = bd.last[b]
                old = bd.pos(b, i)
                r = bd.moved(b, i) if trial else old
                p = last if last not in (0, i) else 0
                reqs.append((b, r, p, (back.pop(b, None) or bd.pos(b, p)) if p else None))
                if trial and m % 3 == 0:
                    back[b] = old                                           # rejected: the host puts it back without a word
            (b2, r2, p2, rp2), (b1, r1, p1, rp1) = reqs
            bd.call(b2, i, r2, p2, rp2, op="post")
            if m % 25 == 7 and not trial:
                j = bd.other(1, i)
                bd.call(1, j, bd.moved(1, j), i, bd.pos(1, i))              # another single call on lattice 2: the reply is dropped
            if m % 25 == 19 and trial:
                bd.exclusive(m % 2, ("model_energy", "download")[m % 2])    # an exclusive entry point: the reply may predate it
            bd.call(b1, i, r1, p1, rp1)
            bd.emit(op="collect", ils=2)

    for m in range(moves):
        keep = dict(back)
        bd.attempt(lambda: (back.clear(), back.update(keep), move(m)))      # (a move drawn again starts from the same books)
    bd.emit(op="collect", ils=1)                                           # never posted on lattice 1: 2


def _shared_slots(bd, rounds):
    """Ten boxes, eight slots: boxes 1/9 and 2/10 share one.  post(x), post(y), collect(x), collect(y) and post(y), patched(x),
    collect(y) for both pairs and both orders; then everything is read back through an exclusive entry point."""
    def group(k, x, y):
        i, j = bd.other(x - 1), bd.other(y - 1)
        bd.call(x - 1, i, bd.moved(x - 1, i, firm=True), op="post")
        bd.call(y - 1, j, bd.moved(y - 1, j, firm=True), op="post")
        bd.emit(op="collect", ils=x)
        bd.emit(op="collect", ils=y)
        i, j = bd.other(x - 1), bd.other(y - 1)
        bd.call(y - 1, j, bd.moved(y - 1, j, firm=True), op="post")
        bd.call(x - 1, i, bd.moved(x - 1, i, firm=True))
        bd.emit(op="collect", ils=y)
        if k % 2:
            for b in (x, y):
                bd.exclusive(b - 1, "download")

    for k in range(rounds):
        for x, y in ((1, 9), (9, 1), (2, 10), (10, 2)):
            bd.attempt(group, k, x, y)
    for b in (1, 9, 2, 10, 5):
        bd.exclusive(b - 1, "model_energy")


def triplet_099(geo):
    """(a, b, c, target): molecules (1-based) of box 0 and the position that puts c almost behind b as seen from a -- on the line
    a -> b, 1.45 |ab| from a -- so that the triplet b--a--c has cos(theta) >= 0.99: the construction of
    test_moment_path_of_the_move_kernel_and_the_triplets_it_must_decline, with c a molecule that is on a's and b's lists."""
    x = geo.xs[0]
    nn, jn, vn = geo.lists[0]
    a = 101
    central = lambda i: [int(jn[i - 1, s]) for s in range(nn[i - 1]) if vn[i - 1, s] == 1]      # noqa: E731
    b = min(central(a), key=lambda j: np.linalg.norm(x[j - 1] - x[a - 1]))
    both = [k for k in central(b) if k in central(a) and k not in (a, b) and a in central(k) and b in central(k)]
    c = min(both, key=lambda k: np.linalg.norm(x[k - 1] - x[b - 1]))
    target = x[a - 1] + 1.45 * (x[b - 1] - x[a - 1]) + np.array([0.02, -0.01, 0.015])
    return a, b, c, _t(target)


def _around_099(geo):
    """a, b, c and everybody on their lists: left alone until the tail, so that the lists a rebuild makes still hold the triplet."""
    nn, jn, _ = geo.lists[0]
    out = set()
    for m in triplet_099(geo)[:3]:
        out |= {m} | {int(j) for j in jn[m - 1, :nn[m - 1]]}
    return out


def _tail_099(bd):
    """The 0.99 case: c is pushed behind b (a request of its own), the next request carries it as a moved prev -- the update of
    its moments must be declined, the box's moment path is off from there -- and 30 more requests follow, a, b, c and their
    neighbours among them.  The counters are read right before the push; no exclusive entry point from the push on (it would
    restart the server and its moments)."""
    a, b, c, target = triplet_099(bd.geo)
    bd.avoid = set()
    bd.emit(op="counts", ils=1, mark="at_push")        # (an exclusive entry point, the last one: what was served up to here)
    last = bd.last[0]
    bd.call(0, c, target, last if last not in (0, c) else 0, bd.pos(0, last) if last not in (0, c) else None, mark="push")
    bd.call(0, a, bd.pos(0, a), c, target, mark="decline")
    bd.old.clear()
    around = [a, b, c, bd.geo.nearest(0, c), bd.geo.nearest(0, a, exclude=(b,)), bd.geo.nearest(0, b, exclude=(a,))]
    for k in range(30):
        i = around[(k // 2) % len(around)] if k % 2 == 0 else bd.other(0, c)
        last = bd.last[0]
        if i == last:
            bd.call(0, i, bd.pos(0, i), mark="after")
        elif last == c:                                                      # c stays where it was pushed: the triplet stays
            bd.call(0, i, bd.pos(0, i), c, target, mark="after")
        else:
            bd.call(0, i, bd.moved(0, i) if i != c else target, last, bd.pos(0, last), mark="after")


def _drift(bd, n):
    """n consecutive requests of the caller's own pattern on box 0, two thirds of them with a moved prev, no exclusive entry."""
    for k in range(n):
        bd.attempt(bd.protocol_step, 0, accept=bool(k % 3))


def _idle(bd):
    """One call, 1.5 s of silence (the server leaves after 300000 empty polls, 0.6 s at most), then a neighbour of the molecule
    moved last is asked about without prev: the restarted server makes its moments from the committed positions."""
    def step():
        bd.emit(op="counts", ils=1)
        a = bd.other(0)
        bd.call(0, a, bd.moved(0, a, firm=True))
        bd.emit(op="sleep", seconds=1.5)
        bd.plain(0, bd.geo.nearest(0, a, bd.D[0]), stale=a)
        bd.emit(op="counts", ils=1)

    bd.attempt(step)


#: name -> (box set, builder).  The first three are "the scripts of part A": every shape, on every box set.
SCRIPTS = {
    "ic1536": ("ic1536", lambda bd: (bd.avoid.update(_around_099(bd.geo)), _mixed(bd, 1, 22, 9), _tail_099(bd))),
    "pair48": ("pair48", lambda bd: (_mixed(bd, 2, 22, 9), _post_collect_two(bd, 12))),
    "ten48": ("ten48", lambda bd: (_mixed(bd, 10, 22, 9), _shared_slots(bd, 2))),
    "post_collect": ("pair48", lambda bd: _post_collect_two(bd, 100)),
    "shared_slots": ("ten48", lambda bd: _shared_slots(bd, 6)),
    "drift": ("ic1536", lambda bd: _drift(bd, 1500)),
    "idle": ("ic1536", _idle),
}
PART_A = ("ic1536", "pair48", "ten48")
_SEEDS = {"ic1536": 11, "pair48": 12, "ten48": 13, "post_collect": 14, "shared_slots": 15, "drift": 16, "idle": 17}
_SCRIPT_CACHE = {}


def script(name, oracle=None):
    """(box set name, ops) of script `name`: seeded, the same list in every process."""
    if name not in _SCRIPT_CACHE:
        boxset, build = SCRIPTS[name]
        bd = _Builder(geometry(boxset, oracle), _SEEDS[name])
        build(bd)
        _SCRIPT_CACHE[name] = (boxset, bd.ops)
    return _SCRIPT_CACHE[name]


# ------------------------------------------------------------------------------------------------------------------
# what a script contains
# ------------------------------------------------------------------------------------------------------------------
def count_shapes(geo, ops):
    """{shape: occurrences} read off the ops themselves (not off the builders' notes), with the ledger's positions: who was really
    asked about last, whether its override is covered by this request, whether a prev has moved."""
    D = [x.copy() for x in geo.xs]
    last = [0] * len(D)             # molecule asked about last
    carried = [False] * len(D)      # ... with an r_imol (so its committed position is news to whoever tracks positions incrementally)
    before = [None] * len(D)        # ... its position before that request
    shapes = {k: 0 for k in ("noprev_nbr_plain", "noprev_nbr_r", "wrong_prev_nbr", "prev_is_imol", "revert", "moved",
                             "same_twice", "no_r_moved_prev", "moved_prev_is_nbr", "case_099")}
    for op in ops:
        if op["op"] in ("exclusive", "counts"):
            carried = [False] * len(D)          # (positions are read back whole: nothing is news after it)
            continue
        if op["op"] not in SINGLE:
            continue
        b, i = op["ils"] - 1, op["i"]
        r = op.get("r")
        p, rp = op.get("p", 0), op.get("rp")
        has_o2 = rp is not None and p >= 1 and p != i
        a = last[b]
        uncovered = carried[b] and a not in (0, i) and not (has_o2 and p == a) and _t(D[b][a - 1]) != before[b]
        nbr = uncovered and geo.is_neighbour(b, i, a)
        if nbr and not has_o2:
            shapes["noprev_nbr_r" if r is not None else "noprev_nbr_plain"] += 1
        if nbr and has_o2:
            shapes["wrong_prev_nbr"] += 1
        if rp is not None and p == i:
            shapes["prev_is_imol"] += 1
        if has_o2:
            was = before[b] if (p == a and carried[b]) else _t(D[b][p - 1])     # the position the moments hold for p
            if tuple(rp) == was:
                shapes["revert"] += 1
            else:
                shapes["moved"] += 1
                if r is None:
                    shapes["no_r_moved_prev"] += 1
                if geo.is_neighbour(b, i, p):
                    shapes["moved_prev_is_nbr"] += 1
        if a == i and carried[b] and r is not None and tuple(r) != _t(D[b][i - 1]):
            shapes["same_twice"] += 1
        if op.get("mark") == "decline":
            shapes["case_099"] += 1
        if not (a == i and carried[b]):     # (asked about again: whoever tracks positions still holds the one from before the first time)
            before[b] = _t(D[b][i - 1])
            carried[b] = r is not None
        commit(D, op)
        last[b] = i
    return shapes


# ------------------------------------------------------------------------------------------------------------------
# replayer 1: the ledger and the oracle
# ------------------------------------------------------------------------------------------------------------------
def digest(x):
    return hashlib.sha256(np.ascontiguousarray(x, dtype=np.float64).tobytes()).hexdigest()


def replay_ledger(oracle, geo, ops, checkpoints=()):
    """One record per op: {"e": energy} for a single call, {"e": energy, "expect": "rc0" | "rc2" | "either"} for a collect,
    {"e": full-box energy, "pos": digest of D[b]} for an exclusive entry point, {} otherwise.  A single call on a stale-sensitive
    spot (op["stale"] = the molecule nobody covered) also gets "e_stale": the oracle with that molecule left where it was.
    `checkpoints`: op indices after which (D, lists) are snapshot into the returned list."""
    D = [x.copy() for x in geo.xs]
    lists = list(geo.lists)
    nb = len(D)
    nslots = min(nb, NSLOTS_MAX)
    pending = {}                    # box -> [posted op, energy as of the post, "rc0" | "rc2" | "either"]
    before = {}                     # (box, molecule) -> position before its last override
    records, snaps = [], []

    def local(b, i, X=None):
        return oracle.local_energy(i, D[b] if X is None else X, geo.iv[b], *lists[b])

    def single(op):
        b = op["ils"] - 1
        for m, _ in overrides(op):
            before[(b, m)] = _t(D[b][m - 1])
        commit(D, op)
        rec = {"e": local(b, op["i"])}
        if "stale" in op:
            X = D[b].copy()
            X[op["stale"] - 1] = before[(b, op["stale"])]
            rec["e_stale"] = local(b, op["i"], X)
        return rec

    for k, op in enumerate(ops):
        kind = op["op"]
        rec = {}
        if kind in SINGLE:
            b = op["ils"] - 1
            for q, pend in pending.items():                  # the slot holds one request: whoever comes next waits for it and drops its reply
                if q == b:
                    pend[2] = "rc2"
                elif q % nslots == b % nslots and pend[2] == "rc0":
                    pend[2] = "either"
            rec = single(op)
            if kind == "post":
                pending[b] = [op, rec["e"], "rc0"]
                rec = {"posted": True}
        elif kind == "collect":
            b = op["ils"] - 1
            pend = pending.pop(b, None)
            if pend is not None and pend[2] != "rc0":         # (asked again, or maybe: that is a single call on this lattice)
                for q, other in pending.items():
                    if q % nslots == b % nslots and other[2] == "rc0":
                        other[2] = "either"
            if pend is None:
                rec = {"expect": "rc2", "e": None}
            elif pend[2] == "rc2":                            # the reply is gone: the caller asks again, and THAT is the answer
                rec = dict(single(dict(pend[0], op="patched")), expect="rc2")
            else:
                rec = {"expect": pend[2], "e": pend[1]}
        elif kind == "exclusive":
            b = op["ils"] - 1
            for pend in pending.values():
                pend[2] = "rc2"
            if op["kind"] == "build":
                lists[b] = oracle.neighbours(D[b], geo.iv[b])
            rec = {"e": oracle.model_energy(D[b], geo.iv[b], *lists[b]), "pos": digest(D[b])}
        elif kind == "counts":                                # (mw_server_counts is an exclusive entry point too)
            for pend in pending.values():
                pend[2] = "rc2"
        records.append(rec)
        if k in checkpoints:
            snaps.append(([x.copy() for x in D], list(lists)))
    return (records, snaps) if checkpoints else records


# ------------------------------------------------------------------------------------------------------------------
# replayer 2: the raw ctypes library
# ------------------------------------------------------------------------------------------------------------------
def replay_engine(em, ops):
    """The same ops through em.L.mw_local_energy* (no Python wrapper in between).  One record per op: {"rc", "e"} for a single
    call, {"rc"} for a post (the server switched off answers 2: the request is then asked with `patched` on the spot and its
    answer kept for the collect), {"rc", "e", "reasked"} for a collect (rc 2 with a request on file: asked again with
    `patched`), {"e", "pos"} for an exclusive entry point, {"counts": [...]} for counts."""
    L = em.L
    vec = ctypes.c_double * 3
    e = ctypes.c_double(0.0)
    posted = {}                     # box -> [op, answer kept (server off) or None, reply lost since (server off: the caller's own books)]
    records = []

    def chk(rc):
        if rc not in (0, 2):
            raise RuntimeError(L.mw_last_error().decode())
        return rc

    def args(op):
        return (op["ils"], op["i"], vec(*op["r"]) if op.get("r") is not None else None,
                op.get("p", 0), vec(*op["rp"]) if op.get("rp") is not None else None)

    def patched(op):
        if chk(L.mw_local_energy_patched(*args(op), ctypes.byref(e))) != 0:
            raise RuntimeError("mw_local_energy_patched returned 2")
        return e.value

    for op in ops:
        kind = op["op"]
        rec = {}
        if kind in SINGLE and op["ils"] in posted:
            posted[op["ils"]][2] = True         # (another single call on the lattice: the served path drops the posted reply)
        if kind in ("exclusive", "counts"):
            for pend in posted.values():
                pend[2] = True
        if kind == "patched":
            rec = {"rc": 0, "e": patched(op)}
        elif kind == "plain":
            rec = {"rc": chk(L.mw_local_energy(op["ils"], op["i"], ctypes.byref(e))), "e": e.value}
        elif kind == "post":
            rc = chk(L.mw_local_energy_post(*args(op)))
            posted[op["ils"]] = [op, patched(op) if rc == 2 else None, False]
            rec = {"rc": rc}
        elif kind == "collect":
            rc = chk(L.mw_local_energy_collect(op["ils"], ctypes.byref(e)))
            rec = {"rc": rc, "e": e.value if rc == 0 else None, "reasked": False}
            op0, kept, lost = posted.pop(op["ils"], (None, None, False))
            if rc == 2 and op0 is not None:
                if kept is not None and not lost:
                    rec["e"] = kept
                else:
                    rec["e"], rec["reasked"] = patched(op0), True
        elif kind == "exclusive":
            ils = op["ils"]
            if op["kind"] == "build":
                mn, mx = ctypes.c_int(0), ctypes.c_int(0)
                chk(L.mw_build_neighbours(ils, ctypes.byref(mn), ctypes.byref(mx)))
            x = np.zeros((em.nwater, 3))
            if op["kind"] == "download":
                chk(L.mw_download_positions(ils, x.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
            chk(L.mw_model_energy(ils, ctypes.byref(e)))
            chk(L.mw_download_positions(ils, x.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
            rec = {"e": e.value, "pos": digest(x)}
        elif kind == "sleep":
            time.sleep(op["seconds"])
        elif kind == "counts":
            rec = {"counts": server_counts(L, op["ils"])}
        records.append(rec)
    return records


def server_counts(L, ils):
    if not hasattr(L, "mw_server_counts"):
        return None
    out = (ctypes.c_longlong * 5)()
    if L.mw_server_counts(ils, out) != 0:
        raise RuntimeError(L.mw_last_error().decode())
    return [int(v) for v in out]


# ------------------------------------------------------------------------------------------------------------------
# engine against ledger
# ------------------------------------------------------------------------------------------------------------------
def rel(a, b):
    return abs(a - b) / abs(b)


def compare(ops, got, want, rtol, server_off=False):
    """Every way `got` (replay_engine, energies as floats) misses `want` (replay_ledger): a list of strings, empty when it holds."""
    bad = []
    assert len(ops) == len(got) == len(want)
    for k, (op, g, w) in enumerate(zip(ops, got, want)):
        kind = op["op"]
        where = f"op {k} {kind} box {op.get('ils')} molecule {op.get('i')}"
        if kind in ("patched", "plain"):
            if g["rc"] != 0 or not rel(g["e"], w["e"]) <= rtol:
                bad.append(f"{where}: rc {g['rc']}, {g['e']!r} against {w['e']!r} (rel {rel(g['e'], w['e']):.3e})")
        elif kind == "post":
            if g["rc"] != (2 if server_off else 0):
                bad.append(f"{where}: post returned {g['rc']}")
        elif kind == "collect":
            if server_off:
                ok_rc = g["rc"] == 2
            else:
                ok_rc = g["rc"] == {"rc0": 0, "rc2": 2}.get(w["expect"], g["rc"]) and g["rc"] in (0, 2)
            if not ok_rc:
                bad.append(f"{where}: collect returned {g['rc']}, the contract says {w['expect']}")
            if w["e"] is None:
                if g["e"] is not None:
                    bad.append(f"{where}: an energy though nothing was posted")
            elif g["e"] is None or not rel(g["e"], w["e"]) <= rtol:
                bad.append(f"{where}: rc {g['rc']}, {g['e']!r} against {w['e']!r}")
        elif kind == "exclusive":
            if not rel(g["e"], w["e"]) <= rtol:
                bad.append(f"{where} {op['kind']}: full-box energy {g['e']!r} against {w['e']!r} (rel {rel(g['e'], w['e']):.3e})")
            if g["pos"] != w["pos"]:
                bad.append(f"{where} {op['kind']}: downloaded positions are not the ledger's")
    return bad


def energies(ops, records):
    """The energies of a replay in op order (single calls, collects that have one, exclusive entry points) as an array."""
    return np.array([r["e"] for op, r in zip(ops, records) if r.get("e") is not None], dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------------
# the child process of the GPU tests
# ------------------------------------------------------------------------------------------------------------------
def _hexed(records):
    return [dict(r, e=float(r["e"]).hex()) if r.get("e") is not None else r for r in records]


def unhex(records):
    return [dict(r, e=float.fromhex(r["e"])) if r.get("e") is not None else r for r in records]


def main(name):
    from mc_water_ls_mw_amd.energy import load_boxes
    boxset, ops = script(name)
    geo = geometry(boxset)
    em = load_boxes(geo.hs, geo.xs)
    try:
        records = replay_engine(em, ops)
        counts = [server_counts(em.L, b + 1) for b in range(len(geo.xs))]
    finally:
        em.energy_deinit()
    print(json.dumps({"records": _hexed(records), "counts": counts}))


if __name__ == "__main__":
    main(sys.argv[1])
