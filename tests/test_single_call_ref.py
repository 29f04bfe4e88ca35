"""CPU: the request scripts of tests/single_call_ref.py are what tests/test_gpu_single_call_abi.py needs them to be -- every
request shape the C ABI admits occurs often enough, every stale-sensitive spot really is sensitive, every energy is one the
plain relative bar applies to, and the ledger reproduces a from-scratch evaluation.  Without these the GPU test could pass
without having asked the question."""
import numpy as np
import pytest

import single_call_ref as ref

#: what a script set must contain at least (summed over the three scripts of part A)
MINIMA = {"noprev_nbr_plain": 20, "noprev_nbr_r": 20, "wrong_prev_nbr": 20, "prev_is_imol": 5, "revert": 50, "moved": 50,
          "same_twice": 10, "no_r_moved_prev": 10, "moved_prev_is_nbr": 20, "case_099": 1}
#: a stale copy of the uncovered molecule must change the answer by at least this, relative: 10^4 times the parity bar
SENSITIVE = 1e-6


@pytest.fixture(scope="module")
def ledgers(c_oracle):
    out = {}
    for name in ref.SCRIPTS:
        boxset, ops = ref.script(name, c_oracle)
        geo = ref.geometry(boxset, c_oracle)
        n = len(ops)
        sync = [k for k, op in enumerate(ops) if op["op"] in ("patched", "plain")]
        marks = tuple(sorted({max(k for k in sync if k <= max(t, sync[0])) for t in (n // 3, 2 * n // 3, n - 1)}))
        records, snaps = ref.replay_ledger(c_oracle, geo, ops, checkpoints=marks)
        out[name] = (geo, ops, records, snaps, marks)
    return out


@pytest.mark.parametrize("name", ref.PART_A)
def test_every_request_shape_occurs(name, ledgers):
    """Each script of part A on its own holds every shape (the 0.99 case: the 1536-molecule box only)."""
    geo, ops, _, _, _ = ledgers[name]
    shapes = ref.count_shapes(geo, ops)
    for shape, least in MINIMA.items():
        if shape == "case_099" and name != "ic1536":
            continue
        assert shapes[shape] >= least, (name, shape, shapes)


def test_shapes_of_the_directed_scripts(ledgers):
    geo, ops, _, _, _ = ledgers["drift"]
    shapes = ref.count_shapes(geo, ops)
    assert len(ops) == 1500 and all(op["op"] == "patched" for op in ops)
    assert shapes["moved"] >= 900 and shapes["revert"] >= 400, shapes          # two thirds move prev, no exclusive entry
    geo, ops, _, _, _ = ledgers["post_collect"]
    kinds = [op["op"] for op in ops]
    assert kinds.count("post") == 200 and kinds.count("collect") == 202 and kinds.count("exclusive") >= 4
    geo, ops, records, _, _ = ledgers["shared_slots"]
    expects = [r["expect"] for op, r in zip(ops, records) if op["op"] == "collect"]
    assert expects.count("either") == len(expects) >= 36, expects                # a shared slot really was contended, every time
    geo, ops, records, _, _ = ledgers["post_collect"]
    expects = [r["expect"] for op, r in zip(ops, records) if op["op"] == "collect"]
    assert expects.count("rc0") >= 180 and expects.count("rc2") >= 10 and "either" not in expects, expects


@pytest.mark.parametrize("name", list(ref.SCRIPTS))
def test_stale_spots_are_sensitive_and_every_energy_is_comparable(name, ledgers):
    geo, ops, records, _, _ = ledgers[name]
    nstale = 0
    for k, (op, rec) in enumerate(zip(ops, records)):
        if op["op"] == "exclusive":
            assert abs(rec["e"]) >= 1e-6, (name, k)
        elif rec.get("e") is not None:
            assert 1e-6 <= ref.E_FLOOR <= abs(rec["e"]) < ref.E_CEIL <= 1.0, (name, k, op, rec["e"])   # (no mask anywhere: the relative bars are the bars)
        if "stale" in op:
            nstale += 1
            assert ref.rel(rec["e_stale"], rec["e"]) >= SENSITIVE, (name, k, op, rec)
    if name in ref.PART_A:
        assert nstale >= 60, nstale
    if name == "idle":
        assert nstale == 1


@pytest.mark.parametrize("name", list(ref.SCRIPTS))
def test_ledger_reproduces_a_from_scratch_evaluation(name, ledgers, c_oracle):
    """At three checkpoints, each right after a synchronous single call: the ledger's positions are the uploaded ones with the
    overrides of every request so far applied in order (a lost reply's request is asked again at its collect), written out here
    a second time without the ledger's machinery -- and the answer just given is that molecule's row of a from-scratch
    COracle.local_energy_all on them, to the bit."""
    geo, ops, records, snaps, marks = ledgers[name]
    assert len(snaps) == len(marks) == (2 if name == "idle" else 3)          # (the idle script is two calls long)
    D = [x.copy() for x in geo.xs]
    posted = {}
    k0 = 0

    def apply(op):                   # the three rules of the contract, spelt out here (not ref.commit: a second derivation)
        if op["op"] == "plain":
            return
        if op["rp"] is not None and op["p"] >= 1 and op["p"] != op["i"]:
            D[op["ils"] - 1][op["p"] - 1] = op["rp"]
        if op["r"] is not None:
            D[op["ils"] - 1][op["i"] - 1] = op["r"]

    for (Dk, lists), mark in zip(snaps, marks):
        for op, rec in zip(ops[k0:mark + 1], records[k0:mark + 1]):
            if op["op"] in ref.SINGLE:
                apply(op)
                if op["op"] == "post":
                    posted[op["ils"]] = op
            elif op["op"] == "collect" and op["ils"] in posted:
                again = posted.pop(op["ils"])
                if rec["expect"] == "rc2":
                    apply(again)
        k0 = mark + 1
        for b in range(len(D)):
            assert np.array_equal(D[b], Dk[b]), (name, mark, b)
        op = ops[mark]
        assert op["op"] in ("patched", "plain")
        b = op["ils"] - 1
        scratch = c_oracle.local_energy_all(Dk[b], geo.iv[b], *lists[b])
        assert scratch[op["i"] - 1] == records[mark]["e"], (name, mark)


def _local_energy_py(i, x, iv, nn, jn, vn, drop_099):
    """mwo_local_energy (molint.F90:220-404) in plain Python for ONE molecule, with the cos(theta) >= 0.99 rule (:367) on or off."""
    # (the constants: oracle/mw_oracle.c)
    ang = 1.0 / 0.5291772108
    sigma, eps, lam = 2.3925 * ang, 6.189 / 627.509469, 23.15
    A, B, gam, a = 7.049556277, 0.6022245584, 1.2, 1.8
    cos0 = float(np.float32(-0.33331324756))
    rcsq, sig_a = (sigma * a) ** 2, sigma * a
    ri = x[i - 1]
    nbrs = [(int(jn[i - 1, s]), iv[vn[i - 1, s] - 1]) for s in range(nn[i - 1])]
    evdw = etb = 0.0
    for ln, (j, jiv) in enumerate(nbrs):
        rj = x[j - 1] + jiv
        av = rj - ri
        r2 = float(av @ av)
        if r2 >= rcsq:
            continue
        r1 = np.sqrt(r2)
        evdw += A * eps * (B * (sigma * sigma / r2) ** 2 - 1.0) * np.exp(sigma / (r1 - sig_a))
        exp3 = np.exp(gam * sigma / (r1 - sig_a))
        slots = [((x[k - 1] + kiv) - ri, av) for k, kiv in nbrs[ln + 1:]]
        slots += [(((x[int(jn[j - 1, s]) - 1] + iv[vn[j - 1, s] - 1]) + jiv) - rj, -av) for s in range(nn[j - 1])]
        it = 0.0
        for bv, cv in slots:
            s2 = float(bv @ bv)
            if s2 < rcsq:
                s1 = np.sqrt(s2)
                ct = float(cv @ bv) / (r1 * s1)
                if ct < 0.99 or not drop_099:
                    it += (ct - cos0) ** 2 * np.exp(gam * sigma / (s1 - sig_a))
        etb += it * exp3
    return evdw + lam * eps * etb


def test_the_099_case_is_one(ledgers, c_oracle):
    """The pushed molecule really makes a triplet the reference drops: with the rule ignored the local energy of the molecule it
    stands behind changes by far more than the tolerance -- and the plain-Python restatement used for that is the oracle's
    (same energy with the rule on).  From the push on the script holds 30 more requests and no exclusive entry point."""
    geo, ops, records, snaps, _ = ledgers["ic1536"]
    a, b, c, target = ref.triplet_099(geo)
    push = next(k for k, op in enumerate(ops) if op.get("mark") == "push")
    assert ops[push]["i"] == c and ops[push]["r"] == target
    assert ops[push + 1].get("mark") == "decline" and ops[push + 1]["p"] == c and ops[push + 1]["rp"] == target
    tail = ops[push + 2:]
    assert len(tail) == 30 and all(op["op"] == "patched" for op in tail)
    asked = {op["i"] for op in tail}
    assert {a, b, c} <= asked and any(geo.is_neighbour(0, c, i) for i in asked - {a, b, c})
    assert all(op["op"] != "exclusive" for op in ops[push:])
    D, lists = snaps[-1]                                         # the end of the script: c is still where it was pushed
    assert ref._t(D[0][c - 1]) == target
    with_rule = _local_energy_py(a, D[0], geo.iv[0], *lists[0], drop_099=True)
    without = _local_energy_py(a, D[0], geo.iv[0], *lists[0], drop_099=False)
    want = c_oracle.local_energy(a, D[0], geo.iv[0], *lists[0])
    assert abs(with_rule - want) <= 1e-13 * abs(want)
    assert ref.rel(without, want) > 1e-6, (without, want)
