"""GPU: every request shape the C ABI of the single local-energy call admits (mw_local_energy, mw_local_energy_patched,
mw_local_energy_post, mw_local_energy_collect -- the raw ctypes library, not the Python wrapper) against the contract written
down as a host ledger plus the C oracle (tests/single_call_ref.py; tests/test_single_call_ref.py holds the scripts to what
they must contain).  Behind the entry points sit the resident k_local_server with its incrementally kept moments and the
one-launch k_local_energy_single.

Bars: engine against ledger and oracle 1e-10 relative (conftest.RTOL); MW_SERVER_REQ=device against host the same bits; moment
path against MW_SERVER_MOMENTS=0 against MW_LOCAL_SERVER=0 1e-12 relative (another summation order: the figure of
test_single_call_paths_agree); committed positions after an exclusive entry point bitwise; full-box energies RTOL.

The engine reads its switches once per process, so every configuration replays its script in a fresh child process (one at a
time, MW_SERVER_TIMEOUT=5: a lost reply fails in seconds) that prints its answers as hex floats; the parent compares.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import single_call_ref as ref
from conftest import RTOL

pytestmark = pytest.mark.gpu

CONFIGS = {"default": {}, "req_host": {"MW_SERVER_REQ": "host"}, "moments_off": {"MW_SERVER_MOMENTS": "0"},
           "server_off": {"MW_LOCAL_SERVER": "0"}}
SWITCHES = ("MW_SERVER_REQ", "MW_SERVER_MOMENTS", "MW_LOCAL_SERVER", "MW_SERVER_PLAIN_LOADS", "MW_SERVER_STAMPS")


_RUNS = {}
_TROUBLE = []


def _engine(name, config):
    """The engine's records of script `name` under `config`, from a child process: (records, counts per box).  A child is
    started once per (script, configuration): one that failed is not started again by the tests that share its answers."""
    key = (name, config)
    if key not in _RUNS and _TROUBLE:            # (a child that died or hung: nothing more is started on the GPU from here)
        pytest.fail(f"replaying {name} under {config}: not started, an earlier child ended with {_TROUBLE[0]}")
    if key not in _RUNS:
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        env.update(CONFIGS[config], MW_SERVER_TIMEOUT="5")
        try:
            out = subprocess.run([sys.executable, os.path.join(ref.HERE, "single_call_ref.py"), name], capture_output=True,
                                 text=True, timeout=120, env=env)
            if out.returncode == 0:
                z = json.loads(out.stdout.strip().splitlines()[-1])
                _RUNS[key] = (ref.unhex(z["records"]), z["counts"])
            else:
                _RUNS[key] = f"exit status {out.returncode}: {out.stderr[-2000:]}"
        except subprocess.TimeoutExpired:
            _RUNS[key] = "no end within 120 s"
        if isinstance(_RUNS[key], str):
            _TROUBLE.append(_RUNS[key][:200])
    if isinstance(_RUNS[key], str):
        pytest.fail(f"replaying {name} under {config}: {_RUNS[key]}")
    return _RUNS[key]


@functools.lru_cache(maxsize=None)
def _ledger(name):
    from oracle import COracle
    oracle = COracle()
    boxset, ops = ref.script(name, oracle)
    return ops, ref.replay_ledger(oracle, ref.geometry(boxset, oracle), ops)


def _hold(name, config):
    ops, want = _ledger(name)
    got, counts = _engine(name, config)
    bad = ref.compare(ops, got, want, RTOL, server_off=config == "server_off")
    assert not bad, (name, config, len(bad), bad[:8])
    return ops, got, want, counts


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("name", ref.PART_A)
def test_every_request_shape_against_the_ledger(name, config):
    """The scripts of part A -- no prev, a prev that is not the molecule asked about last, prev == imol, silent reverts, moved
    prevs, the same molecule twice, no r_imol, exclusive entry points in between, the 0.99 decline -- on each box set under each
    transport and path.  With the server switched off post and collect return 2 and the caller asks with `patched`."""
    _hold(name, config)


@pytest.mark.parametrize("name", ref.PART_A)
def test_both_transports_return_the_same_bits(name):
    dev, _ = _engine(name, "default")
    host, _ = _engine(name, "req_host")
    assert dev == host


@pytest.mark.parametrize("name", ref.PART_A)
def test_the_three_paths_agree(name):
    ops, _ = _ledger(name)
    e = {c: ref.energies(ops, _engine(name, c)[0]) for c in ("default", "moments_off", "server_off")}
    for c in ("moments_off", "server_off"):
        assert e[c].shape == e["default"].shape
        assert np.all(np.abs(e[c] - e["default"]) <= 1e-12 * np.abs(e["default"])), c


def test_post_and_collect_on_two_lattices():
    """post(2), patched(1), collect(2) over 100 moves as the Fortran module interleaves them: the collected answer is the one as
    of the post and comes with rc 0; collect with nothing posted returns 2; after another single call on the lattice, or an
    exclusive entry point, collect returns 2, the re-asked answer is right and the posted overrides are in the downloaded
    positions (the script reads them back: `compare` holds them to the ledger bit for bit)."""
    ops, got, want, _ = _hold("post_collect", "default")
    rcs = [(w["expect"], g["rc"]) for op, g, w in zip(ops, got, want) if op["op"] == "collect"]
    assert rcs.count(("rc0", 0)) >= 180 and rcs.count(("rc2", 2)) >= 10 and len(rcs) == 202
    assert rcs[0] == ("rc2", 2) and rcs[-1] == ("rc2", 2)               # nothing posted
    assert sum(op["op"] == "exclusive" for op in ops) >= 4


def test_lattices_that_share_a_slot_never_collect_each_others_reply():
    """Ten boxes on eight slots: post(1), post(9), collect(1), collect(9), and post(9), patched(1), collect(9), both pairs, both
    orders.  A collect returns rc 0 with ITS lattice's ledger value or 2 (and the re-ask is right) -- never another lattice's
    energy; the overrides of every post are committed (full-box energies and downloaded positions at the end)."""
    ops, got, want, _ = _hold("shared_slots", "default")
    contended = [(g["rc"], g["reasked"]) for op, g, w in zip(ops, got, want) if op["op"] == "collect" and w["expect"] == "either"]
    assert len(contended) >= 24 and all(rc in (0, 2) for rc, _ in contended)
    assert all(again for rc, again in contended if rc == 2)
    # no two collected answers of the script are within 10^4 bars of each other: another lattice's reply cannot pass `compare`
    values = np.sort([w["e"] for op, w in zip(ops, want) if op["op"] == "collect" and w["e"] is not None])
    assert np.min(np.diff(values) / np.abs(values[1:])) > 1e4 * RTOL


def test_moments_do_not_drift_over_1500_requests():
    """1500 consecutive requests on the 1536-molecule box, two thirds of them moving prev, no exclusive entry point: the child
    collects every answer before anything is compared (the server must not idle out in between); the last hundred meet the bar
    like the first hundred, on one server start and at least 900 incremental moment updates -- fewer, and the moments were
    rebuilt on the way and nothing was shown."""
    ops, got, want, counts = _hold("drift", "default")
    err = np.array([ref.rel(g["e"], w["e"]) for g, w in zip(got, want)])
    print("drift: largest relative error, first / last hundred:", err[:100].max(), err[-100:].max(), "counts", counts)
    assert err[:100].max() <= RTOL and err[-100:].max() <= RTOL
    moments, scan, plain, updates, starts = counts[0]
    assert starts == 1, counts
    assert updates >= 900, counts
    assert moments + scan + plain == 1500, counts


def test_a_server_that_idled_out_restarts_from_the_committed_positions():
    """One call that moves a molecule, 1.5 s of silence (the server leaves after 300000 empty polls: 0.6 s at most), then its
    nearest neighbour asked about without prev: the restarted server makes its moments from the device's positions, so the
    override lane 0 stores after the reply must have reached them.  Reading the counters stops the server, so the first call
    starts it (+1) and the call after the silence starts it again (+1): exactly two, or the server never idled out."""
    ops, got, want, _ = _hold("idle", "default")
    first, last = got[0]["counts"], got[-1]["counts"]
    assert last[4] - first[4] == 2, f"server starts rose by {last[4] - first[4]}, not by 2: {first} -> {last}"
    assert sum(last[:3]) - sum(first[:3]) == 2


def test_the_paths_the_scripts_mean_to_take_are_taken():
    """On the 1536-molecule box under default settings at least 90 % of the requests before the 0.99 push are served by the
    moment path and NONE from the push on: the script reads the counters right before the push (the last exclusive entry point
    of the script) and the child reads them again at the end -- the moment-path counter must not have risen in between, and all
    32 requests from the push on must show up under the scanning or the plain routine.  With MW_SERVER_MOMENTS=0 no request is
    served by the moment path at all; with the server off nothing is served."""
    ops, _ = _ledger("ic1536")
    push = next(k for k, op in enumerate(ops) if op.get("mark") == "push")
    assert ops[push - 1]["op"] == "counts" and all(op["op"] == "patched" for op in ops[push:])
    before = sum(op["op"] in ref.SINGLE for op in ops[:push])
    after = len(ops) - push
    assert after == 32
    records, counts = _engine("ic1536", "default")
    at_push, at_end = records[push - 1]["counts"], counts[0]
    print("ic1536 default counts at the push:", at_push, "at the end:", at_end, "requests before / from the push on:", before, after)
    assert sum(at_push[:3]) == before and sum(at_end[:3]) == before + after
    assert at_push[0] >= 0.9 * before, (at_push, before)
    assert at_end[0] - at_push[0] == 0, (at_push, at_end)                       # not one request on the moment path from the push on
    assert (at_end[1] - at_push[1]) + (at_end[2] - at_push[2]) == after, (at_push, at_end)
    assert at_end[3] == at_push[3], (at_push, at_end)                           # ... and no moment update: the one asked for, c's, was declined
    records, counts = _engine("ic1536", "moments_off")
    off_push, off = records[push - 1]["counts"], counts[0]
    assert off[0] == 0 and off[3] == 0 and off[1] + off[2] == before + after and off_push[1] + off_push[2] == before, (off_push, off)
    records, counts = _engine("ic1536", "server_off")
    assert counts[0] == [0, 0, 0, 0, 0] and records[push - 1]["counts"] == [0, 0, 0, 0, 0]
