"""CPU: the numpy reference of tests/tet_ref.py for the order parameters of include/mw_tet.h -- the known answers of ideal
cubic ice, the definition's symmetries and edge cases, and the preconditions that let tests/test_gpu_tet.py compare counts
exactly, the four nearest neighbours as sets, and leave no molecule out: no gap between ranks 4 and 5 and no distance to
either radius within 1e-9 (relative), for every case and every box of the batches."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden
from boo_ref import batch_set, widths
from tet_ref import (ANG_TO_BOHR, BATCHES, KEEP, MARGIN, batch_radii, case_exact, cases, load_case, preconditions, tet_exact)

CASES = cases()
IDS = [c[0] for c in CASES]


def _f(a):
    return np.asarray(a, dtype=np.float64)


@pytest.fixture(scope="module")
def evaluated():
    """label -> (tet_exact dict, h, xyz, r_search, r_lsi) of every GPU input, computed once."""
    return {case[0]: (case_exact(case),) + load_case(case) for case in CASES}


@pytest.mark.parametrize("reps", [(2, 2, 2), (3, 2, 2)])
def test_ideal_cubic_ice_has_the_known_answers(reps):
    """An ideal diamond lattice with the O-O distance D: four neighbours at D on a regular tetrahedron, twelve at D sqrt(8/3);
    so q = s_k = 1, d5 = D sqrt(8/3), four entries within 3.7 Angstrom and the LSI of the steps (0, 0, 0, d5 - D), 3/16 (d5 - D)^2."""
    from mc_water_ls_mw_amd import lattice as lat
    h, xyz = lat.ice_box("ic", reps, 0.0)
    D = lat.D_OO_ANG * ANG_TO_BOHR
    e = tet_exact(h, xyz, min(5.5 * ANG_TO_BOHR, 0.9999 * widths(h).min()), 3.7 * ANG_TO_BOHR)
    d5 = D * np.sqrt(8.0 / 3.0)
    assert len(xyz) == 8 * reps[0] * reps[1] * reps[2] and np.all(e["counts"][:, 1] == 4) and np.all(e["counts"][:, 0] >= 16)
    want = np.array([1.0, 1.0, d5, 3.0 / 16.0 * (d5 - D) ** 2])
    assert np.abs(_f(e["order"]) - want).max() <= 1e-12
    assert np.abs(_f(e["summary"][:4]) - want).max() <= 1e-12 and np.all(_f(e["summary"][4:]) == len(xyz))
    assert np.all(e["near"] >= 0) and all(len(set(row)) == 4 and i not in row for i, row in enumerate(e["near"].tolist()))


def test_values_are_defined_exactly_where_the_counts_allow(evaluated):
    for label, (e, h, xyz, rs, rl) in evaluated.items():
        n, nl = e["counts"][:, 0], e["counts"][:, 1]
        nan = np.isnan(_f(e["order"]))
        assert np.array_equal(nan[:, 0], n < 4) and np.array_equal(nan[:, 1], n < 4) and np.array_equal(nan[:, 2], n < 5), label
        assert np.array_equal(nan[:, 3], ~((nl >= 1) & (nl + 1 <= np.minimum(n, KEEP)))), label
        assert np.array_equal(e["near"] < 0, np.arange(4)[None, :] >= n[:, None]), label
        assert np.all(nl <= n) and np.array_equal(_f(e["summary"][4:]), (~nan).sum(axis=0)), label
        ok = ~nan
        assert np.all(_f(e["order"])[ok[:, 0], 0] <= 1.0 + 1e-15) and np.all(_f(e["order"])[ok[:, 0], 0] >= -3.0)
        assert np.all(_f(e["order"])[ok[:, 1], 1] <= 1.0) and np.all(_f(e["order"])[ok[:, 3], 3] >= 0.0)


@pytest.mark.parametrize("name", ["ic48_t015", "ih48_t020", "gas20", "ih8_small"])
def test_rotations_and_lattice_translations_change_nothing(name):
    z = load_golden(name)
    h, xyz = z["h"], z["xyz"]
    rs = min(5.5 * ANG_TO_BOHR, 0.9999 * widths(h).min())
    rl = min(3.7 * ANG_TO_BOHR, rs)
    e = tet_exact(h, xyz, rs, rl)
    rng = np.random.default_rng(5)
    rot, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    r = tet_exact(h @ rot.T, xyz @ rot.T, rs, rl)
    m = tet_exact(h, xyz + rng.integers(-2, 3, xyz.shape).astype(np.float64) @ h, rs, rl)
    for o in (r, m):
        assert np.array_equal(o["counts"], e["counts"]) and np.array_equal(np.sort(o["near"], axis=1), np.sort(e["near"], axis=1))
        assert np.array_equal(np.isnan(_f(o["order"])), np.isnan(_f(e["order"])))
        assert np.nanmax(np.abs(_f(o["order"] - e["order"]))) <= 1e-12


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_preconditions_of_the_exact_comparisons(case, evaluated):
    e, h, xyz, rs, rl = evaluated[case[0]]
    assert 0.0 < rl <= rs and rs * (1.0 + 1e-9) <= widths(h).min()
    g45, gs, gl = preconditions(e)
    n = e["counts"][:, 0]
    print(case[0], "N", len(xyz), "n_search", n.min(), n.max(), "4/5 gap %.1e" % g45, "to r_search %.1e" % gs, "to r_lsi %.1e" % gl)
    assert g45 > MARGIN and gs > MARGIN and gl > MARGIN


@pytest.mark.parametrize("name,n", BATCHES)
def test_preconditions_of_every_box_of_the_batches(name, n):
    hs, xs = batch_set(name, n)
    rs, rl = batch_radii(hs)
    for b in range(n):
        assert rs * (1.0 + 1e-9) <= widths(hs[b]).min()
        g45, gs, gl = preconditions(tet_exact(hs[b], xs[b], rs, rl))
        print(name, "box", b, "4/5 gap %.1e" % g45, "to r_search %.1e" % gs, "to r_lsi %.1e" % gl)
        assert g45 > MARGIN and gs > MARGIN and gl > MARGIN


def test_the_inputs_reach_every_branch(evaluated):
    past = {n: int((evaluated[f"gas N = {n}"][0]["counts"][:, 0] > KEEP).sum()) for n in (63, 64, 65)}
    assert past == {63: 63, 64: 64, 65: 65}                              # every molecule drops entries beyond the 16th
    for n in (255, 256, 257):
        e = evaluated[f"gas N = {n}"][0]
        assert (e["counts"][:, 0] < 4).sum() >= 8 and np.isnan(_f(e["order"][:, 3])).sum() >= 10
        assert (e["counts"][:, 0] > KEEP).sum() >= 8                     # (and the cap on both sides in one box)
    for n in (1, 2):
        assert not np.any(evaluated[f"gas N = {n}"][0]["summary"][4:7])
    assert np.all(evaluated["gas N = 65 in one cell"][0]["counts"][:, 0] >= KEEP)
    e = evaluated["ih48_t020 without LSI"][0]
    assert np.all(np.isnan(_f(e["order"][:, 3]))) and e["summary"][7] == 0 and np.isnan(float(e["summary"][3]))
    assert np.array_equal(_f(e["order"][:, :3]), _f(evaluated["ih48_t020"][0]["order"][:, :3]))
    e = evaluated["ih8_small"][0]
    assert any(len(set(row)) < 4 for row in e["near"].tolist())           # several images of one j among the nearest four
    # the LSI with a partly filled table: n_lsi + 1 = n_search <= 16 somewhere
    assert any(np.any((ev[0]["counts"][:, 1] + 1 == ev[0]["counts"][:, 0]) & (ev[0]["counts"][:, 0] <= KEEP)) for ev in evaluated.values())


def test_the_reference_imports_nothing_from_the_package():
    src = open(os.path.join(ROOT, "tests", "tet_ref.py")).read()
    assert not re.search(r"^\s*(from|import)\s+mc_water_ls_mw_amd", src, flags=re.M)
