"""CPU: the two numpy evaluations of S(k) in tests/sk_ref.py against each other and against what the definition demands of
ideal lattices, single atoms, shifted boxes and an ideal gas; structure.kvectors, k_lengths and sq_from_sk."""
import numpy as np
import pytest

from conftest import golden_names, load_golden
from sk_ref import LD, assert_within, delta, have_extended_precision, s_max, sk_exact, sk_tables, vectors_for

pytestmark = pytest.mark.skipif(not have_extended_precision(), reason="np.longdouble has no 64-bit mantissa on this machine")

SMALL = [n for n in golden_names() if not any(t in n for t in ("4096", "32768"))]


def _c(exact):
    return exact[0].astype(np.float64) + 1j * exact[1].astype(np.float64)


@pytest.mark.parametrize("name", SMALL)
def test_tables_agree_with_exact_on_every_small_golden_box(name):
    z = load_golden(name)
    h, xyz = z["h"], z["xyz"]
    assert len(xyz) <= 1536
    nvec = vectors_for(h)
    assert 1 <= len(nvec) <= 4096 and len(xyz) * len(nvec) <= 10 ** 7
    rho, S = sk_tables(h, xyz, nvec)
    assert_within(rho, S, sk_exact(h, xyz, nvec), nvec, len(xyz), s_max(h, xyz), name)


def test_ideal_cubic_ice_has_the_diamond_reflections():
    from mc_water_ls_mw_amd import lattice as lat
    reps = np.array([3, 2, 4])
    h, xyz = lat.ice_box("ic", tuple(reps))
    n = len(xyz)
    hkl = {"full": [(2, 2, 0), (4, 0, 0), (0, 4, 4)], "half": [(1, 1, 1), (3, 1, 1), (1, -3, 1)],
           "none": [(2, 0, 0), (2, 2, 2), (1, 1, 0), (4, 2, 0)]}
    smax = s_max(h, xyz)
    for kind, want in (("full", float(n)), ("half", n / 2.0), ("none", 0.0)):
        nvec = np.array(hkl[kind]) * reps
        for rho, S in (sk_tables(h, xyz, nvec), (_c(sk_exact(h, xyz, nvec)), sk_exact(h, xyz, nvec)[2].astype(np.float64))):
            d = delta(nvec, n, smax)
            bound = (2.0 * np.sqrt(want * n) * d + d * d) / n
            print(kind, S, bound)
            assert np.all(np.abs(S - want) <= bound), (kind, S)
    off = np.array([[2 * reps[0] + 1, 2 * reps[1], 0], [1, 0, 0], [4 * reps[0], 1, 0]])          # not multiples of reps
    rho, S = sk_tables(h, xyz, off)
    d = delta(off, n, smax)
    assert np.all(S <= d * d / n), S


def test_a_single_atom_scatters_with_unit_intensity():
    z = load_golden("single_atom")
    nvec = np.array([[0, 0, 0], [1, 0, 0], [-3, 7, 2], [255, 0, 0], [0, -255, 255], [17, 17, -17]])
    rho, S = sk_tables(z["h"], z["xyz"], nvec)
    re, im, s_ex = sk_exact(z["h"], z["xyz"], nvec)
    assert np.all(np.abs(S - 1.0) <= 4 * 2.0 ** -52)
    assert np.all(np.abs(s_ex.astype(np.float64) - 1.0) <= 2.0 ** -52)
    assert rho[0] == 1.0 and re[0] == 1 and im[0] == 0


def test_a_common_shift_turns_rho_and_keeps_s():
    z = load_golden("ic48_t015")
    h, xyz = z["h"], z["xyz"]
    nvec = vectors_for(h, m_target=300)
    t = np.array([1.234, -0.777, 3.21])
    re0, im0, s0 = sk_exact(h, xyz, nvec)
    re1, im1, s1 = sk_exact(h, xyz + t, nvec)
    from mc_water_ls_mw_amd.structure import _kvec_bohr
    turn = np.exp(-1j * (_kvec_bohr(h, nvec) @ t))
    d = delta(nvec, len(xyz), max(s_max(h, xyz), s_max(h, xyz + t)))
    assert np.all(np.abs((re1 + 1j * im1).astype(np.complex128) - (re0 + 1j * im0).astype(np.complex128) * turn) <= 2 * d)
    assert np.all(np.abs((s1 - s0).astype(np.float64)) <= 2 * (2 * np.sqrt((s0 * len(xyz)).astype(np.float64)) * d + d * d) / len(xyz))


def test_lattice_translations_of_some_molecules_leave_rho_alone():
    z = load_golden("ic64_sheared")
    h, xyz = z["h"], z["xyz"]
    nvec = vectors_for(h, m_target=500)
    rng = np.random.default_rng(5)
    moved = xyz.copy()
    pick = rng.permutation(len(xyz))[:20]
    moved[pick] += rng.integers(-3, 4, (len(pick), 3)).astype(np.float64) @ h
    assert not np.array_equal(moved, xyz)
    exact = sk_exact(h, xyz, nvec)
    smax = s_max(h, moved)
    assert smax > 2.0
    for f in (sk_tables, lambda *a: (_c(sk_exact(*a)), sk_exact(*a)[2].astype(np.float64))):
        rho, S = f(h, moved, nvec)
        assert_within(rho, S, exact, nvec, len(xyz), smax, "translated")


def test_an_ideal_gas_has_unit_mean_intensity():
    rng = np.random.default_rng(2024)
    n = 20000
    h = np.diag([90.0, 100.0, 110.0])
    xyz = rng.random((n, 3)) @ h
    nvec = vectors_for(h, m_target=2100, m_cap=2500)
    m = len(nvec)
    assert m >= 2000
    _, S = sk_tables(h, xyz, nvec)
    # S of a gas is exponentially distributed with mean 1 (and variance 1): the standard error of the mean is 1 / sqrt(M)
    print("mean S", S.mean(), "M", m, "5 standard errors", 5.0 / np.sqrt(m))
    assert abs(S.mean() - 1.0) <= 5.0 / np.sqrt(m)


def _brute_vectors(h, k_max_ang, lim=12):
    from mc_water_ls_mw_amd.structure import k_lengths
    r = np.arange(-lim, lim + 1)
    n = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    k = k_lengths(h, n)
    return n[(k > 0) & (k <= k_max_ang)]


def test_kvectors_is_exactly_the_half_space():
    from mc_water_ls_mw_amd.structure import k_lengths, kvectors
    h = load_golden("ic64_sheared")["h"]
    k_max = 2.9
    full = _brute_vectors(h, k_max)
    assert np.abs(full).max() < 12                                   # the brute-force cube holds the whole sphere
    half = kvectors(h, k_max, half=True)
    both = kvectors(h, k_max, half=False)
    assert half.dtype == np.int32 and half.shape[1] == 3
    assert len(full) % 2 == 0 and len(half) == len(full) // 2 and len(both) == len(full)
    as_set = {tuple(v) for v in half.tolist()}
    assert len(as_set) == len(half)
    assert all((-a, -b, -c) not in as_set for a, b, c in as_set)
    assert as_set | {(-a, -b, -c) for a, b, c in as_set} == {tuple(v) for v in full.tolist()}
    assert {tuple(v) for v in both.tolist()} == {tuple(v) for v in full.tolist()}
    for a, b, c in as_set:
        assert a > 0 or (a == 0 and (b > 0 or (b == 0 and c > 0)))
    k = k_lengths(h, half)
    assert np.all(k > 0) and np.all(k <= k_max) and np.all(np.diff(k) >= 0)
    for i in np.nonzero(np.diff(k) == 0)[0]:
        assert tuple(half[i]) < tuple(half[i + 1])
    # |k| against the definition, 2 pi H^-T n with H's columns the cell vectors
    kv = 2.0 * np.pi * np.linalg.inv(h.T).T @ half[7]
    assert abs(np.linalg.norm(kv) / 0.5291772108 - k[7]) <= 1e-12


def test_sq_from_sk_on_a_hand_made_input():
    from mc_water_ls_mw_amd.structure import sq_from_sk
    klen = np.array([0.5, 1.0, 1.5, 1.6, 3.9, 4.0, 4.5, 0.0])
    S = np.array([[1.0, 2.0, 3.0, 5.0, 7.0, 9.0, 100.0, 100.0], [2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0]])
    q, sq, count = sq_from_sk(S, klen, 4.0, 4)
    assert np.array_equal(q, [0.5, 1.5, 2.5, 3.5])
    assert np.array_equal(count, [2, 2, 0, 2])                          # 1.0 closes bin 0, 4.0 closes bin 3; 4.5 and 0 are outside
    assert np.array_equal(sq[0, [0, 1, 3]], [1.5, 4.0, 8.0]) and np.isnan(sq[0, 2])
    assert np.array_equal(sq[1, [0, 1, 3]], [2.0, 2.0, 2.0]) and np.isnan(sq[1, 2])
    q1, sq1, c1 = sq_from_sk(S[0], klen, 4.0, 4)
    assert sq1.shape == (4,) and np.array_equal(c1, count) and np.array_equal(sq1[[0, 1, 3]], sq[0, [0, 1, 3]])
