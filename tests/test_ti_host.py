"""CPU: the host arithmetic of mc_water_ls_mw_amd.einstein (numpy; neither the library nor a device): the quadrature, the
integrand, the free energy of the Einstein crystal, the Frenkel-Ladd sum and its error, and the error paths."""
import math

import numpy as np
import pytest

from mc_water_ls_mw_amd import einstein, phonons
from mc_water_ls_mw_amd.einstein import MwError

KELVIN = 3.1668115634556e-6
MASS = 18.01528 * 1822.888486209


def test_gauss_legendre_integrates_degree_2n_minus_1_exactly_on_0_1():
    for n in (1, 2, 5, 12, 20):
        x, w = einstein.gauss_legendre(n)
        assert x.shape == (n,) and w.shape == (n,) and np.all(x > 0.0) and np.all(x < 1.0) and np.all(w > 0.0) and np.all(np.diff(x) > 0.0)
        for p in range(2 * n):
            assert abs(np.dot(w, x ** p) - 1.0 / (p + 1)) <= 1e-14, (n, p)
        if n <= 2:                                                                 # the next degree is not exact: 1 / 12 and 1 / 4320 off
            assert abs(np.dot(w, x ** (2 * n)) - 1.0 / (2 * n + 1)) > 1e-4
    with pytest.raises(MwError, match="gauss_legendre"):
        einstein.gauss_legendre(0)


def test_integrand_is_the_spring_energy_without_the_centre_of_mass_minus_the_mw_energy():
    rng = np.random.default_rng(3)
    blocks = rng.uniform(0.1, 1.0, size=(4, 6, 5))
    k = np.array([0.01, 0.02, 0.03, 0.04])
    y = einstein.integrand(blocks, k, 48)
    z = einstein.integrand(blocks, k, 48, com_free=False)
    assert y.shape == (4, 6) and z.shape == (4, 6)
    for b in range(4):
        for j in range(6):
            assert y[b, j] == 0.5 * k[b] * 48.0 * (blocks[b, j, 2] - blocks[b, j, 4]) - blocks[b, j, 0]
            assert z[b, j] == 0.5 * k[b] * 48.0 * blocks[b, j, 2] - blocks[b, j, 0]
    assert np.array_equal(einstein.integrand(blocks, 0.02, 48), einstein.integrand(blocks, np.full(4, 0.02), 48))
    # from displacements: U_E' is the spring energy of the displacements with their mean removed
    u = rng.normal(size=(48, 3))
    f2, f4 = (u * u).sum() / 48, ((u.sum(axis=0) / 48) ** 2).sum()
    row = np.array([[[0.0, 0.0, f2, 0.0, f4]]])
    assert abs(einstein.integrand(row, 0.02, 48)[0, 0] - 0.5 * 0.02 * ((u - u.mean(axis=0)) ** 2).sum()) <= 1e-14
    for bad, pattern in (((blocks[:, :, :4], k, 48), "blocks"), ((blocks, k[:3], 48), "springs"), ((blocks, -k, 48), "springs"), ((blocks, k, 0), "nwater")):
        with pytest.raises(MwError, match=pattern):
            einstein.integrand(*bad)


def test_einstein_free_energy_is_the_harmonic_free_energy_of_equal_frequencies():
    for n, k, T in ((48, 0.02, 100.0), (64, 0.005, 250.0), (2, 0.1, 200.0)):
        kT = T * KELVIN
        omega = np.full(3 * n, math.sqrt(k / MASS))
        want = phonons.harmonic_free_energy(omega, kT)                              # drops three of them as translations
        got = einstein.einstein_free_energy(n, k, MASS, kT)
        assert abs(got - want) <= 1e-13 * abs(want), (got, want)
        assert abs(einstein.einstein_free_energy(n, k, MASS, kT, com_free=False) - phonons.harmonic_free_energy(omega, kT, nzero=0)) <= 1e-13 * abs(want)
        assert abs(got - 3 * (n - 1) * kT * math.log(math.sqrt(k / MASS) / kT)) <= 1e-13 * abs(want)
    for bad in ((48, 0.0, MASS, 1e-3), (48, 0.02, MASS, 0.0), (0, 0.02, MASS, 1e-3), (48, 0.02, -1.0, 1e-3)):
        with pytest.raises(MwError, match="einstein_free_energy"):
            einstein.einstein_free_energy(*bad)


def test_frenkel_ladd_on_a_synthetic_integrand_with_a_known_integral():
    """<U_E' - E>_lambda = 3 lambda^5 - 2 lambda + 1/2 (integral 0 exactly) plus block noise of mean zero per node: F = F_E, and
    the error is that of the weighted block means."""
    x, w = einstein.gauss_legendre(12)
    f = 3.0 * x ** 5 - 2.0 * x + 0.5
    y = np.repeat(f[:, None], 8, axis=1)
    F, err = einstein.frenkel_ladd(x, w, y, -1.25)
    assert abs(F + 1.25) <= 1e-15 and err == 0.0
    noise = np.random.default_rng(5).normal(size=(12, 8)) * 1e-3
    noise -= noise.mean(axis=1, keepdims=True)
    F, err = einstein.frenkel_ladd(x, w, y + noise, -1.25)
    want = math.sqrt(sum(w[i] ** 2 * noise[i].var(ddof=1) / 8 for i in range(12)))
    assert abs(F + 1.25) <= 1e-15 and abs(err - want) <= 1e-15 and 1e-5 < err < 1e-3
    # an integrand with a known nonzero integral: e^lambda, integral e - 1
    F, _ = einstein.frenkel_ladd(x, w, np.exp(x)[:, None] * np.ones((1, 2)), 2.0)
    assert abs(F - (2.0 - (math.e - 1.0))) <= 1e-14
    F, err = einstein.frenkel_ladd(x, w, y[:, :1], 0.0)
    assert abs(F) <= 1e-15 and math.isnan(err)                                        # one block: no error
    for bad, pattern in (((x, w[:5], y, 0.0), "nodes"), ((x, w, y[:5], 0.0), "block_integrands"), ((x, w, y[:, :0], 0.0), "no blocks"),
                         ((x + 1.0, w, y, 0.0), "outside")):
        with pytest.raises(MwError, match=pattern):
            einstein.frenkel_ladd(*bad)


def test_spring_from_msd_and_the_number_of_blocks():
    kT = 250.0 * KELVIN
    assert einstein.spring_from_msd(0.3, kT) == 3.0 * kT / 0.3
    for bad in ((0.0, kT), (0.3, 0.0), (-1.0, kT)):
        with pytest.raises(MwError, match="spring_from_msd"):
            einstein.spring_from_msd(*bad)
    assert einstein.nblocks_of(40, 5, 7) == 5 and einstein.nblocks_of(40, 41, 7) == 0 and einstein.nblocks_of(40, 5, 0) == 0
    assert len(einstein.TRACE_FIELDS) == 5 and len(einstein.TI_ABI_SYMBOLS) == 9


def test_the_runs_check_their_arrays_before_they_load_anything():
    h, s = np.eye(3) * 20.0, np.zeros((4, 3))
    with pytest.raises(MwError, match="lambdas"):
        einstein.einstein_md(np.array([h, h]), np.array([s, s]), [0.1, 0.2, 0.3], 0.02, 1, 1.0)
    with pytest.raises(MwError, match="springs"):
        einstein.einstein_md(np.array([h, h]), np.array([s, s]), 0.5, [0.02], 1, 1.0)
    with pytest.raises(MwError, match="pos"):
        einstein.einstein_md(h, s, 0.5, 0.02, 1, 1.0, pos=np.zeros((5, 3)))
    with pytest.raises(MwError, match="streams"):
        einstein.einstein_md(h, s, 0.5, 0.02, 1, 1.0, streams=[1, 2])
