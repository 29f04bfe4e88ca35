"""CPU: the host arithmetic of mc_water_ls_mw_amd.phonons -- normal modes, the harmonic free energy in both forms, the density
of modes and the participation ratio -- against hand-built matrices and closed forms.  None of it needs the device library."""
import numpy as np
import pytest

from mc_water_ls_mw_amd import phonons
from mc_water_ls_mw_amd.phonons import MwError


def _matrix_with_spectrum(lam, seed=2):
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((len(lam), len(lam))))
    return q @ np.diag(lam) @ q.T, q


def test_normal_modes_of_a_matrix_with_known_spectrum():
    lam = np.array([-4.0, 0.25, 1.0, 9.0, 16.0, 25.0])
    H, q = _matrix_with_spectrum(lam)
    mass = 4.0
    omega = phonons.normal_modes(H, mass=mass)
    assert np.allclose(omega, [-1.0, 0.25, 0.5, 1.5, 2.0, 2.5], atol=1e-12) and np.all(np.diff(omega) >= 0.0)
    # the antisymmetric part of a slightly asymmetric matrix is left out
    skew = np.triu(np.ones((6, 6)), 1) * 1e-3
    assert np.allclose(phonons.normal_modes(H + skew - skew.T, mass=mass), omega, atol=1e-12)
    omega2, vec = phonons.normal_modes(H, mass=mass, vectors=True)
    assert np.allclose(omega2, omega, atol=1e-13) and vec.shape == (6, 6)       # (LAPACK's two drivers differ in the last bits)
    assert np.allclose(np.abs(vec.T @ q), np.eye(6), atol=1e-9)          # the eigenvectors, column m with omega[m], up to sign
    assert np.allclose(phonons.normal_modes(np.diag([2.0, 8.0, 18.0]), mass=2.0), [1.0, 2.0, 3.0])
    assert phonons.normal_modes(np.diag([8.0, 0.0, -2.0]), mass=2.0).tolist() == [-1.0, 0.0, 2.0]      # a zero mode stays zero, a negative one keeps its sign
    assert phonons.normal_modes(np.eye(3))[0] == pytest.approx(1.0 / np.sqrt(phonons.MASS_WATER))
    with pytest.raises(MwError, match="square"):
        phonons.normal_modes(np.zeros((3, 4)))


def test_harmonic_free_energy_against_closed_forms():
    kT = 0.5
    omega = np.array([1e-9, -2e-9, 3e-10, 0.25, 1.0, 2.0])              # three translations and three given frequencies
    classical = kT * (np.log(0.25 / kT) + np.log(1.0 / kT) + np.log(2.0 / kT))
    assert phonons.harmonic_free_energy(omega, kT) == pytest.approx(classical, rel=1e-14)
    assert classical == pytest.approx(kT * np.log(0.25 * 1.0 * 2.0 / kT ** 3), rel=1e-13)
    quantum = sum(kT * np.log(2.0 * np.sinh(w / (2 * kT))) for w in (0.25, 1.0, 2.0))   # w / 2 + kT ln(1 - exp(-w / kT)) = kT ln(2 sinh(w / 2 kT))
    assert phonons.harmonic_free_energy(omega, kT, quantum=True) == pytest.approx(quantum, rel=1e-13)
    # the quantum form tends to the classical one where kT is far above every frequency, and to the zero-point energy far below
    assert phonons.harmonic_free_energy(omega, 1e4, quantum=True) == pytest.approx(phonons.harmonic_free_energy(omega, 1e4), rel=1e-8)
    assert phonons.harmonic_free_energy(omega, 1e-3, quantum=True) == pytest.approx(0.5 * (0.25 + 1.0 + 2.0), rel=1e-12)
    # nzero: the modes of smallest |omega| go, whatever their order and sign
    assert phonons.harmonic_free_energy([2.0, 1e-9, 0.25, -2e-9, 1.0, 3e-10], kT) == pytest.approx(classical, rel=1e-14)
    assert phonons.harmonic_free_energy([0.25, 1.0, 2.0], kT, nzero=0) == pytest.approx(classical, rel=1e-14)
    assert phonons.harmonic_free_energy([0.25, 1.0, 2.0], kT, nzero=1) == pytest.approx(kT * (np.log(1.0 / kT) + np.log(2.0 / kT)), rel=1e-14)


def test_harmonic_free_energy_raises_for_a_kept_mode_that_is_not_positive():
    with pytest.raises(MwError, match="not positive.*not a minimum"):
        phonons.harmonic_free_energy([1e-9, 1e-9, 1e-9, -0.5, 1.0, 2.0], 0.5)
    with pytest.raises(MwError, match="not positive"):
        phonons.harmonic_free_energy([0.0, 1.0], 0.5, nzero=0)
    with pytest.raises(MwError, match="not positive"):
        phonons.harmonic_free_energy([-0.5, 1e-9, 1e-9, 1e-9, 1.0], 0.5, quantum=True)
    with pytest.raises(MwError, match="kT"):
        phonons.harmonic_free_energy([1.0, 2.0], 0.0, nzero=0)
    with pytest.raises(MwError, match="nzero"):
        phonons.harmonic_free_energy([1.0, 2.0], 0.5, nzero=3)


def test_mode_dos_counts():
    omega = [0.05, 0.1, 0.15, 0.15, 0.3, 0.45, 0.5, 0.9]
    counts = phonons.mode_dos(omega, [0.0, 0.1, 0.2, 0.5, 1.0])
    assert counts.tolist() == [1, 3, 2, 2] and counts.sum() == len(omega)
    assert phonons.mode_dos(omega, [0.2, 0.4]).tolist() == [1]            # modes outside the edges are not counted
    assert phonons.mode_dos([0.5], [0.0, 0.5]).tolist() == [1]            # the last bin is closed


def test_participation_ratio_of_uniform_and_localised_vectors():
    n = 7
    uniform = np.tile([1.0, 0.0, 0.0], n) / np.sqrt(n)
    local = np.zeros(3 * n)
    local[3 * 4:3 * 4 + 3] = np.array([1.0, 2.0, 2.0]) / 3.0
    half = np.zeros(3 * n + 3)                                          # four of eight molecules move equally
    half[:12] = 1.0
    assert phonons.participation_ratio(uniform) == pytest.approx([1.0])
    assert phonons.participation_ratio(local) == pytest.approx([1.0 / n])
    assert phonons.participation_ratio(half) == pytest.approx([0.5])
    assert phonons.participation_ratio(np.stack([uniform, local], axis=1)) == pytest.approx([1.0, 1.0 / n])
    assert phonons.participation_ratio(5.0 * uniform) == pytest.approx([1.0])      # the norm does not matter
    with pytest.raises(MwError, match="3 N"):
        phonons.participation_ratio(np.ones(7))
