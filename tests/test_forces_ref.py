"""CPU: the numpy force/virial reference (tests/forces_ref.py) is the gradient of the C oracle's energy.

Its energy equals COracle.model_energy, its forces equal central differences of that energy in every coordinate, its virial
equals the central difference under a small symmetric strain of positions and cell (same list, image vectors of the strained
cell), the forces sum to zero and the virial is symmetric.  This is what makes the GPU force tests' reference trustworthy.
"""
import numpy as np
import pytest

from conftest import load_golden
from forces_ref import model_forces, strained

BOXES = ["dimer", "gas20", "ih8_small", "ic64_sheared", "ih48_t020"]


def _box(name):
    z = load_golden(name)
    return z["h"], z["xyz"], z["ivect"], z["nn"], z["jn"], z["vn"]


@pytest.mark.parametrize("name", BOXES)
def test_energy_equals_the_oracle(name, c_oracle):
    h, xyz, iv, nn, jn, vn = _box(name)
    e, _, _ = model_forces(xyz, iv, nn, jn, vn)
    e_ref = c_oracle.model_energy(xyz, iv, nn, jn, vn)
    assert abs(e - e_ref) <= 1e-12 * abs(e_ref), (e, e_ref)


@pytest.mark.parametrize("name", BOXES)
def test_forces_are_central_differences_of_the_oracle_energy(name, c_oracle):
    h, xyz, iv, nn, jn, vn = _box(name)
    _, f, _ = model_forces(xyz, iv, nn, jn, vn)
    assert np.abs(f).max() > 0.0
    step = 1e-5
    fd = np.zeros_like(f)
    for i in range(len(xyz)):
        for c in range(3):
            xp, xm = xyz.copy(), xyz.copy()
            xp[i, c] += step
            xm[i, c] -= step
            fd[i, c] = -(c_oracle.model_energy(xp, iv, nn, jn, vn) - c_oracle.model_energy(xm, iv, nn, jn, vn)) / (2 * step)
    err = np.abs(f - fd).max()
    assert err <= 1e-7 * np.abs(f).max(), (err, np.abs(f).max())


@pytest.mark.parametrize("name", BOXES)
def test_virial_is_the_strain_derivative_of_the_oracle_energy(name, c_oracle):
    h, xyz, iv, nn, jn, vn = _box(name)
    _, _, w = model_forces(xyz, iv, nn, jn, vn)
    step = 1e-6
    fd = np.zeros((3, 3))
    for a in range(3):
        for b in range(a, 3):
            eps = np.zeros((3, 3))
            eps[a, b] = eps[b, a] = step          # symmetric strain: a != b moves both W_ab and W_ba
            es = []
            for sgn in (1.0, -1.0):
                hs, xs = strained(h, xyz, sgn * eps)
                ivs = c_oracle.ivects(hs)
                assert ivs.shape == iv.shape
                es.append(c_oracle.model_energy(xs, ivs, nn, jn, vn))
            dE = (es[0] - es[1]) / (2 * step)
            fd[a, b] = fd[b, a] = -dE if a == b else -dE / 2
    scale = np.abs(w).max()
    assert scale > 0.0
    sym = 0.5 * (w + w.T)
    assert np.abs(sym - fd).max() <= 1e-6 * scale, (w, fd)


@pytest.mark.parametrize("name", BOXES)
def test_forces_sum_to_zero_and_the_virial_is_symmetric(name):
    h, xyz, iv, nn, jn, vn = _box(name)
    _, f, w = model_forces(xyz, iv, nn, jn, vn)
    assert np.abs(f.sum(axis=0)).max() <= 1e-12 * np.abs(f).sum()
    assert np.abs(w - w.T).max() <= 1e-12 * np.abs(w).max()


def test_self_images_move_nothing_but_enter_the_virial(c_oracle):
    """ih8_small's cell edge is below the cutoff: molecules meet images of themselves in range."""
    h, xyz, iv, nn, jn, vn = _box("ih8_small")
    self_entries = sum(int(np.sum(jn[i, :nn[i]] == i + 1)) for i in range(len(xyz)))
    assert self_entries > 0
    # a rigid translation of every molecule changes nothing: the self-image entries contribute no net force
    _, f, _ = model_forces(xyz, iv, nn, jn, vn)
    e0 = c_oracle.model_energy(xyz, iv, nn, jn, vn)
    e1 = c_oracle.model_energy(xyz + np.array([0.3, -0.2, 0.1]), iv, nn, jn, vn)
    assert abs(e1 - e0) <= 1e-12 * abs(e0)
    assert np.abs(f.sum(axis=0)).max() <= 1e-12 * np.abs(f).sum()


def test_single_molecule_has_no_force():
    h, xyz, iv, nn, jn, vn = _box("single_atom")
    _, f, _ = model_forces(xyz, iv, nn, jn, vn)
    assert np.array_equal(f, np.zeros_like(f))
