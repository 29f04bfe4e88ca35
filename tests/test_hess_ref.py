"""CPU: the preconditions of tests/test_gpu_hess.py.  The autograd reference of tests/hess_ref.py restates the energy and the
forces of forces_ref.model_forces over the C oracle's lists, its H v agrees with central differences of those forces, the
synthetic narrow box has what it was made for, and the perfect lattice is a minimum with exactly three zero modes."""
import numpy as np
import pytest

import hess_ref
from conftest import RTOL
from quench_ref import F_ATOL, energy_forces, widths


@pytest.mark.parametrize("name", hess_ref.ORACLE_CASES)
def test_energy_and_gradient_match_the_force_reference(name):
    h, xyz = hess_ref.load_case(name)
    e_ref, f_ref = energy_forces(h, xyz)
    e, grad = hess_ref.energy(name).energy_gradient()
    print(name, "|E - E_ref|", abs(e - e_ref), "max |grad + F|", np.abs(grad + f_ref).max())
    assert abs(e - e_ref) <= RTOL * abs(e_ref)
    assert np.abs(grad + f_ref).max() <= F_ATOL


@pytest.mark.parametrize("name", ("gas20", "ic48_t015", "ic64_sheared", "ic65_interstitial", "ic96", "ih96_disordered", "ih1536_t012", "narrow6", "sc80"))
def test_matvec_matches_central_differences_of_the_forces(name):
    h, xyz = hess_ref.load_case(name)
    v = hess_ref.test_vectors(name)[0]                                  # a seeded unit vector
    hv = hess_ref.matvec_reference(name)[0]
    _, fp = energy_forces(h, xyz + hess_ref.FD_STEP * v)
    _, fm = energy_forces(h, xyz - hess_ref.FD_STEP * v)
    fd = -(fp - fm) / (2.0 * hess_ref.FD_STEP)
    gap = np.abs(fd - hv).max() / np.abs(hv).max()
    print(name, "central differences against H v, relative to max |H v|:", gap)
    assert gap <= 10.0 * hess_ref.FD_GAP_MEASURED


@pytest.mark.parametrize("name", ("dimer", "gas20", "ic48_t015", "narrow6", "sc80"))
def test_reference_is_symmetric_and_obeys_the_sum_rule(name):
    H = hess_ref.dense_reference(name)
    n = H.shape[0] // 3
    scale = max(np.abs(H).max(), 1e-300)
    rows = H.reshape(3 * n, n, 3).sum(axis=1)
    hv = hess_ref.matvec_reference(name)
    dense_hv = np.einsum("ab,vb->va", H, hess_ref.test_vectors(name).reshape(len(hv), -1)).reshape(hv.shape)
    print(name, "max |H|", scale, "asymmetry", np.abs(H - H.T).max(), "sum rule", np.abs(rows).max(), "matvec - dense", np.abs(hv - dense_hv).max())
    assert np.abs(H - H.T).max() <= 1e-13 * scale and np.abs(rows).max() <= 1e-13 * scale
    assert np.abs(hv - dense_hv).max() <= 1e-13 * scale


def test_single_atom_has_the_zero_hessian():
    assert np.array_equal(hess_ref.dense_reference("single_atom"), np.zeros((3, 3)))


def test_narrow_box_has_two_images_of_one_neighbour():
    h, xyz = hess_ref.load_case("narrow6")
    rc = hess_ref.rc()
    assert xyz.shape == (6, 3) and np.allclose(h, np.eye(3) * 1.1 * rc) and widths(h).min() >= rc * (1.0 + 1e-9)
    i, j, shift, n = hess_ref.entries(h, xyz)
    d = xyz[j] + shift - xyz[i]
    assert np.sqrt((d * d).sum(axis=1)).min() > 4.0                     # no pair closer than 4 bohr, images included
    pairs = list(zip(i.tolist(), j.tolist()))
    doubled = sorted({p for p in pairs if pairs.count(p) > 1})
    print("narrow6: entries", len(i), "pairs (i, j) with more than one image:", doubled)
    assert doubled
    assert len({(a, b, *t) for a, b, t in zip(i.tolist(), j.tolist(), n.tolist())}) == len(i)


def test_the_cubic_box_has_rows_wider_than_the_device_table():
    h, xyz = hess_ref.load_case("sc80")
    cols = hess_ref.row_columns(h, xyz)
    i, _, _, _ = hess_ref.entries(h, xyz)
    print("sc80: entries per molecule", np.bincount(i).min(), "...", np.bincount(i).max(), "columns per row", cols.min(), "...", cols.max())
    assert xyz.shape == (80, 3) and widths(h).min() >= hess_ref.rc() * (1.0 + 1e-9)
    assert cols.min() > hess_ref.TABLE_COLUMNS
    for name in ("ic96", "ih96_disordered", "gas20"):                   # and the other cases stay within it
        assert hess_ref.row_columns(*hess_ref.load_case(name)).max() <= hess_ref.TABLE_COLUMNS, name


def test_perfect_lattice_is_a_minimum_with_three_zero_modes():
    lam = np.linalg.eigvalsh(hess_ref.dense_reference("ic96"))
    print("ic96: lowest eigenvalue", lam[0], "largest", lam[-1], "below 1e-12:", int((np.abs(lam) < 1e-12).sum()))
    assert lam[0] >= -1e-12 and int((np.abs(lam) < 1e-12).sum()) == 3
