"""CPU: the numpy reference of the pair-distance histogram (tests/rdf_ref.py) against itself -- the image rule against brute
force over all images, the lattices' coordination shells, the normalisation on an ideal gas, translation and wrap
invariance -- and energy.rdf_from_counts."""
import numpy as np
import pytest

from conftest import golden_names, load_golden
from rdf_ref import ANG_TO_BOHR, assert_cap, assert_same, cumulative, rdf_brute, rdf_fast, widths

NBINS = 200
R10 = 10.0 * ANG_TO_BOHR


def _small_names():
    import os
    from conftest import GOLDEN
    out = []
    for name in golden_names():
        z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
        if "xyz" in z.files and len(z["xyz"]) <= 96:
            out.append(name)
    return out


def test_the_small_set_holds_the_boxes_the_rule_was_derived_on():
    names = _small_names()
    assert "ic64_sheared" in names and "ih8_small" in names and "single_atom" in names and "dimer" in names


@pytest.mark.parametrize("name", _small_names())
def test_the_image_rule_equals_brute_force(name):
    z = load_golden(name)
    wmin = widths(z["h"]).min()
    for r_max in (min(R10, 1.5 * wmin * (1.0 - 1e-6)), 0.499 * wmin):
        hb, eb = rdf_brute(z["h"], z["xyz"], r_max, NBINS)
        hf, ef = rdf_fast(z["h"], z["xyz"], r_max, NBINS, chunk=32)
        assert np.array_equal(eb, ef), (name, r_max)
        assert_cap(eb, name)
        assert_same(hf, hb, eb, (name, r_max))


def test_rdf_fast_refuses_more_than_three_images_per_axis():
    z = load_golden("ih48")
    with pytest.raises(ValueError):
        rdf_fast(z["h"], z["xyz"], 1.51 * widths(z["h"]).min(), NBINS)


def _within(hist, n, r_max, r_ang):
    """Neighbours per molecule within r_ang, which must be a bin edge; exact integer arithmetic."""
    b = r_ang * ANG_TO_BOHR * len(hist) / r_max
    assert abs(b - round(b)) < 1e-9
    total = int(cumulative(hist)[int(round(b))])
    assert total % n == 0
    return total // n


@pytest.mark.parametrize("name,pins", [
    ("ic4096_ideal", {3.5: 4, 4.9: 16, 5.8: 28, 6.6: 34, 7.3: 46, 8.0: 70, 8.6: 86}),
    ("ih4096_ideal", {3.5: 4, 4.5: 16, 4.9: 17, 5.8: 26}),
])
def test_coordination_shells_of_the_ideal_lattices(name, pins):
    z = load_golden(name)
    hist, edge = rdf_fast(z["h"], z["xyz"], R10, NBINS, workers=4)
    assert_cap(edge, name)
    n = len(z["xyz"])
    for r_ang, want in pins.items():
        assert _within(hist, n, R10, r_ang) == want, (name, r_ang)
    # between the shells the histogram is zero: the cumulative count only steps where a shell is
    steps = np.count_nonzero(hist[:int(round(8.6 / 10.0 * NBINS))]) if name == "ic4096_ideal" else None
    if steps is not None:
        assert steps <= 7 * 2                                  # seven shells, each in one bin or straddling an edge
    # the sum rule: every counted triple is in exactly one bin
    s = z["xyz"] @ np.linalg.inv(z["h"])
    ds = s[None, :64, :] - s[:, None, :]
    ds -= np.rint(ds)
    d = np.sqrt(((ds @ z["h"]) ** 2).sum(axis=2))              # these boxes are wider than 2 r_max: nearest image only
    assert widths(z["h"]).min() >= 2.0 * R10 * (1.0 + 1e-9)
    per_molecule = np.count_nonzero((d > 0.0) & (d < R10), axis=0)
    assert np.all(per_molecule == hist.sum() // n) and hist.sum() % n == 0


def test_sum_rule_on_a_small_box_with_images():
    z = load_golden("ih48_t020")
    r_max = 1.4 * widths(z["h"]).min()
    hist, _ = rdf_fast(z["h"], z["xyz"], r_max, 37)
    hist1, _ = rdf_fast(z["h"], z["xyz"], r_max, 1)
    assert hist.sum() == hist1[0]
    assert hist.sum() == rdf_brute(z["h"], z["xyz"], r_max, 1)[0][0]


def test_an_ideal_gas_has_g_of_one():
    """4000 uniform random points in a cubic box: hist[b] is Poisson with mean N rho V_shell(b), so g[b] = hist[b] / mean has
    the standard error 1 / sqrt(mean); every bin with a mean of at least 50 pairs must lie within 5 standard errors of 1."""
    from mc_water_ls_mw_amd.energy import rdf_from_counts
    rng = np.random.default_rng(20251016)
    n, side = 4000, 120.0
    h = np.eye(3) * side
    xyz = rng.random((n, 3)) * side
    r_max_ang = 20.0
    hist, _ = rdf_fast(h, xyz, r_max_ang * ANG_TO_BOHR, 50, workers=4)
    r, g, nn = rdf_from_counts(hist, n, side ** 3, r_max_ang)
    assert r.shape == g.shape == nn.shape == (50,) and abs(r[0] - 0.2) < 1e-12 and abs(r[-1] - 19.8) < 1e-12
    mean = hist / g
    ok = mean >= 50.0
    assert ok.sum() >= 40
    assert np.all(np.abs(g[ok] - 1.0) <= 5.0 / np.sqrt(mean[ok])), np.abs((g[ok] - 1.0) * np.sqrt(mean[ok])).max()
    assert np.array_equal(nn, np.cumsum(hist) / n)
    # the ordered-pair count: n(r_max) -> rho 4 pi r^3 / 3
    rho = n / side ** 3
    expect = rho * 4.0 * np.pi / 3.0 * (r_max_ang * ANG_TO_BOHR) ** 3
    assert abs(nn[-1] - expect) <= 5.0 * np.sqrt(expect / n) + 1e-9


def test_rdf_from_counts_is_vectorised_over_leading_axes():
    from mc_water_ls_mw_amd.energy import rdf_from_counts
    hist = np.arange(24, dtype=np.int64).reshape(2, 3, 4)
    vol = np.array([[1000.0, 1100.0, 1200.0], [900.0, 950.0, 990.0]])
    r, g, n = rdf_from_counts(hist, 10, vol, 8.0)
    assert r.shape == (4,) and g.shape == n.shape == (2, 3, 4)
    for a in range(2):
        for b in range(3):
            r1, g1, n1 = rdf_from_counts(hist[a, b], 10, vol[a, b], 8.0)
            assert np.array_equal(g1, g[a, b]) and np.array_equal(n1, n[a, b]) and np.array_equal(r1, r)
    dr = 2.0 * ANG_TO_BOHR
    assert np.isclose(g[0, 0, 1], hist[0, 0, 1] / (10 * (10 / 1000.0) * 4 * np.pi / 3 * (8 - 1) * dr ** 3), rtol=1e-14)


@pytest.mark.parametrize("name", ["ih48_t020", "ic64_sheared", "ic96"])
def test_translation_and_wrap_invariance(name):
    z = load_golden(name)
    h, xyz = z["h"], z["xyz"]
    r_max = min(R10, 1.5 * widths(h).min() * (1.0 - 1e-6))
    hist, edge = rdf_fast(h, xyz, r_max, NBINS)
    assert_cap(edge, name)
    rng = np.random.default_rng(5)
    moved = xyz + rng.uniform(-30.0, 30.0, 3)
    pick = rng.permutation(len(xyz))[:len(xyz) // 3]
    moved[pick] += rng.integers(-2, 3, (len(pick), 3)).astype(np.float64) @ h
    hist2, edge2 = rdf_fast(h, moved, r_max, NBINS)
    assert_same(hist2, hist, np.maximum(edge, edge2), name)
    hist3, edge3 = rdf_brute(h, moved, r_max, NBINS)           # no wrapping at all: the spread sets the images
    assert_same(hist3, hist, np.maximum(edge, edge3), name)
