"""CPU: the inputs of tests/derived_cases.py test what they claim, and the comparison rules of tests/test_gpu_derived_shapes.py
cannot hide a failure on them -- from the numpy mirrors and the C oracle alone.

Four conditions on the inputs (where a case breaks one, its seed is changed, not the rule): the engine accepts every box (image
table, maxneigh = 64, no pair below 2.0 Angstrom); at most one bin edge of a g(r) case has a pair within rdf_ref.EDGE_TOL of it;
no CHILL+ bond value lies within 1e-9 of a class threshold; rdf_fast equals rdf_brute on every case up to 257 molecules, which is
what licenses rdf_fast as the reference of the larger ones.  Six sensitivity checks: the bug a case is aimed at, written as a
change to the pair weights of rdf_ref's definition, moves that case's histogram by more than the edge allowance."""
import numpy as np
import pytest

import derived_cases as dc
from ice_ref import ANG_TO_BOHR, ECLIPSED, RC_ANG, STAGGERED, ice_classes
from rdf_ref import assert_cap, assert_same, image_range, rdf_brute, rdf_fast, widths

RC = RC_ANG * ANG_TO_BOHR
TILES = {65: 1, 255: 1, 256: 1, 257: 2, 513: 3, 768: 3, 1025: 5, 1281: 6}
SMALL_N = (2, 3, 5, 31, 63, 64)


def _own_boxes():
    """label -> (h, xyz) of every box derived_cases makes itself."""
    out = {"rdf:" + name: (c.h, c.xyz) for name, c in dc.RDF_CASES.items()}
    out["degenerate"] = dc.DEGENERATE
    for n, boxes in dc.BATCHES.items():
        for b, box in enumerate(boxes):
            out[f"batch{n}:{b}"] = box
    return out


OWN = _own_boxes()
FUZZ = {seed: (kind, h, x) for seed, kind, h, x in dc.fuzz_systems()}


# -- every case is what its row says ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(dc.RDF_CASES))
def test_a_case_has_its_stated_size_tiles_parity_and_images(name):
    c = dc.RDF_CASES[name]
    assert c.xyz.shape == (c.n, 3) and c.h.shape == (3, 3)
    kind, _, rest = name.partition("_n")
    if kind in ("small", "tiles", "unwrapped") or kind.startswith("bins"):
        n = int(rest.split("_")[0])
        assert c.n == n and (n <= dc.SMALL_MAX) == (kind in ("small", "unwrapped") or n == 63)
        if kind == "tiles":
            assert -(-n // dc.TILE) == TILES[n]
    if kind.startswith("bins"):
        assert c.nbins == int(kind[4:])
    r = dc.bohr(c.r_max_ang)
    assert tuple(image_range(r, w) for w in widths(c.h)) == c.images          # (raises beyond 1.5 w)
    if name.startswith("images_") and name != "images_limit":
        assert "%d%d%d" % c.images == name[7:]
    if not name.startswith("images_"):
        assert c.r_max_ang == min(10.0, 1.5 * widths(c.h).min() * (1.0 - 1e-6) * dc.BOHR_TO_ANG)


def test_the_table_has_every_row_of_its_plan():
    cases = dc.RDF_CASES
    for n in SMALL_N:                                       # k_rdf_small: odd and even N, orthogonal and sheared
        a, b = cases[f"small_n{n}"], cases[f"small_n{n}_sheared"]
        assert a.n == b.n == n and np.count_nonzero(a.h - np.diag(np.diag(a.h))) == 0
        assert np.count_nonzero(b.h - np.diag(np.diag(b.h))) == 6
        if n <= 5:
            assert widths(a.h).min() * dc.BOHR_TO_ANG >= 9.0 and widths(b.h).min() * dc.BOHR_TO_ANG >= 9.0
    assert {n % 2 for n in SMALL_N} == {0, 1}
    for n, t in TILES.items():                              # k_rdf_tiles: odd and even T, full and ragged last tiles
        assert cases[f"tiles_n{n}_cube"].images == (0, 0, 0) and 1 in cases[f"tiles_n{n}_slab"].images
    assert {t % 2 for t in TILES.values()} == {0, 1} and {n % dc.TILE == 0 for n in TILES} == {True, False}
    assert TILES[257] == 2 and 257 % dc.TILE == 1           # a last tile of one molecule next to a full one
    # all eight image sets on the oblique family, each against rdf_brute
    family = [c for name, c in cases.items() if name.startswith("images_") and name != "images_limit"]
    assert {c.images for c in family} == {(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)}
    assert all(c.n <= 96 and c.n <= dc.BRUTE_MAX and np.count_nonzero(c.h - np.diag(np.diag(c.h))) == 6 for c in family)
    lim = cases["images_limit"]
    w = widths(lim.h)
    assert dc.bohr(lim.r_max_ang) > 1.4999 * w.min() and np.linalg.norm(lim.h, axis=1).min() > 1.03 * w.min()
    for nbins in (1, 7, 4096):
        assert cases[f"bins{nbins}_n63"].n == 63 and cases[f"bins{nbins}_n257"].n == 257
    # unwrapped: odd N, positions up to three cells outside the cell
    u = cases["unwrapped_n31"]
    s = u.xyz @ np.linalg.inv(u.h)
    assert u.n % 2 == 1 and s.min() < -2.0 and s.max() > 3.0
    # the shear matrix: all six off-diagonal entries, of mixed sign
    off = dc.SHEAR_M[~np.eye(3, dtype=bool)]
    assert np.all(off != 0.0) and off.min() < 0.0 < off.max() and np.all(np.diag(dc.SHEAR_M) == 0.0)


def test_generators_return_exactly_n_molecules_in_ascending_site_order():
    from mc_water_ls_mw_amd import lattice as lat
    for n in (1, 2, 63, 64, 65, 257):
        h, x = dc.vacancy_ice(n, 5)
        assert x.shape == (n, 3)
        hg, xg = dc.gas(n, 5, (30.0, 31.0, 32.0))
        assert xg.shape == (n, 3) and dc.min_separation(hg, xg) > dc.MIN_SEP_ANG * ANG_TO_BOHR
    # the kept molecules are a subset of the thermalised lattice, in the lattice's order
    h0, x0 = lat.replicate(*lat.ice_ic_cell(), (2, 2, 2))
    x0 = lat.thermalise(x0, 0.08, 9)
    h, x = dc.vacancy_ice(31, 9, (2, 2, 2))
    idx = [int(np.nonzero(np.all(x0 == r, axis=1))[0][0]) for r in x]
    assert np.array_equal(h, h0) and idx == sorted(idx) and len(set(idx)) == 31
    a, b = dc.vacancy_ice(31, 9, (2, 2, 2), shear=0.3), dc.vacancy_ice(31, 9, (2, 2, 2), shear=0.3)
    assert np.array_equal(a[1], b[1]) and np.allclose(a[1], x @ (np.eye(3) + 0.3 * dc.SHEAR_M), rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        dc.vacancy_ice(65, 1, (2, 2, 2))


# -- the engine accepts every box; no bond value at a threshold -------------------------------------------------------------------
def _lists(c_oracle, h, x):
    iv = c_oracle.ivects(h)
    return (iv,) + tuple(c_oracle.neighbours(x, iv, 64))


def _threshold_margin(x, iv, nn, jn, vn):
    """The smallest distance of a CHILL+ bond value of the box from a class threshold (inf where it has no bond)."""
    _, c, _ = ice_classes(x, iv, nn, jn, vn, RC)
    live = c[(c != 2.0) & ~np.isnan(c)]
    if len(live) == 0:
        return np.inf
    return float(min(np.abs(live - t).min() for t in (STAGGERED,) + ECLIPSED))


@pytest.mark.parametrize("label", list(OWN))
def test_the_engine_accepts_a_box_and_no_bond_value_is_at_a_threshold(label, c_oracle):
    h, x = OWN[label]
    iv, nn, jn, vn = _lists(c_oracle, h, x)
    assert len(iv) <= 1000, "cell too thin for the image table"
    assert nn.max() <= 64, "denser than maxneigh = 64"
    assert dc.min_separation(h, x) > dc.MIN_SEP_ANG * ANG_TO_BOHR
    margin = _threshold_margin(x, iv, nn, jn, vn)
    print(label, "N", len(x), "image vectors", len(iv), "max n_i", int(nn.max()), "threshold margin", margin)
    assert margin > 1e-9


def test_the_fuzz_systems_are_not_skipped_and_no_bond_value_is_at_a_threshold(c_oracle):
    """The two skip rules of tests/test_gpu_fuzz.py on the 36 seeds (measured: none fires) and the threshold margin
    (measured: 8e-5 at the smallest)."""
    skipped, margins = [], []
    for seed, (kind, h, x) in FUZZ.items():
        iv = c_oracle.ivects(h)
        if len(iv) > 1000:
            skipped.append((seed, "image table"))
            continue
        nn, jn, vn = c_oracle.neighbours(x, iv, 64)
        if nn.max() > 64:
            skipped.append((seed, "maxneigh"))
            continue
        margins.append(_threshold_margin(x, iv, nn, jn, vn))
    print("skipped", skipped, "smallest threshold margin", min(margins))
    assert len(skipped) <= 2, skipped
    assert min(margins) > 1e-9


# -- the edge rule cannot hide a failure; rdf_fast is rdf_brute ---------------------------------------------------------------------
@pytest.mark.parametrize("name", list(dc.RDF_CASES))
def test_edge_cap_and_fast_equals_brute(name):
    c = dc.RDF_CASES[name]
    ref, edge = dc.rdf_reference(name)
    assert_cap(edge, name)
    assert ref.shape == (c.nbins,) and ref.sum() > 0
    if c.n <= dc.BRUTE_MAX:
        fast, fast_edge = rdf_fast(c.h, c.xyz, dc.bohr(c.r_max_ang), c.nbins)
        assert np.array_equal(fast, ref) and np.array_equal(fast_edge, edge), name
    else:
        assert name.startswith("tiles_")


def test_unwrapped_positions_have_the_histogram_of_the_wrapped_ones():
    u = dc.RDF_CASES["unwrapped_n31"]
    h, x = dc.vacancy_ice(31, 231, (2, 2, 2), shear=0.3)
    assert not np.array_equal(u.xyz, x)
    ref, edge = dc.rdf_reference("unwrapped_n31")
    assert_same(rdf_brute(h, x, dc.bohr(u.r_max_ang), u.nbins)[0], ref, edge)


def _box_r_ang(label):
    return dc.batch_r_max_ang(dc.BATCHES[int(label[5:].split(":")[0])])


@pytest.mark.parametrize("label", [k for k in OWN if k.startswith("batch")])
def test_edge_cap_of_the_batch_boxes(label):
    h, x = OWN[label]
    _, edge = rdf_brute(h, x, dc.bohr(_box_r_ang(label)), 200)
    assert_cap(edge, label)


@pytest.mark.parametrize("seed", range(36))
def test_edge_cap_of_the_fuzz_systems(seed):
    kind, h, x = FUZZ[seed]
    hist, edge = rdf_brute(h, x, dc.bohr(dc.r_max_ang(h)), 200)
    print(seed, kind, "N", len(x), "pairs", int(hist.sum()), "near an edge", int(edge.sum()))
    assert_cap(edge, seed)


# -- sensitivity: the bug a case is aimed at moves its histogram ----------------------------------------------------------------------
def _weighted(c, weight, minimum_image=False):
    """rdf_ref's definition with a weight on every ordered pair (i, j): weight = 1 everywhere is the histogram itself.
    ``weight`` may have more columns than the box has molecules: column j >= N stands for what a kernel would read there."""
    r = dc.bohr(c.r_max_ang)
    m = [0 if minimum_image else image_range(r, w) for w in widths(c.h)]
    s = c.xyz @ np.linalg.inv(c.h)
    ds = s[None, :, :] - s[:, None, :]
    ds -= np.rint(ds)
    hist = np.zeros(c.nbins)
    for sh in np.array([(a, b, e) for a in range(-m[0], m[0] + 1) for b in range(-m[1], m[1] + 1) for e in range(-m[2], m[2] + 1)], dtype=np.float64):
        d = (ds + sh) @ c.h
        d = np.sqrt((d * d).sum(axis=2))
        ok = (d > 0.0) & (d < r)
        b = np.minimum(np.floor(d[ok] * c.nbins / r).astype(np.int64), c.nbins - 1)
        hist += np.bincount(b, weights=weight[ok], minlength=c.nbins)
    return np.rint(hist).astype(np.int64)


def _caught(name, weight, **kw):
    """True where the comparison rule tells the weighted histogram of a case from its reference."""
    c = dc.RDF_CASES[name]
    ref, edge = dc.rdf_reference(name)
    assert_same(_weighted(c, np.ones((c.n, c.n))), ref, edge, name)           # the frame itself is right
    try:
        assert_same(_weighted(c, weight, **kw), ref, edge, name)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("name", ["small_n2", "small_n64", "small_n64_sheared"])
def test_counting_the_half_way_offset_twice_for_even_n_is_caught(name):
    n = dc.RDF_CASES[name].n
    w = np.ones((n, n))
    i = np.arange(n)
    w[i, (i + n // 2) % n] = 2.0                            # o = N / 2 with the weight of every other offset
    assert _caught(name, w)


@pytest.mark.parametrize("name", ["small_n3", "small_n5", "small_n31", "small_n63", "small_n63_sheared"])
def test_a_phantom_offset_for_odd_n_is_caught(name):
    n = dc.RDF_CASES[name].n
    w = np.ones((n, n))
    i = np.arange(n)
    j = (i + (n + 1) // 2) % n                              # o = (N + 1) / 2: the pairs of o = (N - 1) / 2 once more
    np.add.at(w, (i, j), 1.0)
    np.add.at(w, (j, i), 1.0)
    assert _caught(name, w)


def _tile_weights(n, drop_last_offset):
    """The pair weights of k_rdf_tiles' loop over tile offsets -- 1 within a tile, 2 (both orders) between tiles -- with the last
    offset of every tile left out on request."""
    t = -(-n // dc.TILE)
    tile = np.arange(n) // dc.TILE
    w = np.zeros((n, n))
    for I in range(t):
        noff = (t - 1) // 2 if t % 2 else (t // 2 if I < t // 2 else t // 2 - 1)
        for o in range(noff + 1 - (1 if drop_last_offset else 0)):
            J = (I + o) % t
            rows, cols = tile == I, tile == J
            w[np.ix_(rows, cols)] += 1.0
            if o > 0:
                w[np.ix_(cols, rows)] += 1.0
    return w


@pytest.mark.parametrize("name", ["tiles_n513_cube", "tiles_n768_slab", "tiles_n1025_cube"])
def test_dropping_one_tile_offset_is_caught(name):
    n = dc.RDF_CASES[name].n
    assert -(-n // dc.TILE) in (3, 5)
    assert np.array_equal(_tile_weights(n, False), np.ones((n, n)))            # the loop as it is reaches every pair once
    assert _caught(name, _tile_weights(n, True))


@pytest.mark.parametrize("name", ["tiles_n257_cube", "tiles_n257_slab", "tiles_n513_cube"])
def test_reading_a_full_tile_where_the_last_is_ragged_is_caught(name):
    """A kernel that loops over all 256 slots of the staged tile reads, past the last molecule, what the tile staged before it
    left there: slot k still holds molecule k of the preceding tile."""
    c = dc.RDF_CASES[name]
    n, t = c.n, -(-c.n // dc.TILE)
    last = (t - 1) * dc.TILE
    assert 0 < n - last < dc.TILE
    w = np.ones((n, n))
    stale = np.arange(last - dc.TILE + (n - last), last)    # the molecules whose slots the last tile did not overwrite
    rows = np.arange((t - 2) * dc.TILE, (t - 1) * dc.TILE)  # the tile that streams the last one right after its own
    w[np.ix_(rows, stale)] += 2.0
    assert _caught(name, w)


@pytest.mark.parametrize("name", ["small_n63", "tiles_n65_slab", "tiles_n257_slab", "images_100", "images_010", "images_001",
                                  "images_limit"])
def test_the_minimum_image_alone_is_caught_where_an_axis_has_an_image(name):
    c = dc.RDF_CASES[name]
    assert 1 in c.images
    assert _caught(name, np.ones((c.n, c.n)), minimum_image=True)


# -- the degenerate box ---------------------------------------------------------------------------------------------------------------
def test_the_degenerate_box_is_degenerate(c_oracle):
    h, x = dc.DEGENERATE
    assert len(x) == 9 and widths(h).min() > 25.0 * ANG_TO_BOHR
    d = np.linalg.norm(x[:, None, :] - x[None, :, :], axis=2) * dc.BOHR_TO_ANG
    assert np.allclose([d[0, 1], d[1, 2], d[0, 2]], [2.8, 2.8, 5.6], rtol=0, atol=1e-12)      # collinear, equally spaced
    alone = dc.DEGENERATE_ALONE
    assert np.delete(d[alone], alone).min() > 4.4           # beyond r_c = 3.5 and beyond the potential's a sigma = 4.31
    iv, nn, jn, vn = _lists(c_oracle, h, x)
    cls, c, counts = ice_classes(x, iv, nn, jn, vn, RC)
    n_i = ((c != 2.0).sum(axis=1))
    mid = dc.DEGENERATE_MIDDLE
    assert n_i[mid] == 2 and np.isnan(c[mid][c[mid] != 2.0]).all() and cls[mid] == 0
    assert n_i[alone] == 0 and cls[alone] == 0
    assert n_i[dc.DEGENERATE_CENTRE] == 4 and list(n_i[5:]) == [1, 1, 1, 1] and list(n_i[[0, 2]]) == [1, 1]
    assert np.isnan(c[0][c[0] != 2.0]).all() and np.isnan(c[2][c[2] != 2.0]).all()           # the bonds TO the middle one too
    assert not np.isnan(c[4:]).any()


# -- the batches ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", list(dc.BATCHES))
def test_a_batch_mixes_cells_image_tables_and_image_sets(n, c_oracle):
    boxes = dc.BATCHES[n]
    assert len(boxes) == 5 and all(x.shape == (n, 3) for _, x in boxes)
    assert len(boxes) % 4 == 1                              # the last k_rdf_small workgroup: one live wavefront of four
    nivect = [len(c_oracle.ivects(h)) for h, _ in boxes]
    r = dc.batch_r_max_ang(boxes)
    triples = [dc.image_triple(h, r) for h, _ in boxes]     # (raises if a box cannot take r)
    print(n, "image vectors", nivect, "r_max", r, "g(r) images", triples)
    assert len(set(nivect)) > 1 and len(set(triples)) > 1
    assert len({dc.image_count(h, r) for h, _ in boxes}) > 1
    assert min(widths(h).min() for h, _ in boxes) < 4.3 * ANG_TO_BOHR          # the box thin along one axis
    assert sum(np.count_nonzero(h - np.diag(np.diag(h))) == 6 for h, _ in boxes) >= 3           # two gases and the sheared ice
