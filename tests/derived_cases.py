"""Seeded inputs for tests/test_gpu_derived_shapes.py: boxes at which the engine's derived kernels -- forces and virial
(mw_forces.hip.h), CHILL+ classes and bonds (mw_ice.hip.h), ice clusters (mw_ice_clusters.hip.h) and the pair-distance
histogram (mw_rdf.hip.h) -- take branches that the golden boxes and the stacked ice boxes never reach: odd N in k_rdf_small, an
odd number of tiles and a ragged last tile next to full ones in k_rdf_tiles, 1 and 4096 bins, every per-axis image set on an
oblique cell, a degenerate CHILL+ bond, a molecule with no neighbour, and boxes of different cells in one context.

Nothing here needs a GPU or the C oracle.  tests/test_derived_cases.py establishes on the CPU that every case is what its row
says (N, tiles, parity, image triple), that the engine accepts it, that the comparison rules of the mirrors cannot hide a failure
on it, and that each case tells the bug it is aimed at from a correct result.

Lengths are bohr unless a name ends in _ang.  Every case is made once, at import, from its own seed."""
from __future__ import annotations

import collections
import itertools

import numpy as np

from rdf_ref import image_range, rdf_brute, rdf_fast, widths

BOHR_TO_ANG = 0.5291772108
ANG_TO_BOHR = 1.0 / 0.5291772108
MIN_SEP_ANG = 2.0                               # tests/test_gpu_fuzz.py: the potential explodes below that
R_ANG = 10.0
TILE = 256                                      # kRdfTile
SMALL_MAX = 64                                  # kRdfSmallMax
BRUTE_MAX = 257                                 # rdf_brute is the reference up to here, rdf_fast above
IMAGES = np.array(list(itertools.product((-1, 0, 1), repeat=3)), dtype=np.float64)

#: the shear of `vacancy_ice`: cell and positions are multiplied by I + shear SHEAR_M.  All six off-diagonal entries are set,
#: of mixed sign; the symmetric part is what makes the cell oblique (at shear = 0.3 the angles between the cell vectors of a
#: cubic cell are 75, 100 and 81 degrees and the perpendicular widths 0.94 to 0.96 of the edge lengths), the antisymmetric part
#: turns it away from the axes.
SHEAR_M = np.array([[0.0, 1.0, -0.8], [0.2, 0.0, 0.9], [0.3, -0.4, 0.0]])


def bohr(r_ang):
    return float(r_ang) / 0.5291772108          # as the module converts it


def r_max_ang(h, r_ang=R_ANG):
    """min(r_ang, 1.5 w_min (1 - 1e-6)): the largest range the engine takes for the cell, capped."""
    return min(r_ang, 1.5 * widths(h).min() * (1.0 - 1e-6) * BOHR_TO_ANG)


def image_triple(h, r_ang):
    """Images per axis (0 or 1) by the rule of rdf_ref, for a range in Angstrom."""
    return tuple(image_range(bohr(r_ang), w) for w in widths(h))


def image_count(h, r_ang):
    return int(np.prod([2 * m + 1 for m in image_triple(h, r_ang)]))


def min_separation(h, xyz):
    """The smallest distance between two molecules or a molecule and an image of itself, images up to one cell each way
    after wrapping (enough for any distance below the smallest width)."""
    s = np.asarray(xyz, dtype=np.float64) @ np.linalg.inv(h)
    ds = s[None, :, :] - s[:, None, :]
    ds -= np.rint(ds)
    best = np.inf
    for sh in IMAGES:
        d = (ds + sh) @ h
        r2 = (d * d).sum(axis=2)
        if not sh.any():
            r2 = r2 + np.where(np.eye(len(s), dtype=bool), np.inf, 0.0)
        best = min(best, float(r2.min()))
    return float(np.sqrt(best))


def _default_reps(n):
    r = 2
    while 8 * r ** 3 < n:
        r += 1
    return (r, r, r)


def vacancy_ice(n, seed, reps=None, shear=0.0, sigma_ang=0.08, kind="ic", d_oo_ang=None):
    """(h, xyz): ``reps`` replicas of the 8-molecule ice cell (the smallest cube of at least two cells a side that holds n where
    None; nearest-neighbour distance ``d_oo_ang``, lattice.D_OO_ANG where None), thermalised by ``sigma_ang``, of which a seeded
    random subset of exactly n molecules is kept in ascending order; then cell and positions times I + shear SHEAR_M.  Ice
    around vacancies: any N, odd ones included."""
    from mc_water_ls_mw_amd import lattice as lat
    reps = _default_reps(n) if reps is None else tuple(int(r) for r in reps)
    h, x = {"ic": lat.ice_ic_cell, "ih": lat.ice_ih_cell}[kind](lat.D_OO_ANG if d_oo_ang is None else d_oo_ang)
    h, x = lat.replicate(h, x, reps)
    if not 1 <= n <= len(x):
        raise ValueError(f"{n} molecules do not fit the {len(x)} sites of {reps}")
    x = lat.thermalise(x, sigma_ang, seed)
    keep = np.sort(np.random.default_rng([seed, n]).permutation(len(x))[:n])
    x = x[keep]
    if shear != 0.0:
        m = np.eye(3) + shear * SHEAR_M
        h, x = h @ m, x @ m
    return np.ascontiguousarray(h), np.ascontiguousarray(x)


def gas(n, seed, widths_ang, tilt=0.1):
    """(h, xyz): the gas of tests/test_gpu_fuzz.py -- a cell diag(widths) + uniform(-tilt, tilt) x the smallest width on all nine
    entries, positions uniform in it -- with draws closer than 2.0 Angstrom to an earlier molecule or to any image drawn again:
    exactly n molecules."""
    rng = np.random.default_rng(seed)
    L = np.asarray(widths_ang, dtype=np.float64) * ANG_TO_BOHR
    h = np.diag(L) + rng.uniform(-tilt, tilt, (3, 3)) * L.min()
    shifts = IMAGES @ h
    sep2 = (MIN_SEP_ANG * ANG_TO_BOHR) ** 2
    x = np.zeros((n, 3))
    i = 0
    for _ in range(200 * n):
        t = rng.random(3) @ h
        d = (x[:i] - t)[:, None, :] + shifts[None, :, :]
        if i == 0 or float((d * d).sum(axis=2).min()) > sep2:
            x[i] = t
            i += 1
            if i == n:
                return np.ascontiguousarray(h), np.ascontiguousarray(x)
    raise RuntimeError(f"no room for {n} molecules 2.0 Angstrom apart in {widths_ang}")


def displaced(h, xyz, seed, reach=3):
    """The positions moved by whole lattice vectors, up to ``reach`` per axis either way, every molecule by its own."""
    rng = np.random.default_rng(seed)
    n = rng.integers(-reach, reach + 1, (len(xyz), 3)).astype(np.float64)
    return np.ascontiguousarray(xyz + n @ h)


#: a case of RDF_CASES: the box, the call, and what the row states of it -- N, the per-axis images -- which
#: tests/test_derived_cases.py holds against rdf_ref's rule
RdfCase = collections.namedtuple("RdfCase", "h xyz r_max_ang nbins n images")


def _case(box, images, r_ang=None, nbins=200):
    h, xyz = box
    return RdfCase(h, xyz, r_max_ang(h) if r_ang is None else r_ang, nbins, len(xyz), tuple(images))


def _slab_reps(n):
    m = 2
    while 16 * m * m < n:
        m += 1
    return (m, m, 2)


def _rdf_cases():
    c = {}
    # k_rdf_small: odd and even N, two ice cells a side (12.6 Angstrom), orthogonal and sheared: (1, 1, 1) at 10 Angstrom
    for n in (2, 3, 5, 31, 63, 64):
        c[f"small_n{n}"] = _case(vacancy_ice(n, 100 + n, (2, 2, 2)), (1, 1, 1))
        c[f"small_n{n}_sheared"] = _case(vacancy_ice(n, 200 + n, (2, 2, 2), shear=0.3), (1, 1, 1))
    # k_rdf_tiles: T = 1, 1, 1, 2, 3, 3, 5, 6.  The cube is at least four cells a side (25 Angstrom: no images at 10); the slab is
    # two cells thick (one image across it; the 3 x 3 x 2 slab of N = 65 is narrow enough for one along every axis)
    for n in (65, 255, 256, 257, 513, 768, 1025, 1281):
        cube = tuple(max(4, r) for r in _default_reps(n))
        c[f"tiles_n{n}_cube"] = _case(vacancy_ice(n, 300 + n, cube), (0, 0, 0))
        slab = _slab_reps(n)
        c[f"tiles_n{n}_slab"] = _case(vacancy_ice(n, 400 + n, slab), (1, 1, 1) if slab[0] < 4 else (0, 0, 1))
    # all eight image sets on one oblique family: two cells along an axis for one image at 9 Angstrom, four for none
    for k, reps in enumerate(itertools.product((2, 4), repeat=3)):
        n = 63 if reps == (2, 2, 2) else 95
        images = tuple(1 if r == 2 else 0 for r in reps)
        c["images_%d%d%d" % images] = _case(vacancy_ice(n, 500 + k, reps, shear=0.3), images, r_ang=9.0)
    h, x = vacancy_ice(95, 520, (2, 3, 2), shear=0.3)
    c["images_limit"] = _case((h, x), (1, 1, 1), r_ang=1.5 * widths(h).min() * (1.0 - 1e-6) * BOHR_TO_ANG)
    # the ends of the bin range, on the small kernel (4096 bins: 71 680 B of LDS) and on tiles with a last tile of one molecule
    for nbins in (1, 7, 4096):
        c[f"bins{nbins}_n63"] = _case(vacancy_ice(63, 163, (2, 2, 2)), (1, 1, 1), nbins=nbins)
        c[f"bins{nbins}_n257"] = _case(vacancy_ice(257, 657, _slab_reps(257)), (0, 0, 1), nbins=nbins)
    h, x = vacancy_ice(31, 231, (2, 2, 2), shear=0.3)
    c["unwrapped_n31"] = _case((h, displaced(h, x, 31)), (1, 1, 1))
    for case in c.values():
        case.h.setflags(write=False), case.xyz.setflags(write=False)
    return c


#: name -> RdfCase
RDF_CASES = _rdf_cases()

_REF = {}


def rdf_reference(name):
    """(hist, edge) of a case of RDF_CASES: rdf_brute up to BRUTE_MAX molecules, rdf_fast above (tests/test_derived_cases.py
    shows the two equal on every case both can do).  Computed once."""
    if name not in _REF:
        c = RDF_CASES[name]
        if c.n <= BRUTE_MAX:
            _REF[name] = rdf_brute(c.h, c.xyz, bohr(c.r_max_ang), c.nbins)
        else:
            _REF[name] = rdf_fast(c.h, c.xyz, bohr(c.r_max_ang), c.nbins, workers=8)
        for a in _REF[name]:
            a.setflags(write=False)
    return _REF[name]


def _degenerate():
    """Nine molecules in a cube of 30 Angstrom, the three groups further apart than the list reaches: 0, 1, 2 on a line 2.8
    Angstrom apart (the middle one, 1, has two antipodal neighbours: q = 0); 3 alone; 4 with 5 .. 8 around it at 2.75 Angstrom
    in a slightly distorted tetrahedron (4 has four neighbours, each of them one)."""
    u = np.array([2.0, -1.0, 3.0]) / np.sqrt(14.0)
    line = np.array([10.0, 11.0, 9.0]) + 2.8 * np.arange(3)[:, None] * u[None, :]
    alone = np.array([[22.0, 7.0, 21.0]])
    tet = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) / np.sqrt(3.0)
    tet = tet + np.array([[0.03, -0.02, 0.01], [-0.04, 0.02, 0.03], [0.01, 0.05, -0.02], [0.02, -0.01, -0.05]])
    centre = np.array([9.0, 21.0, 20.0])
    five = np.concatenate([centre[None, :], centre + 2.75 * tet])
    h = np.eye(3) * 30.0 * ANG_TO_BOHR
    xyz = np.concatenate([line, alone, five]) * ANG_TO_BOHR
    h.setflags(write=False), xyz.setflags(write=False)
    return h, np.ascontiguousarray(xyz)


#: (h, xyz) and who is who in it
DEGENERATE = _degenerate()
DEGENERATE_MIDDLE, DEGENERATE_ALONE, DEGENERATE_CENTRE = 1, 3, 4


def fuzz_systems():
    """[(seed, kind, h, xyz)]: the 36 systems tests/test_gpu_fuzz.py holds the energy paths to."""
    from test_gpu_fuzz import random_system
    return [(seed,) + tuple(random_system(np.random.default_rng(7000 + seed))) for seed in range(36)]


def _batches():
    """Five boxes of one N for one engine context: a gas, cubic ice with vacancies two cells wide, sheared hexagonal ice with
    vacancies, a box of hexagonal ice one cell thin along x -- at d_OO = 2.6 Angstrom that cell vector (4.25 Angstrom) is shorter
    than the potential's a sigma, so the engine's image table reaches two cells along it and has 45 vectors, not 27 -- and a
    second, smaller gas.  Their cells differ, and so do their image tables and their g(r) image sets."""
    out = {}
    for n, wide, cubic, sheared, thin, tight in ((63, (17.0, 21.0, 25.0), (2, 2, 2), (4, 2, 2), (1, 3, 3), (10.0, 11.0, 12.0)),
                                                 (257, (24.0, 27.0, 31.0), (2, 4, 5), (6, 4, 3), (1, 6, 6), (17.0, 18.0, 19.0))):
        out[n] = [gas(n, 700 + n, wide), vacancy_ice(n, 710 + n, cubic), vacancy_ice(n, 720 + n, sheared, shear=0.3, kind="ih"),
                  vacancy_ice(n, 730 + n, thin, kind="ih", d_oo_ang=2.6), gas(n, 740 + n, tight, tilt=0.05)]
        for h, x in out[n]:
            h.setflags(write=False), x.setflags(write=False)
    return out


#: N -> [(h, xyz)] x 5
BATCHES = _batches()


def batch_r_max_ang(boxes):
    """The range every box of a batch takes: min(10 Angstrom, 1.5 w_min (1 - 1e-6)) of the narrowest."""
    return min(r_max_ang(h) for h, _ in boxes)
