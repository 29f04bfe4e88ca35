"""The inputs of tests/test_gpu_lib_cells.py and tests/test_gpu_lib_cells_forces.py and their references: boxes at which the
cell grid, the counting sort and the two walks of csrc/mw_lib_cells.h can go wrong, with the entry count of every molecule from
tests/adf_ref.py.  tests/test_lib_cells.py asserts on the CPU that no pair of any of them lies within adf_ref.MARGIN of the
cutoff, which is what lets the GPU tests compare the counts of the ten libraries on that layer exactly.

Two tables.  CASES: five boxes sized in units of 3.5 Angstrom, for the four analysis libraries (libmw_adf, libmw_rings, libmw_boo,
libmw_tet).  GRID_SHAPES and `random_boxes`: boxes made by one seeded generator, `grid_box`, for a radius the caller names, so that
the analysis libraries see them at 3.5 Angstrom and the six force libraries (libmw_quench, libmw_md, libmw_npt, libmw_flex,
libmw_hess, libmw_ti) at a sigma with a floor under every pair distance.  Each shape is one the grid of a library reaches on
purpose (`GRID_SHAPES`); tests/test_lib_cells.py asserts that adf_ref.cell_grid gives each its grid and that each tells a walk that
loses an image from one that does not."""
from __future__ import annotations

import itertools
import zlib

import numpy as np

import md_ref
from adf_ref import adf_exact, cell_grid
from boo_ref import widths

BOHR_TO_ANG = 0.5291772108
R_ANG = 3.5                                     # what the wrappers are given
RC = R_ANG / BOHR_TO_ANG                        # what the libraries see of it, bohr
WIDE = 7.2 * RC                                 # 7 x 7 x 7 = 343 cells: more than the 256 lanes of the scan
_REF = {}


def _gas(n, h, seed):
    """n molecules uniform in s over [-0.3, 1.3)^3: some of them outside the cell."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray((rng.random((n, 3)) * 1.6 - 0.3) @ h)


def _one_cell():
    h = np.eye(3) * (1.5 * RC)
    return h[None], _gas(65, h, 6501)[None]


def _many_cells():
    h = np.eye(3) * WIDE
    return h[None], _gas(200, h, 20001)[None]


def _small_side():
    h = np.eye(3) * (WIDE * (64.0 / 200.0) ** (1.0 / 3.0))
    return h[None], _gas(64, h, 6401)[None]


def _three_cells():
    hs = (np.eye(3) * (5.3 * RC), np.diag([4.2, 5.5, 6.7]) * RC, np.array([[5.0, 0.0, 0.0], [1.1, 4.6, 0.0], [-0.8, 1.3, 5.6]]) * RC)
    return np.stack(hs), np.stack([_gas(96, h, 9601 + b) for b, h in enumerate(hs)])


def _shifted():
    """`_many_cells` with every tenth molecule put on an s_k = 0 plane, some on two (a coordinate of exactly 0 in this cubic
    cell), then every third molecule moved by whole lattice vectors, up to three per axis either way."""
    cells, pos = _many_cells()
    pos = pos.copy()
    rng = np.random.default_rng(20002)
    for i in range(0, 200, 10):
        k = (i // 10) % 3
        pos[0, i, k] = 0.0
        if i % 50 == 0:
            pos[0, i, (k + 1) % 3] = 0.0
    moved = np.arange(200) % 3 == 1
    pos[0, moved] += rng.integers(-3, 4, size=(int(moved.sum()), 3)).astype(np.float64) @ cells[0]
    return cells, pos


#: label -> (cells [nboxes, 3, 3], pos [nboxes, n, 3]), bohr
CASES = {"n65_one_cell": _one_cell, "n200_343_cells": _many_cells, "n64_small": _small_side, "n96_three_cells": _three_cells,
         "n200_shifted_on_planes": _shifted}


def reference(label):
    """(cells, pos, counts [nboxes, n] int32, gap_r): the entry counts by adf_ref and the smallest |r^2 - rc^2| / rc^2 of the case.
    Computed once."""
    if label not in _REF:
        cells, pos = CASES[label]()
        refs = [adf_exact(h, xyz, RC, np.array([-1.0, 1.0])) for h, xyz in zip(cells, pos)]
        _REF[label] = (cells, pos, np.stack([r["counts"] for r in refs]), min(r["gap_r"] for r in refs))
    return _REF[label]


# -- the grid shapes: one generator, two families -------------------------------------------------------------------------------
R2_ANG = 3.0                                    # the second radius of the tetrahedral calls on these boxes (r_lsi)
RC2 = R2_ANG / BOHR_TO_ANG
#: the radius the force family's boxes are sized in, and the floor under every pair distance of theirs over all images (bohr):
#: tests/test_gpu_fuzz.py takes 2.0 Angstrom as the distance below which the potential explodes
R_FORCE = md_ref.A_SIGMA * (1.0 + 1e-6)
MIN_SEP = 2.3 / BOHR_TO_ANG
IMAGES = np.array(list(itertools.product((-1, 0, 1), repeat=3)), dtype=np.float64)
RANDOM_SEED = 4242
NRANDOM = 12
_BOXES = {}


def _tri(d, f=(0.0, 0.0, 0.0)):
    """The lower-triangular cell with the diagonal d and the off-diagonals h_21 = f_0 d_1, h_31 = f_1 d_2, h_32 = f_2 d_2 (d
    0-based): its widths are d_0 / sqrt(1 + f_0^2 + (f_0 f_2 - f_1)^2), d_1 / sqrt(1 + f_2^2) and d_2."""
    return np.array([[d[0], 0.0, 0.0], [f[0] * d[1], d[1], 0.0], [f[1] * d[2], f[2] * d[2], d[2]]], dtype=np.float64)


_SKEW = _tri((1.3, 1.25, 1.2), (0.5, 0.4, -0.45))                       # widths 1.015, 1.14, 1.2
#: an oblique cell with room for 65 molecules 2.3 Angstrom apart, every width still below twice the radius and a lattice vector
#: of 1.5 radii: widths 1.905, 1.912 and 1.45 against edges 6.1, 6.07 and 1.50 (the volume is the product of the diagonal, not
#: of the widths; two images of a neighbour are a lattice vector apart, so a short one is what puts both in range)
_SKEW_ROOMY = _tri((6.1, 1.95, 1.45), (2.95, 0.15, -0.2))
_LONG, _LONGER, _LONGEST = np.diag([128.5, 1.2, 1.2]), np.diag([200.5, 1.2, 1.2]), np.diag([300.5, 1.2, 1.2])
#: label -> (the cell of the analysis family, the cell of the force family -- widened where 2.3 Angstrom need the room, the grid
#: kept --, both in units of the radius; N; the grid of the general geometry or None for the small one).  Where two images of a
#: neighbour are to be in range, one lattice vector of the force family's cell stays at 1.45 to 1.5 radii: the potential vanishes
#: so smoothly at a sigma that a second image beyond 0.9 a sigma is worth less than the energy bar.
#:   g222               every axis sends the offsets -1 and +1 into the same other cell, with different shifts
#:   g123               one, two and three cells in one box
#:   g121_skew          perpendicular widths (1.62, 2.95, 1.30) against edges up to 4.3; the force family's is more oblique,
#:                      (1.91, 2.91, 1.45) against edges up to 6.6
#:   g555_lowered       (9, 8, 7) lowered to fit the 130 cells of 65 molecules: cells wider than the radius, empty neighbours
#:   g128_long          128 cells in a row: more cells than members, most of them empty, and a linear index that is all x
#:   g130_long_lowered  200 cells along x lowered to 130: lowering on one axis only
#:   g300_long          300 cells in a row for 160 molecules: more cells than the 256 lanes of k_cells_scan, so that every lane
#:                      sums more than one cell (per > 1) on a grid that is anything but a cube
#:   small_skew(_n2)    walk_small's eight images in an oblique cell, every width below twice the radius; 64 and 2 molecules
#:   n65_skew           the same cell on the general path: all 27 offsets land in the one cell
GRID_SHAPES = {
    "g222": (_tri((2.5, 2.5, 2.5)), _tri((2.9, 2.9, 2.9)), 72, (2, 2, 2)),
    "g123": (_tri((1.4, 2.6, 3.3)), _tri((1.45, 2.98, 3.98)), 66, (1, 2, 3)),
    "g121_skew": (_tri((2.4, 3.6, 1.3), (0.6, -0.5, 0.7)), _tri((4.4, 2.97, 1.45), (2.0, 0.15, -0.2)), 70, (1, 2, 1)),
    "g555_lowered": (_tri((9.05, 8.05, 7.05)), _tri((9.05, 8.05, 7.05)), 65, (5, 5, 5)),
    "g128_long": (_LONG, _LONG, 65, (128, 1, 1)),
    "g130_long_lowered": (_LONGER, _LONGER, 65, (130, 1, 1)),
    "g300_long": (_LONGEST, _LONGEST, 160, (300, 1, 1)),
    "small_skew": (_SKEW, _SKEW_ROOMY, 64, None),
    "small_skew_n2": (_SKEW, _SKEW, 2, None),
    "n65_skew": (_SKEW, _SKEW_ROOMY, 65, (1, 1, 1)),
}
#: the unlowered grids of the two lowered cases, and the cap they are lowered to
UNLOWERED = {"g555_lowered": ((9, 8, 7), 130), "g130_long_lowered": ((200, 1, 1), 130)}
#: the cases with a lattice vector shorter than twice the radius: two images of one neighbour can both be in range
NARROW = ("g123", "g121_skew", "g128_long", "g130_long_lowered", "g300_long", "small_skew", "small_skew_n2", "n65_skew")
RANDOM_LABELS = tuple(f"random{k}" for k in range(NRANDOM))
LABELS = tuple(GRID_SHAPES) + RANDOM_LABELS


def wrapped(h, xyz):
    """The positions moved into the cell by whole lattice vectors (the mirrors of the force family look one image each way)."""
    s = np.asarray(xyz, dtype=np.float64) @ np.linalg.inv(h)
    return np.ascontiguousarray((s - np.floor(s)) @ h)


def _fill(h, n, r, min_sep, rng):
    """n positions in the cell h, or None where no room is found.  s uniform in [0, 1)^3; every second draw is moved to within
    half a radius of a face of the cell, so that wide cells have pairs across their boundary too; every tenth molecule of the
    first sixty sits on an s_k = 0 plane (k cycles where the cell is orthorhombic, k = 2 in a lower-triangular one: the planes
    whose fractional coordinate comes out as exactly 0 again; a face of 1.2 radii each way has no room for more than two 2.3
    Angstrom apart); a draw within ``min_sep`` of an earlier molecule or one of its images is drawn
    again.  Then every third molecule that is on no plane is moved by whole lattice vectors, up to three per axis either way (one
    along an axis longer than 20 radii)."""
    w = widths(h)
    diagonal = bool(np.all(h == np.diag(np.diag(h))))
    shifts = IMAGES @ h
    s = np.zeros((n, 3))
    for i in range(n):
        for _ in range(4000):
            t = rng.random(3)
            if rng.random() < 0.5:
                k = int(rng.integers(3))
                t[k] = ((rng.random() - 0.5) * min(1.0, r / w[k])) % 1.0
            if i % 10 == 0 and i < 60:
                t[(i // 10) % 3 if diagonal else 2] = 0.0
            if min_sep > 0.0 and i > 0:
                d = ((s[:i] - t) @ h)[:, None, :] + shifts[None, :, :]
                if float((d * d).sum(axis=2).min()) < min_sep * min_sep:
                    continue
            s[i] = t
            break
        else:
            return None
    pos = s @ h
    moved = (np.arange(n) % 3 == 1) & (np.arange(n) % 10 != 0)
    reach = np.where(w > 20.0 * r, 1, 3)                 # (a coordinate of thousands of bohr has an ulp near the 1e-12 of the bars)
    pos[moved] += rng.integers(-reach, reach + 1, size=(int(moved.sum()), 3)).astype(np.float64) @ h
    return np.ascontiguousarray(pos)


def grid_box(label, r, min_sep=0.0):
    """(cell [3, 3], pos [N, 3]) in bohr of a case of GRID_SHAPES for the radius ``r``: the analysis family's cell for ``min_sep``
    = 0, the force family's with no pair closer than ``min_sep`` over all images.  Seeded by the label."""
    analysis, force, n, _ = GRID_SHAPES[label]
    h = np.ascontiguousarray((force if min_sep > 0.0 else analysis) * r)
    rng = np.random.default_rng([zlib.crc32(label.encode()), int(min_sep > 0.0)])
    for _ in range(50):
        pos = _fill(h, n, r, min_sep, rng)
        if pos is not None:
            return h, pos
    raise RuntimeError(f"{label}: no room for {n} molecules {min_sep} bohr apart")


def random_boxes(seed, r, min_sep=0.0):
    """NRANDOM boxes [(cell, pos)]: box k from the generator seeded (seed, k) -- N from 65 to 160, a lower-triangular cell with
    off-diagonals up to +-0.6 of the diagonal element of their row and widths in [1.05 r, 4.5 r], filled as `grid_box` fills its
    cells.  A draw that breaks the width rule, that leaves a molecule less than max(0.1 r^3, 1.7 min_sep^3) of volume (beyond
    that no room is found for ``min_sep``, and the analysis libraries would see hundreds of entries per molecule) or in which no
    room is found is drawn again from the same generator: every k yields a box."""
    out = []
    for k in range(NRANDOM):
        rng = np.random.default_rng([seed, k])
        while True:
            n = int(rng.integers(65, 161))
            h = _tri(rng.uniform(1.05, 6.0, 3) * r, rng.uniform(-0.6, 0.6, 3))
            w = widths(h)
            if w.min() < 1.05 * r or w.max() > 4.5 * r or abs(np.linalg.det(h)) < n * max(0.1 * r ** 3, 1.7 * min_sep ** 3):
                continue
            pos = _fill(h, n, r, min_sep, rng)
            if pos is not None:
                out.append((np.ascontiguousarray(h), pos))
                break
    return out


def _box(family, label):
    """(cell, pos) of a label of LABELS in a family, made once and read-only."""
    r, sep = (RC, 0.0) if family == "analysis" else (R_FORCE, MIN_SEP)
    if (family, label) not in _BOXES:
        if label in GRID_SHAPES:
            _BOXES[family, label] = grid_box(label, r, sep)
        else:
            for k, box in enumerate(random_boxes(RANDOM_SEED, r, sep)):
                _BOXES[family, RANDOM_LABELS[k]] = box
        for a in _BOXES[family, label]:
            a.setflags(write=False)
    return _BOXES[family, label]


def analysis_box(label):
    """The box the four analysis libraries see at R_ANG."""
    return _box("analysis", label)


def force_box(label):
    """The box the six force libraries see: sized in units of R_FORCE, no pair closer than MIN_SEP."""
    return _box("force", label)


def expected_plan(label, h, n, r):
    """(small geometry, grid) a library must report for the box at its radius ``r``: GRID_SHAPES' grid for its cases (asserted
    against adf_ref.cell_grid in tests/test_lib_cells.py), adf_ref.cell_grid's for the random boxes and the small geometry."""
    grid = GRID_SHAPES[label][3] if label in GRID_SHAPES else None
    return n <= 64, grid if grid is not None else cell_grid(h, r, n)


def grid_reference(label):
    """The adf_exact dict of the analysis box of a label at RC with the 97 bins in cos(theta), computed once."""
    from adf_ref import EDGE_SETS
    if ("grid", label) not in _REF:
        h, pos = analysis_box(label)
        _REF["grid", label] = adf_exact(h, pos, RC, EDGE_SETS["cos97"])
    return _REF["grid", label]


# -- what a walk that loses images would see (reference code alone) -----------------------------------------------------------
def image_entries(h, xyz, r, images="all"):
    """(i, j, v, d): the entries (j, image v of IMAGES) of every molecule i with 0 < |d| < r, d = r_j + IMAGES[v] H - r_i over the
    wrapped positions, ordered by i.  ``images``: "all"; "minimum": the nearest image of every pair alone (what a minimum-image
    walk sees); "none": no image across the cell's boundary."""
    x = wrapped(h, xyz)
    d = x[None, :, None, :] + (IMAGES @ h)[None, None, :, :] - x[:, None, None, :]
    r2 = (d * d).sum(axis=3)
    hit = (r2 < r * r) & (r2 > 0.0)
    if images == "minimum":
        hit &= r2 == r2.min(axis=2, keepdims=True)
    elif images == "none":
        hit &= np.all(IMAGES == 0.0, axis=1)[None, None, :]
    else:
        assert images == "all"
    i, j, v = np.nonzero(hit)
    return i, j, v, d[i, j, v]


def cutoff_gap(h, xyz, r):
    """(the smallest |d^2 - r^2| / r^2, the smallest |d|) over every pair and image of the wrapped positions."""
    x = wrapped(h, xyz)
    d = x[None, :, None, :] + (IMAGES @ h)[None, None, :, :] - x[:, None, None, :]
    r2 = (d * d).sum(axis=3)
    r2 = r2[r2 > 0.0]
    return float(np.abs(r2 - r * r).min() / (r * r)), float(np.sqrt(r2.min()))


def image_counts(h, xyz, r, images="all"):
    return np.bincount(image_entries(h, xyz, r, images)[0], minlength=len(xyz)).astype(np.int32)


def pairs_with_two_images(h, xyz, r):
    """The number of ordered pairs (i, j) with more than one image of j among the entries of i."""
    i, j, _, _ = image_entries(h, xyz, r)
    return int((np.bincount(i * len(xyz) + j) > 1).sum())


def restricted_energy_forces(h, xyz, images="all"):
    """(counts, E, F) of forces_ref.model_forces over the lists `image_entries` gives at a sigma."""
    from forces_ref import model_forces
    x = wrapped(h, xyz)
    n = len(x)
    i, j, v, _ = image_entries(h, xyz, md_ref.A_SIGMA, images)
    nn = np.bincount(i, minlength=n).astype(np.int32)
    slot = np.arange(len(i)) - np.concatenate([[0], np.cumsum(nn)])[:-1][i]
    jn = np.zeros((n, max(1, int(nn.max(initial=0)))), dtype=np.int32)
    vn = np.zeros_like(jn)
    jn[i, slot], vn[i, slot] = j + 1, v + 1
    e, f, _ = model_forces(x, IMAGES @ h, nn, jn, vn)
    return nn, float(e), f


# -- the mirrors of the force family on these boxes -----------------------------------------------------------------------------
def force_reference(label):
    """dict of the force box of a label: e, f from quench_ref.energy_forces, w from npt_ref.energy_forces_virial, wab from
    flex_ref.energy_forces_stress, each over the wrapped positions (a whole lattice vector changes none of them).  Computed once."""
    import flex_ref
    import npt_ref
    import quench_ref
    if ("force", label) not in _REF:
        h, pos = force_box(label)
        x = wrapped(h, pos)
        e, f = quench_ref.energy_forces(h, x)
        _, _, w = npt_ref.energy_forces_virial(h, x)
        _, _, wab = flex_ref.energy_forces_stress(h, x)
        _REF["force", label] = dict(e=e, f=f, w=w, wab=wab)
    return _REF["force", label]


def measure_spreads(label):
    """(spread of W, spread of a component of W_ab) of the force box of a label: the mirrors against themselves with forces
    perturbed by +-quench_ref.F_ATOL, by the routines npt_ref.point and flex_ref.point are made of."""
    import flex_ref
    import npt_ref
    h, pos = force_box(label)
    x = wrapped(h, pos)
    w = [float(npt_ref.run(h, x, 0, md_ref.BAR_DT, force_noise=g)["w"]) for g in (None, np.random.default_rng(99))]
    wab = [flex_ref.run(h, x, 0, md_ref.BAR_DT, force_noise=g)["w"] for g in (None, np.random.default_rng(99))]
    return abs(w[1] - w[0]), float(np.abs(wab[1] - wab[0]).max())


#: label -> the spreads `measure_spreads` gives, measured on the CPU (tests/test_lib_cells.py measures them again and holds these
#: to them), Hartree
W_SPREAD_MEASURED = {"g222": 4.80e-09, "g123": 4.16e-09, "g121_skew": 5.28e-09, "g555_lowered": 4.00e-09, "g128_long": 4.00e-09,
                     "g130_long_lowered": 4.00e-09, "g300_long": 8.60e-09, "small_skew": 3.74e-09, "small_skew_n2": 6.94e-10, "n65_skew": 4.00e-09,
                     "random0": 4.22e-09, "random1": 4.00e-09, "random2": 4.68e-09, "random3": 3.92e-09, "random4": 4.10e-09,
                     "random5": 4.21e-09, "random6": 4.21e-09, "random7": 4.77e-09, "random8": 8.35e-09, "random9": 4.47e-09,
                     "random10": 4.80e-09, "random11": 1.03e-08}
W_AB_SPREAD_MEASURED = {"g222": 1.87e-09, "g123": 2.10e-09, "g121_skew": 2.52e-09, "g555_lowered": 2.25e-09, "g128_long": 2.25e-09,
                        "g130_long_lowered": 2.25e-09, "g300_long": 5.52e-09, "small_skew": 1.93e-09, "small_skew_n2": 4.50e-10, "n65_skew": 2.25e-09,
                        "random0": 1.57e-09, "random1": 2.25e-09, "random2": 1.66e-09, "random3": 2.34e-09, "random4": 2.66e-09,
                        "random5": 2.66e-09, "random6": 2.66e-09, "random7": 2.64e-09, "random8": 4.79e-09, "random9": 2.43e-09,
                        "random10": 1.87e-09, "random11": 6.06e-09}


def w_bar(label):
    """The bar on W of a box: the larger of npt_ref.W_TOL and ten times the box's own recorded spread."""
    import npt_ref
    return max(npt_ref.W_TOL, 10.0 * W_SPREAD_MEASURED[label])


def w_ab_bar(label):
    import flex_ref
    return max(flex_ref.W_AB_TOL, 10.0 * W_AB_SPREAD_MEASURED[label])


# -- the one trajectory -----------------------------------------------------------------------------------------------------------
TRAJECTORY_LABEL, TRAJECTORY_STEPS, TRAJECTORY_VEL_SEED = "g123", 20, 7


def trajectory_velocities():
    h, pos = force_box(TRAJECTORY_LABEL)
    return md_ref.maxwell_boltzmann(1, len(pos), md_ref.BAR_KT, md_ref.MASS_WATER, TRAJECTORY_VEL_SEED)[0]


def trajectory_reference():
    """md_ref.run over 20 NVE steps of 5 fs on the force box of g123 from `trajectory_velocities`, the forces those of
    quench_ref.energy_forces at the wrapped positions.  Computed once."""
    import quench_ref
    if "trajectory" not in _REF:
        h, pos = force_box(TRAJECTORY_LABEL)
        _REF["trajectory"] = md_ref.run(h, pos, TRAJECTORY_STEPS, md_ref.BAR_DT, vel=trajectory_velocities(),
                                        forces_of=lambda hh, x: quench_ref.energy_forces(hh, wrapped(hh, x)))
    return _REF["trajectory"]


def cells_of(h, xyz, grid):
    """The linear grid cell of every molecule, by the rule of csrc/mw_lib_cells.h."""
    s = np.asarray(xyz, dtype=np.float64) @ np.linalg.inv(h)
    g = np.asarray(grid, dtype=np.int64)
    c = np.clip(np.floor((s - np.floor(s)) * g).astype(np.int64), 0, g - 1)
    return (c[:, 2] * g[1] + c[:, 1]) * g[0] + c[:, 0]
