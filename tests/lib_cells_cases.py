"""The inputs of tests/test_gpu_lib_cells.py and their reference: boxes at which the cell grid and the counting sort of
csrc/mw_lib_cells.h can go wrong, with the entry count of every molecule from tests/adf_ref.py.  tests/test_lib_cells.py
asserts on the CPU that no pair of any of them lies within adf_ref.MARGIN of the cutoff, which is what lets the GPU test
compare the counts of the four libraries exactly."""
from __future__ import annotations

import numpy as np

from adf_ref import adf_exact

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
