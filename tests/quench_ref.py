"""numpy mirror of the contract of include/mw_quench.h: FIRE per box on the full-box mW energy at fixed cell, and the cases
tests/test_quench_ref.py (CPU, the preconditions) and tests/test_gpu_quench.py (the device) share.

Energy and forces are forces_ref.model_forces over the C oracle's image vectors and lists, rebuilt from the current
positions at every evaluation; the steps are the nine of the header, in its order.  The mirror shares no code with the
library and does not reproduce its rounding: the device is held to it within tolerances, not bit for bit.

Tolerances.  Energies: conftest.RTOL = 1e-10 relative.  Positions: POS_TOL below.  The minimum is flat along its softest
mode, so where a quench stops along it depends on the stopping iteration, and the device's rounding may move that by one or
two.  Measured with the mirror on the CPU, max |x(ftol 1e-10) - x(ftol 1e-12)| over BAR_CASES, the five cases that were
fixed before any device result, is 1.8e-8 ... 4.3e-8 bohr (ic48_t015 4.2e-8, ih48_t020 1.8e-8, ic64_sheared 2.5e-8, ic96
4.3e-8, ih96_disordered 4.3e-8); POS_TOL is ten times the largest: 4.3e-7 bohr.  The 65-molecule box is this suite's own
choice and is held to that bar, not part of it: its spread is 2.2e-7 bohr and L-BFGS-B lands 2.3e-7 bohr from the mirror.
(tests/test_quench_ref.py measures all of this again and holds the bar to it.)
"""
from __future__ import annotations

import functools

import numpy as np

from forces_ref import model_forces

FIRE_DEFAULTS = (20.0, 200.0, 0.2, 0.1, 0.99, 1.1, 0.5, 5.0)     # dt0, dtmax, maxstep, alpha0, f_alpha, f_inc, f_dec, n_min
FTOL = 1e-10                                                      # Hartree / bohr, the quenches the device is compared at
#: the largest spread max |x(ftol 1e-10) - x(ftol 1e-12)| of the mirror over BAR_CASES, measured (module docstring), bohr
POS_SPREAD_MEASURED = 4.3e-8
#: the position bar: ten times that
POS_TOL = 10.0 * POS_SPREAD_MEASURED
#: forces of a single-point evaluation, Hartree / bohr absolute (tests/test_gpu_forces.py holds the engine to 1e-10 relative
#: to the largest force, which is below 1 here: this is the same kind of bar and no wider)
F_ATOL = 1e-10
COM_TOL = 1e-12                                                   # bohr: the centre of mass stays where it was

#: cases the device's quench is compared against the mirror at (48, 64, 65 and 96 molecules, and the disordered one)
QUENCH_CASES = ("ic48_t015", "ih48_t020", "ic64_sheared", "ic65_interstitial", "ic96", "ih96_disordered")
#: the cases the position bar is measured on
BAR_CASES = ("ic48_t015", "ih48_t020", "ic64_sheared", "ic96", "ih96_disordered")
#: cases of the single-point comparison (max_iter = 0)
POINT_CASES = ("dimer", "single_atom", "gas20", "ic48_t015", "ic64_sheared", "ic96", "ih1536_t012", "ic65_interstitial")


@functools.lru_cache(maxsize=None)
def load_case(name):
    """(h [3, 3], xyz [n, 3]) in bohr.  Golden boxes by name; ``ic65_interstitial``: ic64_sheared with one molecule more at the
    fractional position (19, 5, 17) / 24, the centre of a cavity 5.43 bohr from its nearest molecules (65 molecules: the first
    size of the general geometry); ``ih96_disordered``: the (3, 2, 2) Ih box shaken with sigma = 0.5
    Angstrom, seed 5."""
    from mc_water_ls_mw_amd import lattice as lat
    if name == "ic65_interstitial":
        from conftest import load_golden
        z = load_golden("ic64_sheared")
        h = z["h"]
        xyz = np.vstack([z["xyz"], (np.array([19.0, 5.0, 17.0]) / 24.0) @ h])
    elif name == "ih96_disordered":
        h, xyz = lat.ice_box("ih", (3, 2, 2), 0.5, seed=5)
    else:
        from conftest import load_golden
        z = load_golden(name)
        h, xyz = z["h"], z["xyz"]
    h, xyz = np.ascontiguousarray(h, dtype=np.float64), np.ascontiguousarray(xyz, dtype=np.float64)
    h.setflags(write=False), xyz.setflags(write=False)
    return h, xyz


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import COracle
    return COracle()


def energy_forces(h, xyz):
    """(E, F [n, 3]) of one box: forces_ref.model_forces over the C oracle's lists built from these positions."""
    C = _oracle()
    iv = C.ivects(h)
    nn, jn, vn = C.neighbours(xyz, iv)
    e, f, _ = model_forces(xyz, iv, nn, jn, vn)
    return float(e), f


def quench(h, xyz, ftol=FTOL, max_iter=10000, fire=None):
    """The contract's FIRE on one box.  Returns a dict: pos, forces, stats [6] (E at the start, E at the end, fmax at the
    start, fmax at the end, the largest and the rms displacement), iters (iterations, converged) and energies, the E of every
    evaluation."""
    dt0, dtmax, maxstep, alpha0, f_alpha, f_inc, f_dec, n_min = FIRE_DEFAULTS if fire is None else fire
    x0 = np.array(xyz, dtype=np.float64)
    x, v = x0.copy(), np.zeros_like(x0)
    dt, alpha, npos, t = dt0, alpha0, 0, 0
    energies = []
    while True:
        e, f = energy_forces(h, x)                                     # 1
        fmax = float(np.abs(f).max())
        energies.append(e)
        if t == 0:
            e_start, f_start = e, fmax
        if fmax <= ftol:                                               # 2
            converged = 1
            break
        if t == max_iter:                                              # 3
            converged = 0
            break
        p = float((f * v).sum())                                       # 4
        if p > 0.0:                                                    # 5
            npos += 1
            v = (1.0 - alpha) * v + alpha * f * np.sqrt((v * v).sum() / (f * f).sum())
            if npos > n_min:
                dt = min(dt * f_inc, dtmax)
                alpha *= f_alpha
        else:                                                          # 6
            npos = 0
            v = np.zeros_like(v)
            dt *= f_dec
            alpha = alpha0
        v = v + dt * f                                                 # 7
        dx = dt * v
        largest = float(np.sqrt((dx * dx).sum(axis=1)).max())          # 8
        if largest > maxstep:
            dx = dx * (maxstep / largest)
        x = x + dx                                                     # 9
        t += 1
    disp = np.sqrt(((x - x0) ** 2).sum(axis=1))
    stats = np.array([e_start, e, f_start, fmax, disp.max(), np.sqrt((disp * disp).mean())])
    return dict(pos=x, forces=f, stats=stats, iters=np.array([t, converged], dtype=np.int32), energies=np.array(energies))


@functools.lru_cache(maxsize=None)
def reference(name, ftol=FTOL):
    """The mirror's quench of a case at the defaults, computed once per process and shared: treat it as read-only."""
    h, xyz = load_case(name)
    r = quench(h, xyz, ftol)
    for k in ("pos", "forces", "stats", "iters", "energies"):
        r[k].setflags(write=False)
    return r


def widths(h):
    vol = abs(np.linalg.det(h))
    return np.array([vol / np.linalg.norm(np.cross(h[(k + 1) % 3], h[(k + 2) % 3])) for k in range(3)])
