"""numpy mirror of the contract of include/mw_ti.h: the BAOAB step of md_ref (Philox, Box-Muller, the guard) on the mixed energy
(1 - lambda) E_mW + lambda 1/2 k sum |x - s|^2, the five trace fields and the block means, and the bars tests/test_ti_ref.py (CPU,
the preconditions) and tests/test_gpu_ti.py (the device) share.  Energy and forces of mW are quench_ref.energy_forces.  The
mirror shares no code with the library and does not reproduce its rounding: the device is held to it within bars.

Bars (all measured with the mirror on the CPU, none from a device result; tests/test_ti_ref.py measures every one again and holds
the constants to it).  The experiment is md_ref's: 40 steps of 5 fs from md_ref.bar_velocities (250 K, seed 7), NVE and Langevin
with gamma = 1 / (100 fs), seed 2024 and stream 3, over BAR_CASES at lambda = 0.3 and 0.8 with k = 0.02 Hartree / bohr^2; the sites
are the case's positions minus seeded uniform noise of +-0.2 bohr (seed 31), so that u is not zero at step 0; equil_steps = 5 and
block_steps = 7 (five blocks).  Every run is made once as is and once with every F_mW perturbed by seeded uniform noise of
+-quench_ref.F_ATOL per component; the spread is the largest deviation between the two over BAR_CASES, both lambdas and both
ensembles.  Measured:
    positions 1.04e-8 bohr (ih96_disordered), velocities 5.21e-12 bohr / atu,
    trace (all 41 rows): E_mW 6.35e-10 and K 3.38e-10 Hartree, sum |u|^2 / N 5.88e-10 bohr^2, fmax 4.94e-10 Hartree / bohr,
    |sum u / N|^2 6.82e-11 bohr^2;  block means: 2.80e-10, 1.73e-10, 5.16e-10, 7.15e-11, 5.26e-11 in the same units.
ic65_interstitial shows 7.42e-9 bohr, 3.73e-12 bohr / atu and at most 4.28e-10 in a trace column: it is held to the bars and is
not part of them.
(the figures held are SPREAD_* below).  The bars are ten times the spreads, the factor of md_ref and quench_ref.  The spreads
are smaller than md_ref's because the spring at k = 0.02 holds a perturbed trajectory near the unperturbed one.

Closed forms (lambda = 1: the mW force does not enter the state).  One coordinate of one molecule is a linear map per step,
a = hk k: NVE (u, v) -> M (u, v), M = [[1 - dt a, dt], [-a (2 - dt a), 1 - dt a]] (nve_matrix); Langevin (u, v) -> T (u, v) + G (0,
c2 xi) with T = A D O D A, G = A D, A = [[1, 0], [-a, 1]], D = [[1, hd], [0, 1]], O = diag(1, c1), whose stationary covariance
solves the discrete Lyapunov equation S = T S T' + c2^2 G e2 e2' G' (langevin_stationary).  At dt = 5 fs, gamma = 1 / (100 fs),
250 K this gives k <u^2> / kT = 1 to 1e-14 for k = 0.005 ... 0.1 while m <v^2> / kT runs from 0.998 to 0.967: BAOAB samples the
positions of a harmonic oscillator exactly and the velocities not, so a velocity bar must come from the Lyapunov value.
"""
from __future__ import annotations

import functools

import numpy as np

import md_ref
from md_ref import BAR_DT, BAR_GAMMA, BAR_KT, BAR_SEED, BAR_STEPS, MASS_WATER
from quench_ref import BAR_CASES, F_ATOL, energy_forces, load_case

#: the experiment of the bars beyond md_ref's
BAR_LAMBDAS, BAR_SPRING, BAR_SITE_NOISE, BAR_SITE_SEED, BAR_EQUIL, BAR_BLOCK, BAR_STREAM = (0.3, 0.8), 0.02, 0.2, 31, 5, 7, 3
#: cases the device is compared against the mirror at: the bar cases and the first size of the general geometry
TRAJECTORY_CASES = BAR_CASES + ("ic65_interstitial",)
#: the largest deviation between the mirror and the mirror with F_mW perturbed by +-F_ATOL (module docstring), measured
SPREAD_POS = 1.04e-8
SPREAD_VEL = 5.21e-12
SPREAD_TRACE = (6.35e-10, 3.38e-10, 5.88e-10, 4.94e-10, 6.82e-11)
SPREAD_BLOCKS = (2.80e-10, 1.73e-10, 5.16e-10, 7.15e-11, 5.26e-11)
POS_TOL = 10.0 * SPREAD_POS
VEL_TOL = 10.0 * SPREAD_VEL
TRACE_TOL = tuple(10.0 * s for s in SPREAD_TRACE)
BLOCKS_TOL = tuple(10.0 * s for s in SPREAD_BLOCKS)


def nblocks_of(nsteps, equil_steps, block_steps):
    return (nsteps - equil_steps) // block_steps if block_steps > 0 and nsteps >= equil_steps else 0


def mixed_force(lam, k, f_mw, u):
    """F_tot of the header: F_mW at lambda = 0, -(lambda k) u at lambda = 1, their mixture between."""
    if lam == 0.0:
        return f_mw
    if lam == 1.0:
        return -(lam * k) * u
    return -(lam * k) * u + (1.0 - lam) * f_mw


def run(h, sites, lam, k, nsteps, dt, kT=0.0, gamma=0.0, pos=None, vel=None, mass=MASS_WATER, seed=0, stream=0, step0=0, sample_every=1,
        equil_steps=0, block_steps=0, force_noise=None, forces_of=energy_forces):
    """The contract on one box.  Returns a dict: pos, vel, forces (F_tot), trace [nsteps // sample_every + 1, 5], blocks [nblocks,
    5] and status (steps completed, frozen).  ``force_noise``: a numpy Generator; every F_mW is then perturbed by uniform noise of
    +-F_ATOL per component."""
    hk, hd, c1, c2, hm = md_ref.constants(dt, mass, kT, gamma)
    s = np.array(sites, dtype=np.float64)
    x = s.copy() if pos is None else np.array(pos, dtype=np.float64)
    n = len(x)
    v = np.zeros_like(x) if vel is None else np.array(vel, dtype=np.float64)

    def evaluate(x):
        e, f = forces_of(h, x)
        if force_noise is not None:
            f = f + force_noise.uniform(-F_ATOL, F_ATOL, size=f.shape)
        return e, mixed_force(lam, k, f, x - s)

    def row(e, f):
        u = x - s
        c = u.sum(axis=0) / n
        return np.array([e, hm * (v * v).sum(), (u * u).sum() / n, np.abs(f).max(), (c * c).sum()])

    nb = nblocks_of(nsteps, equil_steps, block_steps)
    trace = np.zeros((nsteps // sample_every + 1, 5))
    blocks = np.zeros((nb, 5))
    acc = np.zeros(5)
    e, f = evaluate(x)
    cur = row(e, f)
    trace[0] = cur
    steps, frozen = 0, 0
    for st in range(nsteps):
        if not frozen:
            v1 = v + hk * f                                            # 1
            if md_ref._guard_fails(hd, v1):                            # 2
                v, frozen = v1, 1
            else:
                x1 = x + hd * v1
                v2 = c1 * v1 + c2 * md_ref.normals(seed, stream, step0 + st, n) if gamma > 0.0 else v1      # 3
                if md_ref._guard_fails(hd, v2):                        # 4
                    x, v, frozen = x1, v2, 1
                else:
                    x = x1 + hd * v2
                    v = v2
                    e, f = evaluate(x)                                 # 5
                    v = v + hk * f                                     # 6
                    steps = st + 1
                    cur = row(e, f)
                    if steps % sample_every == 0:
                        trace[steps // sample_every] = cur
        t = st - equil_steps
        if nb and t >= 0 and t // block_steps < nb:                    # a frozen box contributes its last row
            acc = acc + cur
            if t % block_steps == block_steps - 1:
                blocks[t // block_steps] = acc / float(block_steps)
                acc = np.zeros(5)
    if frozen:
        trace[steps // sample_every + 1:] = cur
    return dict(pos=x, vel=v, forces=f, trace=trace, blocks=blocks, status=np.array([steps, frozen], dtype=np.int32))


def bar_sites(name):
    """The Einstein sites of the bar's experiment: the case's positions minus seeded uniform noise of +-0.2 bohr."""
    _, xyz = load_case(name)
    return np.ascontiguousarray(xyz - np.random.default_rng(BAR_SITE_SEED).uniform(-BAR_SITE_NOISE, BAR_SITE_NOISE, size=xyz.shape))


@functools.lru_cache(maxsize=None)
def reference(name, langevin, lam, noisy=False):
    """The mirror's 40-step trajectory of a case in the bar's experiment (sample_every = 1), computed once per process and shared:
    read-only."""
    h, xyz = load_case(name)
    r = run(h, bar_sites(name), lam, BAR_SPRING, BAR_STEPS, BAR_DT, BAR_KT if langevin else 0.0, BAR_GAMMA if langevin else 0.0, pos=xyz,
            vel=md_ref.bar_velocities(name), seed=BAR_SEED, stream=BAR_STREAM, equil_steps=BAR_EQUIL, block_steps=BAR_BLOCK,
            force_noise=np.random.default_rng(99) if noisy else None)
    for key in r:
        r[key].setflags(write=False)
    return r


def spreads(cases=BAR_CASES):
    """(positions, velocities, trace [5], blocks [5]): the largest deviations between reference(...) and reference(..., noisy=True)
    over ``cases``, BAR_LAMBDAS and both ensembles."""
    pos = vel = 0.0
    trace, blocks = np.zeros(5), np.zeros(5)
    for name in cases:
        for lam in BAR_LAMBDAS:
            for langevin in (False, True):
                a, b = reference(name, langevin, lam), reference(name, langevin, lam, True)
                pos = max(pos, float(np.abs(a["pos"] - b["pos"]).max()))
                vel = max(vel, float(np.abs(a["vel"] - b["vel"]).max()))
                trace = np.maximum(trace, np.abs(a["trace"] - b["trace"]).max(axis=0))
                blocks = np.maximum(blocks, np.abs(a["blocks"] - b["blocks"]).max(axis=0))
    return pos, vel, trace, blocks


# -- lambda = 1 in closed form ----------------------------------------------------------------------------------------------------
def nve_matrix(k, dt, mass=MASS_WATER):
    """The 2 x 2 map of (u, v) of one coordinate over one NVE step at lambda = 1."""
    a = dt / (2.0 * mass) * k
    return np.array([[1.0 - dt * a, dt], [-a * (2.0 - dt * a), 1.0 - dt * a]])


def nve_exact(u0, v0, k, dt, nsteps, mass=MASS_WATER):
    """(u, v) after ``nsteps`` NVE steps at lambda = 1 from the displacements ``u0`` and velocities ``v0`` (arrays of one shape)."""
    M = np.linalg.matrix_power(nve_matrix(k, dt, mass), int(nsteps))
    return M[0, 0] * u0 + M[0, 1] * v0, M[1, 0] * u0 + M[1, 1] * v0


def langevin_stationary(k, dt, kT, gamma, mass=MASS_WATER):
    """(<u^2>, <v^2>, <u v>) of one coordinate at the end of a step in the stationary state of the lambda = 1 Langevin step."""
    hk, hd, c1, c2, _ = md_ref.constants(dt, mass, kT, gamma)
    a = hk * k
    A, D, O = np.array([[1.0, 0.0], [-a, 1.0]]), np.array([[1.0, hd], [0.0, 1.0]]), np.diag([1.0, c1])
    T, G = A @ D @ O @ D @ A, A @ D
    g = G[:, 1] * c2
    S = np.linalg.solve(np.eye(4) - np.kron(T, T), np.outer(g, g).ravel()).reshape(2, 2)
    return float(S[0, 0]), float(S[1, 1]), float(S[0, 1])
