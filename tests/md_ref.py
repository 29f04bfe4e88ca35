"""numpy mirror of the contract of include/mw_md.h: BAOAB per box on the full-box mW energy at fixed cell, NVE or Langevin with
the Philox4x32-10 / Box-Muller noise of the header, and the bars tests/test_md_ref.py (CPU, the preconditions) and
tests/test_gpu_md.py (the device) share.

Energy and forces are quench_ref.energy_forces (forces_ref.model_forces over the C oracle's lists, rebuilt from the current
positions at every evaluation); Philox and the Box-Muller rule are written again here in numpy.  The mirror shares no code with
the library and does not reproduce its rounding: the device is held to it within bars, not bit for bit.

Bars (all measured with the mirror on the CPU, none chosen from a device result; tests/test_md_ref.py measures every one again
and holds the constants to it).  The experiment of the trajectory bar: 40 steps of 5 fs from maxwell_boltzmann velocities at
250 K (seed 7), NVE and Langevin with gamma = 1 / (100 fs), once as is and once with every force evaluation perturbed by
seeded uniform noise of +-quench_ref.F_ATOL = 1e-10 Hartree / bohr per component -- the bar this project already holds this
force code to.  The spread is the largest deviation between the two runs after 40 steps over BAR_CASES:
    case              positions NVE / Langevin (bohr)   velocities NVE / Langevin (bohr / atu)
    ic48_t015         1.02e-8 / 6.89e-9                 5.08e-12 / 2.90e-12
    ih48_t020         1.16e-8 / 6.41e-9                 6.35e-12 / 3.44e-12
    ic64_sheared      3.81e-8 / 1.58e-8                 9.94e-12 / 3.30e-12
    ic96              1.10e-8 / 6.70e-9                 4.78e-12 / 2.90e-12
    ih96_disordered   3.73e-8 / 1.51e-8                 2.79e-11 / 5.57e-12
and the trace's columns over all 41 rows, largest at ih96_disordered NVE: E 2.06e-9 and K 1.71e-9 Hartree, the mean squared
displacement 9.04e-9 bohr^2, fmax 5.94e-10 Hartree / bohr.  ic65_interstitial shows 3.71e-8 / 1.70e-8 bohr, 1.72e-11 / 4.88e-12
and 1.52e-8 bohr^2 in the mean squared displacement.  Reversal (40 steps, v -> -v, 40 steps): the mirror returns to within
7.1e-15 ... 3.6e-14 bohr (ih96_disordered).  Energy: on ih48_t020 the largest |E + K - (E + K)(0)| over 400 steps of 5 fs is
1.0221e-3 Hartree and over 800 steps of 2.5 fs 2.5540e-4: ratio 4.0019 (second order: 4); the force noise moves the ratio by 3.03e-7.
(see POS_SPREAD_MEASURED and its neighbours for the figures held; the 65-molecule box is held to the bars and is not part of
them).  The bars are ten times the spreads, the quench suite's factor.
"""
from __future__ import annotations

import functools
import math

import numpy as np

from quench_ref import BAR_CASES, F_ATOL, energy_forces, load_case

MASS_WATER = 18.01528 * 1822.888486209
FS = 1.0e-15 / 2.4188843265857e-17
KELVIN = 3.1668115634556e-6
A_SIGMA = 2.3925 / 0.5291772108 * 1.8                              # bohr
LIM2 = (A_SIGMA / 4.0) ** 2

#: the experiment of the trajectory bar
BAR_STEPS, BAR_DT, BAR_KT, BAR_GAMMA, BAR_VEL_SEED, BAR_SEED = 40, 5.0 * FS, 250.0 * KELVIN, 1.0 / (100.0 * FS), 7, 2024
#: cases the device's trajectories are compared against the mirror at: the bar cases and the first size of the general geometry
TRAJECTORY_CASES = BAR_CASES + ("ic65_interstitial",)
#: the largest deviation after 40 steps between the mirror and the mirror with forces perturbed by +-F_ATOL, over BAR_CASES
#: and both ensembles, measured (module docstring): positions in bohr, velocities in bohr per atomic time unit, the trace's
#: columns (E and K in Hartree, the mean squared displacement in bohr^2, fmax in Hartree / bohr) over all 41 rows
POS_SPREAD_MEASURED = 3.81e-8
VEL_SPREAD_MEASURED = 2.79e-11
TRACE_SPREAD_MEASURED = (2.06e-9, 1.71e-9, 9.04e-9, 5.94e-10)
POS_TOL = 10.0 * POS_SPREAD_MEASURED
VEL_TOL = 10.0 * VEL_SPREAD_MEASURED
TRACE_TOL = tuple(10.0 * s for s in TRACE_SPREAD_MEASURED)
#: reversal: 40 steps NVE, the velocities negated, 40 more: the mirror's own largest |x - x(0)| over BAR_CASES, measured, bohr
REVERSAL_RETURN_MEASURED = 3.56e-14
REVERSAL_TOL = 10.0 * REVERSAL_RETURN_MEASURED
#: energy conservation: the largest |E + K - (E + K)(0)| over 400 steps of 5 fs NVE divided by the same over 800 steps of 2.5 fs,
#: the mirror on ih48_t020 from the bar's velocities, measured; and the difference the force noise makes in that ratio
ENERGY_STEPS = 400
ENERGY_RATIO_MEASURED = 4.0018987
ENERGY_RATIO_NOISE_MEASURED = 3.03e-7
ENERGY_RATIO_TOL = 10.0 * ENERGY_RATIO_NOISE_MEASURED


# -- Philox4x32-10 and the normals -------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """The four output words of the counters (arrays or scalars, 32-bit values) under the key (k0, k1)."""
    M0, M1, W0, W1, MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK) for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.asarray(k0, dtype=np.uint64) & np.uint64(MASK), np.asarray(k1, dtype=np.uint64) & np.uint64(MASK)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + np.uint64(W0)) & np.uint64(MASK), (k1 + np.uint64(W1)) & np.uint64(MASK)
    return c


def words(seed, stream, step, nmol):
    """[4, nmol] output words of the molecules 0 .. nmol - 1 of the box with stream identity ``stream`` at step index ``step``."""
    seed, stream, step = int(seed), int(stream), int(step)
    key = seed ^ stream
    mol = np.arange(nmol, dtype=np.uint64)
    return np.array(philox4x32_10(step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF, mol, 0, key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF))


def normals(seed, stream, step, nmol):
    """[nmol, 3] xi of the header: u = (w + 0.5) 2^-32, two Box-Muller pairs, the first three normals."""
    u = (words(seed, stream, step, nmol).astype(np.float64) + 0.5) * 2.0 ** -32
    r0, t0 = np.sqrt(-2.0 * np.log(u[0])), (2.0 * math.pi) * u[1]
    r1, t1 = np.sqrt(-2.0 * np.log(u[2])), (2.0 * math.pi) * u[3]
    return np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1)], axis=1)


def constants(dt, mass, kT, gamma):
    """(hk, hd, c1, c2, hm) as the header forms them."""
    c1 = math.exp(-gamma * dt)
    return dt / (2.0 * mass), dt / 2.0, c1, math.sqrt((kT / mass) * (1.0 - c1 * c1)), mass / 2.0


def maxwell_boltzmann(nboxes, nwater, kT, mass=MASS_WATER, seed=0):
    """The rule of dynamics.maxwell_boltzmann, written again."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((int(nboxes), int(nwater), 3)) * np.sqrt(float(kT) / float(mass))
    return np.ascontiguousarray(v - v.mean(axis=1, keepdims=True))


# -- the step ------------------------------------------------------------------------------------
def _guard_fails(hd, v):
    d = hd * v
    return not bool(np.all((d * d).sum(axis=1) <= LIM2))


def run(h, xyz, nsteps, dt, kT=0.0, gamma=0.0, vel=None, mass=MASS_WATER, seed=0, stream=0, step0=0, sample_every=1, pos_ref=None, force_noise=None,
        forces_of=energy_forces):
    """The contract's BAOAB on one box.  Returns a dict: pos, vel, forces, trace [nsteps // sample_every + 1, 4] and status
    (steps completed, frozen).  ``force_noise``: a numpy Generator; every force evaluation is then perturbed by uniform noise
    of +-F_ATOL per component (the experiment of the bars)."""
    hk, hd, c1, c2, hm = constants(dt, mass, kT, gamma)
    x = np.array(xyz, dtype=np.float64)
    n = len(x)
    v = np.zeros_like(x) if vel is None else np.array(vel, dtype=np.float64)
    ref = x.copy() if pos_ref is None else np.array(pos_ref, dtype=np.float64)

    def evaluate(x):
        e, f = forces_of(h, x)
        if force_noise is not None:
            f = f + force_noise.uniform(-F_ATOL, F_ATOL, size=f.shape)
        return e, f

    def row(e, f):
        return np.array([e, hm * (v * v).sum(), ((x - ref) ** 2).sum() / n, np.abs(f).max()])

    trace = np.zeros((nsteps // sample_every + 1, 4))
    e, f = evaluate(x)
    cur = row(e, f)
    trace[0] = cur
    steps, frozen = 0, 0
    for s in range(nsteps):
        v = v + hk * f                                                 # 1
        if _guard_fails(hd, v):                                        # 2
            frozen = 1
            break
        x = x + hd * v
        if gamma > 0.0:                                                # 3
            v = c1 * v + c2 * normals(seed, stream, step0 + s, n)
        if _guard_fails(hd, v):                                        # 4
            frozen = 1
            break
        x = x + hd * v
        e, f = evaluate(x)                                             # 5
        v = v + hk * f                                                 # 6
        steps = s + 1
        cur = row(e, f)
        if steps % sample_every == 0:
            trace[steps // sample_every] = cur
    if frozen:
        trace[steps // sample_every + 1:] = cur
    return dict(pos=x, vel=v, forces=f, trace=trace, status=np.array([steps, frozen], dtype=np.int32))


def free_gas20():
    """(h, xyz) of 20 molecules that exert no force on each other: a 4 x 5 grid of 30 bohr in a 120 x 150 x 30 bohr cell, every
    distance to a molecule or an image 30 bohr at the start, a sigma = 8.14 bohr: 200 thermostatted steps of 5 fs at 250 K move a
    molecule by 2 bohr rms, so that no pair comes into range (22 bohr to go, eight standard deviations of the pair's distance).  (The golden gas20 is a dense gas, E = 7.0
    Hartree: its forces are far from zero, and the experiments that need v' = c1 v + c2 xi exactly cannot use it.)"""
    ij = np.array([(i, j) for i in range(4) for j in range(5)], dtype=np.float64)
    xyz = np.column_stack([30.0 * ij[:, 0] + 1.0, 30.0 * ij[:, 1] + 2.0, np.full(20, 3.0)])
    return np.diag([120.0, 150.0, 30.0]), np.ascontiguousarray(xyz)


def bar_velocities(name):
    """The velocities every trajectory experiment starts from: maxwell_boltzmann at 250 K, seed 7."""
    _, xyz = load_case(name)
    return maxwell_boltzmann(1, len(xyz), BAR_KT, MASS_WATER, BAR_VEL_SEED)[0]


@functools.lru_cache(maxsize=None)
def reference(name, langevin, noisy=False):
    """The mirror's 40-step trajectory of a case in the bar's experiment, computed once per process and shared: read-only."""
    h, xyz = load_case(name)
    r = run(h, xyz, BAR_STEPS, BAR_DT, BAR_KT if langevin else 0.0, BAR_GAMMA if langevin else 0.0, vel=bar_velocities(name), seed=BAR_SEED,
            stream=3, force_noise=np.random.default_rng(99) if noisy else None)
    for k in r:
        r[k].setflags(write=False)
    return r


def energy_drift(trace):
    """The largest |E + K - (E + K)(0)| of a trace."""
    tot = trace[:, 0] + trace[:, 1]
    return float(np.abs(tot - tot[0]).max())


def energy_ratio(name, noisy=False, steps=ENERGY_STEPS, forces_of=energy_forces):
    """(ratio, drift at dt, drift at dt / 2) of the mirror: ``steps`` steps of 5 fs against twice as many of 2.5 fs, NVE."""
    h, xyz = load_case(name)
    v = bar_velocities(name)
    rng = (lambda: np.random.default_rng(99)) if noisy else (lambda: None)
    a = energy_drift(run(h, xyz, steps, BAR_DT, vel=v, force_noise=rng(), forces_of=forces_of)["trace"])
    b = energy_drift(run(h, xyz, 2 * steps, BAR_DT / 2.0, vel=v, force_noise=rng(), forces_of=forces_of)["trace"])
    return a / b, a, b
