"""numpy mirror of the contract of include/mw_npt.h: the BAOAB step of tests/md_ref.py with the cell as part of the state, the
scalar virial W = tr of forces_ref.model_forces' virial, and the barostat stage restated from the header; and the bars
tests/test_npt_ref.py (CPU, the preconditions) and tests/test_gpu_npt.py (the device) share.

Energy, forces and virial are forces_ref.model_forces over the C oracle's image vectors and lists, rebuilt from the current cell
and positions at every evaluation: the mirror has no cell grid.  Philox, the normals and the constants of the step are md_ref's.
The mirror shares no code with the library and does not reproduce its rounding: the device is held to it within bars.

Bars (all measured with the mirror on the CPU, none chosen from a device result; tests/test_npt_ref.py measures every one again
and holds the constants to it), formed as md_ref forms its own: ten times the spread of the mirror against itself with every
force evaluation perturbed by seeded uniform noise of +-quench_ref.F_ATOL = 1e-10 Hartree / bohr per component.  The virial is a
sum of d . dE/dd over entries with |d| < a sigma, so the same perturbation of a molecule's gradient moves W by delta_i . d_i with
|d_i| < a sigma; the noisy mirror takes d_i = a sigma (1, 1, 1) / sqrt(3) for every molecule: W' = W - a sigma / sqrt(3) sum
delta.  The experiment of the trajectory bar: BAR_STEPS = 40 steps of 5 fs from md_ref.bar_velocities, the barostat at
BAR_PRESSURE = 1 atm with tau_p = 1 ps and beta_T = 4.5e-10 / Pa, baro_every = 1 and 5, deterministic (kT = 0, gamma = 0) and
Langevin (250 K, gamma = 1 / (100 fs), with the barostat's noise), over md_ref's BAR_CASES.  Largest deviations after 40 steps:
positions 3.89e-8 bohr (ih96_disordered, deterministic, baro_every = 5), velocities 1.71e-11 bohr per atomic time unit, cell
components 2.20e-9 bohr (ic64_sheared), and the trace's columns over all rows: E 1.09e-9 and K 1.42e-9 Hartree, the mean squared
displacement 7.80e-9 bohr^2, fmax 4.20e-10 Hartree / bohr, V 3.67e-6 bohr^3, P 3.77e-13 Hartree / bohr^3 (see the constants
below for the figures held; ic65_interstitial is held to the bars and is not part of them).  Single point: W moves by at most
7.64e-9 Hartree over BAR_CASES (ic96 and ih96_disordered); the other POINT_CASES are held to that bar.

The free ensemble (test (b) of the issue): N = 20 molecules without forces, thermostatted, the barostat every step.  With
P = 2 K / (3 V) the stationary law of the stage in eps = ln V is p(V) ~ V^N exp(-pressure V / kT): <V> = (N + 1) kT / pressure,
var V = (N + 1) (kT / pressure)^2.  `free_volumes` is the mirror's step with the forces switched off, vectorised over boxes,
with numpy's generator for the noise (the statistics, not the stream, are its subject; the device's stream is held to the
mirror's by the trajectory tests).  One application relaxes ln V at the rate cb * pressure, so the relaxation time is
1 / (cb pressure) applications.  FREE_CB is chosen so that MW_NPT_MAX_DLNV = 0.3 is more than 8 standard deviations
cn / sqrt(V) of the noise term at the mean volume.  The Euler step of the stage leaves a bias of first order in cb pressure in
<V>; FREE_HALVING_MEASURED is the difference of the mean volumes at cb and cb / 2, and to first order the bias at cb is twice
it (FREE_BIAS).  At cb pressure = 0.01 the difference is inside the sampling error of the two means -- the bias of the mean is
small -- and it is recorded as measured, like that of the variance.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import md_ref
from forces_ref import model_forces
from md_ref import A_SIGMA, BAR_DT, BAR_GAMMA, BAR_KT, BAR_SEED, BAR_STEPS, FS, LIM2, MASS_WATER
from quench_ref import BAR_CASES, F_ATOL, load_case, _oracle

PASCAL = 1.0 / 2.9421015697e13
ATM = 101325.0 * PASCAL
MAX_DLNV = 0.3
GUARD = 1.0 + 1e-9

#: the experiment of the trajectory bar
BAR_PRESSURE, BAR_TAU_P, BAR_BETA_T = ATM, 1000.0 * FS, 4.5e-10 / PASCAL
BAR_BARO = (1, 5)
#: cases of the single-point comparison of W
POINT_CASES = ("dimer", "gas20", "ic48_t015", "ih48_t020", "ic64_sheared", "ic65_interstitial", "ic96", "ih96_disordered", "ih1536_t012")
#: the largest deviations after 40 steps between the mirror and the mirror with perturbed forces, over BAR_CASES, both modes and
#: both baro_every, measured (module docstring)
POS_SPREAD_MEASURED = 3.89e-8
VEL_SPREAD_MEASURED = 1.71e-11
CELL_SPREAD_MEASURED = 2.20e-9
TRACE_SPREAD_MEASURED = (1.09e-9, 1.42e-9, 7.80e-9, 4.20e-10, 3.67e-6, 3.77e-13)
W_SPREAD_MEASURED = 7.64e-9
POS_TOL = 10.0 * POS_SPREAD_MEASURED
VEL_TOL = 10.0 * VEL_SPREAD_MEASURED
CELL_TOL = 10.0 * CELL_SPREAD_MEASURED
TRACE_TOL = tuple(10.0 * s for s in TRACE_SPREAD_MEASURED)
W_TOL = 10.0 * W_SPREAD_MEASURED

#: the free ensemble: N, kT (hot, so that the pair term's second virial coefficient is small: see FREE_B2), the cell -- three times
#: that of md_ref.free_gas20 each way, 360 x 450 x 90 bohr --, the pressure whose mean volume that cell is, cb pressure = 0.01 per
#: application (the noise term's standard deviation sqrt(2 * 0.01 / (N + 1)) = 0.031 at the mean volume: MW_NPT_MAX_DLNV is 9.7 of
#: them), 2400 applications = 24 relaxation times, the thermostat and the step
FREE_N = 20
FREE_KT = 0.05
FREE_SCALE = 3.0
FREE_VOLUME = 120.0 * 150.0 * 30.0 * FREE_SCALE ** 3
FREE_PRESSURE = (FREE_N + 1) * FREE_KT / FREE_VOLUME
FREE_RATE = 0.01
FREE_CB = FREE_RATE / FREE_PRESSURE
FREE_APPLICATIONS = 2400
FREE_GAMMA_DT = 0.1
FREE_DT = 2.0 * FS
#: (<V>(cb) - <V>(cb / 2)) / ((N + 1) kT / pressure), FREE_BOXES boxes, seeds 5 and 6, measured; to first order the bias of <V> at
#: cb is twice this
FREE_BOXES = 16384
FREE_HALVING_MEASURED = 5.26e-4
FREE_BIAS = 2.0 * abs(FREE_HALVING_MEASURED)
#: the same for the variance over (N + 1) (kT / pressure)^2
FREE_VAR_HALVING_MEASURED = 1.22e-3
FREE_VAR_BIAS = 2.0 * abs(FREE_VAR_HALVING_MEASURED)
#: the second virial coefficient of the mW pair term at FREE_KT, -2 pi int (exp(-phi / kT) - 1) r^2 dr over r < a sigma by the
#: midpoint rule (second_virial below), bohr^3, measured; the device test needs N |B2| / V below a tenth of its standard error
FREE_B2_MEASURED = -3.80


def widths(h):
    vol = abs(np.linalg.det(h))
    return np.array([vol / np.linalg.norm(np.cross(h[(k + 1) % 3], h[(k + 2) % 3])) for k in range(3)])


def cell_ok(h):
    """The cell rule of the header: a sigma (1 + 1e-9) <= the smallest perpendicular width, the determinant finite and not 0."""
    det = np.linalg.det(h)
    return bool(np.isfinite(det) and det != 0.0 and A_SIGMA * GUARD <= widths(h).min())


def energy_forces_virial(h, xyz):
    """(E, F [n, 3], W) of one box: forces_ref.model_forces over the C oracle's lists built from this cell and these positions."""
    C = _oracle()
    iv = C.ivects(h)
    nn, jn, vn = C.neighbours(xyz, iv)
    e, f, vir = model_forces(xyz, iv, nn, jn, vn)
    return float(e), f, float(np.trace(vir))


def barostat_constants(dt, kT, tau_p, beta_T, baro_every):
    """(cb, cn) as the header forms them."""
    dtb = float(baro_every) * dt
    cb = beta_T * dtb / tau_p
    return cb, math.sqrt(2.0 * kT * cb)


def box_normal(seed, stream, step):
    """The barostat's normal: Philox counter (step low, step high, 0xFFFFFFFF, 1) under the box's key, the first Box-Muller normal."""
    key = int(seed) ^ int(stream)
    w = md_ref.philox4x32_10(step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF, 0xFFFFFFFF, 1, key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF)
    u = (np.array(w).astype(np.float64) + 0.5) * 2.0 ** -32
    return float(np.sqrt(-2.0 * np.log(u[0])) * np.cos((2.0 * math.pi) * u[1]))


def _guard_fails(hd, v):
    d = hd * v
    return not bool(np.all((d * d).sum(axis=1) <= LIM2))


def run(h, xyz, nsteps, dt, pressure=ATM, kT=0.0, gamma=0.0, tau_p=BAR_TAU_P, beta_T=BAR_BETA_T, baro_every=0, vel=None, mass=MASS_WATER, seed=0,
        stream=0, step0=0, sample_every=1, pos_ref=None, force_noise=None, forces_of=energy_forces_virial):
    """The contract's step on one box.  Returns a dict: pos, vel, forces, cell, ref, trace [nsteps // sample_every + 1, 6],
    status (steps completed, 0 / 1 / 2) and w, the virial at the end.  ``force_noise``: a numpy Generator; every evaluation is
    then perturbed as the module docstring says."""
    hk, hd, c1, c2, hm = md_ref.constants(dt, mass, kT, gamma)
    cb, cn = barostat_constants(dt, kT, tau_p, beta_T, baro_every)
    h = np.array(h, dtype=np.float64)
    x = np.array(xyz, dtype=np.float64)
    n = len(x)
    v = np.zeros_like(x) if vel is None else np.array(vel, dtype=np.float64)
    ref = x.copy() if pos_ref is None else np.array(pos_ref, dtype=np.float64)

    def evaluate(h, x):
        e, f, w = forces_of(h, x)
        if force_noise is not None:
            d = force_noise.uniform(-F_ATOL, F_ATOL, size=f.shape)
            f, w = f + d, w - A_SIGMA / math.sqrt(3.0) * float(d.sum())
        return e, f, w

    def row(e, f, w):
        vol = abs(np.linalg.det(h))
        k = hm * (v * v).sum()
        return np.array([e, k, ((x - ref) ** 2).sum() / n, np.abs(f).max(), vol, (2.0 * k + w) / (3.0 * vol)])

    trace = np.zeros((nsteps // sample_every + 1, 6))
    e, f, w = evaluate(h, x)
    cur = row(e, f, w)
    trace[0] = cur
    steps, code = 0, 0
    for s in range(nsteps):
        t = step0 + s
        v = v + hk * f                                                 # 1
        if _guard_fails(hd, v):                                        # 2
            code = 1
            break
        x = x + hd * v
        if gamma > 0.0:                                                # 3
            v = c1 * v + c2 * md_ref.normals(seed, stream, t, n)
        if _guard_fails(hd, v):                                        # 4
            code = 1
            break
        x = x + hd * v
        e, f, w = evaluate(h, x)                                       # 5
        v = v + hk * f                                                 # 6
        steps = s + 1
        cur = row(e, f, w)
        if steps % sample_every == 0:
            trace[steps // sample_every] = cur
        if baro_every > 0 and (t + 1) % baro_every == 0:               # the barostat stage
            vol = cur[4]
            de = -(cb * (pressure - cur[5]))
            if kT > 0.0:
                de = de + cn * box_normal(seed, stream, t) / math.sqrt(vol)
            mu = math.exp(de / 3.0) if abs(de) <= MAX_DLNV else float("nan")
            if not (abs(de) <= MAX_DLNV) or not cell_ok(mu * h):
                code = 2
                break
            h, x, ref, v = mu * h, mu * x, mu * ref, v / mu
            e, f, w = evaluate(h, x)
            cur = row(e, f, w)
            if steps % sample_every == 0:
                trace[steps // sample_every] = cur
    if code:
        trace[steps // sample_every + 1:] = cur
    return dict(pos=x, vel=v, forces=f, cell=h, ref=ref, trace=trace, status=np.array([steps, code], dtype=np.int32), w=np.array(w))


def bar_kwargs(langevin, baro_every):
    return dict(pressure=BAR_PRESSURE, kT=BAR_KT if langevin else 0.0, gamma=BAR_GAMMA if langevin else 0.0, tau_p=BAR_TAU_P, beta_T=BAR_BETA_T,
                baro_every=baro_every, seed=BAR_SEED)


@functools.lru_cache(maxsize=None)
def reference(name, langevin, baro_every, noisy=False):
    """The mirror's 40-step trajectory of a case in the bar's experiment, computed once per process and shared: read-only."""
    h, xyz = load_case(name)
    r = run(h, xyz, BAR_STEPS, BAR_DT, vel=md_ref.bar_velocities(name), stream=3, force_noise=np.random.default_rng(99) if noisy else None,
            **bar_kwargs(langevin, baro_every))
    for k in r:
        r[k].setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def point(name, noisy=False):
    """(E, F, W) of a case's own positions, with or without the perturbation of the bars."""
    h, xyz = load_case(name)
    r = run(h, xyz, 0, BAR_DT, force_noise=np.random.default_rng(99) if noisy else None)
    return float(r["trace"][0, 0]), r["forces"], float(r["w"])


def narrow_gas(n, margin=1e-6):
    """(h, xyz) of n molecules that exert no force on each other in a cell whose first width is a sigma (1 + 1e-9) (1 + margin):
    a square grid of 22 bohr in y and z (a sigma = 8.14 bohr), the images along x just beyond the cutoff."""
    m = int(math.ceil(math.sqrt(n)))
    ij = np.array([(i, j) for i in range(m) for j in range(m)][:n], dtype=np.float64)
    xyz = np.column_stack([np.full(n, 1.0), 22.0 * ij[:, 0] + 2.0, 22.0 * ij[:, 1] + 3.0])
    return np.diag([A_SIGMA * GUARD * (1.0 + margin), 22.0 * m, 22.0 * m]), np.ascontiguousarray(xyz)


def at_a_grid_edge(name, axis, multiple, margin):
    """(h, xyz) of a case scaled so that its width along ``axis`` is ``multiple`` a sigma (1 + 1e-9) (1 + margin)."""
    h, xyz = load_case(name)
    s = multiple * A_SIGMA * GUARD * (1.0 + margin) / widths(h)[axis]
    return s * h, s * xyz


#: the grid-edge runs of ic96, deterministic, the barostat every step: (axis, multiple, margin, pressure) -- expanded by 2 % until its
#: third width is 0.5 % above 6 cutoffs and pressed together with 3000 atm; compressed by 4 % until its first width is 0.5 % below 3
#: (and its second 0.7 % below 2) and left to expand at 1 atm
EDGE_CASES = ((2, 6, 5e-3, 3000.0 * ATM), (0, 3, -5e-3, ATM))


@functools.lru_cache(maxsize=None)
def edge_reference(axis, multiple, margin, pressure):
    h, xyz = at_a_grid_edge("ic96", axis, multiple, margin)
    r = run(h, xyz, BAR_STEPS, BAR_DT, vel=md_ref.bar_velocities("ic96"), pressure=pressure, baro_every=1)
    for k in r:
        r[k].setflags(write=False)
    return r


#: the physics smoke: ic96 below the melting point of mW ice (274 K), 300 steps of 5 fs with the thermostat of the bars, 1 atm, the
#: barostat every 10 steps, sampled every 10; the spread under force noise of V and of the enthalpy-like sum E + K + pressure V
#: over the 31 rows, measured
SMOKE_CASE, SMOKE_STEPS, SMOKE_EVERY = "ic96", 300, 10
SMOKE_V_SPREAD_MEASURED = 6.01e-6
SMOKE_H_SPREAD_MEASURED = 5.04e-10
SMOKE_V_TOL = 10.0 * SMOKE_V_SPREAD_MEASURED
SMOKE_H_TOL = 10.0 * SMOKE_H_SPREAD_MEASURED


@functools.lru_cache(maxsize=None)
def smoke_reference(noisy=False):
    h, xyz = load_case(SMOKE_CASE)
    r = run(h, xyz, SMOKE_STEPS, BAR_DT, vel=md_ref.bar_velocities(SMOKE_CASE), stream=3, sample_every=SMOKE_EVERY,
            force_noise=np.random.default_rng(99) if noisy else None, **bar_kwargs(True, SMOKE_EVERY))
    for k in r:
        r[k].setflags(write=False)
    return r


def enthalpy(trace, pressure=BAR_PRESSURE):
    return trace[:, 0] + trace[:, 1] + pressure * trace[:, 4]


def free_volumes(nboxes, cb, applications, seed, n=FREE_N, kT=FREE_KT, pressure=FREE_PRESSURE, gamma_dt=FREE_GAMMA_DT):
    """(final volumes [nboxes], any refused) of the mirror's step with the forces switched off and baro_every = 1, from the mean
    volume and equilibrium velocities.  Without forces the kicks are zero and the drifts move nothing the volume sees; what is
    left of a step is the thermostat v = c1 v + c2 xi and the barostat stage with W = 0, P = 2 K / (3 V), V <- mu^3 V, v <- v / mu.
    The stage sees the velocities through K alone, and K' = hm |c1 v + c2 xi|^2 given K is hm c2^2 times a noncentral chi-square
    of 3 n degrees with noncentrality c1^2 |v|^2 / c2^2 whatever the direction of v: the mirror carries (V, K) per box, which is
    the same chain in law as carrying every velocity (the mass drops out: K is carried in units of kT)."""
    rng = np.random.default_rng(seed)
    c1 = math.exp(-gamma_dt)
    s2 = 1.0 - c1 * c1                                  # c2^2 in units of kT / mass
    cn = math.sqrt(2.0 * kT * cb)
    vol = np.full(nboxes, (n + 1) * kT / pressure)
    q = rng.chisquare(3 * n, nboxes)                    # |v|^2 in units of kT / mass; K = kT q / 2
    refused = False
    for _ in range(applications):
        q = s2 * rng.noncentral_chisquare(3 * n, c1 * c1 * q / s2)
        p = (2.0 * (0.5 * kT * q) + 0.0) / (3.0 * vol)
        de = -(cb * (pressure - p)) + cn * rng.standard_normal(nboxes) / np.sqrt(vol)
        refused = refused or bool(np.any(~(np.abs(de) <= MAX_DLNV)))
        mu = np.exp(de / 3.0)
        vol = vol * mu ** 3
        q = q / (mu * mu)
    return vol, refused


def pair_energy(r):
    """The mW pair term phi(r) = A eps (B (sigma / r)^4 - 1) exp(sigma / (r - a sigma)) below a sigma, 0 beyond (Hartree, bohr)."""
    from forces_ref import constants
    sigma, eps, _, big_a, big_b, _, small_a, _ = (float(c) for c in constants())
    r = np.asarray(r, dtype=np.float64)
    inr = r < small_a * sigma
    den = np.where(inr, r - small_a * sigma, -1.0)
    return np.where(inr, big_a * eps * (big_b * (sigma / r) ** 4 - 1.0) * np.exp(sigma / den), 0.0)


def second_virial(kT, points=200000):
    """B2 = -2 pi int_0^(a sigma) (exp(-phi / kT) - 1) r^2 dr of the pair term, midpoint rule, bohr^3."""
    dr = A_SIGMA / points
    r = (np.arange(points) + 0.5) * dr
    return float(-2.0 * math.pi * ((np.exp(-pair_energy(r) / kT) - 1.0) * r * r).sum() * dr)
