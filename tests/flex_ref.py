"""numpy mirror of the contract of include/mw_flex.h: the BAOAB step of tests/md_ref.py with the cell as part of the state, the
3 x 3 virial of forces_ref.model_forces used whole, the kinetic tensor, and the per-axis barostat stage restated from the header;
and the bars tests/test_flex_ref.py (CPU, the preconditions) and tests/test_gpu_flex.py (the device) share.

Energy, forces and virial are forces_ref.model_forces over the C oracle's image vectors and lists, rebuilt from the current cell
and positions at every evaluation, as in npt_ref.  Philox, the normals and the constants of the step are md_ref's, the cell rule
npt_ref's.  The mirror shares no code with the library and does not reproduce its rounding: the device is held to it within bars.
The scalar P of the mirror is formed from the trace of its tensor.

Bars (all measured with the mirror on the CPU, none chosen from a device result; tests/test_flex_ref.py measures every one again
and holds the constants to it), formed as npt_ref forms its own: ten times the spread of the mirror against itself with every
force evaluation perturbed by seeded uniform noise delta of +-quench_ref.F_ATOL per component.  The virial tensor is a sum of
d_a dE/dd_b over entries with |d| < a sigma, so the perturbation of a molecule's gradient moves W_ab by the symmetrised
delta_a d_b; as npt_ref does for W, the noisy mirror takes d = a sigma (1, 1, 1) / sqrt(3) for every molecule:
W_ab' = W_ab - a sigma / sqrt(3) (sum delta_a + sum delta_b) / 2, whose trace is npt_ref's W'.  The experiment of the trajectory
bar is npt_ref's (40 steps of 5 fs, 1 atm, tau_p = 1 ps, beta_T = 4.5e-10 / Pa, baro_every = 1 and 5, deterministic and Langevin)
over md_ref's BAR_CASES in the couplings 1, 2 and 3 with axis = 2.  ic65_interstitial and the run with axis = 0 are held to the
bars and are not part of them.

The free ensemble: N = 20 molecules without forces in an orthorhombic cell, thermostatted, the barostat every step.  The law of
the header: p(V) ~ V^N exp(-pressure V / kT) in every coupling.  `free_lengths` is the mirror's stage with the forces switched
off, vectorised over boxes, with numpy's generator; it carries the three lengths and, per axis, |v_a|^2 in units of kT / mass
(a noncentral chi-square of N degrees under the thermostat, as npt_ref carries |v|^2).  The start is a cube of npt_ref's
FREE_VOLUME (244 bohr, 30 cutoffs wide).  cb pressure = FREE_RATE = 0.005 per application, half of npt_ref's: the noise term of a
single axis has the standard deviation sqrt(2 FREE_RATE / (3 (N + 1))) = 0.0126 at the mean volume, and MW_FLEX_MAX_DLNL = 0.1 is
7.9 of them (at npt_ref's 0.01 it would be 5.6, which 3 10^7 draws of the device test reach).  ln V relaxes at FREE_RATE per
application in couplings 1 and 2 (three axes at cb3 each) and at FREE_RATE / 3 in coupling 3: FREE_APPLICATIONS = 800 and 800
are 4 relaxation times, 2400 in coupling 3 are 4 too.  The boxes start at the mean volume with equilibrium velocities, so what
has to grow is the variance, which is 1 - exp(-8) of its stationary value after 4 relaxation times.  The shape modes diffuse
freely: after 800 applications ln of a length has spread by about 0.3 in coupling 1, and tests/test_flex_ref.py asserts that the
smallest length over all boxes and applications stays above twice the cutoff.  The Euler bias is measured by halving cb as
npt_ref does.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import md_ref
import npt_ref
from forces_ref import model_forces
from md_ref import A_SIGMA, BAR_DT, BAR_STEPS, LIM2, MASS_WATER
from npt_ref import ATM, BAR_BARO, BAR_BETA_T, BAR_TAU_P, MAX_DLNV, bar_kwargs, cell_ok
from quench_ref import F_ATOL, load_case, _oracle

ISO, ANISO, SEMI, UNIAXIAL = 0, 1, 2, 3
MAX_DLNL = 0.1
TRACE_FIELDS = 15
#: the couplings and axes of the trajectory experiment: (coupling, axis); the last one is held to the bars, not part of them
BAR_COUPLINGS = ((ANISO, 2), (SEMI, 2), (UNIAXIAL, 2))
EXTRA_COUPLING = (SEMI, 0)

#: the largest deviations after 40 steps between the mirror and the mirror with perturbed forces, over BAR_CASES, BAR_COUPLINGS,
#: both modes and both baro_every, measured (module docstring)
POS_SPREAD_MEASURED = 3.90e-8
VEL_SPREAD_MEASURED = 2.13e-11
CELL_SPREAD_MEASURED = 4.05e-9
TRACE_SPREAD_MEASURED = (1.34e-9, 1.60e-9, 8.19e-9, 6.14e-10, 3.64e-6, 4.43e-13,
                         5.45e-13, 5.62e-13, 6.75e-13, 3.32e-13, 3.80e-13, 3.45e-13, 2.35e-9, 2.06e-9, 4.02e-9)
#: the single point: the largest change of a component of W_ab over npt_ref's POINT_CASES that are BAR_CASES, measured (Hartree)
W_AB_SPREAD_MEASURED = 3.92e-9
POS_TOL = 10.0 * POS_SPREAD_MEASURED
VEL_TOL = 10.0 * VEL_SPREAD_MEASURED
CELL_TOL = 10.0 * CELL_SPREAD_MEASURED
TRACE_TOL = tuple(10.0 * s for s in TRACE_SPREAD_MEASURED)
W_AB_TOL = 10.0 * W_AB_SPREAD_MEASURED

#: the free ensemble (module docstring)
FREE_N = npt_ref.FREE_N
FREE_KT = npt_ref.FREE_KT
FREE_VOLUME = npt_ref.FREE_VOLUME
FREE_PRESSURE = npt_ref.FREE_PRESSURE
FREE_SIDE = FREE_VOLUME ** (1.0 / 3.0)
FREE_RATE = 0.005
FREE_CB = FREE_RATE / FREE_PRESSURE
FREE_APPLICATIONS = {ANISO: 800, SEMI: 800, UNIAXIAL: 2400}
FREE_GAMMA_DT = npt_ref.FREE_GAMMA_DT
FREE_DT = npt_ref.FREE_DT
FREE_BOXES = 16384
#: (<V>(cb) - <V>(cb / 2)) / ((N + 1) kT / pressure) per coupling, FREE_BOXES boxes, seeds 5 and 6, measured; to first order the
#: bias of <V> at cb is twice this -- and the same for the variance over (N + 1) (kT / pressure)^2
FREE_HALVING_MEASURED = {ANISO: -3.15e-4, SEMI: -2.91e-3, UNIAXIAL: -7.63e-4}
FREE_VAR_HALVING_MEASURED = {ANISO: -3.34e-3, SEMI: -2.16e-2, UNIAXIAL: 1.95e-2}
FREE_BIAS = {c: 2.0 * abs(v) for c, v in FREE_HALVING_MEASURED.items()}
FREE_VAR_BIAS = {c: 2.0 * abs(v) for c, v in FREE_VAR_HALVING_MEASURED.items()}


def groups(coupling, axis):
    """The groups of Cartesian axes that share a scale factor, each sorted: its first axis names its normal."""
    a, b = sorted(((axis + 1) % 3, (axis + 2) % 3))
    return {ISO: ((0, 1, 2),), ANISO: ((0,), (1,), (2,)), SEMI: ((a, b), (axis,)), UNIAXIAL: ((axis,),)}[coupling]


def energy_forces_stress(h, xyz):
    """(E, F [n, 3], W_ab [3, 3]) of one box: forces_ref.model_forces over the C oracle's lists built from this cell and these
    positions."""
    C = _oracle()
    iv = C.ivects(h)
    nn, jn, vn = C.neighbours(xyz, iv)
    e, f, vir = model_forces(xyz, iv, nn, jn, vn)
    return float(e), f, np.array(vir, dtype=np.float64)


def barostat_constants(dt, kT, tau_p, beta_T, baro_every):
    """(cb, cn, cb3, cn_1, cn_2) as the header forms them."""
    cb, cn = npt_ref.barostat_constants(dt, kT, tau_p, beta_T, baro_every)
    cb3 = cb / 3.0
    return cb, cn, cb3, math.sqrt(2.0 * kT * cb3 / 1.0), math.sqrt(2.0 * kT * cb3 / 2.0)


def group_normal(seed, stream, step, word):
    """A barostat's normal: Philox counter (step low, step high, 0xFFFFFFFF, word) under the box's key, the first Box-Muller normal."""
    key = int(seed) ^ int(stream)
    w = md_ref.philox4x32_10(step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF, 0xFFFFFFFF, word, key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF)
    u = (np.array(w).astype(np.float64) + 0.5) * 2.0 ** -32
    return float(np.sqrt(-2.0 * np.log(u[0])) * np.cos((2.0 * math.pi) * u[1]))


def _guard_fails(hd, v):
    d = hd * v
    return not bool(np.all((d * d).sum(axis=1) <= LIM2))


PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def decide(cur, kT, pressure, consts, coupling, axis, seed, stream, t):
    """mu [3] of the stage from the row ``cur``, or None when the guard refuses; an axis that no group holds has mu = 1."""
    cb, cn, cb3, cn1, cn2 = consts
    vol = cur[4]
    if coupling == ISO:
        de = -(cb * (pressure - cur[5]))
        if kT > 0.0:
            de = de + cn * group_normal(seed, stream, t, 1) / math.sqrt(vol)
        if not (abs(de) <= MAX_DLNV):
            return None
        return np.full(3, math.exp(de / 3.0))
    mu = np.ones(3)
    for g in groups(coupling, axis):
        pg = cur[6 + g[0]] if len(g) == 1 else 0.5 * (cur[6 + g[0]] + cur[6 + g[1]])
        de = -(cb3 * (pressure - pg))
        if kT > 0.0:
            de = de + (cn1 if len(g) == 1 else cn2) * group_normal(seed, stream, t, 2 + g[0]) / math.sqrt(vol)
        if not (abs(de) <= MAX_DLNL):
            return None
        mu[list(g)] = math.exp(de)
    return mu


def run(h, xyz, nsteps, dt, pressure=ATM, kT=0.0, gamma=0.0, tau_p=BAR_TAU_P, beta_T=BAR_BETA_T, baro_every=0, coupling=ANISO, axis=2, vel=None,
        mass=MASS_WATER, seed=0, stream=0, step0=0, sample_every=1, pos_ref=None, force_noise=None, forces_of=energy_forces_stress):
    """The contract's step on one box.  Returns a dict: pos, vel, forces, cell, ref, trace [nsteps // sample_every + 1, 15],
    status (steps completed, 0 / 1 / 2) and w [3, 3], the virial tensor at the end.  ``force_noise``: a numpy Generator; every
    evaluation is then perturbed as the module docstring says."""
    hk, hd, c1, c2, hm = md_ref.constants(dt, mass, kT, gamma)
    consts = barostat_constants(dt, kT, tau_p, beta_T, baro_every)
    h = np.array(h, dtype=np.float64)
    x = np.array(xyz, dtype=np.float64)
    n = len(x)
    v = np.zeros_like(x) if vel is None else np.array(vel, dtype=np.float64)
    ref = x.copy() if pos_ref is None else np.array(pos_ref, dtype=np.float64)

    def evaluate(h, x):
        e, f, w = forces_of(h, x)
        if force_noise is not None:
            d = force_noise.uniform(-F_ATOL, F_ATOL, size=f.shape)
            s = d.sum(axis=0)
            f, w = f + d, w - A_SIGMA / math.sqrt(3.0) * 0.5 * (s[:, None] + s[None, :])
        return e, f, w

    def row(e, f, w):
        vol = abs(np.linalg.det(h))
        kab = hm * (v.T @ v)
        p = (2.0 * kab + w) / vol
        k = hm * (v * v).sum()
        return np.array([e, k, ((x - ref) ** 2).sum() / n, np.abs(f).max(), vol, (2.0 * k + np.trace(w)) / (3.0 * vol)]
                        + [p[a, b] for a, b in PAIRS] + [np.linalg.norm(h[k]) for k in range(3)])

    trace = np.zeros((nsteps // sample_every + 1, TRACE_FIELDS))
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
            mu = decide(cur, kT, pressure, consts, coupling, axis, seed, stream, t)
            if mu is None or not cell_ok(h * mu[None, :]):
                code = 2
                break
            h, x, ref, v = h * mu[None, :], x * mu[None, :], ref * mu[None, :], v / mu[None, :]
            e, f, w = evaluate(h, x)
            cur = row(e, f, w)
            if steps % sample_every == 0:
                trace[steps // sample_every] = cur
    if code:
        trace[steps // sample_every + 1:] = cur
    return dict(pos=x, vel=v, forces=f, cell=h, ref=ref, trace=trace, status=np.array([steps, code], dtype=np.int32), w=np.array(w))


@functools.lru_cache(maxsize=None)
def reference(name, langevin, baro_every, coupling, axis, noisy=False):
    """The mirror's 40-step trajectory of a case in the bar's experiment, computed once per process and shared: read-only."""
    h, xyz = load_case(name)
    r = run(h, xyz, BAR_STEPS, BAR_DT, vel=md_ref.bar_velocities(name), stream=3, coupling=coupling, axis=axis,
            force_noise=np.random.default_rng(99) if noisy else None, **bar_kwargs(langevin, baro_every))
    for k in r:
        r[k].setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def point(name, noisy=False):
    """(E, F, W_ab) of a case's own positions, with or without the perturbation of the bars."""
    h, xyz = load_case(name)
    r = run(h, xyz, 0, BAR_DT, force_noise=np.random.default_rng(99) if noisy else None)
    return float(r["trace"][0, 0]), r["forces"], r["w"]


def at_a_grid_edge(name, axis, multiple, margin):
    """(h, xyz) of a case with an orthorhombic cell whose Cartesian axis ``axis`` alone is scaled until its width is ``multiple``
    a sigma (1 + 1e-9) (1 + margin): built as npt_ref.at_a_grid_edge builds its boxes, one axis at a time."""
    h, xyz = load_case(name)
    s = np.ones(3)
    s[axis] = multiple * A_SIGMA * npt_ref.GUARD * (1.0 + margin) / npt_ref.widths(h)[axis]
    return h * s[None, :], xyz * s[None, :]


#: the grid-edge runs of ic96 (orthorhombic), deterministic, the barostat every step, MW_FLEX_UNIAXIAL along the axis: (axis,
#: multiple, margin, pressure) -- axis 2 stretched by 2 % until its width is 0.3 % above 6 cutoffs and pressed together with 3000
#: atm; axis 0 compressed by 4 % until its width is 0.3 % below 3 and left to expand at 1 atm
EDGE_CASES = ((2, 6, 3e-3, 3000.0 * ATM), (0, 3, -3e-3, ATM))


@functools.lru_cache(maxsize=None)
def edge_reference(axis, multiple, margin, pressure):
    h, xyz = at_a_grid_edge("ic96", axis, multiple, margin)
    r = run(h, xyz, BAR_STEPS, BAR_DT, vel=md_ref.bar_velocities("ic96"), pressure=pressure, baro_every=1, coupling=UNIAXIAL, axis=axis)
    for k in r:
        r[k].setflags(write=False)
    return r


def free_lengths(nboxes, cb, applications, seed, coupling, axis=2, n=FREE_N, kT=FREE_KT, pressure=FREE_PRESSURE, gamma_dt=FREE_GAMMA_DT, side=FREE_SIDE):
    """(final lengths [nboxes, 3], the smallest length any box had, any refused) of the mirror's stage with the forces switched
    off and baro_every = 1, from a cube of ``side`` and equilibrium velocities (module docstring): per application the thermostat,
    P_aa = kT q_a / V, then per group de_G, mu_G = exp(de_G), L_a <- mu_G L_a, q_a <- q_a / mu_G^2."""
    rng = np.random.default_rng(seed)
    c1 = math.exp(-gamma_dt)
    s2 = 1.0 - c1 * c1                                  # c2^2 in units of kT / mass
    cb3 = cb / 3.0
    cn = {1: math.sqrt(2.0 * kT * cb3 / 1.0), 2: math.sqrt(2.0 * kT * cb3 / 2.0)}
    L = np.full((nboxes, 3), float(side))
    q = rng.chisquare(n, (nboxes, 3))                   # sum over the molecules of v_a^2 in units of kT / mass
    smallest, refused = float(side), False
    for _ in range(applications):
        q = s2 * rng.noncentral_chisquare(n, c1 * c1 * q / s2)
        vol = L.prod(axis=1)
        p = kT * q / vol[:, None]
        for g in groups(coupling, axis):
            pg = p[:, g[0]] if len(g) == 1 else 0.5 * (p[:, g[0]] + p[:, g[1]])
            de = -(cb3 * (pressure - pg)) + cn[len(g)] * rng.standard_normal(nboxes) / np.sqrt(vol)
            refused = refused or bool(np.any(~(np.abs(de) <= MAX_DLNL)))
            mu = np.exp(de)
            for a in g:
                L[:, a] *= mu
                q[:, a] /= mu * mu
        smallest = min(smallest, float(L.min()))
    return L, smallest, refused
