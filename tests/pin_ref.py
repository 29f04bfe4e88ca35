"""numpy mirror of the contract of include/mw_pin.h over tests/flex_ref.py: the step, the barostat stage and the rows of flex_ref
with the force of the bias 1/2 kappa (Q - a)^2 on one collective density mode added to every evaluation, the columns Q and U_b and
the block averages; and the bars tests/test_pin_ref.py (CPU, the preconditions) and tests/test_gpu_pin.py (the device) share.

The bias is written from the definition: s = x inv(h), theta = 2 pi s.n, rho = sum exp(i theta), Q = |rho| / sqrt(N), and the force
-kappa (Q - a) Re(conj(rho) i exp(i theta_j)) / (|rho| sqrt(N)) k with k = 2 pi inv(h) n, in complex arithmetic.  It shares no code
with the library and does not reproduce its rounding.  Energy, forces and virial of mW are flex_ref.energy_forces_stress; the virial
of the bias is zero (tests/test_pin_ref.py shows U_b unchanged by every scaling of the barostat at fixed s).

The biased cases.  For a golden box the triple is the one of largest S(n) among one of every pair +-n with |n_a| <= NMAX, from
sk_ref.sk_tables (pinning.choose_wavevector restated); SKEW_CASE also runs with the best triple that has three nonzero components,
one of them negative.  The anchor is 0.8 Q_0, and kappa is the one at which the largest component of F_b at the start equals the
median |component| of F_mW there: the bias is neither negligible nor dominant.

Bars (all measured with the mirror on the CPU, none chosen from a device result; tests/test_pin_ref.py measures every one again and
holds the constants to it), formed as flex_ref forms its own: ten times the spread of the mirror against itself with every force
evaluation (the total force) perturbed by seeded uniform noise of +-quench_ref.F_ATOL per component and the virial as flex_ref's
noisy mirror perturbs it.  The experiment: 40 steps of md_ref.BAR_DT over md_ref's BAR_CASES with their biases, deterministic and
Langevin, in BAR_RUNS = (uniaxial, baro_every 1), (aniso, baro_every 5), (uniaxial, baro_every 5), (aniso, baro_every 1) with
axis = 2, and the blocks of equil_steps = BLOCK_EQUIL, block_steps = BLOCK_STEPS.  SKEW_CASE's second triple and ic65_interstitial
are held to the bars and are not part of them.

The free ensemble: FREE_N = 20 molecules without forces in a fixed cube of flex_ref.FREE_SIDE, thermostatted, bias on.  The
stationary law is exact for any N: the positions are uniform reweighted by exp(-U_b / kT), so Q is |the sum of N independent uniform
unit phasors| / sqrt(N) reweighted by exp(-1/2 kappa (Q - a)^2 / kT).  `free_law` draws it directly; `free_q` is the mirror's step
with the mW forces switched off, vectorised over boxes, with numpy's generator.  FREE_NVEC has |n| = 28: k = 0.72 / bohr, the
phases diffuse by 0.1 rad^2 per step of FREE_DT and decorrelate within some 20 steps; FREE_STEPS = 400 steps from uniform positions
are 20 of those times.  The time-step bias is measured by halving dt (and doubling the steps).
"""
from __future__ import annotations

import functools
import math

import numpy as np

import flex_ref
import md_ref
import sk_ref
from flex_ref import ANISO, ISO, PAIRS, SEMI, UNIAXIAL           # noqa: F401 (the couplings, for the tests)
from md_ref import A_SIGMA, BAR_DT, BAR_STEPS, MASS_WATER
from npt_ref import ATM, BAR_BETA_T, BAR_TAU_P, bar_kwargs, cell_ok
from quench_ref import BAR_CASES, F_ATOL, load_case           # noqa: F401

TRACE_FIELDS = 17
BLOCK_FIELDS = 4
NMAX = 8
ANCHOR_FRACTION = 0.8
SKEW_CASE = "ic64_sheared"
#: (coupling, axis, baro_every) of the bar's experiment
BAR_RUNS = ((UNIAXIAL, 2, 1), (ANISO, 2, 5), (UNIAXIAL, 2, 5), (ANISO, 2, 1))
BLOCK_EQUIL, BLOCK_STEPS = 8, 8

#: the largest deviations after 40 steps between the biased mirror and the same with perturbed forces, over BAR_CASES, BAR_RUNS and
#: both modes, measured (module docstring)
POS_SPREAD_MEASURED = 5.20e-8
VEL_SPREAD_MEASURED = 3.96e-11
CELL_SPREAD_MEASURED = 2.64e-9
TRACE_SPREAD_MEASURED = (8.96e-10, 8.71e-10, 1.58e-8, 6.08e-10, 2.66e-6, 3.13e-13, 5.61e-13, 5.40e-13, 4.97e-13, 3.43e-13, 3.91e-13, 3.31e-13,
                         2.66e-9, 1.93e-9, 2.33e-9, 3.01e-9, 2.10e-10)
BLOCK_SPREAD_MEASURED = (2.75e-9, 3.14e-8, 2.42e-6, 4.25e-10)
POS_TOL = 10.0 * POS_SPREAD_MEASURED
VEL_TOL = 10.0 * VEL_SPREAD_MEASURED
CELL_TOL = 10.0 * CELL_SPREAD_MEASURED
TRACE_TOL = tuple(10.0 * s for s in TRACE_SPREAD_MEASURED)
BLOCK_TOL = tuple(10.0 * s for s in BLOCK_SPREAD_MEASURED)

#: the free ensemble (module docstring)
FREE_N = flex_ref.FREE_N
FREE_KT = flex_ref.FREE_KT
FREE_SIDE = flex_ref.FREE_SIDE
FREE_DT = flex_ref.FREE_DT
FREE_GAMMA_DT = flex_ref.FREE_GAMMA_DT
FREE_NVEC = (24, -12, 8)
FREE_KAPPA = 4.0 * FREE_KT
FREE_ANCHOR = 2.0
FREE_STEPS = 400
FREE_BOXES = 4096
FREE_DRAWS = 4_000_000
#: <Q>(dt) - <Q>(dt / 2) and var Q(dt) - var Q(dt / 2) of free_q, FREE_HALVING_BOXES boxes, seeds 5 and 6, measured; the bars take
#: twice the absolute value.  (With 16 times as many boxes the differences were -2.2e-3 and 7.1e-4, one standard error of theirs: the
#: time-step bias is below what these ensembles resolve, and the recorded figures are mostly their noise.)
FREE_HALVING_BOXES = 8192
FREE_HALVING_MEASURED = -8.05e-3
FREE_VAR_HALVING_MEASURED = -5.81e-3
FREE_BIAS = 2.0 * abs(FREE_HALVING_MEASURED)
FREE_VAR_BIAS = 2.0 * abs(FREE_VAR_HALVING_MEASURED)


# ---- the bias -------------------------------------------------------------------------------------------------------
def mode(h, xyz, nvec):
    """rho(n) = sum_j exp(2 pi i n.s_j) of one box and the phasors exp(i theta_j) [N]."""
    s = np.asarray(xyz, dtype=np.float64) @ np.linalg.inv(np.asarray(h, dtype=np.float64))
    e = np.exp(2j * math.pi * (s @ np.asarray(nvec, dtype=np.float64)))
    return e.sum(), e


def bias(h, xyz, nvec, kappa, anchor):
    """(Q, U_b, F_b [N, 3]) of one box."""
    n = len(xyz)
    rho, e = mode(h, xyz, nvec)
    r = abs(rho)
    q = r / math.sqrt(n)
    u = 0.5 * kappa * (q - anchor) ** 2
    if r == 0.0 or kappa == 0.0:
        return q, u, np.zeros((n, 3))
    k = 2.0 * math.pi * (np.linalg.inv(np.asarray(h, dtype=np.float64)) @ np.asarray(nvec, dtype=np.float64))
    dq = (np.conj(rho) * 1j * e).real / (r * math.sqrt(n))                # dQ / d theta_j
    return q, u, (-kappa * (q - anchor)) * dq[:, None] * k[None, :]


def half_space(nmax=NMAX, axis=None):
    r = np.arange(-nmax, nmax + 1)
    n = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    n = n[(n[:, 0] > 0) | ((n[:, 0] == 0) & ((n[:, 1] > 0) | ((n[:, 1] == 0) & (n[:, 2] > 0))))]
    return n if axis is None else n[n[:, axis] == 0]


def choose_wavevector(h, xyz, axis=None, nmax=NMAX, skew=False):
    """pinning.choose_wavevector restated over sk_ref; ``skew``: among the triples with three nonzero components, one negative."""
    n = half_space(nmax, axis)
    if skew:
        n = n[np.all(n != 0, axis=1) & np.any(n < 0, axis=1)]
    return n[int(np.argmax(sk_ref.sk_tables(h, xyz, n)[1]))].copy()


@functools.lru_cache(maxsize=None)
def bias_case(name, skew=False):
    """(nvec (3 ints), kappa, anchor, Q_0) of a golden box (module docstring)."""
    h, xyz = load_case(name)
    nvec = choose_wavevector(h, xyz, skew=skew)
    f_mw = flex_ref.energy_forces_stress(h, xyz)[1]
    q0 = bias(h, xyz, nvec, 0.0, 0.0)[0]
    anchor = ANCHOR_FRACTION * q0
    fb1 = bias(h, xyz, nvec, 1.0, anchor)[2]
    kappa = float(np.median(np.abs(f_mw)) / np.abs(fb1).max())
    return tuple(int(v) for v in nvec), kappa, float(anchor), float(q0)


# ---- the step -------------------------------------------------------------------------------------------------------
def nblocks(nsteps, equil_steps, block_steps):
    return (nsteps - equil_steps) // block_steps if block_steps > 0 and nsteps >= equil_steps else 0


def run(h, xyz, nvec, kappa, anchor, nsteps, dt, pressure=ATM, kT=0.0, gamma=0.0, tau_p=BAR_TAU_P, beta_T=BAR_BETA_T, baro_every=0, coupling=UNIAXIAL,
        axis=2, vel=None, mass=MASS_WATER, seed=0, stream=0, step0=0, sample_every=1, pos_ref=None, equil_steps=0, block_steps=0, force_noise=None):
    """The contract's step on one box.  Returns a dict: pos, vel, forces (total), cell, ref, trace [nsteps // sample_every + 1,
    17], blocks [nblocks, 4], status (steps completed, 0 / 1 / 2), fb (the force of the bias at the end)."""
    hk, hd, c1, c2, hm = md_ref.constants(dt, mass, kT, gamma)
    consts = flex_ref.barostat_constants(dt, kT, tau_p, beta_T, baro_every)
    h = np.array(h, dtype=np.float64)
    x = np.array(xyz, dtype=np.float64)
    n = len(x)
    v = np.zeros_like(x) if vel is None else np.array(vel, dtype=np.float64)
    ref = x.copy() if pos_ref is None else np.array(pos_ref, dtype=np.float64)

    def evaluate(h, x):
        e, f, w = flex_ref.energy_forces_stress(h, x)
        q, u, fb = bias(h, x, nvec, kappa, anchor) if kappa != 0.0 else (0.0, 0.0, np.zeros_like(x))
        f = f + fb
        if force_noise is not None:
            d = force_noise.uniform(-F_ATOL, F_ATOL, size=f.shape)
            s = d.sum(axis=0)
            f, w = f + d, w - A_SIGMA / math.sqrt(3.0) * 0.5 * (s[:, None] + s[None, :])
        return e, f, w, q, u, fb

    def row(e, f, w, q, u):
        vol = abs(np.linalg.det(h))
        kab = hm * (v.T @ v)
        p = (2.0 * kab + w) / vol
        k = hm * (v * v).sum()
        return np.array([e, k, ((x - ref) ** 2).sum() / n, np.abs(f).max(), vol, (2.0 * k + np.trace(w)) / (3.0 * vol)]
                        + [p[a, b] for a, b in PAIRS] + [np.linalg.norm(h[k]) for k in range(3)] + [q, u])

    trace = np.zeros((nsteps // sample_every + 1, TRACE_FIELDS))
    nbl = nblocks(nsteps, equil_steps, block_steps)
    blocks, acc = np.zeros((nbl, BLOCK_FIELDS)), np.zeros(BLOCK_FIELDS)

    def tally(s, cur):                                                 # the row after step s of the call
        nonlocal acc
        t = s - equil_steps
        if nbl == 0 or t < 0 or t // block_steps >= nbl:
            return
        acc = acc + np.array([cur[15], cur[15] * cur[15], cur[4], cur[0]])
        if t % block_steps == block_steps - 1:
            blocks[t // block_steps] = acc / block_steps
            acc = np.zeros(BLOCK_FIELDS)

    e, f, w, q, u, fb = evaluate(h, x)
    cur = row(e, f, w, q, u)
    trace[0] = cur
    steps, code = 0, 0
    for s in range(nsteps):
        t = step0 + s
        v = v + hk * f                                                 # 1
        if flex_ref._guard_fails(hd, v):                               # 2
            code = 1
            break
        x = x + hd * v
        if gamma > 0.0:                                                # 3
            v = c1 * v + c2 * md_ref.normals(seed, stream, t, n)
        if flex_ref._guard_fails(hd, v):                               # 4
            code = 1
            break
        x = x + hd * v
        e, f, w, q, u, fb = evaluate(h, x)                             # 5
        v = v + hk * f                                                 # 6
        steps = s + 1
        cur = row(e, f, w, q, u)
        if steps % sample_every == 0:
            trace[steps // sample_every] = cur
        if baro_every > 0 and (t + 1) % baro_every == 0:               # the barostat stage, flex_ref's
            mu = flex_ref.decide(cur, kT, pressure, consts, coupling, axis, seed, stream, t)
            if mu is None or not cell_ok(h * mu[None, :]):
                code = 2
                tally(s, cur)
                break
            h, x, ref, v = h * mu[None, :], x * mu[None, :], ref * mu[None, :], v / mu[None, :]
            e, f, w, q, u, fb = evaluate(h, x)
            cur = row(e, f, w, q, u)
            if steps % sample_every == 0:
                trace[steps // sample_every] = cur
        tally(s, cur)
    if code:
        trace[steps // sample_every + 1:] = cur
        for s in range(steps, nsteps):                                 # a frozen box contributes its last row
            tally(s, cur)
    return dict(pos=x, vel=v, forces=f, cell=h, ref=ref, trace=trace, blocks=blocks, status=np.array([steps, code], dtype=np.int32), fb=fb)


@functools.lru_cache(maxsize=None)
def reference(name, langevin, baro_every, coupling, axis, biased=True, noisy=False, skew=False):
    """The mirror's 40-step trajectory of a case in the bar's experiment, computed once per process and shared: read-only.
    ``biased`` False: the same run with kappa = 0."""
    h, xyz = load_case(name)
    nvec, kappa, anchor, _ = bias_case(name, skew)
    r = run(h, xyz, nvec, kappa if biased else 0.0, anchor, BAR_STEPS, BAR_DT, vel=md_ref.bar_velocities(name), stream=3, coupling=coupling, axis=axis,
            equil_steps=BLOCK_EQUIL, block_steps=BLOCK_STEPS, force_noise=np.random.default_rng(99) if noisy else None, **bar_kwargs(langevin, baro_every))
    for k in r:
        r[k].setflags(write=False)
    return r


# ---- the free ensemble ------------------------------------------------------------------------------------------------
def free_q_of(x, side=FREE_SIDE, nvec=FREE_NVEC):
    """(Q [nb], rho [nb], phasors [nb, N]) of boxes x [nb, N, 3] in the cube."""
    e = np.exp(2j * math.pi * ((x / side) @ np.asarray(nvec, dtype=np.float64)))
    rho = e.sum(axis=1)
    return np.abs(rho) / math.sqrt(x.shape[1]), rho, e


def free_start(nboxes, seed, n=FREE_N, side=FREE_SIDE, kT=FREE_KT, mass=MASS_WATER):
    """Uniform positions and equilibrium velocities [nboxes, n, 3]."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, side, (nboxes, n, 3)), rng.standard_normal((nboxes, n, 3)) * math.sqrt(kT / mass)


def free_q(nboxes, dt, steps, seed, n=FREE_N, kT=FREE_KT, kappa=FREE_KAPPA, anchor=FREE_ANCHOR, gamma=FREE_GAMMA_DT / FREE_DT, side=FREE_SIDE,
           nvec=FREE_NVEC, mass=MASS_WATER):
    """Q [nboxes] after ``steps`` BAOAB steps of the bias force alone from free_start, the noise from numpy's generator."""
    hk, hd, c1, c2, _ = md_ref.constants(dt, mass, kT, gamma)
    x, v = free_start(nboxes, seed, n, side, kT, mass)
    rng = np.random.default_rng(seed + 1000)
    k = 2.0 * math.pi * np.asarray(nvec, dtype=np.float64) / side

    def force(x):
        q, rho, e = free_q_of(x, side, nvec)
        dq = (np.conj(rho)[:, None] * 1j * e).real / (np.abs(rho)[:, None] * math.sqrt(n))
        return (-kappa * (q - anchor))[:, None, None] * dq[:, :, None] * k[None, None, :]

    f = force(x)
    for _ in range(steps):
        v = v + hk * f
        x = x + hd * v
        v = c1 * v + c2 * rng.standard_normal(v.shape)
        x = x + hd * v
        f = force(x)
        v = v + hk * f
    return free_q_of(x, side, nvec)[0]


@functools.lru_cache(maxsize=None)
def free_law(draws=FREE_DRAWS, seed=3, n=FREE_N, kT=FREE_KT, kappa=FREE_KAPPA, anchor=FREE_ANCHOR):
    """(<Q>, var Q, the standard error of each) of the exact law by self-normalised importance sampling from the unbiased one:
    ``draws`` sums of n uniform unit phasors, weights exp(-U_b / kT); the errors by the delta method."""
    rng = np.random.default_rng(seed)
    q = np.empty(draws)
    for a in range(0, draws, 250_000):
        m = min(250_000, draws - a)
        q[a:a + m] = np.abs(np.exp(2j * math.pi * rng.random((m, n))).sum(axis=1)) / math.sqrt(n)
    w = np.exp(-0.5 * kappa * (q - anchor) ** 2 / kT)
    w = w / w.sum()
    mean = float((w * q).sum())
    var = float((w * (q - mean) ** 2).sum())
    se_mean = math.sqrt(float((w * w * (q - mean) ** 2).sum()))
    se_var = math.sqrt(float((w * w * ((q - mean) ** 2 - var) ** 2).sum()))
    return mean, var, se_mean, se_var
