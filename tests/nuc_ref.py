"""numpy mirror of the contract of include/mw_nuc.h, and the inputs tests/test_nuc_ref.py (CPU, the preconditions) and
tests/test_gpu_nuc.py (the device) share.

The order parameter is boo_ref.boo_tables restricted to what the header uses (n_i, conn_i from s_ij > threshold); a molecule is
solid-like with conn_i >= min_conn; the bonds are the entries between two solid-like molecules that are not images of one
molecule; a union-find over them gives the clusters, labelled by the smallest molecule of each (1-based, 0 for a molecule that
is not solid-like); lambda is the largest size, a tie going to the smallest label.  The trajectory is flex_ref.run's, restated
with the evaluation and the stopping rule at the contract's steps: at entry and after every step e with (e + 1) % check_every
== 0, after the barostat application if there is one.  The mirror shares no code with the library and does not reproduce its
rounding: integers are compared exactly, which the preconditions below make legitimate, and the state is held to flex_ref's bars.

Preconditions.  Single points: no |d| within 1e-9 rc of rc and no s_ij within 1e-6 of the threshold (boo_ref's own bars).
Trajectories: the device's positions may differ from the mirror's by flex_ref.POS_TOL, so s_ij may differ by the spread
S_SPREAD_MEASURED (the largest change of an s_ij over the trajectory inputs when every coordinate of the mirror's positions is
moved by a seeded uniform +-POS_TOL; tests/test_nuc_ref.py measures it again), and a distance by 2 sqrt(3) POS_TOL; at every
evaluation of the mirror's trajectories the gap of every s_ij to the threshold is at least ten times that spread and the gap of
every distance to rc at least ten times that shift.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import boo_ref
import flex_ref
import md_ref
from boo_ref import ANG_TO_BOHR
from md_ref import A_SIGMA, BAR_DT, BAR_STEPS, LIM2, MASS_WATER
from npt_ref import ATM, BAR_BETA_T, BAR_TAU_P, bar_kwargs, cell_ok
from quench_ref import load_case

REACHED_HI, REACHED_LO = 3, 4
TRACE_FIELDS = 18
#: the defaults of mc_water_ls_mw_amd.nucleation (a choice of that module)
RC_ANG, THRESHOLD, MIN_CONN = 3.5, 0.5, 3

#: the largest |change of an s_ij| over TRAJ_RUNS' inputs under +-flex_ref.POS_TOL per coordinate, measured (module docstring)
S_SPREAD_MEASURED = 4.7e-7
S_GAP = 10.0 * S_SPREAD_MEASURED
D_GAP = 10.0 * 2.0 * math.sqrt(3.0) * flex_ref.POS_TOL


# -- the order parameter and the clusters -------------------------------------------------------------------------------------
def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def clusters_union_find(solid, i, j):
    """label [N] int32: 0, or the 1-based index of the smallest molecule of the cluster, from the bonds (i[k], j[k]) between
    solid-like molecules (i == j, an image of the molecule itself, is no bond)."""
    n = len(solid)
    parent = np.arange(n)
    for a, b in zip(i, j):
        if a == b or not (solid[a] and solid[b]):
            continue
        ra, rb = _find(parent, a), _find(parent, b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    label = np.zeros(n, dtype=np.int32)
    for a in range(n):
        if solid[a]:
            label[a] = _find(parent, a) + 1
    return label


def clusters_flood_fill(solid, i, j):
    """The same labels by a brute-force flood fill over an adjacency matrix, sharing nothing with the union-find."""
    n = len(solid)
    adj = np.zeros((n, n), dtype=bool)
    ok = solid[i] & solid[j] & (i != j)
    adj[i[ok], j[ok]] = True
    adj |= adj.T
    label = np.zeros(n, dtype=np.int32)
    for a in range(n):
        if not solid[a] or label[a]:
            continue
        seen = np.zeros(n, dtype=bool)
        seen[a] = True
        front = seen.copy()
        while front.any():
            front = adj[front].any(axis=0) & ~seen
            seen |= front
        label[seen] = a + 1                                  # a is the smallest: every smaller member would have claimed it
    return label


def op_of(label):
    """(solid-like, clusters, lambda, the label of the largest cluster): a tie goes to the smallest label."""
    lab = label[label > 0]
    if len(lab) == 0:
        return np.zeros(4, dtype=np.int32)
    roots, sizes = np.unique(lab, return_counts=True)
    k = int(np.argmax(sizes))                                # (the first of equals: roots ascend)
    return np.array([len(lab), len(roots), sizes[k], roots[k]], dtype=np.int32)


def order(h, xyz, rc, threshold, min_conn, grid=None):
    """dict: nn [N, 2] (n_i, conn_i), label [N], op [4], s [E] (NaN where a side is degenerate), r [E]."""
    t = boo_ref.boo_tables(h, xyz, rc, threshold, grid=grid)
    solid = t["conn"] >= min_conn
    label = clusters_union_find(solid, t["i"], t["j"])
    return dict(nn=np.stack([t["n"], t["conn"]], axis=1).astype(np.int32), label=label, op=op_of(label), s=t["s"], r=t["r"], i=t["i"], j=t["j"],
                solid=solid)


def gaps(o, rc, threshold, h=None, xyz=None, grid=None):
    """(nearest | |d| - rc |, nearest |s_ij - threshold|) of an `order` dict; with the box given, the distances beyond rc count
    too (boo_ref.nearest_to_cutoff)."""
    s = o["s"]
    gs = float(np.nanmin(np.abs(s - threshold))) if np.any(np.isfinite(s)) else np.inf
    gd = boo_ref.nearest_to_cutoff(h, xyz, rc, grid) if h is not None else (float(np.abs(o["r"] - rc).min()) if len(o["r"]) else np.inf)
    return gd, gs


def s_spread(h, xyz, rc, tol, seed):
    """The largest |change of an s_ij| when every coordinate moves by a seeded uniform +-tol (entries matched by (i, j, order);
    inf if the entries themselves change)."""
    a = boo_ref.boo_tables(h, xyz, rc, 0.0)
    rng = np.random.default_rng(seed)
    b = boo_ref.boo_tables(h, xyz + rng.uniform(-tol, tol, size=np.shape(xyz)), rc, 0.0)
    if len(a["i"]) != len(b["i"]) or not (np.array_equal(a["i"], b["i"]) and np.array_equal(a["j"], b["j"])):
        return np.inf
    d = np.abs(a["s"] - b["s"])
    return float(np.nanmax(d)) if np.any(np.isfinite(d)) else 0.0


# -- the trajectory -----------------------------------------------------------------------------------------------------------
def run(h, xyz, nsteps, dt, rc, threshold, min_conn, check_every=1, lam_lo=-1, lam_hi=None, pressure=ATM, kT=0.0, gamma=0.0, tau_p=BAR_TAU_P,
        beta_T=BAR_BETA_T, baro_every=0, coupling=flex_ref.ANISO, axis=2, vel=None, mass=MASS_WATER, seed=0, stream=0, step0=0, sample_every=1,
        pos_ref=None):
    """The contract's step on one box: flex_ref.run with the evaluation of the order parameter and the stopping rule.  Returns a
    dict: pos, vel, forces, cell, ref, trace [nsteps // sample_every + 1, 18], status (steps completed, 0 .. 4), nn, label, op of
    the final state, and evals: [(steps completed, op, gap to rc, gap to the threshold)] of every evaluation."""
    assert nsteps % check_every == 0
    hk, hd, c1, c2, hm = md_ref.constants(dt, mass, kT, gamma)
    consts = flex_ref.barostat_constants(dt, kT, tau_p, beta_T, baro_every)
    h = np.array(h, dtype=np.float64)
    x = np.array(xyz, dtype=np.float64)
    n = len(x)
    lam_hi = n + 1 if lam_hi is None else lam_hi
    v = np.zeros_like(x) if vel is None else np.array(vel, dtype=np.float64)
    ref = x.copy() if pos_ref is None else np.array(pos_ref, dtype=np.float64)
    evals = []

    def row(e, f, w):
        vol = abs(np.linalg.det(h))
        kab = hm * (v.T @ v)
        p = (2.0 * kab + w) / vol
        k = hm * (v * v).sum()
        return np.array([e, k, ((x - ref) ** 2).sum() / n, np.abs(f).max(), vol, (2.0 * k + np.trace(w)) / (3.0 * vol)]
                        + [p[a, b] for a, b in flex_ref.PAIRS] + [np.linalg.norm(h[k]) for k in range(3)] + [0.0, 0.0, 0.0])

    def evaluate_order(steps):
        o = order(h, x, rc, threshold, min_conn)
        evals.append((steps, o["op"].copy()) + gaps(o, rc, threshold, h, x))
        return o

    def verdict(o):
        lam = int(o["op"][2])
        return REACHED_HI if lam >= lam_hi else REACHED_LO if lam <= lam_lo else 0

    trace = np.zeros((nsteps // sample_every + 1, TRACE_FIELDS))
    e, f, w = flex_ref.energy_forces_stress(h, x)
    cur = row(e, f, w)
    o = evaluate_order(0)
    opcols = np.array([o["op"][2], o["op"][0], o["op"][1]], dtype=np.float64)
    cur[15:] = opcols
    trace[0] = cur
    steps, code = 0, verdict(o)
    for s in range(nsteps if code == 0 else 0):
        t = step0 + s
        v1 = v + hk * f                                                # 1
        if flex_ref._guard_fails(hd, v1):                              # 2
            v, code = v1, 1
            break
        v = v1
        x = x + hd * v
        if gamma > 0.0:                                                # 3
            v = c1 * v + c2 * md_ref.normals(seed, stream, t, n)
        if flex_ref._guard_fails(hd, v):                               # 4
            code = 1
            break
        x = x + hd * v
        e, f, w = flex_ref.energy_forces_stress(h, x)                  # 5
        v = v + hk * f                                                 # 6
        steps = s + 1
        cur = row(e, f, w)
        cur[15:] = opcols
        if steps % sample_every == 0:
            trace[steps // sample_every] = cur
        if baro_every > 0 and (t + 1) % baro_every == 0:               # the barostat stage
            mu = flex_ref.decide(cur, kT, pressure, consts, coupling, axis, seed, stream, t)
            if mu is None or not cell_ok(h * mu[None, :]):
                code = 2
                break
            h, x, ref, v = h * mu[None, :], x * mu[None, :], ref * mu[None, :], v / mu[None, :]
            e, f, w = flex_ref.energy_forces_stress(h, x)
            cur = row(e, f, w)
            cur[15:] = opcols
            if steps % sample_every == 0:
                trace[steps // sample_every] = cur
        if steps % check_every == 0:
            o = evaluate_order(steps)
            opcols = np.array([o["op"][2], o["op"][0], o["op"][1]], dtype=np.float64)
            cur[15:] = opcols
            if steps % sample_every == 0:
                trace[steps // sample_every] = cur
            code = verdict(o)
            if code:
                break
    if code:
        trace[steps // sample_every + 1:] = cur
    if code in (1, 2):                                                 # a guard froze the box: its final state is evaluated for the outputs alone
        o = order(h, x, rc, threshold, min_conn)
    return dict(pos=x, vel=v, forces=f, cell=h, ref=ref, trace=trace, status=np.array([steps, code], dtype=np.int32), nn=o["nn"], label=o["label"],
                op=o["op"], evals=evals)


# -- the inputs of the GPU tests ----------------------------------------------------------------------------------------------
#: the trajectory runs of tests/test_gpu_nuc.py: (case, langevin); 40 steps of 5 fs from md_ref.bar_velocities, the barostat
#: every 5 steps in coupling ANISO, a check every 5 steps: every check follows a barostat application
TRAJ_RUNS = (("ic65_interstitial", False), ("ic65_interstitial", True), ("ic96", False), ("ic96", True))
TRAJ_CHECK = 5
TRAJ_BARO = 5
#: the order parameter of the trajectory runs: (rc in Angstrom, threshold, min_conn) per case, chosen for the gaps the module
#: docstring asks for (tests/test_nuc_ref.py holds them)
TRAJ_ORDER = {"ic65_interstitial": (3.5, 0.5, 3), "ic96": (3.5, 0.5, 3)}


def traj_kwargs(name, langevin):
    rc_ang, thr, mc = TRAJ_ORDER[name]
    kw = dict(bar_kwargs(langevin, TRAJ_BARO))
    return rc_ang, thr, mc, kw


@functools.lru_cache(maxsize=None)
def reference(name, langevin, lam_lo=-1, lam_hi=None):
    """The mirror's trajectory of a TRAJ_RUNS entry, computed once per process and shared: read-only."""
    h, xyz = load_case(name)
    rc_ang, thr, mc, kw = traj_kwargs(name, langevin)
    r = run(h, xyz, BAR_STEPS, BAR_DT, rc_ang * ANG_TO_BOHR, thr, mc, check_every=TRAJ_CHECK, lam_lo=lam_lo, lam_hi=lam_hi,
            vel=md_ref.bar_velocities(name), stream=3, coupling=flex_ref.ANISO, axis=2, **kw)
    for k, a in r.items():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


def bounds_from(ref, n):
    """(lam_lo, lam_hi) that stop an unbounded mirror run `ref` at the first evaluation whose lambda differs from the entry's --
    or at entry when none does."""
    lam = [int(op[2]) for _, op, _, _ in ref["evals"]]
    for v in lam[1:]:
        if v < lam[0]:
            return v, n + 1
        if v > lam[0]:
            return -1, v
    return -1, lam[0]


def gas_case(n, one_cell=False):
    """(h, xyz, rc in Angstrom, threshold, min_conn) of a gas box of boo_ref with a cutoff inside the supported range: boo_ref's
    own where that is below a sigma, and 0.98 a sigma (dozens of entries per molecule, far above MW_NUC_LIST) for `one_cell`."""
    h, xyz = boo_ref.gas_box(n, 1000 + n)
    rc_ang = 0.98 * A_SIGMA / ANG_TO_BOHR if one_cell else min(boo_ref.gas_rc_ang(n), 0.98 * A_SIGMA / ANG_TO_BOHR)
    return h, xyz, rc_ang, 0.3, 1


#: the thermalised ic96 of the single-point test: sigma (Angstrom) and seed, searched for at least three clusters and a molecule
#: that is not solid-like, with the single-point gaps
SHAKEN = dict(sigma_ang=0.35, seed=4)
#: the seeded box: the (4, 3, 3) Ih box shaken with sigma = 0.7 Angstrom (seed 12) as the disordered host, an Ic seed of 6 Angstrom
SEEDED = dict(reps=(4, 3, 3), sigma_ang=0.7, seed=12, kind="ic", radius_ang=6.0)


def shaken_ic96():
    from mc_water_ls_mw_amd import lattice as lat
    h, xyz = load_case("ic96")
    return h, lat.thermalise(xyz, SHAKEN["sigma_ang"], SHAKEN["seed"])


def seeded():
    """(h, xyz, nseed) of the seeded box."""
    from mc_water_ls_mw_amd import lattice as lat
    from mc_water_ls_mw_amd.nucleation import seeded_box
    h, xyz = lat.ice_box("ih", SEEDED["reps"], SEEDED["sigma_ang"], seed=SEEDED["seed"])
    return seeded_box(h, xyz, SEEDED["kind"], SEEDED["radius_ang"])


def single_cases():
    """[(label, h, xyz, rc in Angstrom, threshold, min_conn, grid)]: every input of the single-point test; grid says how the
    reference finds the neighbours (boo_ref.entries)."""
    from cluster_ref import defect_box
    out = []
    for name in ("ic65_interstitial", "ih1536_t012"):
        h, xyz = load_case(name)
        out.append((name, h, xyz, RC_ANG, THRESHOLD, MIN_CONN, len(xyz) > 256))
    h, xyz = shaken_ic96()
    out.append(("ic96 shaken", h, xyz, RC_ANG, THRESHOLD, MIN_CONN, False))
    h, xyz, rc_ang, thr, mc = gas_case(65, one_cell=True)
    out.append(("gas N = 65, rc = 0.98 a sigma", h, xyz, rc_ang, thr, mc, False))
    for n in (65, 255, 256, 257):
        h, xyz, rc_ang, thr, mc = gas_case(n)
        out.append((f"gas N = {n}", h, xyz, rc_ang, thr, mc, False))
    h, xyz = defect_box()
    out.append(("defect box", h, xyz, RC_ANG, THRESHOLD, MIN_CONN, False))
    h, xyz, _ = seeded()
    out.append(("seeded box", h, xyz, RC_ANG, THRESHOLD, MIN_CONN, False))
    return out


@functools.lru_cache(maxsize=None)
def single_reference(k):
    """`order` of case k of `single_cases`, computed once per process."""
    _, h, xyz, rc_ang, thr, mc, grid = single_cases()[k]
    return order(h, xyz, rc_ang * ANG_TO_BOHR, thr, mc, grid=grid)


#: the batch of the stopping test: five boxes of 96 molecules whose lambda moves both ways within 40 steps of Langevin dynamics at
#: md_ref.BAR_KT -- three shaken ic96 boxes at rest, which order again, and two thermal ic96 boxes with velocities of six times
#: that temperature, which disorder -- (sigma in Angstrom or None, seed, velocity scale)
STOP_BOXES = ((0.35, 4, 0.0), (0.35, 5, 0.0), (0.3, 8, 0.0), (None, 31, math.sqrt(6.0)), (None, 32, math.sqrt(6.0)))
STOP_STREAMS = (11, 3, 2 ** 40, 5, 0)


def stop_batch():
    """(cells [5, 3, 3], positions [5, 96, 3], velocities [5, 96, 3]) of the stopping test."""
    from mc_water_ls_mw_amd import lattice as lat
    h, xyz = load_case("ic96")
    xs, vs = [], []
    for sigma, seed, scale in STOP_BOXES:
        xs.append(np.array(xyz) if sigma is None else lat.thermalise(xyz, sigma, seed))
        vs.append(scale * md_ref.maxwell_boltzmann(1, len(xyz), md_ref.BAR_KT, seed=seed)[0])
    return np.array([h] * len(xs)), np.array(xs), np.array(vs)


def first_records(lam):
    """(k_hi, k_lo): the first evaluation k >= 1 whose lambda exceeds every earlier one, and the first that is below every earlier
    one (None where there is none)."""
    k_hi = next((k for k in range(1, len(lam)) if lam[k] > max(lam[:k])), None)
    k_lo = next((k for k in range(1, len(lam)) if lam[k] < min(lam[:k])), None)
    return k_hi, k_lo
