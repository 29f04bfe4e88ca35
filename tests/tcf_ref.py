"""A numpy mirror of include/mw_tcf.h, written from the header and not from the kernels, the extended-precision reference the
device results are held against, the a-priori rounding bound (the *bar*) of every output value, and the inputs of the GPU
tests (tests/test_gpu_tcf.py), which tests/test_tcf_ref.py checks on the CPU.

``evaluate(..., dtype=np.float64)`` is the mirror in numpy's own order of summation; ``evaluate(..., dtype=np.longdouble)`` is
the reference (a 64-bit mantissa is asserted; where the platform has none the float64 terms are added with math.fsum) and
also returns the bars.

The bar.  u = 2^-53.  For box b and lag l let n = n_l be the number of terms (origins x molecules).  Every output is
(sum of n terms) / n, so its error against exact arithmetic on the same inputs is bounded, to first order in u, by

    [ (n + 4) u sum|term|  +  sum (error of each term) ] / n  +  u |value|

-- (n - 1) u sum|term| is the bound of a sum of n numbers in ANY fixed order (so it covers the tiles' partial sums added in
tile order as well as numpy's pairwise order), the "+ 4" swallows the second-order part for n < 10^8, and the last u is the
division.  The terms' own errors:

  d2 = fma(Dx, Dx, fma(Dy, Dy, Dz Dz)), D = y' - y: each component of D carries one rounding (relative u), its square two
    more, the three-term sum two more: at most 6 u d2, with or without fma.  Under REMOVE_COM each y = x - c carries the
    error of the centre, a sum of N numbers of size <= X = max|x| of the box divided by N, plus the rounding of the
    difference: e_y = (N + 4) u X per component.  D then carries 2 e_y per component, and d2 moves by at most
    2 |D|_1 (2 e_y) + 3 (2 e_y)^2.  Together err(d2) = 6 u d2 + 4 e_y |D|_1 + 12 e_y^2.
  d2^2: relative 2 x 6 u + u = 13 u, plus 2 d2 a + a^2 for the absolute part a = 4 e_y |D|_1 + 12 e_y^2.
  v . v': three products and two sums: 4 u sum_c |v_c v'_c|, plus e_v (|v|_1 + |v'|_1) + 3 e_v^2 under REMOVE_COM with
    e_v = (N + 4) u max|v|.
  sinc(x), x = q sqrt(d2): sqrt halves the relative error of d2 and adds u, the product adds u: |dx| <= 5 u x (6 u x is
    used); |sinc'| < 1/2, so the argument's error moves the term by at most 3 u x; the device library's sin is taken as good
    to 2 ulp (4 u relative) and the division adds u, and |sinc| <= 1: (3 x + 6) u per term -- "q r plus a few ulp".  Under
    REMOVE_COM |D|_2 moves by at most 4 e_y, x by q 4 e_y, the term by 2 q e_y.

Nothing here is tuned to any device output.  The histograms are integers and must match exactly, which they can only be asked
to do where no d2 lies within a relative 10^-9 of an edge (fma against separate rounding moves d2 by a few u only):
the ``margin`` entry measures that on the reference, and the inputs below are chosen, with fixed seeds, to satisfy it.
"""
import math
from collections import namedtuple
from functools import lru_cache

import numpy as np

U = 2.0 ** -53
WRONG = ("origin", "lag", "every", "com", "molecule", "frame")

Case = namedtuple("Case", "name nframes nboxes nwater nlags every nq nedges hist_lags remove_com seed drift")


def n_origins(nframes, lag, every):
    return (nframes - 1 - lag) // every + 1


def _sinc(x):
    safe = np.where(x == 0, 1, x)
    return np.where(x == 0, 1, np.sin(safe) / safe)


def evaluate(frames, vel, nlags, every, q=(), edges2=(), hist_lags=(), remove_com=False, dtype=np.float64, wrong=None):
    """{msd, mqd [B, nlags], vacf [B, nlags] or None, fs [B, nlags, nq], hist [B, nh, nedges + 1] int64, margin} and, with
    dtype=np.longdouble, the bars {bar_msd, bar_mqd, bar_vacf, bar_fs}.  ``wrong``: one of WRONG, a deliberately broken mirror."""
    frames = np.asarray(frames, dtype=np.float64)
    T, B, N, _ = frames.shape
    ext = dtype is np.longdouble
    if ext:
        assert np.finfo(np.longdouble).nmant >= 63, "no extended precision on this platform"
    x = frames.astype(dtype)
    v = None if vel is None else np.asarray(vel, dtype=np.float64).astype(dtype)
    if wrong == "molecule":
        x, v = x[:, :, :-1], None if v is None else v[:, :, :-1]
    if wrong == "frame":
        x, v = x[:-1], None if v is None else v[:-1]
    if wrong == "every":
        every = 1
    Tn, Nn = x.shape[0], x.shape[2]
    if remove_com and wrong != "com":
        x = x - x.sum(axis=2, keepdims=True) / dtype(Nn)
        if v is not None:
            v = v - v.sum(axis=2, keepdims=True) / dtype(Nn)
    q = np.asarray(q, dtype=np.float64)
    e2 = np.asarray(edges2, dtype=np.float64)
    hist_lags = [int(h) for h in hist_lags]
    out = dict(msd=np.full((B, nlags), np.nan), mqd=np.full((B, nlags), np.nan), vacf=None if v is None else np.full((B, nlags), np.nan),
               fs=np.full((B, nlags, len(q)), np.nan), hist=np.zeros((B, len(hist_lags), len(e2) + 1), dtype=np.int64), margin=np.inf)
    if ext:
        out.update(bar_msd=np.zeros((B, nlags)), bar_mqd=np.zeros((B, nlags)), bar_vacf=np.zeros((B, nlags)), bar_fs=np.zeros((B, nlags, len(q))))
        ey = ((N + 4) * U * np.abs(frames).max(axis=(0, 2, 3)) if remove_com else np.zeros(B))[None, :, None]          # [1, B, 1]
        ev = ((N + 4) * U * np.abs(np.asarray(vel)).max(axis=(0, 2, 3)) if remove_com and vel is not None else np.zeros(B))[None, :, None]
    total = lambda a: a.sum(axis=(0, 2))                                   # noqa: E731  (over origins and molecules: per box)
    for lag in range(nlags):
        use = lag
        if wrong == "lag":
            use = lag + 1 if lag + 1 <= Tn - 1 else lag - 1
        o = np.arange(0, Tn - use, every) if 0 <= use <= Tn - 1 else np.zeros(0, dtype=int)
        if wrong == "origin":
            o = o[:-1]
        n = len(o) * Nn
        if n == 0:
            continue                                                       # (stays NaN: a broken mirror without a term misses any bar)
        d = x[o + use] - x[o]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        msd, mqd = total(d2) / dtype(n), total(d2 * d2) / dtype(n)
        out["msd"][:, lag], out["mqd"][:, lag] = msd, mqd
        r = np.sqrt(d2)
        sincs = [_sinc(dtype(qa) * r) for qa in q]
        for a, s in enumerate(sincs):
            out["fs"][:, lag, a] = total(s) / dtype(n)
        if v is not None:
            dots = (v[o] * v[o + use]).sum(axis=-1)
            out["vacf"][:, lag] = total(dots) / dtype(n)
        if lag in hist_lags and len(e2):
            for b in range(B):
                flat = d2[:, b].ravel()
                slot = np.searchsorted(e2.astype(dtype), flat, side="right")
                for h, hl in enumerate(hist_lags):
                    if hl == lag:
                        out["hist"][b, h] = np.bincount(slot, minlength=len(e2) + 1)
                out["margin"] = min(out["margin"], float(np.min(np.abs(flat[:, None] - e2[None, :]) / np.maximum(e2[None, :], 1e-300))))
        if ext and wrong is None:
            f = lambda a: np.asarray(a, dtype=np.float64)                  # noqa: E731
            d2f, abs1 = f(d2), f(np.abs(d).sum(axis=-1))
            a_abs = 4.0 * ey * abs1 + 12.0 * ey * ey
            out["bar_msd"][:, lag] = ((n + 4) * U * total(d2f) + total(6.0 * U * d2f + a_abs)) / n + U * np.abs(f(msd))
            out["bar_mqd"][:, lag] = ((n + 4) * U * total(d2f * d2f) + total(13.0 * U * d2f * d2f + 2.0 * d2f * a_abs + a_abs * a_abs)) / n + U * np.abs(f(mqd))
            for a, s in enumerate(sincs):
                xq = q[a] * np.sqrt(d2f)
                out["bar_fs"][:, lag, a] = ((n + 4) * U * total(np.abs(f(s))) + total((3.0 * xq + 6.0) * U + 2.0 * q[a] * ey)) / n + U * np.abs(out["fs"][:, lag, a])
            if v is not None:
                av = f((np.abs(v[o]) * np.abs(v[o + use])).sum(axis=-1))
                l1 = f(np.abs(v[o]).sum(axis=-1) + np.abs(v[o + use]).sum(axis=-1))
                out["bar_vacf"][:, lag] = ((n + 4) * U * total(av) + total(4.0 * U * av + ev * l1 + 3.0 * ev * ev)) / n + U * np.abs(out["vacf"][:, lag])
    return out


def evaluate_fsum(frames, vel, nlags, every, q=(), remove_com=False):
    """The reference where long double is no wider than double: float64 terms, added exactly (math.fsum).  Without the bars'
    inputs in extended precision it serves the comparison only."""
    ref = evaluate(frames, vel, nlags, every, q, remove_com=remove_com)
    x = np.asarray(frames, dtype=np.float64)
    if remove_com:
        x = x - x.mean(axis=2, keepdims=True)
    T, B, N, _ = x.shape
    for lag in range(nlags):
        o = np.arange(0, T - lag, every)
        d = x[o + lag] - x[o]
        d2 = (d * d).sum(axis=-1)
        for b in range(B):
            ref["msd"][b, lag] = math.fsum(d2[:, b].ravel()) / (len(o) * N)
            ref["mqd"][b, lag] = math.fsum((d2[:, b] ** 2).ravel()) / (len(o) * N)
    return ref


# ---- the inputs of the GPU tests -----------------------------------------------------------------------------------------------
def cases(plan):
    """The cases of tests/test_gpu_tcf.py for the plan's tile, lag block and frame window (timecorr.tcf_plan): the smallest
    shapes at which each boundary of the plan is crossed."""
    tile, lb, win = plan["tile"], plan["lag_block"], plan["frame_window"]
    out, seed = [], [100]

    def add(name, nframes, nboxes, nwater, nlags=None, every=1, nq=4, nedges=9, hist_lags=None, remove_com=False, drift=1.0):
        nlags = nframes if nlags is None else nlags
        hl = tuple(sorted({0, nlags // 2, nlags - 1})) if hist_lags is None else tuple(hist_lags)
        seed[0] += 1
        out.append(Case(name, nframes, nboxes, nwater, nlags, every, nq, nedges, hl, remove_com, seed[0], drift))

    for k, (label, n) in enumerate((("1", 1), ("tile-1", tile - 1), ("tile", tile), ("tile+1", tile + 1), ("2tile+3", 2 * tile + 3))):
        add("nwater_" + label, 12, 1, n, remove_com=bool(k % 2), nq=(0, 4, 5, 16, 1)[k])
    add("nwater_200", 40, 5, 200, nlags=20, every=2, remove_com=True)
    for label, nl in (("1", 1), ("2", 2), ("block", lb), ("block+1", lb + 1), ("all", lb + 12)):
        add("nlags_" + label, lb + 12, 1, 3, nlags=nl, nq=2, remove_com=nl == lb + 1)
    for label, nf in (("1", 1), ("2", 2), ("window", win), ("window+1", win + 1), ("300", 300)):
        add("nframes_" + label, nf, 2 if nf == 300 else 1, 3, nq=3 if nf < 300 else 1, remove_com=nf == win)
    add("every3", 12, 5, tile + 1, every=3, remove_com=True)
    add("every3long", 101, 1, 2, every=3, nq=16)
    add("every40", lb + 12, 1, 3, every=40, nq=1)                           # chunks of origins that hold no origin
    add("single_origin", 12, 2, 5, every=12)
    add("single_origin_far", 12, 1, 5, every=1 << 30, remove_com=True)
    add("no_q", 12, 2, 5, nq=0)
    add("no_edges", 12, 2, 5, nedges=0, hist_lags=())
    add("edges1025", 12, 1, 5, nedges=1025)
    add("farm600", 16, 600, 8, nq=16, remove_com=True)
    return out


@lru_cache(maxsize=None)
def make_input(case):
    """(frames [T, B, N, 3], vel [T, B, N, 3], q [nq], edges [nedges] in bohr): random walks with a drift of their own per box,
    velocities that forget exponentially, all from the case's seed."""
    rng = np.random.default_rng(case.seed)
    T, B, N = case.nframes, case.nboxes, case.nwater
    steps = rng.normal(0.0, 0.3, (T, B, N, 3))
    steps[0] = 0.0
    drift = case.drift * rng.normal(0.0, 0.2, (1, B, 1, 3))
    frames = rng.uniform(0.0, 30.0, (1, B, N, 3)) + np.cumsum(steps, axis=0) + drift * np.arange(T)[:, None, None, None]
    vel = np.empty((T, B, N, 3))
    vel[0] = rng.normal(0.0, 1e-3, (B, N, 3))
    for t in range(1, T):
        vel[t] = 0.9 * vel[t - 1] + rng.normal(0.0, 4e-4, (B, N, 3))
    vel += case.drift * rng.normal(0.0, 1e-3, (1, B, 1, 3))
    q = np.linspace(0.4, 3.4, case.nq) if case.nq > 1 else np.full(case.nq, 1.7)
    edges = np.linspace(0.05, 0.6 * math.sqrt(T) + 0.4 * case.drift * T * (0 if case.remove_com else 1) + 0.5, case.nedges) if case.nedges else np.zeros(0)
    for a in (frames, vel, q, edges):
        a.setflags(write=False)
    return np.ascontiguousarray(frames), np.ascontiguousarray(vel), q, edges


@lru_cache(maxsize=None)
def reference(case):
    """The long-double reference and the bars of a case, computed once and shared."""
    frames, vel, q, edges = make_input(case)
    ref = evaluate(frames, vel, case.nlags, case.every, q, edges * edges, case.hist_lags, case.remove_com, dtype=np.longdouble)
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref


def worst(got, ref):
    """{output: (largest |got - ref|, its bar, the largest ratio of a difference to its bar)} over the floating outputs."""
    rows = {}
    for name in ("msd", "mqd", "vacf", "fs"):
        if got.get(name) is None or ref.get(name) is None or ref[name].size == 0:
            continue
        diff = np.abs(np.asarray(got[name], dtype=np.float64) - ref[name])
        bar = ref["bar_" + name]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(np.isnan(diff), np.inf, np.where(diff == 0.0, 0.0, diff / bar))   # (lag 0: msd = 0 exactly and its bar is 0)
        k = np.unravel_index(np.argmax(ratio), ratio.shape)
        rows[name] = (float(diff[k]), float(bar[k]), float(ratio[k]))
    return rows
