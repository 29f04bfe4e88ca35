"""A numpy mirror of include/mw_coll.h, written from the header and not from the kernels, the extended-precision reference the
device results are held against, the a-priori bars of the floating outputs, and the inputs of the GPU tests
(tests/test_gpu_coll.py), which tests/test_coll_ref.py checks on the CPU.

``evaluate(..., dtype=np.float64)`` is the mirror in numpy's own rounding and order of summation (per-axis phasor tables and
complex products for the modes, cofactor rows times 1 / det for the pair pass); ``evaluate(..., dtype=np.longdouble)`` is the
reference (a 64-bit mantissa is asserted; the modes by cos and sin of 2 pi n . s directly, the inverse cell refined by Newton
steps) and also returns the bars and the margins.

Bars.  u = 2^-53.
  rho: |rho - rho_exact| <= delta(n) = sk_ref.delta(nvec, nwater, s_max), s_max the largest |H^-1 r| of the box over all frames
    (the positions are unwrapped): derived in tests/sk_ref.py from the rounding of s carried into the phase, three sincospi
    results, two complex products and a sequential sum.
  fkt: F = sum_o A_o conj(B_o) / (o N) with A, B modes that each carry an error of modulus <= delta.  Per origin the product
    moves by at most delta (|A| + |B|) + delta^2.  The sum bound of tests/tcf_ref.py's docstring adds (o + 4) u sum|terms|,
    with the terms all four real products of an origin, (|A_re| + |A_im|) (|B_re| + |B_im|) -- it is four to eight orders
    below the first part at these shapes.  Both are divided by o N, and u |F| is the division:
        bar(F) = [ sum_o (delta (|A_o| + |B_o|) + delta^2) + (o + 4) u sum_o (|A_re| + |A_im|) (|B_re| + |B_im|) ] / (o N) + u |F|
    for the modulus of the complex difference.  Nothing here is tuned to any device output.

The integer outputs must match exactly, which they can only be asked to do where the reference finds no d within a relative
10^-9 of a bin edge or of r_max and no d2 within a relative 10^-9 of a^2 (two correct evaluations differ by a few u): the
``near_edges`` and ``near_a2`` entries count such terms on the reference, and the inputs below are chosen, with fixed seeds, so
that both are zero (tests/test_coll_ref.py asserts it for every case).
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import sk_ref

U = 2.0 ** -53
LD = np.longdouble
REL = 1e-9
WRONG = ("origin", "lag", "self", "images", "conj", "q2tile")
VECTORS = ((1, 0, 0), (-1, 0, 0), (1, 2, -1), (-1, -2, 1), (0, 0, 3), (2, -3, 0))

Case = namedtuple("Case", "name nframes nboxes nwater nlags every M nbins rfrac hist_lags a seed side")


def n_origins(nframes, lag, every):
    return (nframes - 1 - lag) // every + 1


def origins(nframes, lag, every):
    return np.arange(0, nframes - lag, every) if 0 <= lag <= nframes - 1 else np.zeros(0, dtype=int)


# ---- the cell -------------------------------------------------------------------------------------------------------------------
def pair_cell(h, r_max):
    """(g [3, 3] rows of the inverse, w [3] widths, m [3] image range) by the header's arithmetic; ValueError beyond 1.5 w."""
    h = np.asarray(h, dtype=np.float64)
    c = np.array([np.cross(h[1], h[2]), np.cross(h[2], h[0]), np.cross(h[0], h[1])])
    det = h[0, 0] * c[0, 0] + h[0, 1] * c[0, 1] + h[0, 2] * c[0, 2]
    w = abs(det) / np.sqrt((c * c).sum(axis=1))
    g = c * (1.0 / det)
    r = r_max * (1.0 + 1e-9)
    m = []
    for k in range(3):
        if r <= 0.5 * w[k]:
            m.append(0)
        elif r <= 1.5 * w[k]:
            m.append(1)
        else:
            raise ValueError(f"r_max = {r_max} beyond 1.5 x the cell width {w[k]}")
    return g, w, m


def inverse_cofactor(h):
    """H^-1 as the header forms it for the modes: cofactors over the determinant (no fma in numpy: within the bars)."""
    h = np.asarray(h, dtype=np.float64)
    c = np.array([np.cross(h[1], h[2]), np.cross(h[2], h[0]), np.cross(h[0], h[1])])
    det = (h[0] * c[0]).sum()
    return (c / det).T                                      # s = r @ this


# ---- the modes ------------------------------------------------------------------------------------------------------------------
def modes(h, x, nvec, dtype=np.float64):
    """rho [T, M] complex (dtype float64) or (re, im) long double [T, M] of the frames x [T, N, 3] in the cell h."""
    nvec = np.asarray(nvec, dtype=np.int64).reshape(-1, 3)
    T, N, _ = x.shape
    if dtype is LD:
        s = x.astype(LD) @ sk_ref.inverse_ld(h)
        s = s - np.rint(s)
        t = s @ nvec.T.astype(LD)                            # [T, N, M]
        t = t - np.rint(t)
        ph = sk_ref.TWO_PI_LD * t
        return np.cos(ph).sum(axis=1), -np.sin(ph).sum(axis=1)
    s = x @ inverse_cofactor(h)
    s = s - np.rint(s)
    rho = np.zeros((T, len(nvec)), dtype=np.complex128)
    if len(nvec) == 0:
        return rho
    tables = []
    for a in range(3):
        mm = np.arange(int(np.abs(nvec[:, a]).max()) + 1, dtype=np.float64)
        ph = 2.0 * np.pi * mm[None, :, None] * s[:, None, :, a]
        tables.append(np.cos(ph) + 1j * np.sin(ph))          # [T, nmax_a + 1, N]
    e = []
    for a in range(3):
        t = tables[a][:, np.abs(nvec[:, a])]                 # [T, M, N]
        e.append(np.where((nvec[:, a] < 0)[None, :, None], np.conj(t), t))
    return np.conj((e[0] * e[1]) * e[2]).sum(axis=2)


# ---- the pair counts ------------------------------------------------------------------------------------------------------------
def pair_counts(h, x, lag, every, r_max, nbins, dtype=np.float64, wrong=None):
    """(hist int64 [nbins], near: the number of terms within a relative REL of a bin edge or of r_max) of one box and lag."""
    h = np.asarray(h, dtype=np.float64)
    g, _, m = pair_cell(h, r_max)
    if wrong == "images":
        m = [0, 0, 0]
    T, N, _ = x.shape
    hd, gd = h.astype(dtype), g.astype(dtype)
    if dtype is LD:
        gd = sk_ref.inverse_ld(h).T
    s = x.astype(dtype) @ gd.T
    shifts = [(a, b, c) for a in range(-m[0], m[0] + 1) for b in range(-m[1], m[1] + 1) for c in range(-m[2], m[2] + 1)]
    hist = np.zeros(nbins, dtype=np.int64)
    near = 0
    rm, scale, dr = dtype(r_max), dtype(nbins) / dtype(r_max), dtype(r_max) / dtype(nbins)
    eye = np.eye(N, dtype=bool)
    for o in origins(T, lag, every)[:-1 if wrong == "origin" else None]:
        ds = s[o + lag][None, :, :] - s[o][:, None, :]        # [i, j, 3]
        ds = ds - np.rint(ds)
        for sh in shifts:
            d = (ds + np.array(sh, dtype=dtype)) @ hd
            r2 = (d * d).sum(axis=2)
            keep = np.ones((N, N), dtype=bool)
            if sh == (0, 0, 0) and wrong != "self":
                keep = ~eye
            dist = np.sqrt(r2[keep])
            k = np.rint(dist / dr)
            edge = k * dr
            near += int(np.count_nonzero((np.abs(dist - edge) <= REL * edge) & (k >= 1) & (k <= nbins)))
            dist = dist[dist < rm]
            b = np.minimum(np.floor(dist * scale).astype(np.int64), nbins - 1)
            hist += np.bincount(b, minlength=nbins)
    return hist, near


def pair_counts_brute(h, x, lag, every, r_max, nbins):
    """The same counts with no wrapping and no image rule: every lattice translation that can reach, on the positions as they
    are (rdf_ref.rdf_brute's enumeration across two frames)."""
    h = np.asarray(h, dtype=np.float64)
    w = pair_cell(h, 1e-3)[1]
    T, N, _ = x.shape
    s = x @ np.linalg.inv(h)
    hist = np.zeros(nbins, dtype=np.int64)
    eye = np.eye(N, dtype=bool)
    for o in origins(T, lag, every):
        both = np.concatenate([s[o], s[o + lag]])
        spread = both.max(axis=0) - both.min(axis=0)
        reach = [int(np.floor(r_max / wk + sp)) + 1 for wk, sp in zip(w, spread)]
        for n1 in range(-reach[0], reach[0] + 1):
            for n2 in range(-reach[1], reach[1] + 1):
                for n3 in range(-reach[2], reach[2] + 1):
                    t = n1 * h[0] + n2 * h[1] + n3 * h[2]
                    d = (x[o + lag][None, :, :] + t) - x[o][:, None, :]
                    d = np.sqrt((d * d).sum(axis=2))
                    d = d[~eye] if (n1, n2, n3) == (0, 0, 0) else d.ravel()
                    d = d[d < r_max]
                    hist += np.bincount(np.minimum(np.floor(d * nbins / r_max).astype(np.int64), nbins - 1), minlength=nbins)
    return hist


# ---- everything of a call ---------------------------------------------------------------------------------------------------------
def evaluate(cells, frames, nlags, every, nvec=(), r_max=0.0, nbins=0, hist_lags=(), a=0.0, dtype=np.float64, wrong=None):
    """{rho [T, B, M] complex, fkt [B, nlags, M] complex, gd [B, nh, nbins] int64, qsum, q2sum [B, nlags] int64, near_edges,
    near_a2} and, with dtype=np.longdouble, {bar_rho [T, B, M], bar_fkt [B, nlags, M]} (rho and fkt then as complex128 rounded
    from long double, and rho_ld / fkt_ld as (re, im) pairs).  ``wrong``: one of WRONG, a deliberately broken mirror."""
    frames = np.asarray(frames, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.float64)
    T, B, N, _ = frames.shape
    nvec = np.asarray(nvec, dtype=np.int64).reshape(-1, 3)
    M = len(nvec)
    ext = dtype is LD
    if ext:
        assert sk_ref.have_extended_precision(), "no extended precision on this platform"
    hist_lags = [int(v) for v in hist_lags]
    every = min(int(every), T)
    out = dict(rho=np.zeros((T, B, M), dtype=np.complex128), fkt=np.full((B, nlags, M), np.nan + 0j), gd=np.zeros((B, len(hist_lags), max(nbins, 0)), dtype=np.int64),
               qsum=np.zeros((B, nlags), dtype=np.int64), q2sum=np.zeros((B, nlags), dtype=np.int64), near_edges=0, near_a2=0)
    if ext:
        out.update(bar_rho=np.zeros((T, B, M)), bar_fkt=np.zeros((B, nlags, M)), rho_ld=[None] * B, fkt_ld=[None] * B)
    for b in range(B):
        h, x = cells[b], frames[:, b]
        if M:
            if ext:
                re, im = modes(h, x, nvec, LD)
                delta = sk_ref.delta(nvec, N, float(np.abs(x @ np.linalg.inv(h)).max()))
                out["bar_rho"][:, b] = delta[None, :]
                out["rho_ld"][b] = (re, im)
            else:
                rho = modes(h, x, nvec)
                re, im = rho.real, rho.imag
            out["rho"][:, b] = np.asarray(re, dtype=np.float64) + 1j * np.asarray(im, dtype=np.float64)
            fre, fim = np.zeros((nlags, M), dtype=dtype), np.zeros((nlags, M), dtype=dtype)
            for lag in range(nlags):
                use = lag
                if wrong == "lag":
                    use = lag + 1 if lag + 1 <= T - 1 else lag - 1
                o = origins(T, use, every)
                if wrong == "origin":
                    o = o[:-1]
                if len(o) == 0:
                    fre[lag] = fim[lag] = np.nan
                    continue
                Ar, Ai, Br, Bi = re[o + use], im[o + use], re[o], im[o]
                if wrong == "conj":
                    Ai, Bi = -Ai, -Bi                         # conj(A) B instead of A conj(B)
                nl = dtype(len(o)) * dtype(N)
                fre[lag] = (Ar * Br + Ai * Bi).sum(axis=0) / nl
                fim[lag] = (Ai * Br - Ar * Bi).sum(axis=0) / nl
                if ext and wrong is None:
                    f = lambda v: np.asarray(v, dtype=np.float64)                  # noqa: E731
                    modA, modB = f(np.sqrt(Ar * Ar + Ai * Ai)), f(np.sqrt(Br * Br + Bi * Bi))
                    per_origin = (delta[None, :] * (modA + modB) + delta[None, :] ** 2).sum(axis=0)
                    terms = f((np.abs(Ar) + np.abs(Ai)) * (np.abs(Br) + np.abs(Bi))).sum(axis=0)
                    modF = f(np.sqrt(fre[lag] ** 2 + fim[lag] ** 2))
                    out["bar_fkt"][b, lag] = (per_origin + (len(o) + 4) * U * terms) / (len(o) * N) + U * modF
            out["fkt"][b] = np.asarray(fre, dtype=np.float64) + 1j * np.asarray(fim, dtype=np.float64)
            if ext:
                out["fkt_ld"][b] = (fre, fim)
        if nbins > 0:
            for k, lag in enumerate(hist_lags):
                use = lag
                if wrong == "lag":
                    use = lag + 1 if lag + 1 <= T - 1 else lag - 1
                hist, near = pair_counts(h, x, use, every, r_max, nbins, dtype, wrong)
                out["gd"][b, k] = hist
                out["near_edges"] += near
        if a > 0.0:
            xd = x.astype(dtype)
            a2 = dtype(a) * dtype(a)
            for lag in range(nlags):
                use = lag
                if wrong == "lag":
                    use = lag + 1 if lag + 1 <= T - 1 else lag - 1
                o = origins(T, use, every)
                if wrong == "origin":
                    o = o[:-1]
                if len(o) == 0:
                    continue
                d = xd[o + use] - xd[o]
                d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]      # [o, N]
                inside = d2 < a2
                out["near_a2"] += int(np.count_nonzero(np.abs(d2 - a2) <= REL * a2))
                Q = inside.sum(axis=1).astype(np.int64)
                out["qsum"][b, lag] = Q.sum()
                if wrong == "q2tile":
                    half = N // 2
                    Q1, Q2 = inside[:, :half].sum(axis=1).astype(np.int64), inside[:, half:].sum(axis=1).astype(np.int64)
                    out["q2sum"][b, lag] = (Q1 * Q1 + Q2 * Q2).sum()
                else:
                    out["q2sum"][b, lag] = (Q * Q).sum()
    return out


def evaluate_brute(cells, frames, nlags, every, nvec=(), r_max=0.0, nbins=0, hist_lags=(), a=0.0):
    """A second formulation, written differently: the modes as one complex exponential of the unreduced phase, F by a loop over
    origins of complex products, the pair counts by every translation that can reach with no wrapping, Q molecule by molecule."""
    frames = np.asarray(frames, dtype=np.float64)
    T, B, N, _ = frames.shape
    nvec = np.asarray(nvec, dtype=np.int64).reshape(-1, 3)
    every = min(int(every), T)
    out = dict(rho=np.zeros((T, B, len(nvec)), dtype=np.complex128), fkt=np.zeros((B, nlags, len(nvec)), dtype=np.complex128),
               gd=np.zeros((B, len(hist_lags), max(nbins, 0)), dtype=np.int64), qsum=np.zeros((B, nlags), dtype=np.int64),
               q2sum=np.zeros((B, nlags), dtype=np.int64))
    for b in range(B):
        h, x = np.asarray(cells[b], dtype=np.float64), frames[:, b]
        if len(nvec):
            k = 2.0 * np.pi * nvec @ np.linalg.inv(h).T           # [M, 3]
            rho = np.exp(-1j * np.einsum("tjc,mc->tjm", x, k)).sum(axis=1)
            out["rho"][:, b] = rho
            for lag in range(nlags):
                acc, count = np.zeros(len(nvec), dtype=np.complex128), 0
                t0 = 0
                while t0 + lag <= T - 1:
                    acc += rho[t0 + lag] * np.conj(rho[t0])
                    count += 1
                    t0 += every
                out["fkt"][b, lag] = acc / (count * N)
        if nbins > 0:
            for kk, lag in enumerate(hist_lags):
                out["gd"][b, kk] = pair_counts_brute(h, x, lag, every, r_max, nbins)
        if a > 0.0:
            for lag in range(nlags):
                t0 = 0
                while t0 + lag <= T - 1:
                    Q = sum(1 for j in range(N) if float(((x[t0 + lag, j] - x[t0, j]) ** 2).sum()) < a * a)
                    out["qsum"][b, lag] += Q
                    out["q2sum"][b, lag] += Q * Q
                    t0 += every
    return out


# ---- the inputs of the GPU tests -----------------------------------------------------------------------------------------------
def cases(plan):
    """The cases of tests/test_gpu_coll.py for the plan's pair tile and lag block (collective.coll_plan): the smallest shapes at
    which each boundary of the plan is crossed."""
    tile, lb = plan["pair_tile"], plan["lag_block"]
    out, seed = [], [400]

    def add(name, nframes, nboxes, nwater, nlags=None, every=1, M=4, nbins=16, rfrac=0.45, hist_lags=None, a=0.55, side=9.0, reseed=0):
        nlags = nframes if nlags is None else nlags
        hl = tuple(sorted({0, nlags // 2, nlags - 1})) if hist_lags is None else tuple(hist_lags)
        seed[0] += 1 + reseed                                               # (reseed: the next seed leaves a term within 1e-9 of a bin edge)
        out.append(Case(name, nframes, nboxes, nwater, nlags, every, M, nbins, rfrac, hl if nbins else (), a, seed[0], side))

    for k, n in enumerate((1, 2, 63, 64, 65)):
        add("nwater_%d" % n, 5, 2, n, rfrac=(0.45, 1.2)[k % 2], M=(4, 6, 4, 6, 4)[k])
    for k, (label, n) in enumerate((("tile-1", tile - 1), ("tile", tile), ("tile+1", tile + 1))):
        add("nwater_" + label, 3, 1, n, rfrac=(0.45, 0.7, 0.45)[k], hist_lags=(0, 2), nbins=32, side=14.0)
    add("nwater_1025", 2, 1, 1025, M=3, nbins=0, side=30.0)               # mw_sk.h's segment rule: one segment of 1024 and one molecule
    add("nwater_8193", 2, 1, 8193, M=3, nbins=0, side=60.0)               # segments of 2048
    add("nframes_1", 1, 2, 5)
    add("nframes_2", 2, 2, 5, rfrac=1.2)
    for label, nl in (("1", 1), ("2", 2), ("block-1", lb - 1), ("block", lb), ("block+1", lb + 1)):
        add("nlags_" + label, lb + 6, 1, 3, nlags=nl, M=2, nbins=8, hist_lags=(0, nl - 1))
    add("every3", 12, 3, 9, every=3, M=6, rfrac=1.2)
    add("every_far", 12, 2, 5, every=1000)
    add("M0", 6, 2, 5, M=0)
    add("M1", 6, 2, 5, M=1)
    add("nbins_1", 6, 1, 7, nbins=1, rfrac=0.9)
    add("nbins_4096", 6, 1, 7, nbins=4096, rfrac=1.2, reseed=1)
    add("no_overlap", 6, 2, 5, a=0.0)
    add("farm600", 16, 600, 8, M=6, hist_lags=(1, 9), every=2)
    return out


def cell_of(case, b):
    """An oblique cell of about the case's side, a little different for every box."""
    L = case.side * (1.0 + 0.01 * (b % 7))
    return np.array([[L, 0.0, 0.0], [0.17 * L, 0.96 * L, 0.0], [-0.11 * L, 0.13 * L, 1.05 * L]])


@lru_cache(maxsize=None)
def make_input(case):
    """(cells [B, 3, 3], frames [T, B, N, 3], nvec [M, 3] int32, r_max): random walks with a small drift of their own per box, from
    uniform positions in the cell, unwrapped; r_max = the case's fraction of the smallest perpendicular width of any box."""
    rng = np.random.default_rng(case.seed)
    T, B, N = case.nframes, case.nboxes, case.nwater
    cells = np.array([cell_of(case, b) for b in range(B)])
    start = np.einsum("bna,bac->bnc", rng.uniform(0.0, 1.0, (B, N, 3)), cells)
    steps = rng.normal(0.0, 0.25, (T, B, N, 3))
    steps[0] = 0.0
    drift = rng.normal(0.0, 0.05, (1, B, 1, 3))
    frames = np.ascontiguousarray(start[None] + np.cumsum(steps, axis=0) + drift * np.arange(T)[:, None, None, None])
    nvec = np.array(VECTORS[:case.M], dtype=np.int32).reshape(-1, 3)
    wmin = min(float(pair_cell(cells[b], 1e-3)[1].min()) for b in range(B))
    for arr in (cells, frames, nvec):
        arr.setflags(write=False)
    return cells, frames, nvec, case.rfrac * wmin


@lru_cache(maxsize=None)
def reference(case):
    """The long-double reference, the bars and the margins of a case, computed once and shared."""
    cells, frames, nvec, r_max = make_input(case)
    ref = evaluate(cells, frames, case.nlags, case.every, nvec, r_max, case.nbins, case.hist_lags, case.a, dtype=LD)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def worst(got, ref):
    """{output: (largest |got - ref|, its bar, the largest ratio of a difference to its bar)} over rho and fkt; the reference is
    taken in long double where it is there."""
    rows = {}
    for name in ("rho", "fkt"):
        if got.get(name) is None or ref[name].size == 0:
            continue
        g = np.asarray(got[name])
        if ref.get(name + "_ld") is not None:
            diff = np.empty(g.shape)
            for b, (re, im) in enumerate(ref[name + "_ld"]):
                gb = g[:, b] if name == "rho" else g[b]
                d = np.sqrt(((gb.real.astype(LD) - re) ** 2 + (gb.imag.astype(LD) - im) ** 2).astype(np.float64))
                if name == "rho":
                    diff[:, b] = d
                else:
                    diff[b] = d
        else:
            diff = np.abs(g - ref[name])
        bar = ref["bar_" + name]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(np.isnan(diff), np.inf, np.where(diff == 0.0, 0.0, diff / bar))
        k = np.unravel_index(np.argmax(ratio), ratio.shape)
        rows[name] = (float(diff[k]), float(bar[k]), float(ratio[k]))
    return rows
