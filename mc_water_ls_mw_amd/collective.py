"""Collective time correlations of trajectories over the C ABI of ``libmw_coll.so`` (include/mw_coll.h): per box the density
modes rho(n, t) of every frame, the coherent intermediate scattering function F(n, t), integer histograms of the distinct van
Hove function G_d(r, t) and the sums over the time origins of the overlap Q and of Q^2, and the host arithmetic for what is
read off them (shell averages F(q, t), the dynamic structure factor S(q, omega), relaxation times, G_d(r, t) normalised to the
ideal gas, the four-point susceptibility chi_4(t)).

Frames are ``[nframes, nboxes, nwater, 3]`` float64, unwrapped and equally spaced in time -- what ``dynamics.trajectory``
records --, positions in bohr; a cell is [3, 3] with ROW k the lattice vector h_(k+1) and is fixed over the trajectory; lags
count frames.  There is no CPU path: without the library or a device the calls raise.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from ._devlib import DevLib, MwError, check_device_tensors

PKG = os.path.dirname(os.path.abspath(__file__))
COLL_LIB_PATH = os.path.join(PKG, "libmw_coll.so")

#: every symbol include/mw_coll.h declares
COLL_ABI_SYMBOLS = ("mw_coll_init", "mw_coll_finalize", "mw_coll_is_initialised", "mw_coll_last_error", "mw_coll_compute",
                    "mw_coll_compute_device", "mw_coll_plan", "mw_coll_last", "mw_coll_elapsed_ms")
#: the fields of mw_coll_plan / mw_coll_last, in order
PLAN_FIELDS = ("boxes_per_chunk", "chunks", "mode_units", "segments", "segment_molecules", "small", "lag_block", "pair_tile", "pair_tiles",
               "pair_small", "slabs", "origins_per_slab", "lds_bytes", "scratch_bytes_per_box")
OUTPUTS = ("rho", "fkt", "gd", "qsum", "q2sum")
MAX_VECTORS, MAX_COMPONENT, MAX_BINS, MAX_HIST_LAGS, MAX_FRAMES = 4096, 255, 4096, 64, 65536


def _argtypes(L):
    for f in (L.mw_coll_compute, L.mw_coll_compute_device):
        f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                      ctypes.c_void_p, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p,
                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.mw_coll_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                               ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int]


_dev = DevLib("coll", COLL_LIB_PATH, "the collective time correlations", PLAN_FIELDS, setup=_argtypes)

load_coll_library = _dev.load                    # (path=COLL_LIB_PATH): dlopen libmw_coll.so; raises if it has not been built
coll_finalize = _dev.finalize


def _fields(out):
    return dict(zip(PLAN_FIELDS, (int(v) for v in out)))


def coll_init(device=0):
    """Initialise the library on ``device`` (the compute functions do it on device 0 when nobody has)."""
    return _dev.live(device)


def coll_plan(nframes, nwater, nlags=None, origin_every=1, M=0, nmax=(0, 0, 0), nbins=0, nh=0, overlap=False, nboxes=1):
    """{field: value} of PLAN_FIELDS: the launch rules of ``nboxes`` boxes of ``nwater`` molecules over ``nframes`` frames and
    ``nlags`` lags (None: nframes) with ``M`` vectors of largest components ``nmax``, ``nbins`` bins at ``nh`` selected lags and
    the overlap asked for or not (mw_coll_plan), no device needed."""
    L = _dev.load()
    out = _dev.plan_out()
    nm = (ctypes.c_int * 3)(*(int(v) for v in nmax))
    _dev.chk(L.mw_coll_plan(int(nframes), int(nwater), int(nframes if nlags is None else nlags), int(origin_every), int(M), nm, int(nbins), int(nh),
                            1 if overlap else 0, int(nboxes), out, len(out)))
    return _fields(out)


def coll_last():
    """{field: value} of PLAN_FIELDS for the last call that launched."""
    L = _dev.load()
    out = _dev.plan_out()
    _dev.chk(L.mw_coll_last(out, len(out)))
    return _fields(out)


def coll_elapsed_ms():
    """(modes, correlate, pairs, overlap) of the last call in milliseconds, summed over its chunks, from the library's event
    timers."""
    L = _dev.load()
    t = [ctypes.c_float(0.0) for _ in range(4)]
    _dev.chk(L.mw_coll_elapsed_ms(*[ctypes.byref(v) for v in t]))
    return tuple(v.value for v in t)


def n_origins(nframes, lags, origin_every=1):
    """o_l = (nframes - 1 - l) // origin_every + 1 for every lag of ``lags``."""
    return (int(nframes) - 1 - np.asarray(lags, dtype=np.int64)) // int(origin_every) + 1


def _lists(cells, nb, nvec, hist_lags):
    cells = np.ascontiguousarray(cells, dtype=np.float64)
    if cells.ndim == 2:
        cells = np.ascontiguousarray(np.broadcast_to(cells, (nb, 3, 3)))
    if cells.shape != (nb, 3, 3):
        raise MwError(f"cells {cells.shape}: expected [{nb}, 3, 3] (or one [3, 3] for every box)")
    nv = np.zeros((0, 3), dtype=np.int32) if nvec is None else np.ascontiguousarray(np.asarray(nvec, dtype=np.int64).reshape(-1, 3), dtype=np.int32)
    hl = np.ascontiguousarray(np.atleast_1d(np.asarray(hist_lags, dtype=np.int64)), dtype=np.int32).reshape(-1)
    return cells, nv, hl


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def _wanted(outputs, M, nbins, nh, overlap_a):
    """The outputs of ``outputs`` the call's lists allow: rho and fkt need vectors, gd bins and selected lags, the sums a length."""
    unknown = [k for k in outputs if k not in OUTPUTS]
    if unknown:
        raise MwError(f"outputs {unknown}: expected names of {OUTPUTS}")
    can = dict(rho=M > 0, fkt=M > 0, gd=nbins > 0 and nh > 0, qsum=overlap_a != 0.0, q2sum=overlap_a != 0.0)
    if tuple(outputs) not in (OUTPUTS, OUTPUTS[1:]): # the two default sets take what the lists allow; a chosen name must be possible
        needs = dict(rho="nvec", fkt="nvec", gd="nbins > 0 and hist_lags", qsum="overlap_a > 0", q2sum="overlap_a > 0")
        for k in outputs:
            if not can[k]:
                raise MwError(f"outputs names {k!r}, which needs {needs[k]}")
    return {k: k in outputs and can[k] for k in OUTPUTS}


def collective_correlations(cells, frames, nlags=None, origin_every=1, nvec=None, r_max=0.0, nbins=0, hist_lags=(), overlap_a=0.0, outputs=OUTPUTS):
    """(rho [nframes, nboxes, M] complex, fkt [nboxes, nlags, M] complex, gd [nboxes, nh, nbins] int64, qsum [nboxes, nlags]
    int64, q2sum [nboxes, nlags] int64) of the trajectory ``frames`` [nframes, nboxes, nwater, 3] in the cells ``cells``
    [nboxes, 3, 3] (one [3, 3]: the cell of every box): the density modes of every frame at the integer triples ``nvec``
    [M, 3]; F(n, l) = <rho(n, t0 + l) conj rho(n, t0)> / nwater over the origins 0, ``origin_every``, ... for every lag
    l = 0 .. ``nlags`` - 1 (None: every one); the counts of the distances |r_j(t0 + l) + n . h - r_i(t0)| below ``r_max`` (bohr)
    in ``nbins`` bins at the lags ``hist_lags``, over all origins, (j, n) != (i, 0); and the sums over the origins of
    Q = #{j: |x_j(t0 + l) - x_j(t0)| < overlap_a} and of Q^2.  An output that ``outputs`` does not name is None, and its work is
    not done.  With ``outputs`` all five names, or all but rho, an output whose lists are absent (no nvec; nbins = 0 or no
    hist_lags; overlap_a = 0) is None as well; any other choice of names must be possible, or the call raises.  A trajectory of one box may
    come as [nframes, nwater, 3], and then the results lose the box axis."""
    frames = np.ascontiguousarray(frames, dtype=np.float64)
    single = frames.ndim == 3
    if single:
        frames = frames[:, None]
    if frames.ndim != 4 or frames.shape[3] != 3:
        raise MwError(f"frames {frames.shape}: expected [nframes, nboxes, nwater, 3]")
    nf, nb, n = frames.shape[:3]
    cells, nv, hl = _lists(cells, nb, nvec, hist_lags)
    nlags = nf if nlags is None else int(nlags)
    M, nl = len(nv), max(nlags, 1)
    want = _wanted(outputs, M, int(nbins), hl.size, float(overlap_a))
    L = _dev.live()
    rho = np.zeros((nf, nb, M), dtype=np.complex128) if want["rho"] else None
    fkt = np.zeros((nb, nl, M), dtype=np.complex128) if want["fkt"] else None
    gd = np.zeros((nb, hl.size, int(nbins)), dtype=np.int64) if want["gd"] else None
    qsum = np.zeros((nb, nl), dtype=np.int64) if want["qsum"] else None
    q2sum = np.zeros((nb, nl), dtype=np.int64) if want["q2sum"] else None
    _dev.chk(L.mw_coll_compute(nf, nb, n, cells.ctypes.data, frames.ctypes.data, nlags, int(origin_every), M, _ptr(nv), float(r_max), int(nbins),
                               hl.size, _ptr(hl), float(overlap_a), _ptr(rho), _ptr(fkt), _ptr(gd), _ptr(qsum), _ptr(q2sum)))
    out = (rho, fkt, gd, qsum, q2sum)
    if single:
        return tuple(None if a is None else (a[:, 0] if k == 0 else a[0]) for k, a in enumerate(out))
    return out


def collective_correlations_torch(cells, frames_t, nlags=None, origin_every=1, nvec=None, r_max=0.0, nbins=0, hist_lags=(), overlap_a=0.0,
                                  outputs=OUTPUTS):
    """The same five results as tensors on the device of ``frames_t`` [nframes, nboxes, nwater, 3], a contiguous float64 device
    tensor on the device the library lives on (mw_coll_compute_device); rho and fkt are complex128.  ``cells`` (array or tensor),
    ``nvec`` and ``hist_lags`` are host lists."""
    import torch
    dev = check_device_tensors((frames_t, torch.float64, "frames_t"))
    if frames_t.ndim != 4 or frames_t.shape[3] != 3:
        raise MwError(f"frames_t {tuple(frames_t.shape)}: expected [nframes, nboxes, nwater, 3]")
    nf, nb, n = (int(v) for v in frames_t.shape[:3])
    if isinstance(cells, torch.Tensor):
        cells = cells.detach().cpu().numpy()
    cells, nv, hl = _lists(cells, nb, nvec, hist_lags)
    nlags = nf if nlags is None else int(nlags)
    M, nl = len(nv), max(nlags, 1)
    want = _wanted(outputs, M, int(nbins), hl.size, float(overlap_a))
    L = _dev.live(dev.index or 0)                  # raises if the library lives on another device
    new = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)     # noqa: E731
    rho = new(nf, nb, M, 2) if want["rho"] else None
    fkt = new(nb, nl, M, 2) if want["fkt"] else None
    gd = new(nb, hl.size, int(nbins), dtype=torch.int64) if want["gd"] else None
    qsum = new(nb, nl, dtype=torch.int64) if want["qsum"] else None
    q2sum = new(nb, nl, dtype=torch.int64) if want["q2sum"] else None
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
    torch.cuda.synchronize(dev)
    _dev.chk(L.mw_coll_compute_device(nf, nb, n, cells.ctypes.data, frames_t.data_ptr(), nlags, int(origin_every), M, _ptr(nv), float(r_max),
                                      int(nbins), hl.size, _ptr(hl), float(overlap_a), ptr(rho), ptr(fkt), ptr(gd), ptr(qsum), ptr(q2sum)))
    cplx = lambda t: None if t is None else torch.view_as_complex(t)       # noqa: E731
    return cplx(rho), cplx(fkt), gd, qsum, q2sum


# ---- host arithmetic for what is read off the results --------------------------------------------------------------------------
def wave_numbers(nvec, cells):
    """|k_n| [nboxes, M] in inverse bohr: k_n = 2 pi H^-T n, i.e. 2 pi n @ inv(h).T for a cell h with rows h_k."""
    cells = np.asarray(cells, dtype=np.float64)
    cells = cells[None] if cells.ndim == 2 else cells
    nv = np.asarray(nvec, dtype=np.float64).reshape(-1, 3)
    k = 2.0 * np.pi * np.einsum("ma,bca->bmc", nv, np.linalg.inv(cells))
    return np.sqrt((k * k).sum(axis=-1))


def coherent_scattering(fkt, nvec, cells, edges):
    """(q_mid [nshells], F [nboxes, nlags, nshells], F_norm [nboxes, nlags, nshells], count [nboxes, nshells]): the real part of
    ``fkt`` [nboxes, nlags, M] averaged over the vectors whose |k_n| lies in [edges[s], edges[s + 1]) (inverse bohr), per box,
    and the same divided by its lag-0 value, F(q, t) / F(q, 0) = F(q, t) / S(q).  A shell without a vector gives NaN."""
    fkt = np.asarray(fkt)
    e = np.asarray(edges, dtype=np.float64)
    if fkt.ndim != 3 or e.ndim != 1 or len(e) < 2:
        raise MwError(f"fkt {fkt.shape} / edges {e.shape}: expected [nboxes, nlags, M] and at least two edges")
    q = wave_numbers(nvec, cells)
    if q.shape[0] == 1 and fkt.shape[0] > 1:
        q = np.broadcast_to(q, (fkt.shape[0], q.shape[1]))
    if q.shape != (fkt.shape[0], fkt.shape[2]):
        raise MwError(f"nvec / cells give wave numbers {q.shape}, fkt is {fkt.shape}")
    ns = len(e) - 1
    F = np.full((fkt.shape[0], fkt.shape[1], ns), np.nan)
    count = np.zeros((fkt.shape[0], ns), dtype=np.int64)
    for b in range(fkt.shape[0]):
        shell = np.searchsorted(e, q[b], side="right") - 1
        for s in range(ns):
            sel = shell == s
            count[b, s] = int(sel.sum())
            if count[b, s]:
                F[b, :, s] = fkt[b][:, sel].real.mean(axis=1)
    f0 = F[:, :1]
    with np.errstate(invalid="ignore", divide="ignore"):
        norm = np.where(f0 != 0, F / f0, np.nan)
    return 0.5 * (e[:-1] + e[1:]), F, norm, count


def dynamic_structure_factor(F_t, dt_frame, window="hann"):
    """(omega [nlags], S [..., nlags]): S(q, omega) = (1 / pi) x the cosine transform of F(q, t), ``F_t`` [..., nlags] with the
    lags last, at the angular frequencies omega_k = pi k / ((nlags - 1) dt_frame), with the trapezoid rule.  ``window``: "hann"
    tapers the curve to 0 at the last lag (0.5 (1 + cos(pi l / (nlags - 1)))), None leaves it as it is."""
    F_t = np.asarray(F_t, dtype=np.float64)
    nl = F_t.shape[-1]
    if nl < 2:
        raise MwError("dynamic_structure_factor: at least two lags are required")
    l = np.arange(nl, dtype=np.float64)
    if window == "hann":
        w = 0.5 * (1.0 + np.cos(np.pi * l / (nl - 1)))
    elif window is None:
        w = np.ones(nl)
    else:
        raise MwError(f"dynamic_structure_factor: window = {window!r} is neither 'hann' nor None")
    trap = np.ones(nl)
    trap[0] = trap[-1] = 0.5
    omega = np.pi * l / ((nl - 1) * float(dt_frame))
    kernel = np.cos(np.outer(l, l) * (np.pi / (nl - 1))) * trap[:, None]         # [lag, k]
    return omega, ((F_t * w) @ kernel) * (float(dt_frame) / np.pi)


def relaxation_time(F_t, dt_frame, level=1.0 / np.e):
    """tau [...]: the first time at which ``F_t`` [..., nlags] divided by its lag-0 value falls to ``level``, interpolated
    linearly between the two lags around the crossing; NaN where it never does (or the lag-0 value is 0)."""
    F_t = np.asarray(F_t, dtype=np.float64)
    flat = F_t.reshape(-1, F_t.shape[-1])
    tau = np.full(len(flat), np.nan)
    for r, row in enumerate(flat):
        if not row[0] != 0 or not np.isfinite(row[0]):
            continue
        c = row / row[0]
        below = np.nonzero(c <= level)[0]
        if len(below) == 0 or below[0] == 0:
            continue
        k = below[0]
        tau[r] = (k - 1 + (c[k - 1] - level) / (c[k - 1] - c[k])) * float(dt_frame)
    return tau.reshape(F_t.shape[:-1])


def distinct_van_hove_from_counts(gd, cells, nwater, r_max, n_origins):
    """(r_mid [nbins], g [nboxes, nh, nbins]): G_d(r, t) / rho from the counts ``gd`` [nboxes, nh, nbins]: each divided by what an
    ideal gas of the box's density would give, n_origins x nwater x (nwater / V) x the volume of the bin's shell, so that an
    ideal gas gives 1.  ``n_origins`` [nh] (or one number): the origins of each selected lag (``n_origins``(nframes, hist_lags,
    origin_every))."""
    gd = np.asarray(gd)
    cells = np.asarray(cells, dtype=np.float64)
    cells = cells[None] if cells.ndim == 2 else cells
    if gd.ndim != 3:
        raise MwError(f"gd {gd.shape}: expected [nboxes, nh, nbins]")
    nbins = gd.shape[-1]
    edges = float(r_max) * np.arange(nbins + 1, dtype=np.float64) / nbins
    shell = 4.0 * np.pi / 3.0 * (edges[1:] ** 3 - edges[:-1] ** 3)
    vol = np.abs(np.linalg.det(cells))
    o = np.broadcast_to(np.asarray(n_origins, dtype=np.float64), (gd.shape[1],))
    ideal = o[None, :, None] * float(nwater) * (float(nwater) / vol)[:, None, None] * shell[None, None, :]
    return 0.5 * (edges[:-1] + edges[1:]), gd / ideal


def chi4_from_sums(qsum, q2sum, n_origins, nwater):
    """(<Q> / N, chi_4 = (<Q^2> - <Q>^2) / N) [..., nlags] from the sums over the origins ``qsum`` and ``q2sum`` [..., nlags] and
    the number of origins of every lag ``n_origins`` [nlags]."""
    o = np.asarray(n_origins, dtype=np.float64)
    mean = np.asarray(qsum, dtype=np.float64) / o
    mean2 = np.asarray(q2sum, dtype=np.float64) / o
    return mean / float(nwater), (mean2 - mean * mean) / float(nwater)
