"""Time correlation functions of trajectories over the C ABI of ``libmw_tcf.so`` (include/mw_tcf.h): per box the mean
squared displacement, the mean quartic displacement, the velocity autocorrelation function, the self-intermediate scattering
function F_s(q, t) and integer histograms of the displacement (the self part of the van Hove function), each averaged over
every time origin and every molecule, and the host arithmetic for what is read off these curves (the diffusion coefficient,
the non-Gaussian parameter, the vibrational density of states, G_s(r)).

Frames are ``[nframes, nboxes, nwater, 3]`` float64, unwrapped and equally spaced in time -- what ``dynamics.trajectory``
records --, positions in bohr, velocities in bohr per atomic time unit, wave numbers in inverse bohr; lags count frames.  No
cell is needed.  There is no CPU path: without the library or a device the calls raise.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from ._devlib import DevLib, MwError, check_device_tensors

PKG = os.path.dirname(os.path.abspath(__file__))
TCF_LIB_PATH = os.path.join(PKG, "libmw_tcf.so")

#: every symbol include/mw_tcf.h declares
TCF_ABI_SYMBOLS = ("mw_tcf_init", "mw_tcf_finalize", "mw_tcf_is_initialised", "mw_tcf_last_error", "mw_tcf_compute",
                   "mw_tcf_compute_device", "mw_tcf_plan", "mw_tcf_last", "mw_tcf_elapsed_ms")
#: the fields of mw_tcf_plan / mw_tcf_last, in order
PLAN_FIELDS = ("boxes_per_chunk", "chunks", "tile", "lag_block", "origin_chunk", "frame_window", "lds_bytes", "scratch_bytes_per_box",
               "tiles", "lag_blocks")
REMOVE_COM = 1                                  # MW_TCF_REMOVE_COM
MAX_Q, MAX_EDGES, MAX_HIST_LAGS = 16, 1025, 64


def _argtypes(L):
    for f in (L.mw_tcf_compute, L.mw_tcf_compute_device):
        f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                      ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p,
                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.mw_tcf_plan.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_int,
                              ctypes.POINTER(ctypes.c_int), ctypes.c_int]


_dev = DevLib("tcf", TCF_LIB_PATH, "the time correlation functions", PLAN_FIELDS, setup=_argtypes)

load_tcf_library = _dev.load                     # (path=TCF_LIB_PATH): dlopen libmw_tcf.so; raises if it has not been built
tcf_finalize = _dev.finalize


def _fields(out):
    return dict(zip(PLAN_FIELDS, (int(v) for v in out)))


def tcf_init(device=0):
    """Initialise the library on ``device`` (the compute functions do it on device 0 when nobody has)."""
    return _dev.live(device)


def tcf_plan(nframes, nwater, nlags=None, nq=0, nedges=0, remove_com=False, nboxes=1):
    """{field: value} of PLAN_FIELDS: the launch rules of ``nboxes`` boxes of ``nwater`` molecules over ``nframes`` frames
    and ``nlags`` lags (None: nframes) with ``nq`` wave numbers and ``nedges`` histogram edges (mw_tcf_plan), no device
    needed."""
    L = _dev.load()
    out = _dev.plan_out()
    _dev.chk(L.mw_tcf_plan(int(nframes), int(nwater), int(nframes if nlags is None else nlags), int(nq), int(nedges),
                           REMOVE_COM if remove_com else 0, int(nboxes), out, len(out)))
    return _fields(out)


def tcf_last():
    """{field: value} of PLAN_FIELDS for the last call that launched."""
    L = _dev.load()
    out = _dev.plan_out()
    _dev.chk(L.mw_tcf_last(out, len(out)))
    return _fields(out)


def tcf_elapsed_ms():
    """(centre, correlate, reduce) of the last call in milliseconds, summed over its chunks, from the library's event timers:
    the centring pass (0 without ``remove_com``), the correlation pass with the histograms, and the sum over the tiles."""
    L = _dev.load()
    t = [ctypes.c_float(0.0) for _ in range(3)]
    _dev.chk(L.mw_tcf_elapsed_ms(*[ctypes.byref(v) for v in t]))
    return tuple(v.value for v in t)


def _lists(q, edges, hist_lags):
    """(q, edges squared, hist_lags) as the host arrays the library takes; lengths are checked by the library."""
    qa = np.zeros(0) if q is None else np.ascontiguousarray(np.atleast_1d(q), dtype=np.float64)
    e = np.zeros(0) if edges is None else np.ascontiguousarray(np.atleast_1d(edges), dtype=np.float64)
    if qa.ndim != 1 or e.ndim != 1:
        raise MwError(f"q {qa.shape} / edges {e.shape}: expected one-dimensional lists")
    if np.any(e < 0.0):
        raise MwError("edges are distances in bohr and must not be negative")
    hl = np.ascontiguousarray(np.atleast_1d(np.asarray(hist_lags, dtype=np.int64)), dtype=np.int32).reshape(-1)
    return qa, np.ascontiguousarray(e * e), hl


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def time_correlations(frames, vel_frames=None, nlags=None, origin_every=1, q=None, edges=None, hist_lags=(), remove_com=False):
    """(msd [nboxes, nlags], mqd [nboxes, nlags], vacf [nboxes, nlags] or None, fs [nboxes, nlags, nq] or None, hist [nboxes,
    nh, nedges + 1] int64 or None) of the trajectory ``frames`` [nframes, nboxes, nwater, 3] (and ``vel_frames`` of the same
    shape, None: no vacf): for every lag l = 0 .. ``nlags`` - 1 (None: every one) the averages over the origins 0,
    ``origin_every``, 2 ``origin_every``, ... and the molecules of the squared displacement (bohr^2), of its square, of
    v(t0) . v(t0 + l) and of sinc(q |d|) for the wave numbers ``q`` (inverse bohr; None: no fs); hist = the counts of |d| at
    the lags ``hist_lags`` below the first of ``edges`` (bohr, ascending), in the bins between them, and at or beyond the last
    (None or no hist_lags: no hist).  ``remove_com``: every frame's centre (and mean velocity) is taken away first.  A
    trajectory of one box may come as [nframes, nwater, 3], and then the results lose the box axis."""
    frames = np.ascontiguousarray(frames, dtype=np.float64)
    single = frames.ndim == 3
    if single:
        frames = frames[:, None]
    if frames.ndim != 4 or frames.shape[3] != 3:
        raise MwError(f"frames {frames.shape}: expected [nframes, nboxes, nwater, 3]")
    if vel_frames is not None:
        vel_frames = np.ascontiguousarray(vel_frames, dtype=np.float64)
        if single and vel_frames.ndim == 3:
            vel_frames = vel_frames[:, None]
        if vel_frames.shape != frames.shape:
            raise MwError(f"vel_frames {vel_frames.shape}: expected the shape of frames, {frames.shape}")
    nf, nb, n = frames.shape[:3]
    nlags = nf if nlags is None else int(nlags)
    qa, e2, hl = _lists(q, edges, hist_lags)
    want_hist = e2.size > 0 and hl.size > 0
    L = _dev.live()
    nl = max(nlags, 1)
    msd, mqd = np.zeros((nb, nl)), np.zeros((nb, nl))
    vacf = np.zeros((nb, nl)) if vel_frames is not None else None
    fs = np.zeros((nb, nl, qa.size)) if qa.size else None
    hist = np.zeros((nb, hl.size, e2.size + 1), dtype=np.int64) if want_hist else None
    _dev.chk(L.mw_tcf_compute(nf, nb, n, frames.ctypes.data, None if vel_frames is None else vel_frames.ctypes.data, nlags, int(origin_every),
                              qa.size, _ptr(qa), e2.size, _ptr(e2), hl.size, _ptr(hl), REMOVE_COM if remove_com else 0, msd.ctypes.data,
                              mqd.ctypes.data, _ptr(vacf), _ptr(fs), _ptr(hist)))
    out = (msd, mqd, vacf, fs, hist)
    return tuple(None if a is None else a[0] for a in out) if single else out


def time_correlations_torch(frames_t, vel_frames_t=None, nlags=None, origin_every=1, q=None, edges=None, hist_lags=(), remove_com=False):
    """The same five results as tensors on the device of the inputs: ``frames_t`` [nframes, nboxes, nwater, 3] and the optional
    ``vel_frames_t`` are contiguous float64 device tensors on the device the library lives on (mw_tcf_compute_device); ``q``,
    ``edges`` and ``hist_lags`` stay host lists."""
    import torch
    named = [(frames_t, torch.float64, "frames_t")]
    if vel_frames_t is not None:
        named.append((vel_frames_t, torch.float64, "vel_frames_t"))
    dev = check_device_tensors(*named)
    if frames_t.ndim != 4 or frames_t.shape[3] != 3:
        raise MwError(f"frames_t {tuple(frames_t.shape)}: expected [nframes, nboxes, nwater, 3]")
    if vel_frames_t is not None and tuple(vel_frames_t.shape) != tuple(frames_t.shape):
        raise MwError(f"vel_frames_t {tuple(vel_frames_t.shape)}: expected the shape of frames_t, {tuple(frames_t.shape)}")
    nf, nb, n = (int(v) for v in frames_t.shape[:3])
    nlags = nf if nlags is None else int(nlags)
    qa, e2, hl = _lists(q, edges, hist_lags)
    want_hist = e2.size > 0 and hl.size > 0
    L = _dev.live(dev.index or 0)                  # raises if the library lives on another device
    nl = max(nlags, 1)
    new = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)     # noqa: E731
    msd, mqd = new(nb, nl), new(nb, nl)
    vacf = new(nb, nl) if vel_frames_t is not None else None
    fs = new(nb, nl, qa.size) if qa.size else None
    hist = new(nb, hl.size, e2.size + 1, dtype=torch.int64) if want_hist else None
    ptr = lambda t: None if t is None else t.data_ptr()                    # noqa: E731
    torch.cuda.synchronize(dev)
    _dev.chk(L.mw_tcf_compute_device(nf, nb, n, frames_t.data_ptr(), ptr(vel_frames_t), nlags, int(origin_every), qa.size, _ptr(qa), e2.size,
                                     _ptr(e2), hl.size, _ptr(hl), REMOVE_COM if remove_com else 0, msd.data_ptr(), mqd.data_ptr(), ptr(vacf),
                                     ptr(fs), ptr(hist)))
    return msd, mqd, vacf, fs, hist


# ---- host arithmetic for what is read off the curves ---------------------------------------------------------------------------
def non_gaussian(msd, mqd):
    """alpha_2 = 3 <d^4> / (5 <d^2>^2) - 1 per lag (0 for a Gaussian displacement distribution); 0 where msd is 0."""
    msd, mqd = np.asarray(msd, dtype=np.float64), np.asarray(mqd, dtype=np.float64)
    den = 5.0 * msd * msd
    return np.divide(3.0 * mqd, den, out=np.ones(msd.shape), where=den > 0) - 1.0


def diffusion_from_msd(msd, dt_frame, fit=None):
    """D = the least-squares slope of msd [..., nlags] against time over the lags ``fit`` = (first, last) inclusive (None: the
    second half of the lags), divided by 6; ``dt_frame`` is the time between two frames, so D is in bohr^2 per that unit."""
    msd = np.asarray(msd, dtype=np.float64)
    nl = msd.shape[-1]
    first, last = (nl // 2, nl - 1) if fit is None else (int(fit[0]), int(fit[1]))
    if not (0 <= first < last < nl):
        raise MwError(f"diffusion_from_msd: fit = ({first}, {last}) is not a window of at least two of the {nl} lags")
    t = np.arange(first, last + 1, dtype=np.float64) * float(dt_frame)
    tc = t - t.mean()
    y = msd[..., first:last + 1]
    return (y * tc).sum(axis=-1) / (tc * tc).sum() / 6.0


def diffusion_from_vacf(vacf, dt_frame):
    """D = (1 / 3) x the trapezoid integral of vacf [..., nlags] over time (Green-Kubo)."""
    vacf = np.asarray(vacf, dtype=np.float64)
    return (vacf.sum(axis=-1) - 0.5 * (vacf[..., 0] + vacf[..., -1])) * float(dt_frame) / 3.0


def vdos(vacf, dt_frame, window="hann"):
    """(omega [nlags], spectrum [..., nlags]): the cosine transform of vacf [..., nlags] normalised by its lag-0 value, at the
    angular frequencies omega_k = pi k / ((nlags - 1) dt_frame), with the trapezoid rule.  ``window``: "hann" tapers the curve to
    0 at the last lag (0.5 (1 + cos(pi l / (nlags - 1)))), None leaves it as it is."""
    vacf = np.asarray(vacf, dtype=np.float64)
    nl = vacf.shape[-1]
    if nl < 2:
        raise MwError("vdos: at least two lags are required")
    l = np.arange(nl, dtype=np.float64)
    if window == "hann":
        w = 0.5 * (1.0 + np.cos(np.pi * l / (nl - 1)))
    elif window is None:
        w = np.ones(nl)
    else:
        raise MwError(f"vdos: window = {window!r} is neither 'hann' nor None")
    c0 = vacf[..., :1]
    c = np.divide(vacf, c0, out=np.zeros(vacf.shape), where=c0 != 0) * w
    trap = np.ones(nl)
    trap[0] = trap[-1] = 0.5
    omega = np.pi * l / ((nl - 1) * float(dt_frame))
    kernel = np.cos(np.outer(l, l) * (np.pi / (nl - 1))) * trap[:, None]         # [lag, k]
    return omega, (c @ kernel) * float(dt_frame)


def van_hove_from_counts(hist, edges):
    """(r_mid [nbins], p [..., nbins]): the bin centres in bohr and 4 pi r^2 G_s(r), the density of |d| per bohr, from counts
    ``hist`` [..., nedges + 1] over the edges ``edges`` [nedges] in bohr, normalised so that the sum of p x bin width plus the
    fractions below the first and beyond the last edge is 1; a row without counts gives zeros.  Host arithmetic."""
    hist = np.asarray(hist)
    e = np.asarray(edges, dtype=np.float64)
    if e.ndim != 1 or len(e) < 2 or hist.shape[-1] != len(e) + 1:
        raise MwError(f"hist {hist.shape} / edges {e.shape}: expected [..., nedges + 1] and [nedges]")
    total = hist.sum(axis=-1, keepdims=True).astype(np.float64)
    inner = hist[..., 1:-1]
    frac = np.divide(inner, total, out=np.zeros(inner.shape, dtype=np.float64), where=total > 0)
    return 0.5 * (e[:-1] + e[1:]), frac / (e[1:] - e[:-1])
