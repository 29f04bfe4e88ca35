"""Times libmw_tcf.so (timecorr.time_correlations_torch) against the plain torch expression of the same sums, one lag at a
time, on the same device tensors: two shapes (a few large boxes, a farm of small ones), each with nq = 0 and nq = 4 and with
and without velocities.  Event timers, two warm-up calls, seven repetitions of each alternating, median with smallest and
largest.  Writes one JSON document, profiles/tcf_measurements.json by default.

    python tools/tcf_measurements.py [--out FILE] [--reps 7] [--small]
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

SHAPES = (dict(name="8 x 4096 molecules, 1024 frames, 512 lags", nboxes=8, nwater=4096, nframes=1024, nlags=512),
          dict(name="4096 x 48 molecules, 256 frames, 128 lags", nboxes=4096, nwater=48, nframes=256, nlags=128))
SMALL = (dict(name="2 x 256 molecules, 64 frames, 32 lags", nboxes=2, nwater=256, nframes=64, nlags=32),)
Q4 = (0.8, 1.7, 2.4, 3.3)


def torch_baseline(frames, vel, nlags, q):
    """The same sums in plain torch, one lag at a time (every frame an origin)."""
    T, B = frames.shape[0], frames.shape[1]
    msd = torch.zeros((B, nlags), dtype=torch.float64, device=frames.device)
    mqd, vacf = torch.zeros_like(msd), torch.zeros_like(msd) if vel is not None else None
    fs = torch.zeros((B, nlags, len(q)), dtype=torch.float64, device=frames.device) if q else None
    for lag in range(nlags):
        d = frames[lag:] - frames[:T - lag]
        d2 = (d * d).sum(dim=-1)
        msd[:, lag] = d2.mean(dim=(0, 2))
        mqd[:, lag] = (d2 * d2).mean(dim=(0, 2))
        if q:
            r = torch.sqrt(d2)
            for a, qa in enumerate(q):
                fs[:, lag, a] = torch.sinc(r * (qa / math.pi)).mean(dim=(0, 2))
        if vel is not None:
            vacf[:, lag] = (vel[:T - lag] * vel[lag:]).sum(dim=-1).mean(dim=(0, 2))
    return msd, mqd, vacf, fs


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def stats(ms):
    s = sorted(ms)
    return dict(median_ms=s[len(s) // 2], min_ms=s[0], max_ms=s[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "tcf_measurements.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="one tiny shape, to try the script")
    args = ap.parse_args()
    from mc_water_ls_mw_amd.timecorr import tcf_elapsed_ms, tcf_finalize, tcf_last, time_correlations_torch
    dev = torch.device("cuda", 0)
    rows = []
    for shape in (SMALL if args.small else SHAPES):
        T, B, N, nlags = shape["nframes"], shape["nboxes"], shape["nwater"], shape["nlags"]
        gen = torch.Generator(device=dev).manual_seed(7)
        frames = torch.cumsum(0.3 * torch.randn((T, B, N, 3), dtype=torch.float64, device=dev, generator=gen), dim=0).contiguous()
        vel = (1e-3 * torch.randn((T, B, N, 3), dtype=torch.float64, device=dev, generator=gen)).contiguous()
        for q in ((), Q4):
            for with_vel in (False, True):
                v = vel if with_vel else None
                lib = lambda: time_correlations_torch(frames, v, nlags, 1, list(q) or None)        # noqa: E731
                base = lambda: torch_baseline(frames, v, nlags, q)                                  # noqa: E731
                for _ in range(2):
                    got, want = lib(), base()
                    torch.cuda.synchronize()
                worst = {}
                for name, g, w in zip(("msd", "mqd", "vacf", "fs"), got, want):
                    if g is not None:
                        worst[name] = float(((g - w).abs() / w.abs().clamp_min(1e-300)).max())
                t_lib, t_base, parts = [], [], []
                for _ in range(args.reps):
                    t_lib.append(timed(lib)[0])
                    parts.append(tcf_elapsed_ms())
                    t_base.append(timed(base)[0])
                row = dict(shape=shape["name"], nq=len(q), velocities=with_vel, library=stats(t_lib), torch=stats(t_base), plan=tcf_last(),
                           library_passes_ms=dict(zip(("centre", "correlate", "reduce"), sorted(parts, key=lambda p: p[1])[len(parts) // 2])),
                           largest_relative_difference_to_torch=worst)
                row["torch_over_library"] = row["torch"]["median_ms"] / row["library"]["median_ms"]
                terms = B * N * sum(T - lag for lag in range(nlags))
                row["terms"] = terms
                row["library_terms_per_ns"] = terms / (row["library"]["median_ms"] * 1e6)
                print(json.dumps(row), flush=True)
                rows.append(row)
        del frames, vel
        torch.cuda.empty_cache()
    tcf_finalize()
    doc = dict(device=torch.cuda.get_device_name(0), method="torch.cuda events around each call; 2 warm-up calls of each, then %d repetitions alternating "
               "library / torch; median, min, max" % args.reps, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
