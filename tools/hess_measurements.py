"""Times libmw_hess.so on device tensors with the library's own event timers (phonons.hess_elapsed_ms): the products H v
beside a single-point force evaluation of the same boxes by libmw_quench.so (max_iter = 0, quench.quench_elapsed_ms), and the
dense assembly as bytes of matrix written per second.  Two warm-up calls, then seven repetitions of each, alternating where two
libraries are compared; median with smallest and largest.  Writes one JSON document, profiles/hess_measurements.json by
default.

    python tools/hess_measurements.py [--out FILE] [--reps 7] [--small]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

MATVEC = (dict(name="512 boxes x 4096 molecules, 4 vectors", reps=(8, 8, 8), nboxes=512, nvec=4),
          dict(name="1 box x 4096 molecules, 64 vectors", reps=(8, 8, 8), nboxes=1, nvec=64))
DENSE = (dict(name="64 boxes x 1536 molecules", reps=(8, 6, 4), nboxes=64), dict(name="1 box x 4096 molecules", reps=(8, 8, 8), nboxes=1))
SMALL_MATVEC = (dict(name="3 boxes x 96 molecules, 5 vectors", reps=(3, 2, 2), nboxes=3, nvec=5),)
SMALL_DENSE = (dict(name="3 boxes x 96 molecules", reps=(3, 2, 2), nboxes=3),)
COPY_CEILING = 5.2e12                                                   # bytes / s, the copy rate DESIGN.md holds kernels against


def boxes(reps, nboxes, dev):
    """nboxes thermal Ih boxes (sigma = 0.12 Angstrom), eight distinct ones repeated, as device tensors."""
    from mc_water_ls_mw_amd import lattice as lat
    made = [lat.ice_box("ih", reps, 0.12, seed=500 + k) for k in range(min(nboxes, 8))]
    hs = np.array([made[b % len(made)][0] for b in range(nboxes)])
    xs = np.array([made[b % len(made)][1] for b in range(nboxes)])
    return torch.from_numpy(hs).to(dev), torch.from_numpy(xs).to(dev)


def stats(ms):
    s = sorted(ms)
    return dict(median_ms=s[len(s) // 2], min_ms=s[0], max_ms=s[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "hess_measurements.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--small", action="store_true", help="tiny shapes, to try the script")
    args = ap.parse_args()
    from mc_water_ls_mw_amd.phonons import hess_elapsed_ms, hess_finalize, hess_last, hessian_matvec_torch, hessian_torch
    from mc_water_ls_mw_amd.quench import inherent_structures_torch, quench_elapsed_ms, quench_finalize
    dev = torch.device("cuda", 0)
    rows = []
    for shape in (SMALL_MATVEC if args.small else MATVEC):
        ct, pt = boxes(shape["reps"], shape["nboxes"], dev)
        nb, n, nvec = pt.shape[0], pt.shape[1], shape["nvec"]
        gen = torch.Generator(device=dev).manual_seed(11)
        vt = torch.randn((nb, nvec, n, 3), dtype=torch.float64, device=dev, generator=gen)
        for _ in range(2):
            out, ef = hessian_matvec_torch(ct, pt, vt)
            _, _, st, _ = inherent_structures_torch(ct, pt, 1e-10, 0)
        assert bool(torch.isfinite(out).all()) and float((ef[:, 0] - st[:, 1]).abs().max()) <= 1e-10 * float(st[:, 1].abs().max())
        t_h, t_q = [], []
        for _ in range(args.reps):
            hessian_matvec_torch(ct, pt, vt)
            t_h.append(hess_elapsed_ms())
            inherent_structures_torch(ct, pt, 1e-10, 0)
            t_q.append(quench_elapsed_ms())
        apply_ms = stats([t[2] for t in t_h])
        first_ms = stats([t[1] for t in t_h])                            # the moment pass with the forces behind ef
        force_ms = stats([t[1] + t[2] for t in t_q])                     # the quench library's moment and force passes
        row = dict(kind="matvec", shape=shape["name"], nboxes=nb, nwater=n, nvec=nvec, plan=hess_last(), sort_ms=stats([t[0] for t in t_h]),
                   moments_and_forces_ms=first_ms, apply_ms=apply_ms, apply_ms_per_vector=apply_ms["median_ms"] / nvec,
                   quench_sort_ms=stats([t[0] for t in t_q]), quench_moments_and_forces_ms=force_ms,
                   vector_over_force_evaluation=apply_ms["median_ms"] / nvec / force_ms["median_ms"])
        print(json.dumps(row), flush=True)
        rows.append(row)
        del vt, out
        torch.cuda.empty_cache()
    for shape in (SMALL_DENSE if args.small else DENSE):
        ct, pt = boxes(shape["reps"], shape["nboxes"], dev)
        nb, n = pt.shape[0], pt.shape[1]
        for _ in range(2):
            H, ef = hessian_torch(ct, pt)
        asym = float((H[0] - H[0].T).abs().max())
        t_h = []
        for _ in range(args.reps):
            H, ef = hessian_torch(ct, pt)
            t_h.append(hess_elapsed_ms())
        asm = stats([t[3] for t in t_h])
        nbytes = 72 * n * n * nb
        row = dict(kind="dense", shape=shape["name"], nboxes=nb, nwater=n, plan=hess_last(), sort_ms=stats([t[0] for t in t_h]),
                   moments_and_forces_ms=stats([t[1] for t in t_h]), assemble_ms=asm, matrix_bytes=nbytes,
                   bytes_per_s=nbytes / (asm["median_ms"] * 1e-3), fraction_of_copy_ceiling=nbytes / (asm["median_ms"] * 1e-3) / COPY_CEILING,
                   asymmetry_of_first_box=asym)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del H
        torch.cuda.empty_cache()
    hess_finalize()
    quench_finalize()
    doc = dict(device=torch.cuda.get_device_name(0), method="the libraries' event timers after 2 warm-up calls, %d repetitions, hess and quench "
               "alternating; median, min, max" % args.reps, copy_ceiling_bytes_per_s=COPY_CEILING, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
