#!/usr/bin/env python3
"""Collective time correlations (libmw_coll.so): the library's event timers of collective_correlations_torch (modes, correlate,
pairs, overlap), the mode pass next to mw_sk_compute_device on the same (frames x boxes) boxes and vectors, and the pair pass
next to mw_rdf_launch on the same boxes, r_max and nbins, in one session, alternating, for
  a:   8 x 4096 molecules (ice Ih 8 x 8 x 8, sigma 0.15 A), 128 frames, about 500 vectors, 64 lags, every 4th frame an origin,
       4 histogram lags, 512 bins, r_max 10 A (one image per pair);
  f: 512 x 48 molecules (thermalised ih48), 256 frames, about 200 vectors, 64 lags, every frame an origin, 4 histogram lags,
     512 bins, r_max 10 A (27 images per pair).
The frames are random walks from the boxes' positions (0.1 A per frame and axis): the work does not depend on what moved the
molecules.  Two warm-up rounds, then --reps rounds; median (smallest ... largest).  Every case runs in a process of its own
under a time limit; the first one that fails ends the run.  Prints one JSON line.  Run on the GPU box:
    python tools/coll_measurements.py [--reps R] [--case a|f]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R_MAX_ANG, NBINS, ANG = 10.0, 512, 0.5291772108
LIMIT_S = {"a": 400, "f": 400}
SHAPES = {"a": dict(frames=128, nlags=64, every=4, hist_lags=(0, 8, 32, 63), m_target=500),
          "f": dict(frames=256, nlags=64, every=1, hist_lags=(0, 8, 32, 63), m_target=200)}


def boxes_of(case):
    import numpy as np
    from mc_water_ls_mw_amd import lattice as lat
    if case == "f":
        z = np.load(os.path.join(ROOT, "tests", "golden", "ih48.npz"), allow_pickle=False)
        return [z["h"]] * 512, [lat.thermalise(z["xyz"], 0.15, 20250228 + b) for b in range(512)]
    h, xs = None, []
    for b in range(8):
        h, x = lat.ice_box("ih", (8, 8, 8), 0.15, seed=20250228 + b)
        xs.append(x)
    return [h] * 8, xs


def vectors(h, m_target):
    import numpy as np
    from mc_water_ls_mw_amd.structure import BOHR_TO_ANG, kvectors
    vol = abs(np.linalg.det(np.asarray(h, dtype=np.float64))) * BOHR_TO_ANG ** 3
    return kvectors(h, (12.0 * np.pi ** 2 * m_target / vol) ** (1.0 / 3.0), half=True)


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def measure(case, reps):
    import numpy as np
    import torch
    from mc_water_ls_mw_amd import collective, structure
    from mc_water_ls_mw_amd.energy import load_boxes
    shape = SHAPES[case]
    hs, xs = boxes_of(case)
    nb, n, T = len(xs), len(xs[0]), shape["frames"]
    cells = np.ascontiguousarray(np.array(hs, dtype=np.float64))
    nvec = np.ascontiguousarray(vectors(hs[0], shape["m_target"]), dtype=np.int32)
    rng = np.random.default_rng(7)
    steps = rng.normal(0.0, 0.1 / ANG, (T, nb, n, 3))
    steps[0] = 0.0
    frames_t = torch.tensor(np.ascontiguousarray(np.array(xs)[None] + np.cumsum(steps, axis=0))).cuda().contiguous()
    r_max = R_MAX_ANG / ANG
    o = collective.n_origins(T, np.array(shape["hist_lags"]), shape["every"])
    em = load_boxes(hs, xs)
    try:
        sk_cells = torch.tensor(np.ascontiguousarray(np.broadcast_to(cells[None], (T, nb, 3, 3)).reshape(T * nb, 3, 3))).cuda()
        sk_pos, nvec_t = frames_t.reshape(T * nb, n, 3), torch.tensor(nvec).cuda()
        rows = {k: [] for k in ("modes", "correlate", "pairs", "overlap", "coll_wall", "sk", "rdf")}
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        gd = None
        for r in range(reps + 2):
            start.record()
            _, fkt, gd, qsum, q2sum = collective.collective_correlations_torch(cells, frames_t, shape["nlags"], shape["every"], nvec, r_max, NBINS,
                                                                               shape["hist_lags"], 1.0 / ANG, ("fkt", "gd", "qsum", "q2sum"))
            stop.record()
            torch.cuda.synchronize()
            ms = collective.coll_elapsed_ms()
            structure.structure_factor_torch(sk_cells, sk_pos, nvec_t)
            sk = sum(structure.sk_elapsed_ms())
            em.rdf_launch(1, nb, R_MAX_ANG, NBINS, timer_slot=0)
            em.sync()
            rdf = em.timer_ms(0)
            if r >= 2:
                for k, v in zip(("modes", "correlate", "pairs", "overlap"), ms):
                    rows[k].append(v)
                rows["coll_wall"].append(start.elapsed_time(stop))
                rows["sk"].append(sk)
                rows["rdf"].append(rdf)
        plan, disp = collective.coll_last(), em.last_dispatch("rdf")
        images = int(disp["images"])
        pair_images = float(nb) * n * n * images * float(o.sum())              # ordered (i, j, image) of every origin of every selected lag
        rdf_images = float(nb) * n * n * images                                # what mw_rdf counts (it evaluates half and counts twice)
        out = {"case": case, "boxes": nb, "molecules": n, "frames": T, "vectors": int(len(nvec)), "nlags": shape["nlags"], "origin_every": shape["every"],
               "hist_lags": list(shape["hist_lags"]), "origins_of_hist_lags": [int(v) for v in o], "nbins": NBINS, "r_max_ang": R_MAX_ANG, "images": images,
               "reps": reps, "ms": {k: stats(v) for k, v in rows.items()}, "plan": plan, "sk_plan": structure.sk_last(), "rdf_dispatch": disp,
               "mode_over_sk": stats(rows["modes"])["median"] / stats(rows["sk"])["median"],
               "pair_images": pair_images, "pair_images_per_s": pair_images / (1e-3 * stats(rows["pairs"])["median"]),
               "rdf_ordered_pair_images": rdf_images, "rdf_ordered_pair_images_per_s": rdf_images / (1e-3 * stats(rows["rdf"])["median"]),
               "gd_counted": int(gd.sum().item()), "fkt0_mean": float(fkt[:, 0].real.mean().item()), "qsum_lag1": int(qsum[:, 1].sum().item())}
        out["pair_rate_over_rdf_rate"] = out["pair_images_per_s"] / out["rdf_ordered_pair_images_per_s"]
        return out
    finally:
        em.energy_deinit()
        collective.coll_finalize()
        structure.sk_finalize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case", choices=("a", "f"))
    args = ap.parse_args()
    if args.case:
        print(json.dumps(measure(args.case, args.reps)))
        return 0
    out = {"tool": "coll_measurements"}
    for case, key in (("a", "ih4096x8"), ("f", "ih48x512")):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(args.reps)], capture_output=True, text=True,
                               timeout=LIMIT_S[case])
        except subprocess.TimeoutExpired:
            out[key] = {"failed": "time limit"}
            print(json.dumps(out))
            return 1
        if p.returncode != 0:
            out[key] = {"failed": p.returncode, "stderr": p.stderr[-2000:]}
            print(json.dumps(out))
            return 1
        out[key] = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
