#!/usr/bin/env python3
"""Pair-distance histograms of whole farms: device-event timing of mw_rdf_launch (r_max = 10 Angstrom, 200 bins), median of
R launches after warm-up, for
  a: 512 x 4096 molecules (bench.py's ih4096_t015 walkers: seed 20250228 + walker index), one image per pair,
  b:  64 x 32768 molecules,
  c: 16384 x 48 molecules (the replica farm's boxes: thermalised ih48, 27 images per pair), and next to it what a user did
     before: mw_download_positions_range + the numpy reference (tests/rdf_ref.py, rdf_fast) on 16 threads, timed on the
     first --cpu-boxes boxes and scaled to all of them,
each next to the plain energy launch of the same boxes.  Every case runs in a process of its own under a time limit; the
first one that fails ends the run.  Prints one JSON line.  Run on the GPU box:
    python tools/rdf_measurements.py [--reps R] [--case a|b|c]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R_MAX_ANG, NBINS = 10.0, 200
LIMIT_S = {"a": 240, "b": 240, "c": 300}


def boxes_of(case):
    import numpy as np
    from mc_water_ls_mw_amd import lattice as lat
    if case == "c":
        z = np.load(os.path.join(ROOT, "tests", "golden", "ih48.npz"), allow_pickle=False)
        n = 16384
        return [z["h"]] * n, [lat.thermalise(z["xyz"], 0.15, 20250228 + b) for b in range(n)]
    kind, cells, n = ("ih", (8, 8, 8), 512) if case == "a" else ("ih", (16, 16, 16), 64)
    h, xs = None, []
    for b in range(n):
        h, x = lat.ice_box(kind, cells, 0.15, seed=20250228 + b)
        xs.append(x)
    return [h] * n, xs


def cpu_baseline(em, hs, nboxes):
    """Download + rdf_fast of the first nboxes boxes on 16 threads: seconds."""
    import ctypes
    from concurrent.futures import ThreadPoolExecutor
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from rdf_ref import ANG_TO_BOHR, rdf_fast
    t0 = time.perf_counter()
    xyz = np.zeros((nboxes, em.nwater, 3))
    em._chk(em.L.mw_download_positions_range(1, nboxes, xyz.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    t1 = time.perf_counter()
    with ThreadPoolExecutor(16) as pool:
        hists = list(pool.map(lambda b: rdf_fast(hs[b], xyz[b], R_MAX_ANG * ANG_TO_BOHR, NBINS)[0], range(nboxes)))
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, np.array(hists)


def measure(case, reps, cpu_boxes):
    import numpy as np
    import torch  # noqa: F401  (one HIP runtime per process: torch's, loaded first)
    from mc_water_ls_mw_amd.energy import load_boxes
    hs, xs = boxes_of(case)
    boxes = len(xs)
    em = load_boxes(hs, xs)
    try:
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.2:                      # warm-up: clocks up, buffers allocated
            em.rdf_launch(1, boxes, R_MAX_ANG, NBINS)
            em.sync()
        ms = []
        for r in range(reps):
            em.rdf_launch(1, boxes, R_MAX_ANG, NBINS, timer_slot=r)
        em.sync()
        ms = sorted(em.timer_ms(r) for r in range(reps))
        disp = em.last_dispatch("rdf")
        em.timer_start(3000)
        for _ in range(reps):
            em.model_energy_launch(1, boxes)
        em.timer_stop(3000)
        plain = em.timer_ms(3000) / reps
        t0 = time.perf_counter()
        hist = em.rdf_counts_batch(1, boxes, R_MAX_ANG, NBINS)
        wall = time.perf_counter() - t0
        n = int(len(xs[0]))
        tiles = -(-n // 256)
        evals = boxes * (n * (n // 2 + 1) if disp["small"] else 256 * 256 * (tiles * (tiles + 1) // 2))
        out = {"case": case, "boxes": boxes, "molecules": n, "reps": reps, "r_max_ang": R_MAX_ANG, "nbins": NBINS,
               "rdf_ms_median": ms[len(ms) // 2], "rdf_ms_min": ms[0], "rdf_batch_with_copy_back_wall_ms": 1e3 * wall,
               "plain_energy_ms": plain, "dispatch": disp, "pair_evaluations": int(evals),
               "image_evaluations": int(evals) * disp["images"], "counted_ordered_pairs": int(hist.sum()),
               "first_peak_ang": float((np.argmax(hist.sum(axis=0)[:80]) + 0.5) * R_MAX_ANG / NBINS)}
        if case == "c" and cpu_boxes > 0:
            dl, cpu, ref = cpu_baseline(em, hs, cpu_boxes)
            out.update({"cpu_boxes_timed": cpu_boxes, "cpu_download_s": dl, "cpu_rdf_fast_16_threads_s": cpu,
                        "cpu_all_boxes_s_scaled": (dl + cpu) * boxes / cpu_boxes,
                        "cpu_equals_device": bool(np.array_equal(ref, hist[:cpu_boxes]))})
        return out
    finally:
        em.energy_deinit()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--case", choices=("a", "b", "c"))
    ap.add_argument("--cpu-boxes", type=int, default=1024)
    args = ap.parse_args()
    if args.case:
        print(json.dumps(measure(args.case, args.reps, args.cpu_boxes)))
        return 0
    out = {"tool": "rdf_measurements"}
    for case, key in (("a", "ih4096x512"), ("b", "ih32768x64"), ("c", "ih48x16384")):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(args.reps),
                                "--cpu-boxes", str(args.cpu_boxes)], capture_output=True, text=True, timeout=LIMIT_S[case])
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
