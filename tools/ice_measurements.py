#!/usr/bin/env python3
"""Ice structure classes of whole farms: device-event timing of the two passes of mw_ice_classes_launch -- pass 1
(k_ice_q: bond-order vectors from the slot-major list) and pass 2 (k_ice_class: classes and per-box counts) -- median of
R launches after warm-up, for
  512 x 4096 molecules (bench.py's ih4096_t015 walkers: seed 20250228 + walker index) and
   64 x 32768 molecules (boxes too large for LDS: positions gathered through L2),
next to the plain energy launch of the same boxes.  Prints one JSON line.  Run on the GPU box:
    python tools/ice_measurements.py [--reps R]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (one HIP runtime per process: torch's, loaded first)

from mc_water_ls_mw_amd import lattice as lat  # noqa: E402
from mc_water_ls_mw_amd.energy import load_boxes  # noqa: E402


def measure(kind, reps_cells, boxes, reps):
    h = None
    xs = []
    for b in range(boxes):
        h, x = lat.ice_box(kind, reps_cells, 0.15, seed=20250228 + b)
        xs.append(x)
    em = load_boxes([h] * boxes, xs)
    try:
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.2:                      # warm-up: clocks up, buffers allocated
            em.ice_classes_launch(1, boxes)
            em.sync()
        p1, p2 = [], []
        for r in range(reps):
            em.ice_classes_launch(1, boxes, timer_slot=2 * r)
        em.sync()
        for r in range(reps):
            p1.append(em.timer_ms(2 * r))
            p2.append(em.timer_ms(2 * r + 1))
        em.timer_start(3000)
        for _ in range(reps):
            em.model_energy_launch(1, boxes)
        em.timer_stop(3000)
        plain = em.timer_ms(3000) / reps
        _, counts = em.ice_classes_batch(1, boxes)
        tot = sorted(a + b for a, b in zip(p1, p2))
        p1.sort()
        p2.sort()
        return {"boxes": boxes, "molecules": int(len(xs[0])), "reps": reps,
                "pass1_ms_median": p1[len(p1) // 2], "pass2_ms_median": p2[len(p2) // 2],
                "ice_classes_ms_median": tot[len(tot) // 2], "ice_classes_ms_min": tot[0],
                "plain_energy_ms": plain, "list_entries": int(em.neighbour_total(1, boxes)),
                "class_counts": [int(v) for v in counts.sum(axis=0)]}
    finally:
        em.energy_deinit()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    out = {"tool": "ice_measurements",
           "ih4096x512": measure("ih", (8, 8, 8), 512, args.reps),
           "ih32768x64": measure("ih", (16, 16, 16), 64, args.reps)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
