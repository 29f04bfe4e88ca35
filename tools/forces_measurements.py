#!/usr/bin/env python3
"""Forces and virial of whole farms: device-event timing of the two passes of mw_model_forces_launch -- the moment-writing
full-box energy pass and the force pass (k_model_forces + k_sum_virial) -- after warm-up, for
  512 x 4096 molecules (bench.py's ih4096_t015 walkers: seed 20250228 + walker index) and
   64 x 32768 molecules (boxes too large for LDS: positions gathered through L2),
next to the plain energy launch of the same boxes.  Prints one JSON line.  Run on the GPU box:
    python tools/forces_measurements.py [--reps R]
Its kernel-level companion is a separate run under rocprofv3 --kernel-trace --stats."""
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
            em.forces_launch(1, boxes)
            em.sync()
        mom, frc = [], []
        for r in range(reps):
            em.forces_launch(1, boxes, 2 * r)
        em.sync()
        for r in range(reps):
            mom.append(em.timer_ms(2 * r))
            frc.append(em.timer_ms(2 * r + 1))
        em.timer_start(3000)
        for _ in range(reps):
            em.model_energy_launch(1, boxes)
        em.timer_stop(3000)
        plain = em.timer_ms(3000) / reps
        npairs, ntrip = em.model_energy_counts_total(1, boxes)
        entries = em.neighbour_total(1, boxes)
        mom.sort()
        frc.sort()
        tot = sorted(m + f for m, f in zip(mom, frc))
        return {"boxes": boxes, "molecules": int(len(xs[0])), "reps": reps,
                "moment_pass_ms_median": mom[len(mom) // 2], "force_pass_ms_median": frc[len(frc) // 2],
                "forces_virial_ms_median": tot[len(tot) // 2], "forces_virial_ms_min": tot[0],
                "plain_energy_ms": plain, "in_range_entries": int(npairs), "triplets": int(ntrip), "list_entries": int(entries)}
    finally:
        em.energy_deinit()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    out = {"tool": "forces_measurements",
           "ih4096x512": measure("ih", (8, 8, 8), 512, args.reps),
           "ih32768x64": measure("ih", (16, 16, 16), 64, args.reps)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
