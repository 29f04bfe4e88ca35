#!/usr/bin/env python3
"""Ice clusters of whole farms: device-event time of mw_ice_clusters_launch (the two classification passes, then the cluster
pass) and, beside it, of mw_ice_classes_launch of the same build on the same boxes -- each the median of R launches after
warm-up -- for
  512 x 4096 molecules (bench.py's ih4096_t015 walkers: seed 20250228 + walker index), labels and sizes in LDS, and
   64 x 32768 molecules (boxes too large for LDS: labels and sizes in global memory, through L2),
with the default mask (cubic + hexagonal + interfacial ice).  The cluster pass is reported as the difference of the two
entries, next to its own event timer.  Writes profiles/ice_cluster_measurements.json and prints it.  Run on the GPU box:
    python tools/ice_cluster_measurements.py [--reps R] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (one HIP runtime per process: torch's, loaded first)

from mc_water_ls_mw_amd import lattice as lat  # noqa: E402
from mc_water_ls_mw_amd.energy import ICE_CLUSTER_DEFAULT, ice_cluster_mask, ice_clusters_plan, load_boxes  # noqa: E402


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


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
            em.ice_clusters_launch(1, boxes)
            em.ice_classes_launch(1, boxes)
            em.sync()
        base = 3 * reps
        for r in range(reps):                                      # one whole-entry timer and the three per-pass timers
            em.ice_clusters_launch(1, boxes, timer_slot=3 * r)
        em.sync()
        passes = [[em.timer_ms(3 * r + k) for r in range(reps)] for k in range(3)]
        whole = []
        for r in range(reps):
            em.timer_start(base)
            em.ice_clusters_launch(1, boxes)
            em.timer_stop(base)
            whole.append(em.timer_ms(base))
        classes = []
        for r in range(reps):
            em.timer_start(base)
            em.ice_classes_launch(1, boxes)
            em.timer_stop(base)
            classes.append(em.timer_ms(base))
        _, summary = em.ice_clusters_batch(1, boxes)
        last = em.ice_clusters_last()
        plan = ice_clusters_plan(len(xs[0]))
        return {"boxes": boxes, "molecules": int(len(xs[0])), "reps": reps, "mask": ice_cluster_mask(ICE_CLUSTER_DEFAULT),
                "lds_variant": last["lds"], "threads": last["threads"], "lds_bytes": plan["lds_bytes"], "rounds_max": last["rounds"],
                "ice_clusters_launch_ms_median": _median(whole), "ice_clusters_launch_ms_min": min(whole),
                "ice_classes_launch_ms_median": _median(classes), "ice_classes_launch_ms_min": min(classes),
                "cluster_pass_ms_difference": _median(whole) - _median(classes),
                "pass1_ms_median": _median(passes[0]), "pass2_ms_median": _median(passes[1]),
                "cluster_pass_ms_median": _median(passes[2]), "cluster_pass_ms_min": min(passes[2]),
                "selected_total": int(summary[:, 0].sum()), "clusters_total": int(summary[:, 1].sum()),
                "largest_min": int(summary[:, 2].min()), "largest_max": int(summary[:, 2].max())}
    finally:
        em.energy_deinit()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ice_cluster_measurements.json"))
    args = ap.parse_args()
    out = {"tool": "ice_cluster_measurements", "ih4096x512": measure("ih", (8, 8, 8), 512, args.reps)}
    if not ice_clusters_plan(32768)["lds"]:
        out["ih32768x64"] = measure("ih", (16, 16, 16), 64, args.reps)
    text = json.dumps(out)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
