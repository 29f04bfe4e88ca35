"""Time mw_rings_compute_device (libmw_rings.so) on the bench workload's shape and write profiles/rings_measurements.json:

    ih4096x512 at r_cut = 3.5 Angstrom    512 boxes of 4096 molecules (ih4096_t015 replicated), the first shell

    python tools/rings_measurements.py [--out FILE] [--reps 30]

The case runs in a process of its own under its own time limit: the median over `reps` calls, after warm-up, of the library's
event timers (binning, adjacency, walk, summed over the chunks of a call), of their sum and of the wall time of the call --
and, measured in the same process on the same boxes, the yardstick: libmw_adf.so's angle pass at the same radius, which
walks the same grid in the same order as the adjacency pass.  The two libraries alternate call by call, so both see the same
machine.  No list is asked for (list_cap = 0): the walk runs once.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = {"ih4096x512_r3.5": ("ih4096_t015", 512, 3.5, 420)}


def run_case(name, reps):
    import numpy as np
    import torch
    from conftest import load_golden
    from mc_water_ls_mw_amd import angles, rings
    golden, boxes, r_ang, _ = CASES[name]
    z = load_golden(golden)
    dev = torch.device("cuda:0")
    cells = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(z["h"], (boxes, 3, 3)))).to(dev)
    pos = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(z["xyz"], (boxes,) + z["xyz"].shape))).to(dev)
    edges = angles.adf_edges(90, "theta")
    for _ in range(3):
        hist, closed, member, counts, summary, _ = rings.ring_statistics_torch(cells, pos, r_ang)
        angles.angle_counts_torch(cells, pos, r_ang, edges)
    ring, adf, wall = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        rings.ring_statistics_torch(cells, pos, r_ang)
        wall.append((time.perf_counter() - t0) * 1e3)
        ring.append(rings.rings_elapsed_ms())
        angles.angle_counts_torch(cells, pos, r_ang, edges)
        adf.append(angles.adf_elapsed_ms())
    ring, adf = np.array(ring), np.array(adf)
    med, amed = np.median(ring, axis=0), np.median(adf, axis=0)
    out = {"boxes": boxes, "molecules": int(z["xyz"].shape[0]), "reps": reps, "r_cut_ang": r_ang, "list_cap": 0,
           "plan": rings.rings_last(), "binning_ms_median": float(med[0]), "adjacency_ms_median": float(med[1]),
           "walk_ms_median": float(med[2]), "kernels_ms_median": float(np.median(ring.sum(axis=1))),
           "kernels_ms_min": float(ring.sum(axis=1).min()), "adjacency_ms_min": float(ring[:, 1].min()),
           "adjacency_ms_max": float(ring[:, 1].max()), "walk_ms_min": float(ring[:, 2].min()), "walk_ms_max": float(ring[:, 2].max()),
           "call_wall_ms_median": float(np.median(wall)),
           "hist_first_box": hist[0].cpu().numpy().tolist(), "closed_first_box": closed[0].cpu().numpy().tolist(),
           "summary_first_box": summary[0].cpu().numpy().tolist(), "entries_per_molecule_first_box": float(counts[0].cpu().numpy().mean()),
           "adf_plan": angles.adf_last(), "adf_binning_ms_median": float(amed[0]), "adf_angles_ms_median": float(amed[1]),
           "adf_angles_ms_min": float(adf[:, 1].min()), "adf_angles_ms_max": float(adf[:, 1].max())}
    out["adjacency_over_adf_angles"] = out["adjacency_ms_median"] / out["adf_angles_ms_median"]
    out["walk_over_adf_angles"] = out["walk_ms_median"] / out["adf_angles_ms_median"]
    rings.rings_finalize()
    angles.adf_finalize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rings_measurements.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--case", choices=sorted(CASES))
    args = ap.parse_args()
    if args.case:
        print("RESULT " + json.dumps(run_case(args.case, args.reps)), flush=True)
        return 0
    result = {"tool": "rings_measurements"}
    for name, (_, _, _, limit) in CASES.items():
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps)],
                             capture_output=True, text=True, timeout=limit)
        if res.returncode != 0:
            print(res.stdout[-2000:], res.stderr[-4000:], file=sys.stderr)
            return res.returncode or 1                       # nothing more is started on the device after a failure
        line = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        result[name] = json.loads(line[7:])
        print(name, json.dumps(result[name]), flush=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
