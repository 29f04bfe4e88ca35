"""Time mw_adf_compute_device (libmw_adf.so) on the bench workload's shape and write profiles/adf_measurements.json:

    ih4096x512 at r_cut = 3.5 Angstrom    512 boxes of 4096 molecules (ih4096_t015 replicated), the first shell
    ih4096x512 at r_cut = 4.8 Angstrom    the same boxes, the second shell (16 - 20 entries per molecule)

    python tools/adf_measurements.py [--out FILE] [--reps 30]

Each case runs in a process of its own under its own time limit; per case: the median over `reps` calls, after warm-up, of
the library's event timers (binning, angles, reduce, summed over the chunks of a call), of their sum and of the wall time of
the call -- and, measured in the same process on the same boxes, the yardstick: libmw_tet.so's binning and selection pass at
r_search = r_lsi = r_cut, the only other kernel that walks the same grid in the same order (it ranks the entries where this
one pairs them).  The two libraries alternate call by call, so both see the same machine.
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

CASES = {"ih4096x512_r3.5": ("ih4096_t015", 512, 3.5, 300), "ih4096x512_r4.8": ("ih4096_t015", 512, 4.8, 300)}
NBINS = 90


def run_case(name, reps):
    import numpy as np
    import torch
    from conftest import load_golden
    from mc_water_ls_mw_amd import angles, tetrahedral
    golden, boxes, r_ang, _ = CASES[name]
    z = load_golden(golden)
    dev = torch.device("cuda:0")
    cells = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(z["h"], (boxes, 3, 3)))).to(dev)
    pos = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(z["xyz"], (boxes,) + z["xyz"].shape))).to(dev)
    edges = angles.adf_edges(NBINS, "theta")
    for _ in range(3):
        hist, counts, summary = angles.angle_counts_torch(cells, pos, r_ang, edges)
        tetrahedral.tetrahedral_order_torch(cells, pos, r_ang, r_ang)
    adf, tet, wall = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        angles.angle_counts_torch(cells, pos, r_ang, edges)
        wall.append((time.perf_counter() - t0) * 1e3)
        adf.append(angles.adf_elapsed_ms())
        tetrahedral.tetrahedral_order_torch(cells, pos, r_ang, r_ang)
        tet.append(tetrahedral.tet_elapsed_ms())
    adf, tet = np.array(adf), np.array(tet)
    med, tmed = np.median(adf, axis=0), np.median(tet, axis=0)
    s0 = summary[0, 0].cpu().numpy()
    out = {"boxes": boxes, "molecules": int(z["xyz"].shape[0]), "reps": reps, "r_cut_ang": r_ang, "nbins": NBINS, "ngroups": 1,
           "plan": angles.adf_last(), "binning_ms_median": float(med[0]), "angles_ms_median": float(med[1]),
           "reduce_ms_median": float(med[2]), "kernels_ms_median": float(np.median(adf.sum(axis=1))),
           "kernels_ms_min": float(adf.sum(axis=1).min()), "angles_ms_min": float(adf[:, 1].min()), "angles_ms_max": float(adf[:, 1].max()),
           "call_wall_ms_median": float(np.median(wall)),
           "entries_per_molecule_first_box": float(counts[0].cpu().numpy().mean()), "pairs_per_box": int(s0[1]),
           "pairs_binned_first_box": int(s0[2]), "centres_over_the_cap_first_box": int(s0[3]),
           "tet_plan": tetrahedral.tet_last(), "tet_binning_ms_median": float(tmed[0]), "tet_select_ms_median": float(tmed[1]),
           "tet_select_ms_min": float(tet[:, 1].min()), "tet_select_ms_max": float(tet[:, 1].max())}
    out["angles_over_tet_select"] = out["angles_ms_median"] / out["tet_select_ms_median"]
    out["binning_and_angles_over_tet_binning_and_select"] = float((med[0] + med[1]) / (tmed[0] + tmed[1]))
    angles.adf_finalize()
    tetrahedral.tet_finalize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adf_measurements.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--case", choices=sorted(CASES))
    args = ap.parse_args()
    if args.case:
        print("RESULT " + json.dumps(run_case(args.case, args.reps)), flush=True)
        return 0
    result = {"tool": "adf_measurements"}
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
