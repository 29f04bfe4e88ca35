"""Time mw_tet_compute_device (libmw_tet.so) on the three analysis workloads and write profiles/tet_measurements.json:

    ih4096x512    512 boxes of 4096 molecules (ih4096_t015 replicated)     general geometry, several chunks
    ih32768x64    64 boxes of 32768 molecules (ih32768_t015 replicated)    general geometry
    ic48x16384    16 384 boxes of 48 molecules (ic48_t015 replicated)      small geometry, the replica farm's boxes

    python tools/tet_measurements.py [--out FILE] [--reps 50]

Each case runs in a process of its own under its own time limit; per case: the median over `reps` calls, after warm-up, of
the library's event timers (binning, selection, summary, summed over the chunks of a call), of their sum and of the wall
time of the call -- and, measured in the same process on the same boxes, the yardstick: libmw_boo.so's binning and pass 1 at
rc = r_search, the same walk with 22 harmonics in place of a selection (the small geometry of libmw_boo.so is one kernel
that holds both passes, so there the yardstick is an upper bound).
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

CASES = {"ih4096x512": ("ih4096_t015", 512, 300), "ih32768x64": ("ih32768_t015", 64, 300), "ic48x16384": ("ic48_t015", 16384, 300)}
R_SEARCH_ANG, R_LSI_ANG = 5.5, 3.7


def run_case(name, reps):
    import numpy as np
    import torch
    from conftest import load_golden
    from mc_water_ls_mw_amd import bondorder, tetrahedral
    golden, boxes, _ = CASES[name]
    z = load_golden(golden)
    dev = torch.device("cuda:0")
    cells = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(z["h"], (boxes, 3, 3)))).to(dev)
    pos = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(z["xyz"], (boxes,) + z["xyz"].shape))).to(dev)
    for _ in range(5):
        order, near, counts, summary = tetrahedral.tetrahedral_order_torch(cells, pos, R_SEARCH_ANG, R_LSI_ANG)
    parts, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        tetrahedral.tetrahedral_order_torch(cells, pos, R_SEARCH_ANG, R_LSI_ANG)
        wall.append((time.perf_counter() - t0) * 1e3)
        parts.append(tetrahedral.tet_elapsed_ms())
    parts = np.array(parts)
    med = np.median(parts, axis=0)
    c0 = counts[0].cpu().numpy()
    out = {"boxes": boxes, "molecules": int(z["xyz"].shape[0]), "reps": reps, "r_search_ang": R_SEARCH_ANG, "r_lsi_ang": R_LSI_ANG,
           "plan": tetrahedral.tet_last(), "binning_ms_median": float(med[0]), "select_ms_median": float(med[1]),
           "summary_ms_median": float(med[2]), "kernels_ms_median": float(np.median(parts.sum(axis=1))),
           "kernels_ms_min": float(parts.sum(axis=1).min()), "call_wall_ms_median": float(np.median(wall)),
           "entries_per_molecule_first_box": float(c0[:, 0].mean()), "mean_q_first_box": float(summary[0, 0].item()),
           "mean_lsi_bohr2_first_box": float(summary[0, 3].item())}
    tetrahedral.tet_finalize()
    # the yardstick: bond order's binning + pass 1 with rc = r_search on the same boxes
    boo_reps = max(5, reps // 3)
    for _ in range(3):
        bondorder.bond_order_torch(cells, pos, R_SEARCH_ANG, 0.5)
    boo = np.array([(bondorder.bond_order_torch(cells, pos, R_SEARCH_ANG, 0.5), bondorder.boo_elapsed_ms())[1] for _ in range(boo_reps)])
    bmed = np.median(boo, axis=0)
    out.update({"boo_reps": boo_reps, "boo_binning_ms_median": float(bmed[0]), "boo_pass1_ms_median": float(bmed[1]),
                "boo_small_geometry": bool(bondorder.boo_last()["small"])})
    out["select_over_boo_pass1"] = out["select_ms_median"] / out["boo_pass1_ms_median"]
    out["binning_and_select_over_boo_binning_and_pass1"] = (med[0] + med[1]) / (bmed[0] + bmed[1])
    bondorder.boo_finalize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tet_measurements.json"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--case", choices=sorted(CASES))
    args = ap.parse_args()
    if args.case:
        print("RESULT " + json.dumps(run_case(args.case, args.reps)), flush=True)
        return 0
    result = {"tool": "tet_measurements"}
    for name, (_, _, limit) in CASES.items():
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
