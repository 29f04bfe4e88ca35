"""Time mw_boo_compute_device (libmw_boo.so) on the three analysis workloads and write profiles/boo_measurements.json:

    ih4096x512    512 boxes of 4096 molecules (ih4096_t015 replicated)     general geometry, several chunks
    ih32768x64    64 boxes of 32768 molecules (ih32768_t015 replicated)    general geometry
    ic48x16384    16 384 boxes of 48 molecules (ic48_t015 replicated)      small geometry, the replica farm's boxes

    python tools/boo_measurements.py [--out FILE] [--reps 50]

Each case runs in a process of its own under its own time limit; per case: the median over `reps` calls, after warm-up, of
the library's event timers (binning, pass 1, pass 2, summary, summed over the chunks of a call), of their sum and of the wall
time of the call, and the ratio to CHILL+ on the same boxes (profiles/ice_measurements.json), which reads a ready-made
neighbour list where bond order finds its neighbours itself.
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

CASES = {"ih4096x512": ("ih4096_t015", 512, 240), "ih32768x64": ("ih32768_t015", 64, 240), "ic48x16384": ("ic48_t015", 16384, 240)}
CHILL = {"ih4096x512": "ih4096x512", "ih32768x64": "ih32768x64"}


def run_case(name, reps):
    import numpy as np
    import torch
    from conftest import load_golden
    from mc_water_ls_mw_amd import bondorder
    golden, boxes, _ = CASES[name]
    z = load_golden(golden)
    dev = torch.device("cuda:0")
    cells = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(z["h"], (boxes, 3, 3)))).to(dev)
    pos = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(z["xyz"], (boxes,) + z["xyz"].shape))).to(dev)
    for _ in range(5):
        q, nn, summary = bondorder.bond_order_torch(cells, pos, 3.5, 0.5)
    parts, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        bondorder.bond_order_torch(cells, pos, 3.5, 0.5)
        wall.append((time.perf_counter() - t0) * 1e3)
        parts.append(bondorder.boo_elapsed_ms())
    parts = np.array(parts)
    med = np.median(parts, axis=0)
    out = {"boxes": boxes, "molecules": int(z["xyz"].shape[0]), "reps": reps, "plan": bondorder.boo_last(),
           "binning_ms_median": float(med[0]), "pass1_ms_median": float(med[1]), "pass2_ms_median": float(med[2]),
           "summary_ms_median": float(med[3]), "kernels_ms_median": float(np.median(parts.sum(axis=1))),
           "kernels_ms_min": float(parts.sum(axis=1).min()), "call_wall_ms_median": float(np.median(wall)),
           "neighbour_entries": int(nn[:, :, 0].sum().item()), "Q6_first_box": float(summary[0, 1].item()),
           "mean_qbar6_first_box": float(summary[0, 3].item())}
    bondorder.boo_finalize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boo_measurements.json"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--case", choices=sorted(CASES))
    args = ap.parse_args()
    if args.case:
        print("RESULT " + json.dumps(run_case(args.case, args.reps)), flush=True)
        return 0
    chill = json.load(open(os.path.join(ROOT, "profiles", "ice_measurements.json")))
    result = {"tool": "boo_measurements"}
    for name, (_, _, limit) in CASES.items():
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps)],
                             capture_output=True, text=True, timeout=limit)
        if res.returncode != 0:
            print(res.stdout[-2000:], res.stderr[-4000:], file=sys.stderr)
            return res.returncode or 1                       # nothing more is started on the device after a failure
        line = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        result[name] = json.loads(line[7:])
        if name in CHILL:
            ref = chill[CHILL[name]]["ice_classes_ms_median"]
            result[name]["chill_plus_ms_median"] = ref
            result[name]["ratio_to_chill_plus"] = result[name]["kernels_ms_median"] / ref
        print(name, json.dumps(result[name]), flush=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
