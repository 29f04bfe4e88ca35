"""Time one MD step of libmw_md.so against one FIRE iteration of libmw_quench.so on the same boxes and write
profiles/md_measurements.json:

    ih1536x64      64 boxes of 1536 molecules (ih1536 shaken with sigma = 0.12 Angstrom, seed 20250228 + box), general geometry
    ic48x4096      4096 boxes of 48 molecules (ic48 shaken with sigma = 0.15 Angstrom, seed 20250228 + box), small geometry

    python tools/md_measurements.py [--out FILE] [--reps 7] [--quench-lib PATH]

Both libraries run 21 evaluations per call (max_iter = 20 / nsteps = 20) on device tensors, from the same positions; the time
per iteration or step is the sum of the library's event timers over 21.  After two warm-up calls of each, the calls alternate
(quench, MD at constant energy, MD with the thermostat, and again) `reps` times; the record holds the median, the smallest and
the largest of each.  ``--quench-lib`` loads another build of libmw_quench.so (the parent commit's) for the comparison.
Each case runs in a process of its own under its own time limit.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = {"ih1536x64": ("ih1536", 64, 0.12, 300), "ic48x4096": ("ic48", 4096, 0.15, 300)}     # golden box, boxes, sigma, time limit in seconds
EVALS = 21


def run_case(name, reps, quench_lib):
    import numpy as np
    import torch
    from conftest import load_golden
    from mc_water_ls_mw_amd import dynamics, lattice as lat, quench
    if quench_lib:
        quench.load_quench_library(os.path.abspath(quench_lib))
    golden, boxes, sigma, _ = CASES[name]
    z = load_golden(golden)
    xs = np.array([lat.thermalise(z["xyz"], sigma, 20250228 + b) for b in range(boxes)])
    hs = np.ascontiguousarray(np.broadcast_to(z["h"], (boxes, 3, 3)))
    n = xs.shape[1]
    dt, kT = 5.0 * dynamics.FS, 250.0 * dynamics.KELVIN
    dev = torch.device("cuda:0")
    cells, pos = torch.from_numpy(hs).to(dev), torch.from_numpy(xs).to(dev)
    vel = torch.from_numpy(dynamics.maxwell_boltzmann(boxes, n, kT, seed=1)).to(dev)

    def q():
        _, _, _, iters = quench.inherent_structures_torch(cells, pos, 1e-10, EVALS - 1)
        assert int(iters[:, 1].sum()) == 0, "a box converged inside the probe"
        return quench.quench_elapsed_ms()

    def md(gamma):
        _, _, _, _, status = dynamics.molecular_dynamics_torch(cells, pos, EVALS - 1, dt, kT, gamma, vel_t=vel, seed=3, sample_every=EVALS - 1)
        assert int(status[:, 1].sum()) == 0 and int(status[:, 0].min()) == EVALS - 1, "a box froze inside the probe"
        return dynamics.md_elapsed_ms()

    runs = {"quench": q, "md_nve": lambda: md(0.0), "md_langevin": lambda: md(1.0 / (100.0 * dynamics.FS))}
    for _ in range(2):
        for f in runs.values():
            f()
    seen = {k: [] for k in runs}
    for _ in range(reps):
        for k, f in runs.items():
            seen[k].append(f())
    out = {"boxes": boxes, "molecules": int(n), "reps": reps, "evaluations_per_call": EVALS, "quench_plan": quench.quench_last(), "md_plan": dynamics.md_last()}
    for k, rows in seen.items():
        a = np.array(rows) / EVALS
        tot = a.sum(axis=1)
        parts = ("sort", "moments", "forces", "step" if k == "quench" else "drift")
        out[k] = {"ms_median": float(np.median(tot)), "ms_min": float(tot.min()), "ms_max": float(tot.max()),
                  "parts_ms_median": dict(zip(parts, (float(v) for v in np.median(a, axis=0))))}
    for k in ("md_nve", "md_langevin"):
        out[k]["steps_per_second_per_box"] = 1e3 / out[k]["ms_median"]
        out[k]["box_steps_per_second"] = boxes * 1e3 / out[k]["ms_median"]
    quench.quench_finalize()
    dynamics.md_finalize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "md_measurements.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quench-lib", default="")
    ap.add_argument("--case", choices=sorted(CASES))
    args = ap.parse_args()
    if args.case:
        print("RESULT " + json.dumps(run_case(args.case, args.reps, args.quench_lib)), flush=True)
        return 0
    result = {"tool": "md_measurements", "quench_lib": os.path.basename(args.quench_lib) or "libmw_quench.so"}
    for name, case in CASES.items():
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps), "--quench-lib", args.quench_lib],
                             capture_output=True, text=True, timeout=case[3])
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
