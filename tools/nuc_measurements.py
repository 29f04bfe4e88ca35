"""Time one step of libmw_nuc.so between checks against one step of libmw_flex.so at the same settings on the same boxes, and one
evaluation of the order parameter, and write profiles/nuc_measurements.json and profiles/nuc_summary.md:

    ih4096x64      64 boxes of ih4096_t015 (4096 molecules; the cluster labels live in LDS)
    ih32768x8      8 boxes of ih32768_t015 (32768 molecules; the cluster labels live in global memory)

    python tools/nuc_measurements.py [--out FILE] [--summary FILE] [--reps 5]

Every call runs 20 steps on device tensors from the same positions and velocities, with the thermostat (250 K, gamma = 1 /
(100 fs)), in the coupling `uniaxial` along z at 1 atm with the barostat after every tenth step; libmw_nuc.so with check_every =
nsteps and both bounds disabled, so that it evaluates the order parameter twice, at entry and on the final state, and runs the
kernels of libmw_flex.so in between.  The time per step is the sum of the five event timers the libraries share over 21
evaluations, as in tools/flex_measurements.py (in libmw_nuc.so the stage 1 that the entry check defers counts as drift); the time
of one evaluation is (order + clusters) / 2 from mw_nuc_elapsed_ms.  After two warm-up calls of each, the calls alternate `reps`
times; the record holds the median, the smallest and the largest of each, the ratio of the medians, whether libmw_nuc.so's median
lies inside libmw_flex.so's smallest .. largest, one evaluation in units of a step, and the hook / compress rounds per evaluation
(of the call's first box).  Each case runs in a process of its own under its own time limit.  No target is set for the evaluation.
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

CASES = {"ih4096x64": ("ih4096_t015", 64, 300), "ih32768x8": ("ih32768_t015", 8, 300)}     # golden box, boxes, time limit in seconds
STEPS = 20
EVALS = STEPS + 1
EVERY = 10
PARTS = ("sort", "moments", "forces", "drift", "barostat", "order", "clusters")


def run_case(name, reps):
    import numpy as np
    import torch
    from conftest import load_golden
    from mc_water_ls_mw_amd import dynamics, flexcell, npt, nucleation
    golden, boxes, _ = CASES[name]
    z = load_golden(golden)
    xs = np.ascontiguousarray(np.broadcast_to(z["xyz"], (boxes,) + z["xyz"].shape))
    hs = np.ascontiguousarray(np.broadcast_to(z["h"], (boxes, 3, 3)))
    n = xs.shape[1]
    dt, kT, gamma = 5.0 * dynamics.FS, 250.0 * dynamics.KELVIN, 1.0 / (100.0 * dynamics.FS)
    dev = torch.device("cuda:0")
    cells, pos = torch.from_numpy(hs).to(dev), torch.from_numpy(xs).to(dev)
    vel = torch.from_numpy(dynamics.maxwell_boltzmann(boxes, n, kT, seed=1)).to(dev)
    lo = torch.full((boxes,), -1, dtype=torch.int32, device=dev)
    hi = torch.full((boxes,), n + 1, dtype=torch.int32, device=dev)
    common = dict(kT=kT, gamma=gamma, coupling="uniaxial", axis=2, seed=3, sample_every=STEPS, baro_every=EVERY, vel_t=vel)
    ops = []

    def run_flex():
        out = flexcell.molecular_dynamics_flex_torch(cells, pos, STEPS, dt, npt.ATM, **common)
        assert int(out[6][:, 1].sum()) == 0 and int(out[6][:, 0].min()) == STEPS, "a box froze inside the probe"
        return flexcell.flex_elapsed_ms() + (0.0, 0.0), 0

    def run_nuc():
        out = nucleation.nucleus_md_torch(cells, pos, STEPS, dt, lo, hi, check_every=STEPS, pressure=npt.ATM, **common)
        assert int(out[6][:, 1].sum()) == 0 and int(out[6][:, 0].min()) == STEPS, "a box froze inside the probe"
        ops.append(out[9][0].cpu().numpy().tolist())
        return nucleation.nuc_elapsed_ms(), nucleation.nuc_last()["cluster_rounds"]

    runs = {"flex": run_flex, "nuc": run_nuc}
    for _ in range(2):
        for f in runs.values():
            f()
    seen = {k: [] for k in runs}
    rounds = []
    for _ in range(reps):
        for k, f in runs.items():
            t, r = f()
            seen[k].append(t)
            if k == "nuc":
                rounds.append(r)
    out = {"boxes": boxes, "molecules": int(n), "reps": reps, "steps_per_call": STEPS, "flex_plan": flexcell.flex_last(), "nuc_plan": nucleation.nuc_last(),
           "op_of_box_0": ops[-1], "rounds_per_evaluation": float(np.median(rounds)) / 2.0}
    for k, rows in seen.items():
        a = np.array(rows)
        step = a[:, :5].sum(axis=1) / EVALS
        out[k] = {"ms_median": float(np.median(step)), "ms_min": float(step.min()), "ms_max": float(step.max()),
                  "parts_ms_median": dict(zip(PARTS, (float(v) for v in np.median(a / EVALS, axis=0))))}
    ev = np.array(seen["nuc"])[:, 5:] / 2.0
    out["evaluation"] = {"ms_median": float(np.median(ev.sum(axis=1))), "ms_min": float(ev.sum(axis=1).min()), "ms_max": float(ev.sum(axis=1).max()),
                         "order_ms_median": float(np.median(ev[:, 0])), "clusters_ms_median": float(np.median(ev[:, 1]))}
    out["step_ratio_to_flex"] = out["nuc"]["ms_median"] / out["flex"]["ms_median"]
    out["nuc_median_inside_flex_spread"] = bool(out["flex"]["ms_min"] <= out["nuc"]["ms_median"] <= out["flex"]["ms_max"])
    out["evaluation_in_steps"] = out["evaluation"]["ms_median"] / out["flex"]["ms_median"]
    nucleation.nuc_finalize()
    flexcell.flex_finalize()
    return out


def summary(result):
    """The record as a short table."""
    lines = ["# libmw_nuc.so against libmw_flex.so: milliseconds per step, and one evaluation of the order parameter", "",
             "Written by tools/nuc_measurements.py; the figures are profiles/nuc_measurements.json's.  Per step = the sum of the five event",
             "timers the libraries share over a call of %d steps, over %d evaluations; medians (smallest .. largest) of %d alternating"
             % (STEPS, EVALS, result["reps"]),
             "repetitions; Langevin, coupling `uniaxial` along z, 1 atm, the barostat after every tenth step; check_every = nsteps, bounds",
             "disabled.  One evaluation = (order + clusters) / 2 of mw_nuc_elapsed_ms.  Rounds: hook / compress rounds per evaluation, first box.", "",
             "| case | labels | libmw_flex.so step | libmw_nuc.so step | ratio | inside flex's spread | evaluation | order | clusters | in steps | rounds |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for name in CASES:
        r = result[name]
        a, p, e = r["flex"], r["nuc"], r["evaluation"]
        lines.append("| %s: %d x %d | %s | %.4f (%.4f .. %.4f) | %.4f (%.4f .. %.4f) | %.3f | %s | %.4f | %.4f | %.4f | %.2f | %.1f |"
                     % (name, r["boxes"], r["molecules"], "LDS" if r["nuc_plan"]["labels_in_lds"] else "global", a["ms_median"], a["ms_min"], a["ms_max"],
                        p["ms_median"], p["ms_min"], p["ms_max"], r["step_ratio_to_flex"], "yes" if r["nuc_median_inside_flex_spread"] else "no",
                        e["ms_median"], e["order_ms_median"], e["clusters_ms_median"], r["evaluation_in_steps"], r["rounds_per_evaluation"]))
    lines += ["", "## Parts of a step, milliseconds (medians)", "", "| case | library | " + " | ".join(PARTS[:5]) + " |", "|---|---|---|---|---|---|---|"]
    for name in CASES:
        for lib in ("flex", "nuc"):
            q = result[name][lib]["parts_ms_median"]
            lines.append("| %s | %s | %s |" % (name, lib, " | ".join("%.4f" % q[k] for k in PARTS[:5])))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nuc_measurements.json"))
    ap.add_argument("--summary", default=os.path.join(ROOT, "profiles", "nuc_summary.md"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case", choices=sorted(CASES))
    args = ap.parse_args()
    if args.case:
        print("RESULT " + json.dumps(run_case(args.case, args.reps)), flush=True)
        return 0
    result = {"tool": "nuc_measurements", "reps": args.reps}
    for name, case in CASES.items():
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps)], capture_output=True, text=True, timeout=case[2])
        if res.returncode != 0:
            print(res.stdout[-2000:], res.stderr[-4000:], file=sys.stderr)
            return res.returncode or 1                       # nothing more is started on the device after a failure
        line = [ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")][-1]
        result[name] = json.loads(line[7:])
        print(name, json.dumps(result[name]), flush=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    with open(args.summary, "w") as fh:
        fh.write(summary(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
