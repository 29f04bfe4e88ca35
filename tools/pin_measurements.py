"""Time one step of libmw_pin.so, without a bias (kappa = 0 in every box) and with one, against one step of libmw_flex.so at the
same settings on the same boxes, and write profiles/pin_measurements.json and profiles/pin_summary.md:

    ih1536x64      64 boxes of 1536 molecules (ih1536 shaken with sigma = 0.12 Angstrom, seed 20250228 + box), general geometry
    ic48x4096      4096 boxes of 48 molecules (ic48 shaken with sigma = 0.15 Angstrom, seed 20250228 + box), small geometry

    python tools/pin_measurements.py [--out FILE] [--summary FILE] [--reps 7] [--flex-lib PATH]

Every call runs 20 steps on device tensors from the same positions and velocities, with the thermostat (250 K, gamma = 1 /
(100 fs)), in the coupling `uniaxial` along z at 1 atm with the barostat off and after every tenth step; the bias is on the mode
(0, 0, 6) with kappa = 0.02 Hartree and the anchor at 0.8 of the box's own Q.  The time per step is the sum of the library's event
timers over 21, as in tools/flex_measurements.py.  After two warm-up calls of each, the calls alternate `reps` times; the record
holds the median, the smallest and the largest of each, the ratio of the medians to libmw_flex.so's at the same barostat setting, and
the share of the mode kernel (`rho`) in the biased step.  ``--flex-lib`` loads another build of libmw_flex.so (the parent commit's;
this change leaves its code object as it was, so the tree's own is the parent's).  Each case runs in a process of its own under its
own time limit.  The record also holds the register and LDS figures of every kernel of both libraries, read from the gfx950 code
objects.  No target is set: the ratios are reported, and DESIGN.md 3.20 explains them from the kernels' bytes and launches.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from flex_measurements import CASES, EVALS, STEPS, kernel_resources     # noqa: E402

EVERY = (0, 10)
NVEC, KAPPA, ANCHOR_FRACTION = (0, 0, 6), 0.02, 0.8
PARTS = ("sort", "moments", "forces", "drift", "barostat", "rho")


def run_case(name, reps, flex_lib):
    import numpy as np
    import torch
    from conftest import load_golden
    from mc_water_ls_mw_amd import dynamics, flexcell, lattice as lat, npt, pinning
    if flex_lib:
        flexcell.load_flex_library(os.path.abspath(flex_lib))
    golden, boxes, sigma, _ = CASES[name]
    z = load_golden(golden)
    xs = np.array([lat.thermalise(z["xyz"], sigma, 20250228 + b) for b in range(boxes)])
    hs = np.ascontiguousarray(np.broadcast_to(z["h"], (boxes, 3, 3)))
    n = xs.shape[1]
    dt, kT, gamma = 5.0 * dynamics.FS, 250.0 * dynamics.KELVIN, 1.0 / (100.0 * dynamics.FS)
    dev = torch.device("cuda:0")
    cells, pos = torch.from_numpy(hs).to(dev), torch.from_numpy(xs).to(dev)
    vel = torch.from_numpy(dynamics.maxwell_boltzmann(boxes, n, kT, seed=1)).to(dev)
    nvec = torch.tensor([NVEC] * boxes, dtype=torch.int32, device=dev)
    q0 = pinning.order_parameter(hs, xs, NVEC)
    anchors = torch.from_numpy(ANCHOR_FRACTION * q0).to(dev)
    kappas = {False: torch.zeros(boxes, dtype=torch.float64, device=dev), True: torch.full((boxes,), KAPPA, dtype=torch.float64, device=dev)}
    common = dict(kT=kT, gamma=gamma, coupling="uniaxial", axis=2, seed=3, sample_every=STEPS)

    def run_flex(every):
        out = flexcell.molecular_dynamics_flex_torch(cells, pos, STEPS, dt, npt.ATM, baro_every=every, vel_t=vel, **common)
        assert int(out[6][:, 1].sum()) == 0 and int(out[6][:, 0].min()) == STEPS, "a box froze inside the probe"
        return flexcell.flex_elapsed_ms() + (0.0,)

    def run_pin(every, biased):
        out = pinning.interface_pinning_torch(cells, pos, nvec, kappas[biased], anchors, STEPS, dt, npt.ATM, baro_every=every, vel_t=vel, block_steps=5, **common)
        assert int(out[7][:, 1].sum()) == 0 and int(out[7][:, 0].min()) == STEPS, "a box froze inside the probe"
        return pinning.pin_elapsed_ms()

    runs = {}
    for every in EVERY:
        runs["flex_%d" % every] = lambda every=every: run_flex(every)
        runs["pin_off_%d" % every] = lambda every=every: run_pin(every, False)
        runs["pin_on_%d" % every] = lambda every=every: run_pin(every, True)
    for _ in range(2):
        for f in runs.values():
            f()
    seen = {k: [] for k in runs}
    for _ in range(reps):
        for k, f in runs.items():
            seen[k].append(f())
    out = {"boxes": boxes, "molecules": int(n), "reps": reps, "steps_per_call": STEPS, "q0_mean": float(q0.mean()), "flex_plan": flexcell.flex_last(),
           "pin_plan": pinning.pin_last()}
    for k, rows in seen.items():
        a = np.array(rows) / EVALS
        tot = a.sum(axis=1)
        out[k] = {"ms_median": float(np.median(tot)), "ms_min": float(tot.min()), "ms_max": float(tot.max()),
                  "parts_ms_median": dict(zip(PARTS, (float(v) for v in np.median(a, axis=0))))}
    for every in EVERY:
        for which in ("pin_off", "pin_on"):
            k = "%s_%d" % (which, every)
            out[k]["ratio_to_flex"] = out[k]["ms_median"] / out["flex_%d" % every]["ms_median"]
            out[k]["rho_share"] = out[k]["parts_ms_median"]["rho"] / out[k]["ms_median"]
    pinning.pin_finalize()
    flexcell.flex_finalize()
    return out


def summary(result):
    """The record as a short table."""
    lines = ["# libmw_pin.so against libmw_flex.so: milliseconds per step", "",
             "Written by tools/pin_measurements.py; the figures are profiles/pin_measurements.json's.  Per step = the sum of the library's",
             "event timers of a call of %d steps over %d; medians of %d alternating repetitions; Langevin, coupling `uniaxial` along z, 1 atm."
             % (STEPS, EVALS, result["reps"]),
             "`off / 10`: the barostat never, after every tenth step.  `kappa = 0`: no box is biased; `biased`: every box, mode %s." % (NVEC,),
             "`rho`: the share of the kernel that sums the mode (general geometry; the phasors are formed inside the moment pass).", ""]
    for name in CASES:
        r = result[name]
        lines += ["## %s: %d boxes of %d molecules (%s geometry)" % (name, r["boxes"], r["molecules"], "small" if r["pin_plan"]["small"] else "general"), "",
                  "| barostat | libmw_flex.so | kappa = 0 | ratio | biased | ratio | moments ratio | forces ratio | rho share |", "|---|---|---|---|---|---|---|---|---|"]
        for every in EVERY:
            a, p0, p1 = r["flex_%d" % every], r["pin_off_%d" % every], r["pin_on_%d" % every]
            mom = "%.3f" % (p1["parts_ms_median"]["moments"] / a["parts_ms_median"]["moments"]) if a["parts_ms_median"]["moments"] > 0 else "-"
            lines.append("| %s | %.4f | %.4f | %.3f | %.4f | %.3f | %s | %.3f | %.4f |"
                         % ("off" if every == 0 else every, a["ms_median"], p0["ms_median"], p0["ratio_to_flex"], p1["ms_median"], p1["ratio_to_flex"], mom,
                            p1["parts_ms_median"]["forces"] / a["parts_ms_median"]["forces"], p1["rho_share"]))
        lines.append("")
    lines += ["## Registers", "", "| kernel | VGPRs | SGPRs | SGPR spills | VGPR spills | private bytes | LDS bytes |", "|---|---|---|---|---|---|---|"]
    for lib in ("pin_kernels", "flex_kernels"):
        for k, v in sorted(result[lib].items()):
            if k.startswith("k_cells") and lib == "flex_kernels":
                continue
            lines.append("| %s | %d | %d | %d | %d | %d | %d |" % (k, v["vgprs"], v["sgprs"], v["sgpr_spills"], v["vgpr_spills"], v["private_bytes"], v["lds_bytes"]))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pin_measurements.json"))
    ap.add_argument("--summary", default=os.path.join(ROOT, "profiles", "pin_summary.md"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--flex-lib", default="")
    ap.add_argument("--case", choices=sorted(CASES))
    args = ap.parse_args()
    if args.case:
        print("RESULT " + json.dumps(run_case(args.case, args.reps, args.flex_lib)), flush=True)
        return 0
    from mc_water_ls_mw_amd import build
    result = {"tool": "pin_measurements", "reps": args.reps, "flex_lib": os.path.basename(args.flex_lib) or "libmw_flex.so",
              "pin_kernels": kernel_resources(build.PIN_LIB, "pin"), "flex_kernels": kernel_resources(args.flex_lib or build.FLEX_LIB, "flex")}
    for name, case in CASES.items():
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps), "--flex-lib", args.flex_lib],
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
    with open(args.summary, "w") as fh:
        fh.write(summary(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
