"""Time mw_quench_compute_device (libmw_quench.so) on the two shapes the library is for and write
profiles/quench_measurements.json:

    ih4096x512     512 boxes of 4096 molecules (bench.py's ih4096_t015 walkers: seed 20250228 + walker index), general geometry
    ic48x16384     16 384 boxes of 48 molecules (ic48 shaken with sigma = 0.15 Angstrom, seed 20250228 + box), small geometry

    python tools/quench_measurements.py [--out FILE] [--reps 5]

Each case runs in a process of its own under its own time limit and records
  - the time per iteration and its split over sort, moment pass, force pass and step: the library's event timers of a call with
    max_iter = 20 (21 evaluations, 20 steps; no box of either shape converges that early), the median over `reps` calls,
    divided by 21;
  - the whole quench to ftol 1e-6 and to 1e-10: wall time of the call, the timers and the iterations the boxes took;
  - beside those the yardstick of one iteration's force evaluation: the engine's forces_launch on the same boxes (its two
    passes over Verlet lists), the median of the event timers over 20 launches, measured first in the same process and the
    engine shut down before the library starts;
  - the numpy mirror's CPU time (tests/quench_ref.py): seconds per evaluation of one box, and for the 48-molecule shape the
    whole quench of one box to 1e-10.
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

CASES = {"ih4096x512": (512, 900), "ic48x16384": (16384, 600)}     # boxes, time limit in seconds
PROBE_ITERS = 20


def make_boxes(name, boxes):
    import numpy as np
    from mc_water_ls_mw_amd import lattice as lat
    if name == "ih4096x512":
        xs = []
        for b in range(boxes):
            h, x = lat.ice_box("ih", (8, 8, 8), 0.15, seed=20250228 + b)
            xs.append(x)
        return np.ascontiguousarray(np.broadcast_to(h, (boxes, 3, 3))), np.array(xs)
    from conftest import load_golden
    z = load_golden("ic48")
    xs = np.array([lat.thermalise(z["xyz"], 0.15, 20250228 + b) for b in range(boxes)])
    return np.ascontiguousarray(np.broadcast_to(z["h"], (boxes, 3, 3))), xs


def engine_forces_ms(hs, xs, launches=20):
    from mc_water_ls_mw_amd.energy import load_boxes
    boxes = len(xs)
    em = load_boxes(list(hs), list(xs))
    try:
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.2:                      # warm-up: clocks up, buffers allocated
            em.forces_launch(1, boxes)
            em.sync()
        for r in range(launches):
            em.forces_launch(1, boxes, 2 * r)
        em.sync()
        mom = sorted(em.timer_ms(2 * r) for r in range(launches))
        frc = sorted(em.timer_ms(2 * r + 1) for r in range(launches))
        return {"moment_pass_ms_median": mom[launches // 2], "force_pass_ms_median": frc[launches // 2]}
    finally:
        em.energy_deinit()


def run_case(name, reps):
    import numpy as np
    import torch
    import quench_ref
    from mc_water_ls_mw_amd import quench
    boxes, _ = CASES[name]
    hs, xs = make_boxes(name, boxes)
    out = {"boxes": boxes, "molecules": int(xs.shape[1]), "reps": reps, "engine_forces_launch": engine_forces_ms(hs, xs)}
    dev = torch.device("cuda:0")
    cells, pos = torch.from_numpy(hs).to(dev), torch.from_numpy(xs).to(dev)
    for _ in range(2):
        quench.inherent_structures_torch(cells, pos, 1e-10, PROBE_ITERS)
    probe = []
    for _ in range(reps):
        _, _, _, iters = quench.inherent_structures_torch(cells, pos, 1e-10, PROBE_ITERS)
        probe.append(quench.quench_elapsed_ms())
    assert int(iters[:, 1].sum()) == 0, "a box converged inside the probe"
    med = np.median(np.array(probe), axis=0) / (PROBE_ITERS + 1)
    out["plan"] = quench.quench_last()
    out["per_iteration_ms"] = {"sort": float(med[0]), "moments": float(med[1]), "forces": float(med[2]), "step": float(med[3]), "all": float(med.sum())}
    for label, ftol in (("ftol_1e-6", 1e-6), ("ftol_1e-10", 1e-10)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, stats, iters = quench.inherent_structures_torch(cells, pos, ftol, 20000)
        wall = (time.perf_counter() - t0) * 1e3
        it = iters.cpu().numpy()
        st = stats.cpu().numpy()
        out[label] = {"call_wall_ms": wall, "timers_ms": dict(zip(("sort", "moments", "forces", "step"), (float(v) for v in quench.quench_elapsed_ms()))),
                      "converged": int(it[:, 1].sum()), "iterations_min": int(it[:, 0].min()), "iterations_median": float(np.median(it[:, 0])),
                      "iterations_max": int(it[:, 0].max()), "fmax_end_max": float(st[:, 3].max()), "e_end_mean": float(st[:, 1].mean()),
                      "largest_displacement_bohr": float(st[:, 4].max())}
    quench.quench_finalize()
    t0 = time.perf_counter()
    for _ in range(3):
        quench_ref.energy_forces(hs[0], xs[0])
    out["mirror_cpu_s_per_evaluation"] = (time.perf_counter() - t0) / 3
    if xs.shape[1] <= 64:
        t0 = time.perf_counter()
        r = quench_ref.quench(hs[0], xs[0], 1e-10)
        out["mirror_cpu_s_quench_1e-10"] = time.perf_counter() - t0
        out["mirror_iterations_1e-10"] = int(r["iters"][0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quench_measurements.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--case", choices=sorted(CASES))
    args = ap.parse_args()
    if args.case:
        print("RESULT " + json.dumps(run_case(args.case, args.reps)), flush=True)
        return 0
    result = {"tool": "quench_measurements"}
    for name, (_, limit) in CASES.items():
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
