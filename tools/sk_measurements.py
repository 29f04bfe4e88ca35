#!/usr/bin/env python3
"""Structure factors of whole farms: mw_sk_compute_device on device tensors, median of R calls after warm-up, split into the
table pass and the sums by mw_sk_elapsed_ms, for
  a: 512 x 4096 molecules (bench.py's ih4096_t015 walkers: seed 20250228 + walker index), all half-space vectors to 3 / Angstrom,
  b:  64 x 32768 molecules, the same k_max,
  c: 16384 x 48 molecules (the replica farm's boxes: thermalised ih48), all half-space vectors to 6 / Angstrom,
each next to what a user can do today: sk_tables of tests/sk_ref.py (numpy, double precision) on 16 threads on the same
inputs -- for a and b on the first --cpu-boxes boxes, scaled to all of them.  Every case runs in a process of its own under a
time limit; the first one that fails ends the run.  Writes one JSON document to --out (and prints it).  Run on the GPU box:
    python tools/sk_measurements.py [--reps R] [--case a|b|c] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMIT_S = {"a": 420, "b": 540, "c": 420}
K_MAX_ANG = {"a": 3.0, "b": 3.0, "c": 6.0}
CPU_BOXES = {"a": 16, "b": 1}
THREADS = 16


def boxes_of(case):
    import numpy as np
    from mc_water_ls_mw_amd import lattice as lat
    if case == "c":
        z = np.load(os.path.join(ROOT, "tests", "golden", "ih48.npz"), allow_pickle=False)
        n = 16384
        return z["h"], np.array([lat.thermalise(z["xyz"], 0.15, 20250228 + b) for b in range(n)])
    cells, n = ((8, 8, 8), 512) if case == "a" else ((16, 16, 16), 64)
    h, xyz = lat.ice_box("ih", cells)
    return h, np.array([lat.thermalise(xyz, 0.15, 20250228 + b) for b in range(n)])


def cpu_baseline(h, xs, nvec):
    """sk_tables of the boxes xs on THREADS threads (numpy releases the interpreter lock inside its loops): the vectors of
    every box are cut into THREADS pieces when there are fewer boxes than threads.  (seconds, S [boxes, M])"""
    from concurrent.futures import ThreadPoolExecutor
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from sk_ref import sk_tables
    pieces = 1 if len(xs) >= THREADS else THREADS
    cuts = np.linspace(0, len(nvec), pieces + 1).astype(int)
    jobs = [(b, cuts[p], cuts[p + 1]) for b in range(len(xs)) for p in range(pieces)]
    S = np.zeros((len(xs), len(nvec)))

    def work(job):
        b, lo, hi = job
        S[b, lo:hi] = sk_tables(h, xs[b], nvec[lo:hi])[1]

    t0 = time.perf_counter()
    with ThreadPoolExecutor(THREADS) as pool:
        list(pool.map(work, jobs))
    return time.perf_counter() - t0, S


def measure(case, reps, cpu_boxes):
    import numpy as np
    import torch
    from mc_water_ls_mw_amd import structure
    h, xs = boxes_of(case)
    boxes, n = xs.shape[0], xs.shape[1]
    nvec = structure.kvectors(h, K_MAX_ANG[case], half=True)
    dev = torch.device("cuda:0")
    cells_t = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(h, (boxes, 3, 3)))).to(dev)
    pos_t, nvec_t = torch.from_numpy(xs).to(dev), torch.from_numpy(nvec).to(dev)
    t0 = time.perf_counter()
    warm = 0
    while warm < 2 or time.perf_counter() - t0 < 0.5:              # warm-up: clocks up, scratch allocated
        S_t, rho_t = structure.structure_factor_torch(cells_t, pos_t, nvec_t)
        warm += 1
    ph, sm, wall = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        S_t, rho_t = structure.structure_factor_torch(cells_t, pos_t, nvec_t)
        wall.append(1e3 * (time.perf_counter() - t0))
        a, b = structure.sk_elapsed_ms()
        ph.append(a), sm.append(b)
    med = lambda v: float(sorted(v)[len(v) // 2])                  # noqa: E731
    plan = structure.sk_last()
    out = {"case": case, "boxes": boxes, "molecules": n, "vectors": int(len(nvec)), "k_max_ang": K_MAX_ANG[case],
           "nmax": [int(v) for v in np.abs(nvec).max(axis=0)], "reps": reps, "plan": plan,
           "phasors_ms_median": med(ph), "sums_ms_median": med(sm), "device_ms_median": med([a + b for a, b in zip(ph, sm)]),
           "device_ms_min": float(min(a + b for a, b in zip(ph, sm))), "call_wall_ms_median": med(wall),
           "molecule_vector_pairs": int(boxes) * int(n) * int(len(nvec))}
    out["pairs_per_second"] = out["molecule_vector_pairs"] / (1e-3 * out["device_ms_median"])
    nb = boxes if case == "c" else min(cpu_boxes or CPU_BOXES[case], boxes)
    cpu_s, S_cpu = cpu_baseline(h, xs[:nb], nvec)
    S = S_t[:nb].cpu().numpy()
    out.update({"cpu_boxes_timed": nb, "cpu_threads": THREADS, "cpu_sk_tables_s": cpu_s, "cpu_all_boxes_s_scaled": cpu_s * boxes / nb,
                "cpu_over_device_call": cpu_s * boxes / nb / (1e-3 * out["call_wall_ms_median"]),
                "max_abs_S_difference_to_cpu": float(np.abs(S - S_cpu).max()), "max_S": float(S.max())})
    structure.sk_finalize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--case", choices=("a", "b", "c"))
    ap.add_argument("--cpu-boxes", type=int, default=0, help="boxes of cases a and b the numpy baseline is timed on (default 16 and 1)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sk_measurements.json"))
    args = ap.parse_args()
    if args.case:
        print(json.dumps(measure(args.case, args.reps, args.cpu_boxes)))
        return 0
    out, rc = {"tool": "sk_measurements"}, 0
    for case, key in (("c", "ih48x16384"), ("a", "ih4096x512"), ("b", "ih32768x64")):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(args.reps),
                                "--cpu-boxes", str(args.cpu_boxes)], capture_output=True, text=True, timeout=LIMIT_S[case])
        except subprocess.TimeoutExpired:
            out[key], rc = {"failed": "time limit"}, 1
            break
        if p.returncode != 0:
            out[key], rc = {"failed": p.returncode, "stderr": p.stderr[-2000:]}, 1
            break
        out[key] = json.loads(p.stdout.strip().splitlines()[-1])
        print(key, "done: device", out[key]["device_ms_median"], "ms", file=sys.stderr, flush=True)
    text = json.dumps(out, indent=1)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    print(text)
    return rc


if __name__ == "__main__":
    sys.exit(main())
