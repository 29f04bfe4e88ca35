"""Measure libmw_ti.so and write profiles/ti_measurements.json:

(a) the time of one step at lambda = 0.5 against one MD step of libmw_md.so on the two workloads of profiles/md_summary.md,

    ih1536x64      64 boxes of 1536 molecules (ih1536 shaken with sigma = 0.12 Angstrom, seed 20250228 + box), general geometry
    ic48x4096      4096 boxes of 48 molecules (ic48 shaken with sigma = 0.15 Angstrom, seed 20250228 + box), small geometry

    with the protocol of tools/md_measurements.py: 21 evaluations per call on device tensors from the same positions (the
    Einstein sites are the unshaken lattice, k = 0.02 Hartree / bohr^2, blocks of 5 steps so that the accumulators work), the
    time per step the sum of the library's event timers over 21; two warm-up calls of each, then the calls alternate (MD NVE, TI
    NVE, MD Langevin, TI Langevin) `reps` times: median, smallest, largest.  ``--md-lib`` loads another build of libmw_md.so
    (the parent commit's; the library's sources do not change with libmw_ti.so, so the tree's own build is that build).

(b) one physical run: the free energy of a 64-molecule cubic-ice box and a 64-molecule hexagonal-ice box (2 x 2 x 2 cells of 8)
    at 100 K, 200 K and 250 K by Frenkel-Ladd integration over 12 Gauss-Legendre nodes, beside e_min + f_vib of the harmonic
    approximation at the same inherent structure.  Per temperature: the spring is einstein.spring_from_msd of the mean squared
    displacement (centre of mass removed) of the second half of 4000 steps at lambda = 0, averaged over the two lattices; then
    one call of 24 boxes, 40000 steps of 5 fs with gamma = 1 / (100 fs), 5000 left out, 14 blocks of 2500.

    python tools/ti_measurements.py [--out FILE] [--reps 7] [--md-lib PATH]

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
PHYSICAL_LIMIT = 500
EVALS = 21
TEMPERATURES = (100.0, 200.0, 250.0)


def run_case(name, reps, md_lib):
    import numpy as np
    import torch
    from conftest import load_golden
    from mc_water_ls_mw_amd import dynamics, einstein, lattice as lat
    if md_lib:
        dynamics.load_md_library(os.path.abspath(md_lib))
    golden, boxes, sigma, _ = CASES[name]
    z = load_golden(golden)
    xs = np.array([lat.thermalise(z["xyz"], sigma, 20250228 + b) for b in range(boxes)])
    hs = np.ascontiguousarray(np.broadcast_to(z["h"], (boxes, 3, 3)))
    ss = np.ascontiguousarray(np.broadcast_to(z["xyz"], xs.shape))
    n = xs.shape[1]
    dt, kT = 5.0 * dynamics.FS, 250.0 * dynamics.KELVIN
    dev = torch.device("cuda:0")
    cells, pos, sites = torch.from_numpy(hs).to(dev), torch.from_numpy(xs).to(dev), torch.from_numpy(ss).to(dev)
    vel = torch.from_numpy(dynamics.maxwell_boltzmann(boxes, n, kT, seed=1)).to(dev)
    lam = torch.full((boxes,), 0.5, dtype=torch.float64, device=dev)
    spring = torch.full((boxes,), 0.02, dtype=torch.float64, device=dev)

    def md(gamma):
        _, _, _, _, status = dynamics.molecular_dynamics_torch(cells, pos, EVALS - 1, dt, kT, gamma, vel_t=vel, seed=3, sample_every=EVALS - 1, pos_ref_t=sites)
        assert int(status[:, 1].sum()) == 0 and int(status[:, 0].min()) == EVALS - 1, "a box froze inside the probe"
        return dynamics.md_elapsed_ms()

    def ti(gamma):
        _, _, _, _, _, status = einstein.einstein_md_torch(cells, sites, lam, spring, EVALS - 1, dt, kT, gamma, pos_t=pos, vel_t=vel, seed=3,
                                                           sample_every=EVALS - 1, equil_steps=0, block_steps=5)
        assert int(status[:, 1].sum()) == 0 and int(status[:, 0].min()) == EVALS - 1, "a box froze inside the probe"
        return einstein.ti_elapsed_ms()

    g = 1.0 / (100.0 * dynamics.FS)
    runs = {"md_nve": lambda: md(0.0), "ti_nve": lambda: ti(0.0), "md_langevin": lambda: md(g), "ti_langevin": lambda: ti(g)}
    for _ in range(2):
        for f in runs.values():
            f()
    seen = {k: [] for k in runs}
    for _ in range(reps):
        for k, f in runs.items():
            seen[k].append(f())
    out = {"boxes": boxes, "molecules": int(n), "reps": reps, "evaluations_per_call": EVALS, "md_plan": dynamics.md_last(), "ti_plan": einstein.ti_last()}
    for k, rows in seen.items():
        a = np.array(rows) / EVALS
        tot = a.sum(axis=1)
        out[k] = {"ms_median": float(np.median(tot)), "ms_min": float(tot.min()), "ms_max": float(tot.max()),
                  "parts_ms_median": dict(zip(("sort", "moments", "forces", "drift"), (float(v) for v in np.median(a, axis=0))))}
    for e in ("nve", "langevin"):
        out["ratio_" + e] = out["ti_" + e]["ms_median"] / out["md_" + e]["ms_median"]
    einstein.ti_finalize()
    dynamics.md_finalize()
    return out


def run_physical():
    import numpy as np
    from mc_water_ls_mw_amd import dynamics, einstein, lattice as lat, phonons, quench
    boxes = [lat.ice_box("ic", (2, 2, 2), 0.05, seed=1), lat.ice_box("ih", (2, 2, 2), 0.05, seed=2)]
    hs, xs = np.array([b[0] for b in boxes]), np.array([b[1] for b in boxes])
    n = xs.shape[1]
    sites, _, stats, iters = quench.inherent_structures(hs, xs, 1e-10, 20000)
    assert np.all(iters[:, 1] == 1), "a quench did not converge"
    H, _ = phonons.hessian(hs, sites)
    omegas = [phonons.normal_modes(H[b]) for b in range(2)]
    dt, gamma = 5.0 * dynamics.FS, 1.0 / (100.0 * dynamics.FS)
    lam, w = einstein.gauss_legendre(12)
    out = {"molecules": int(n), "lattices": ["ic", "ih"], "nodes": 12, "nsteps": 40000, "equil_steps": 5000, "block_steps": 2500, "e_min": [float(v) for v in stats[:, 1]],
           "temperatures": {}}
    for T in TEMPERATURES:
        kT = T * dynamics.KELVIN
        _, _, _, _, blk, st = einstein.einstein_md(hs, sites, 0.0, 1.0, 4000, dt, kT, gamma, seed=5, equil_steps=2000, block_steps=2000, sample_every=4000)
        assert np.all(st == (4000, 0))
        msd = float((blk[:, 0, 2] - blk[:, 0, 4]).mean())
        k = einstein.spring_from_msd(msd, kT)
        _, _, _, _, blocks, st = einstein.einstein_md(np.repeat(hs, 12, axis=0), np.repeat(sites, 12, axis=0), np.tile(lam, 2), k, 40000, dt, kT, gamma, seed=7,
                                                      streams=np.arange(24), sample_every=40000, equil_steps=5000, block_steps=2500)
        assert np.all(st == (40000, 0)), "a box froze"
        y = einstein.integrand(blocks, k, n).reshape(2, 12, -1)
        f_e = einstein.einstein_free_energy(n, k, dynamics.MASS_WATER, kT)
        rec = {"kT": kT, "msd": msd, "spring": k, "f_einstein": f_e, "elapsed_ms": sum(einstein.ti_elapsed_ms()), "F": [], "err": [], "harmonic": [], "gap": [],
               "integrand_mean": y.mean(axis=2).tolist()}
        for b in range(2):
            F, err = einstein.frenkel_ladd(lam, w, y[b], f_e)
            harm = float(stats[b, 1]) + phonons.harmonic_free_energy(omegas[b], kT)
            rec["F"].append(F), rec["err"].append(err), rec["harmonic"].append(harm), rec["gap"].append(F - harm)
        rec["dF_ih_minus_ic"] = rec["F"][1] - rec["F"][0]
        rec["dF_err"] = float(np.hypot(*rec["err"]))
        rec["dF_harmonic"] = rec["harmonic"][1] - rec["harmonic"][0]
        out["temperatures"]["%g" % T] = rec
    einstein.ti_finalize()
    quench.quench_finalize()
    phonons.hess_finalize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ti_measurements.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--md-lib", default="")
    ap.add_argument("--case", choices=sorted(CASES) + ["physical"])
    args = ap.parse_args()
    if args.case:
        print("RESULT " + json.dumps(run_physical() if args.case == "physical" else run_case(args.case, args.reps, args.md_lib)), flush=True)
        return 0
    result = {"tool": "ti_measurements", "md_lib": os.path.basename(args.md_lib) or "libmw_md.so"}
    for name, limit in [(k, v[3]) for k, v in CASES.items()] + [("physical", PHYSICAL_LIMIT)]:
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps), "--md-lib", args.md_lib],
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
