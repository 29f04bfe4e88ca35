"""Time one step of libmw_npt.so with the barostat off, every step and every tenth step against one step of libmw_md.so on the
same boxes and write profiles/npt_measurements.json:

    ih1536x64      64 boxes of 1536 molecules (ih1536 shaken with sigma = 0.12 Angstrom, seed 20250228 + box), general geometry
    ic48x4096      4096 boxes of 48 molecules (ic48 shaken with sigma = 0.15 Angstrom, seed 20250228 + box), small geometry

    python tools/npt_measurements.py [--out FILE] [--reps 7] [--md-lib PATH]

Every call runs 20 steps (21 evaluations without the barostat, 41 with it every step, 23 with it every tenth) on device
tensors from the same positions and velocities, with the thermostat (250 K, gamma = 1 / (100 fs)), 1 atm, tau_p = 1 ps and
beta_T = 4.5e-10 / Pa; the time per step is the sum of the library's event timers over 21, as in tools/md_measurements.py.  After
two warm-up calls of each, the calls alternate (MD, barostat off, every step, every tenth) `reps` times; the record holds the
median, the smallest and the largest of each.  ``--md-lib`` loads another build of libmw_md.so (the parent commit's).  Each case
runs in a process of its own under its own time limit.  The record also holds the register and LDS figures of every kernel of
libmw_npt.so, read from its gfx950 code object.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = {"ih1536x64": ("ih1536", 64, 0.12, 300), "ic48x4096": ("ic48", 4096, 0.15, 300)}     # golden box, boxes, sigma, time limit in seconds
STEPS = 20
EVALS = STEPS + 1
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def kernel_resources():
    """{kernel: {vgprs, sgprs, sgpr_spills, vgpr_spills, private_bytes, lds_bytes}} of libmw_npt.so's gfx950 code object."""
    from mc_water_ls_mw_amd import build
    data = open(build.NPT_LIB, "rb").read()
    i = data.find(b"__CLANG_OFFLOAD_BUNDLE__")
    n = struct.unpack_from("<Q", data, i + 24)[0]
    off, blob = i + 32, None
    for _ in range(n):
        o, s, tl = struct.unpack_from("<QQQ", data, off)
        off += 24
        if b"gfx950" in data[off:off + tl]:
            blob = data[i + o:i + o + s]
        off += tl
    out = {}
    with tempfile.NamedTemporaryFile(suffix=".co") as fh:
        fh.write(blob)
        fh.flush()
        notes = subprocess.run([READELF, "--notes", fh.name], capture_output=True, text=True, check=True).stdout
    for blk in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.search(r"(k_(?:npt|cells)_[a-z0-9]+)(ILb([01])EEE)?", name)
        get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))     # noqa: E731
        label = m.group(1) + ("" if m.group(3) is None else "<thermostat>" if m.group(3) == "1" else "<nve>")
        out[label] = dict(vgprs=get("vgpr_count"), sgprs=get("sgpr_count"), sgpr_spills=get("sgpr_spill_count"), vgpr_spills=get("vgpr_spill_count"),
                          private_bytes=get("private_segment_fixed_size"), lds_bytes=get("group_segment_fixed_size"))
    return out


def run_case(name, reps, md_lib):
    import numpy as np
    import torch
    from conftest import load_golden
    from mc_water_ls_mw_amd import dynamics, lattice as lat, npt
    if md_lib:
        dynamics.load_md_library(os.path.abspath(md_lib))
    golden, boxes, sigma, _ = CASES[name]
    z = load_golden(golden)
    xs = np.array([lat.thermalise(z["xyz"], sigma, 20250228 + b) for b in range(boxes)])
    hs = np.ascontiguousarray(np.broadcast_to(z["h"], (boxes, 3, 3)))
    n = xs.shape[1]
    dt, kT, gamma = 5.0 * dynamics.FS, 250.0 * dynamics.KELVIN, 1.0 / (100.0 * dynamics.FS)
    dev = torch.device("cuda:0")
    cells, pos = torch.from_numpy(hs).to(dev), torch.from_numpy(xs).to(dev)
    vel = torch.from_numpy(dynamics.maxwell_boltzmann(boxes, n, kT, seed=1)).to(dev)

    def md():
        _, _, _, _, status = dynamics.molecular_dynamics_torch(cells, pos, STEPS, dt, kT, gamma, vel_t=vel, seed=3, sample_every=STEPS)
        assert int(status[:, 1].sum()) == 0 and int(status[:, 0].min()) == STEPS, "a box froze inside the probe"
        return dynamics.md_elapsed_ms() + (0.0,)

    def run_npt(every):
        out = npt.molecular_dynamics_npt_torch(cells, pos, STEPS, dt, npt.ATM, kT, gamma, baro_every=every, vel_t=vel, seed=3, sample_every=STEPS)
        status = out[6]
        assert int(status[:, 1].sum()) == 0 and int(status[:, 0].min()) == STEPS, "a box froze inside the probe"
        return npt.npt_elapsed_ms()

    runs = {"md": md, "npt_off": lambda: run_npt(0), "npt_every_1": lambda: run_npt(1), "npt_every_10": lambda: run_npt(10)}
    for _ in range(2):
        for f in runs.values():
            f()
    seen = {k: [] for k in runs}
    for _ in range(reps):
        for k, f in runs.items():
            seen[k].append(f())
    out = {"boxes": boxes, "molecules": int(n), "reps": reps, "steps_per_call": STEPS, "md_plan": dynamics.md_last(), "npt_plan": npt.npt_last()}
    for k, rows in seen.items():
        a = np.array(rows) / EVALS
        tot = a.sum(axis=1)
        out[k] = {"ms_median": float(np.median(tot)), "ms_min": float(tot.min()), "ms_max": float(tot.max()),
                  "parts_ms_median": dict(zip(("sort", "moments", "forces", "drift", "barostat"), (float(v) for v in np.median(a, axis=0))))}
    for k, evals in (("npt_off", EVALS), ("npt_every_1", EVALS + STEPS), ("npt_every_10", EVALS + STEPS // 10)):
        out[k]["ratio_to_md"] = out[k]["ms_median"] / out["md"]["ms_median"]
        out[k]["ratio_expected_from_evaluations"] = evals / EVALS
    npt.npt_finalize()
    dynamics.md_finalize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "npt_measurements.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--md-lib", default="")
    ap.add_argument("--case", choices=sorted(CASES))
    args = ap.parse_args()
    if args.case:
        print("RESULT " + json.dumps(run_case(args.case, args.reps, args.md_lib)), flush=True)
        return 0
    result = {"tool": "npt_measurements", "md_lib": os.path.basename(args.md_lib) or "libmw_md.so", "kernels": kernel_resources()}
    for name, case in CASES.items():
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps), "--md-lib", args.md_lib],
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
