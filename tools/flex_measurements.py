"""Time one step of libmw_flex.so with the barostat off, every step and every tenth step, in the couplings 0 (isotropic) and 1
(every axis on its own), against one step of libmw_npt.so at the same settings on the same boxes, and write
profiles/flex_measurements.json and profiles/flex_summary.md:

    ih1536x64      64 boxes of 1536 molecules (ih1536 shaken with sigma = 0.12 Angstrom, seed 20250228 + box), general geometry
    ic48x4096      4096 boxes of 48 molecules (ic48 shaken with sigma = 0.15 Angstrom, seed 20250228 + box), small geometry

    python tools/flex_measurements.py [--out FILE] [--summary FILE] [--reps 7] [--npt-lib PATH]

Every call runs 20 steps (21 evaluations without the barostat, 41 with it every step, 23 with it every tenth) on device
tensors from the same positions and velocities, with the thermostat (250 K, gamma = 1 / (100 fs)), 1 atm, tau_p = 1 ps and
beta_T = 4.5e-10 / Pa; the time per step is the sum of the library's event timers over 21, as in tools/npt_measurements.py.
After two warm-up calls of each, the calls alternate (NPT off / 1 / 10, then the same of libmw_flex.so in coupling 0 and in
coupling 1) `reps` times; the record holds the median, the smallest and the largest of each and the ratio of the medians to
libmw_npt.so's at the same barostat setting.  ``--npt-lib`` loads another build of libmw_npt.so (the parent commit's; this
change leaves its code object as it was, so the tree's own is the parent's).  Each case runs in a process of its own under its
own time limit.  The record also holds the register and LDS figures of every kernel of libmw_flex.so and of libmw_npt.so's two
kernels with a force walk, read from the gfx950 code objects.
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
EVERY = (0, 1, 10)
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def kernel_resources(lib, prefix):
    """{kernel: {vgprs, sgprs, sgpr_spills, vgpr_spills, private_bytes, lds_bytes}} of a library's gfx950 code object."""
    data = open(lib, "rb").read()
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
        m = re.search(r"(k_(?:%s|cells)_[a-z0-9]+)(ILb([01])EEE)?" % prefix, name)
        get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))     # noqa: E731
        label = m.group(1) + ("" if m.group(3) is None else "<thermostat>" if m.group(3) == "1" else "<nve>")
        out[label] = dict(vgprs=get("vgpr_count"), sgprs=get("sgpr_count"), sgpr_spills=get("sgpr_spill_count"), vgpr_spills=get("vgpr_spill_count"),
                          private_bytes=get("private_segment_fixed_size"), lds_bytes=get("group_segment_fixed_size"))
    return out


def run_case(name, reps, npt_lib):
    import numpy as np
    import torch
    from conftest import load_golden
    from mc_water_ls_mw_amd import dynamics, flexcell, lattice as lat, npt
    if npt_lib:
        npt.load_npt_library(os.path.abspath(npt_lib))
    golden, boxes, sigma, _ = CASES[name]
    z = load_golden(golden)
    xs = np.array([lat.thermalise(z["xyz"], sigma, 20250228 + b) for b in range(boxes)])
    hs = np.ascontiguousarray(np.broadcast_to(z["h"], (boxes, 3, 3)))
    n = xs.shape[1]
    dt, kT, gamma = 5.0 * dynamics.FS, 250.0 * dynamics.KELVIN, 1.0 / (100.0 * dynamics.FS)
    dev = torch.device("cuda:0")
    cells, pos = torch.from_numpy(hs).to(dev), torch.from_numpy(xs).to(dev)
    vel = torch.from_numpy(dynamics.maxwell_boltzmann(boxes, n, kT, seed=1)).to(dev)

    def run_npt(every):
        out = npt.molecular_dynamics_npt_torch(cells, pos, STEPS, dt, npt.ATM, kT, gamma, baro_every=every, vel_t=vel, seed=3, sample_every=STEPS)
        status = out[6]
        assert int(status[:, 1].sum()) == 0 and int(status[:, 0].min()) == STEPS, "a box froze inside the probe"
        return npt.npt_elapsed_ms()

    def run_flex(every, coupling):
        out = flexcell.molecular_dynamics_flex_torch(cells, pos, STEPS, dt, npt.ATM, kT, gamma, baro_every=every, coupling=coupling, vel_t=vel, seed=3,
                                                     sample_every=STEPS)
        status = out[6]
        assert int(status[:, 1].sum()) == 0 and int(status[:, 0].min()) == STEPS, "a box froze inside the probe"
        return flexcell.flex_elapsed_ms()

    runs = {}
    for every in EVERY:
        runs["npt_%d" % every] = lambda every=every: run_npt(every)
    for coupling in (0, 1):
        for every in EVERY:
            runs["flex%d_%d" % (coupling, every)] = lambda every=every, coupling=coupling: run_flex(every, coupling)
    for _ in range(2):
        for f in runs.values():
            f()
    seen = {k: [] for k in runs}
    for _ in range(reps):
        for k, f in runs.items():
            seen[k].append(f())
    out = {"boxes": boxes, "molecules": int(n), "reps": reps, "steps_per_call": STEPS, "npt_plan": npt.npt_last(), "flex_plan": flexcell.flex_last()}
    for k, rows in seen.items():
        a = np.array(rows) / EVALS
        tot = a.sum(axis=1)
        out[k] = {"ms_median": float(np.median(tot)), "ms_min": float(tot.min()), "ms_max": float(tot.max()),
                  "parts_ms_median": dict(zip(("sort", "moments", "forces", "drift", "barostat"), (float(v) for v in np.median(a, axis=0))))}
    for coupling in (0, 1):
        for every in EVERY:
            k = "flex%d_%d" % (coupling, every)
            out[k]["ratio_to_npt"] = out[k]["ms_median"] / out["npt_%d" % every]["ms_median"]
            out[k]["forces_ratio_to_npt"] = out[k]["parts_ms_median"]["forces"] / out["npt_%d" % every]["parts_ms_median"]["forces"]
    flexcell.flex_finalize()
    npt.npt_finalize()
    return out


def summary(result):
    """The record as a short table."""
    lines = ["# libmw_flex.so against libmw_npt.so: milliseconds per step", "",
             "Written by tools/flex_measurements.py; the figures are profiles/flex_measurements.json's.  Per step = the sum of the library's",
             "event timers of a call of %d steps over %d; medians of %d alternating repetitions; Langevin, 1 atm.  `off / 1 / 10`: the barostat"
             % (STEPS, EVALS, result["reps"]), "never, after every step, after every tenth.", ""]
    for name in CASES:
        r = result[name]
        lines += ["## %s: %d boxes of %d molecules (%s geometry)" % (name, r["boxes"], r["molecules"], "small" if r["flex_plan"]["small"] else "general"), "",
                  "| barostat | libmw_npt.so | coupling 0 | ratio | force pass ratio | coupling 1 | ratio | force pass ratio |", "|---|---|---|---|---|---|---|---|"]
        for every in EVERY:
            a, f0, f1 = r["npt_%d" % every], r["flex0_%d" % every], r["flex1_%d" % every]
            lines.append("| %s | %.4f | %.4f | %.3f | %.3f | %.4f | %.3f | %.3f |" % ("off" if every == 0 else every, a["ms_median"], f0["ms_median"], f0["ratio_to_npt"],
                                                                                 f0["forces_ratio_to_npt"], f1["ms_median"], f1["ratio_to_npt"], f1["forces_ratio_to_npt"]))
        lines.append("")
    lines += ["## Registers", "", "| kernel | VGPRs | SGPRs | SGPR spills | VGPR spills | private bytes | LDS bytes |", "|---|---|---|---|---|---|---|"]
    for lib in ("flex_kernels", "npt_kernels"):
        for k, v in sorted(result[lib].items()):
            if lib == "npt_kernels" and not k.startswith(("k_npt_forces", "k_npt_small")):
                continue
            lines.append("| %s | %d | %d | %d | %d | %d | %d |" % (k, v["vgprs"], v["sgprs"], v["sgpr_spills"], v["vgpr_spills"], v["private_bytes"], v["lds_bytes"]))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flex_measurements.json"))
    ap.add_argument("--summary", default=os.path.join(ROOT, "profiles", "flex_summary.md"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--npt-lib", default="")
    ap.add_argument("--case", choices=sorted(CASES))
    args = ap.parse_args()
    if args.case:
        print("RESULT " + json.dumps(run_case(args.case, args.reps, args.npt_lib)), flush=True)
        return 0
    from mc_water_ls_mw_amd import build
    result = {"tool": "flex_measurements", "reps": args.reps, "npt_lib": os.path.basename(args.npt_lib) or "libmw_npt.so",
              "flex_kernels": kernel_resources(build.FLEX_LIB, "flex"), "npt_kernels": kernel_resources(args.npt_lib or build.NPT_LIB, "npt")}
    for name, case in CASES.items():
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps), "--npt-lib", args.npt_lib],
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
