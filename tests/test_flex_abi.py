"""CPU: libmw_flex.so builds for gfx950, loads without a GPU, exports what include/mw_flex.h declares (and nothing of it leaks
into the other libraries, nor theirs into it), takes the stress from the one shared force header, keeps its kernels free of
scratch memory, rejects bad arguments and uninitialised calls with messages that name the entry and the argument and leaves the
outputs alone, and reports the launch rules of mw_md_plan through mw_flex_plan."""
import ctypes
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
KERNELS = (b"k_cells_bin", b"k_cells_scan", b"k_cells_place", b"k_cells_rank", b"k_flex_check", b"k_flex_begin", b"k_flex_finish", b"k_flex_drift1",
           b"k_flex_drift2", b"k_flex_moments", b"k_flex_forces", b"k_flex_row", b"k_flex_small", b"k_flex_baro", b"k_flex_scale")
A_SIGMA = 2.3925 / 0.5291772108 * 1.8                   # bohr
MASS = 18.01528 * 1822.888486209


def _lib():
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.flexcell import load_flex_library
    build.build_flex()
    return load_flex_library()


def _declared():
    text = open(os.path.join(ROOT, "include", "mw_flex.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mw_flex_\w+)\s*\(", text)))


def test_build_flex_compiles_for_gfx950():
    from mc_water_ls_mw_amd import build
    lib = build.build_flex(force=True)
    assert lib == build.FLEX_LIB and os.path.exists(lib)
    data = open(lib, "rb").read()
    assert b"__CLANG_OFFLOAD_BUNDLE__" in data and b"gfx950" in data
    for kernel in KERNELS:
        assert kernel in data, kernel
    header = os.path.join(ROOT, "include", "mw_flex.h")
    shared = [os.path.join(build.CSRC, f) for f in ("mw_lib_host.h", "mw_lib_cells.h", "mw_lib_forces.h", "mw_common.hip.h")]
    assert sorted(build.FLEX_DEPS) == sorted([build.FLEX_SRC, header, *shared]) and all(os.path.exists(p) for p in build.FLEX_DEPS)
    others = (build.DEPS, build.SK_DEPS, build.BOO_DEPS, build.TET_DEPS, build.ADF_DEPS, build.RINGS_DEPS, build.QUENCH_DEPS, build.QUENCH_BUILD_DEPS,
              build.MD_DEPS, build.NPT_DEPS, build.TCF_DEPS, build.HESS_DEPS, build.TI_DEPS, build.COMMS_DEPS)
    for deps in others:
        assert not any(p in deps for p in (build.FLEX_SRC, header))         # no other library moves with it
    sources = (build.SOURCES[0], build.SK_SRC, build.BOO_SRC, build.TET_SRC, build.ADF_SRC, build.RINGS_SRC, build.QUENCH_SRC, build.MD_SRC, build.NPT_SRC,
               build.TCF_SRC, build.HESS_SRC, build.TI_SRC, build.COMMS_SRC)
    assert not any(p in build.FLEX_DEPS for p in sources)                    # and it moves with no other library's source
    assert not any(p.endswith((".hip", ".hip.h")) and p not in (build.FLEX_SRC, shared[3]) for p in build.FLEX_DEPS)
    assert os.path.basename(build.FLEX_SRC) == "mw_flex.hip"


def test_the_stress_comes_from_the_one_shared_force_header():
    from mc_water_ls_mw_amd import build
    assert build.LIB_FORCES in build.FLEX_DEPS
    text = open(build.FLEX_SRC).read()
    assert '#include "mw_lib_forces.h"' in text and "entry_stress(" in text and "lane_stress(" in text and "lane_virial(" in text
    assert "namespace mwflex" in text and "block_reduce<kSums, 1>" in text and "constexpr int kSums = 16;" in text
    for word in ("struct Sums", "void triplet_grad", "void entry_force", "void entry_virial", "void entry_stress", "struct CellRegs", "double dpp_wave_max",
                 "double block_reduce"):
        assert word not in text, word
    shared = open(build.LIB_FORCES).read()
    for word in ("void entry_force", "void entry_virial", "void entry_stress", "double lane_virial", "double lane_stress"):
        assert shared.count(word) == 1, word
    assert "atomicAdd" not in shared and "atomicAdd" not in text and "contract(off)" in text
    assert text.index("#pragma clang fp contract(off)") < text.index('#include "mw_lib_host.h"')
    # the pieces restated from the MD and NPT libraries are said to be restated; the names other libraries' tests look for are absent
    assert "restated" in text and "MD_DEPS" not in text and "NPT_DEPS" not in text
    for name in (build.FLEX_SRC, build.LIB_FORCES):
        data = open(name).read()
        for word in ("mw_quench", "mw_hess", "k_hess_", "mw_tcf", "k_tcf_"):
            assert word not in data, (name, word)


def test_build_entry_builds_the_library():
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "mwbuild.build_flex(" in text
    text = open(os.path.join(ROOT, "mc_water_ls_mw_amd", "build.py")).read()
    assert re.search(r"for builder in \(.*build_flex\b", text)


def test_every_declared_name_is_exported_and_listed():
    L = _lib()
    from mc_water_ls_mw_amd import dynamics, flexcell, npt
    names = _declared()
    assert len(names) == 9 and sorted(flexcell.FLEX_ABI_SYMBOLS) == names
    for name in names:
        assert hasattr(L, name), name
    text = open(os.path.join(ROOT, "include", "mw_flex.h")).read()
    assert re.search(r"#define\s+MW_FLEX_PLAN_FIELDS\s+10\b", text) and len(dynamics.PLAN_FIELDS) == 10
    assert re.search(r"#define\s+MW_FLEX_TRACE_FIELDS\s+15\b", text) and len(flexcell.TRACE_FIELDS) == 15 and flexcell.TRACE_FIELDS[:6] == npt.TRACE_FIELDS
    assert re.search(r"#define\s+MW_FLEX_MAX_STEPS\s+100000000\b", text) and flexcell.MAX_STEPS == 100000000
    assert re.search(r"#define\s+MW_FLEX_MAX_DLNV\s+0\.3\b", text) and flexcell.MAX_DLNV == 0.3 == npt.MAX_DLNV
    assert re.search(r"#define\s+MW_FLEX_MAX_DLNL\s+0\.1\b", text) and flexcell.MAX_DLNL == 0.1
    for name, value in flexcell.COUPLINGS.items():
        assert re.search(r"#define\s+MW_FLEX_%s\s+%d\b" % (name.upper(), value), text), name
    assert sorted(flexcell.COUPLINGS.values()) == [0, 1, 2, 3]
    import flex_ref
    assert (flex_ref.ISO, flex_ref.ANISO, flex_ref.SEMI, flex_ref.UNIAXIAL) == tuple(flexcell.COUPLINGS[k] for k in ("iso", "aniso", "semi", "uniaxial"))
    assert flex_ref.MAX_DLNL == flexcell.MAX_DLNL and flex_ref.TRACE_FIELDS == 15


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not in this image")
def test_the_libraries_keep_their_prefixes_apart():
    from mc_water_ls_mw_amd import build
    others = [build.build(), build.build_sk(), build.build_boo(), build.build_tet(), build.build_adf(), build.build_rings(), build.build_quench(),
              build.build_md(), build.build_npt(), build.build_tcf(), build.build_hess(), build.build_ti()]
    build.build_flex()

    def defined(lib):
        out = subprocess.run([READELF, "--dyn-syms", "-W", lib], capture_output=True, text=True, check=True).stdout
        rows = [ln.split() for ln in out.splitlines()]
        return {f[7].split("@")[0] for f in rows if len(f) == 8 and f[0].endswith(":") and f[6] != "UND" and f[7].startswith("mw_")}

    assert defined(build.FLEX_LIB) == set(_declared())
    for lib in others:
        assert not any(s.startswith("mw_flex") for s in defined(lib))
        data = open(lib, "rb").read()
        assert b"mw_flex" not in data and b"k_flex_" not in data and b"mwflex" not in data, lib
    data = open(build.FLEX_LIB, "rb").read()
    for word in (b"k_boo_", b"mw_boo", b"mw_sk_", b"k_tet_", b"mw_tet", b"k_adf_", b"mw_adf", b"k_rings_", b"mw_rings", b"k_model_", b"mw_model_",
                 b"k_quench_", b"mw_quench", b"k_md_", b"mw_md", b"k_npt_", b"mw_npt", b"mwnpt", b"k_ti_", b"mw_ti_"):
        assert word not in data, word
    for name in ("mw_hess", "k_hess_", "mw_tcf", "k_tcf_"):
        assert name.encode() not in data, name


def _gfx950_code_object(lib, tmp_path):
    data = open(lib, "rb").read()
    i = data.find(b"__CLANG_OFFLOAD_BUNDLE__")
    assert i >= 0, "no offload bundle"
    n = struct.unpack_from("<Q", data, i + 24)[0]
    off = i + 32
    for _ in range(n):
        o, s, tl = struct.unpack_from("<QQQ", data, off)
        off += 24
        triple = data[off:off + tl]
        off += tl
        if b"gfx950" in triple:
            p = tmp_path / "flex.co"
            p.write_bytes(data[i + o:i + o + s])
            return str(p)
    raise AssertionError("no gfx950 code object")


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not in this image")
def test_no_kernel_uses_a_private_segment_or_spills_vector_registers(tmp_path):
    """No kernel has a private segment or spills a vector register.  The counts are printed: the moment pass keeps four
    wavefronts per SIMD (<= 128 VGPRs); the force pass, with seven accumulators more than the force itself, needs more than
    128 and runs three per SIMD (<= 168), which DESIGN.md 3.19 records with its measured cost; the small kernel stays within the
    256 that let two wavefronts share a SIMD, and parks scalar registers in vector lanes as libmw_npt.so's does."""
    from mc_water_ls_mw_amd import build
    build.build_flex()
    notes = subprocess.run([READELF, "--notes", _gfx950_code_object(build.FLEX_LIB, tmp_path)], capture_output=True, text=True, check=True).stdout
    seen = set()
    for blk in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.match(r"_ZN6mwflex\d+(k_flex_[a-z0-9]+)(E|ILb[01]EEE)", name) or re.match(r"_ZN7mwcells\d+(k_cells_[a-z]+)(E)", name)
        assert m, name                                                       # the library holds no other kernel
        get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))     # noqa: E731
        print(m.group(1), m.group(2), "vgprs", get("vgpr_count"), "sgprs", get("sgpr_count"), "sgpr spills", get("sgpr_spill_count"), "lds", get("group_segment_fixed_size"))
        assert get("private_segment_fixed_size") == 0 and get("vgpr_spill_count") == 0, name
        if m.group(1) != "k_flex_small":
            assert get("sgpr_spill_count") == 0, name
        if m.group(1) == "k_flex_moments":
            assert get("vgpr_count") <= 128, (name, get("vgpr_count"))
        if m.group(1) == "k_flex_forces":
            assert get("vgpr_count") <= 168 and get("group_segment_fixed_size") == 4 * 17 * 8, (name, get("vgpr_count"))
        if m.group(1) == "k_flex_small":
            assert get("vgpr_count") <= 256 and get("group_segment_fixed_size") == 4 * 13 * 64 * 8
        seen.add(m.group(1).encode())
    assert seen == set(KERNELS)


def _args(nboxes=2, nwater=4):
    cells = np.tile(np.eye(3).ravel() * 20.0, (max(nboxes, 1), 1))
    pos = np.arange(max(nboxes, 1) * max(nwater, 1) * 3, dtype=np.float64).reshape(max(nboxes, 1), max(nwater, 1), 3) * 0.7
    return cells, pos


def _run(L, nboxes=2, nwater=4, cells=None, pos=None, vel=None, pos_ref=None, nsteps=10, sample_every=1, dt=100.0, mass=MASS, kT=1e-3, gamma=1e-3,
         pressure=1e-8, tau_p=4e4, beta_T=1e4, baro_every=2, coupling=1, axis=2, entry="mw_flex_run"):
    """One run entry with outputs prefilled so that a write would show."""
    nb = min(max(nboxes, 1), 8)                                           # (counts out of range are rejected before anything is sized by them)
    size = nb * min(max(nwater, 1), 8)
    outs = [np.full(3 * size, -7.0), np.full(3 * size, -7.0), np.full(3 * size, -7.0), np.full(9 * nb, -7.0), np.full(3 * size, -7.0),
            np.full(15 * 200 * nb, -7.0), np.full(2 * nb, -7, dtype=np.int32)]
    f = getattr(L, entry)
    ptr = lambda a: None if a is None else a.ctypes.data                   # noqa: E731
    rc_ = f(nboxes, nwater, ptr(cells), ptr(pos), ptr(vel), ptr(pos_ref), None, 1, 0, nsteps, sample_every, dt, mass, kT, gamma, pressure, tau_p, beta_T,
            baro_every, coupling, axis, *[o.ctypes.data for o in outs])
    clean = all(bool(np.all(o == -7)) for o in outs)
    return rc_, L.mw_flex_last_error().decode(), clean


def _live(L):
    return bool(L.mw_flex_is_initialised())


def test_calls_before_init_fail_with_not_initialised():
    L = _lib()
    assert not _live(L)                                                      # (the CPU tests never initialise it)
    cells, pos = _args()
    for entry in ("mw_flex_run", "mw_flex_run_device"):
        rc_, msg, clean = _run(L, cells=cells, pos=pos, entry=entry)
        assert rc_ != 0 and "not initialised" in msg and entry in msg and clean, msg
    out = (ctypes.c_int * 10)()
    t = [ctypes.c_float(-1.0) for _ in range(5)]
    for name, call in (("mw_flex_last", lambda: L.mw_flex_last(out, 10)), ("mw_flex_elapsed_ms", lambda: L.mw_flex_elapsed_ms(*[ctypes.byref(v) for v in t]))):
        assert call() != 0, name
        msg = L.mw_flex_last_error().decode()
        assert "not initialised" in msg and name in msg, msg
    assert not any(out) and all(v.value == -1.0 for v in t)
    assert L.mw_flex_finalize() == 0                                # nothing to undo is not an error
    from mc_water_ls_mw_amd import flexcell
    with pytest.raises(flexcell.MwError, match="not initialised"):
        flexcell.flex_last()


def test_argument_validation_needs_no_device():
    L = _lib()
    cells, pos = _args(2, 4)
    singular = cells.copy()
    singular[1, 3:6] = singular[1, 0:3]
    narrow = cells.copy()
    narrow[1, 8] = 8.0                                              # box 1 is 8 bohr wide along z: below a sigma = 8.138 bohr
    just_narrow = cells.copy()
    just_narrow[1, 0] = A_SIGMA * (1.0 + 0.5e-9)
    nan, inf = float("nan"), float("inf")

    def spoiled(a, box, value):
        b = a.copy()
        b[box, 2, 1] = value
        return b

    cases = [
        (dict(nboxes=0), "nboxes"), (dict(nboxes=(1 << 24) + 1), "nboxes"), (dict(nwater=0), "nwater"), (dict(nwater=(1 << 22) + 1), "nwater"),
        (dict(cells=None), "cells"), (dict(pos=None), "pos"),
        (dict(nsteps=-1), "nsteps"), (dict(nsteps=100000001), "nsteps"), (dict(sample_every=0), "sample_every"), (dict(sample_every=-3), "sample_every"),
        (dict(dt=0.0), r"\bdt\b"), (dict(dt=-1.0), r"\bdt\b"), (dict(dt=nan), r"\bdt\b"), (dict(dt=inf), r"\bdt\b"),
        (dict(mass=0.0), "mass"), (dict(mass=-1.0), "mass"), (dict(mass=nan), "mass"), (dict(mass=inf), "mass"),
        (dict(kT=-1e-9), "kT"), (dict(kT=nan), "kT"), (dict(kT=inf), "kT"),
        (dict(gamma=-1e-9), "gamma"), (dict(gamma=nan), "gamma"), (dict(gamma=inf), "gamma"),
        (dict(pressure=nan), "pressure"), (dict(pressure=inf), "pressure"), (dict(pressure=-inf), "pressure"),
        (dict(tau_p=0.0), "tau_p"), (dict(tau_p=-1.0), "tau_p"), (dict(tau_p=nan), "tau_p"), (dict(tau_p=inf), "tau_p"),
        (dict(beta_T=0.0), "beta_T"), (dict(beta_T=-1.0), "beta_T"), (dict(beta_T=nan), "beta_T"), (dict(beta_T=inf), "beta_T"),
        (dict(baro_every=-1), "baro_every"),
        (dict(coupling=-1), "coupling"), (dict(coupling=4), "coupling"), (dict(axis=-1), "axis"), (dict(axis=3), "axis"),
        (dict(coupling=0, axis=3), "axis"),                          # checked in every coupling
        (dict(cells=narrow), r"a_sigma.*box 1\b"), (dict(cells=just_narrow), r"a_sigma.*box 1\b"), (dict(cells=singular), r"cells.*box 1\b"),
        (dict(cells=spoiled(cells.reshape(2, 3, 3), 1, nan).reshape(2, 9)), r"cells.*box 1\b"),
        (dict(pos=spoiled(pos, 1, nan)), r"\bpos\b.*box 1\b"), (dict(pos=spoiled(pos, 0, inf)), r"\bpos\b.*box 0\b"),
        (dict(vel=spoiled(pos, 1, nan)), r"\bvel\b.*box 1\b"), (dict(vel=spoiled(pos, 1, -inf)), r"\bvel\b.*box 1\b"),
        (dict(pos_ref=spoiled(pos, 1, nan)), r"\bpos_ref\b.*box 1\b"),
    ]
    for change, pattern in cases:
        kw = dict(cells=cells, pos=pos)
        kw.update(change)
        rc_, msg, clean = _run(L, **kw)
        assert rc_ != 0 and re.search(pattern, msg) and "mw_flex_run" in msg and "not initialised" not in msg and clean, (change, msg)
    # with good arguments -- the bounds themselves included -- the next thing a call without a device meets is the state
    import torch
    if not torch.cuda.is_available() and not _live(L):
        wide = cells.copy()
        wide[1, 0] = A_SIGMA * (1.0 + 1e-9) * (1.0 + 1e-15)
        for kw in (dict(), dict(nsteps=0), dict(nsteps=100000000, sample_every=100000000), dict(kT=0.0, gamma=0.0), dict(cells=wide), dict(vel=pos, pos_ref=pos),
                   dict(pressure=-1e-6), dict(pressure=0.0), dict(baro_every=0), dict(baro_every=1 << 30), dict(coupling=0, axis=0), dict(coupling=2, axis=1),
                   dict(coupling=3, axis=2)):
            full = dict(cells=cells, pos=pos)
            full.update(kw)
            rc_, msg, clean = _run(L, **full)
            assert rc_ != 0 and "not initialised" in msg and clean, msg
    # the device-pointer entry checks what it can see from the host before anything else
    for kw, pattern in ((dict(nboxes=0), "nboxes"), (dict(cells=None), "cells"), (dict(dt=nan), r"\bdt\b"), (dict(nsteps=-5), "nsteps"), (dict(gamma=-1.0), "gamma"),
                        (dict(sample_every=0), "sample_every"), (dict(pressure=nan), "pressure"), (dict(tau_p=0.0), "tau_p"), (dict(beta_T=inf), "beta_T"),
                        (dict(baro_every=-2), "baro_every"), (dict(coupling=7), "coupling"), (dict(axis=5), "axis")):
        full = dict(cells=cells, pos=pos)
        full.update(kw)
        rc_, msg, clean = _run(L, entry="mw_flex_run_device", **full)
        assert rc_ != 0 and re.search(pattern, msg) and "mw_flex_run_device" in msg and clean, msg
    from mc_water_ls_mw_amd import flexcell
    with pytest.raises(flexcell.MwError, match="coupling"):
        flexcell.molecular_dynamics_flex(np.eye(3) * 20.0, np.zeros((4, 3)), 1, 1.0, coupling="sheared")


def test_init_without_a_device_fails_with_its_message():
    import torch
    if torch.cuda.is_available():
        return                                                               # (the no-device behaviour belongs to a machine without one)
    L = _lib()
    assert L.mw_flex_init(0) != 0
    msg = L.mw_flex_last_error().decode()
    assert "no HIP device" in msg and "mw_flex_init" in msg
    assert not L.mw_flex_is_initialised()
    from mc_water_ls_mw_amd import flexcell
    with pytest.raises(flexcell.MwError, match="no HIP device"):
        flexcell.molecular_dynamics_flex(np.eye(3) * 20.0, np.zeros((4, 3)), 1, 1.0)


def test_the_diagnostic_switches_are_checked_by_init():
    """MW_FLEX_SLICE is read before the device is looked for, in a fresh process each."""
    _lib()
    code = ("import sys; from mc_water_ls_mw_amd.flexcell import load_flex_library; L = load_flex_library(); rc = L.mw_flex_init(0); "
            "print(rc != 0, L.mw_flex_last_error().decode())")
    for env in (dict(MW_FLEX_SLICE="0"), dict(MW_FLEX_SLICE="257"), dict(MW_FLEX_SLICE="x")):
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120, env=dict(os.environ, **env))
        assert out.returncode == 0 and out.stdout.startswith("True") and "MW_FLEX_SLICE" in out.stdout and "mw_flex_init" in out.stdout, (out.stdout, out.stderr)


def test_plan_matches_mw_md_plan_and_the_python_arithmetic():
    """The fields of mw_md_plan for the same inputs: geometry, grid, boxes per workgroup and steps per launch are equal; the
    scratch of a box is the molecular dynamics' plus the origin of the displacements, twelve more row doubles, four more ints, the
    cell, par, grid and eight doubles (V, three mu, three lengths), and seventeen partial values per workgroup in place of four;
    the chunking follows from it by the same rule."""
    L = _lib()
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.dynamics import load_md_library, md_plan
    from mc_water_ls_mw_amd.flexcell import MwError, PLAN_FIELDS, flex_plan
    build.build_md()
    assert L is not None and load_md_library() is not None
    budget = 256 << 20                                                       # the default one: nothing in the suite sets MW_FLEX_SCRATCH_MB or MW_MD_SCRATCH_MB in this process
    a16 = lambda v: (v + 15) // 16 * 16                                      # noqa: E731
    cells = (load_golden("ih4096_t015")["h"], np.array([[41.0, 0.0, 0.0], [9.0, 37.0, 0.0], [-6.0, 11.0, 45.0]]))
    for h in cells:
        for n in (2, 48, 64, 65, 96, 1536):
            small = n <= 64
            extra = a16(24 * n) + (a16(8 * 16) - 32) + (a16(4 * 8) - 16) + a16(72) + a16(144) + 16 + a16(8 * 8)
            if not small:
                extra += a16(8 * 17 * (-(-n // 256))) - a16(8 * 4 * (-(-n // 256)))
            for nboxes in (1, 200, 3000000):
                p, q = flex_plan(n, h, nboxes), md_plan(n, h, nboxes)
                assert set(p) == set(PLAN_FIELDS) == set(q)
                for f in ("small", "g1", "g2", "g3", "boxes_per_workgroup", "steps_per_launch"):
                    assert p[f] == q[f], (n, nboxes, f)
                assert p["scratch_bytes_per_box"] == q["scratch_bytes_per_box"] + extra, (n, p, q)
                most = min(budget // p["scratch_bytes_per_box"], (1 << 20) if small else 65535, nboxes)
                assert p["boxes_per_chunk"] == most and p["chunks"] == -(-nboxes // most), (n, nboxes, p)
                assert p["lds_bytes"] == (4 * 13 * 64 * 8 if small else 4 * 17 * 8)
    h = cells[0]
    with pytest.raises(MwError, match="one box.*does not fit"):
        flex_plan(1 << 22, h * 16.0, 1)
    narrow = np.diag([40.0, 40.0, 8.0])
    for bad, pattern in (((0, h, 1), "nwater"), ((8, h, 0), "nboxes"), ((8, h * 0.0, 1), "cell"), ((8, narrow, 1), r"a_sigma.*box 0\b")):
        with pytest.raises(MwError, match=pattern):
            flex_plan(*bad)


def test_the_read_outs_of_a_trace():
    from mc_water_ls_mw_amd import flexcell
    t = np.zeros((2, 3, 15))
    t[..., 6:12] = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    t[..., 12:15] = np.array([10.0, 20.0, 30.0])
    p = flexcell.pressure_tensor(t)
    assert p.shape == (2, 3, 3, 3) and np.array_equal(p[1, 2], np.array([[1.0, 4.0, 5.0], [4.0, 2.0, 6.0], [5.0, 6.0, 3.0]]))
    assert np.array_equal(flexcell.surface_tension(t, axis=2), np.full((2, 3), 30.0 * (3.0 - 1.5) / 2.0))
    assert np.array_equal(flexcell.surface_tension(t, axis=0, interfaces=1), np.full((2, 3), 10.0 * (1.0 - 2.5)))
    with pytest.raises(flexcell.MwError, match="columns"):
        flexcell.pressure_tensor(np.zeros((3, 6)))
    with pytest.raises(flexcell.MwError, match="axis"):
        flexcell.surface_tension(t, axis=3)


def test_flexcell_does_not_import_the_oracle():
    src = open(os.path.join(ROOT, "mc_water_ls_mw_amd", "flexcell.py")).read()
    assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M) and "oracle" not in src
    out = subprocess.run([sys.executable, "-c",
                          "import sys; import mc_water_ls_mw_amd.flexcell; print(int(any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules)))"],
                         capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "0", out.stderr
