"""CPU: libmw_md.so builds for gfx950, loads without a GPU, exports what include/mw_md.h declares (and nothing of it leaks into
the other libraries), shares the force layer with libmw_quench.so through one header, keeps its kernels free of scratch memory,
rejects bad arguments and uninitialised calls with messages that name the entry and the argument and leaves the outputs alone,
and reports its launch rules through mw_md_plan."""
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
KERNELS = (b"k_cells_bin", b"k_cells_scan", b"k_cells_place", b"k_cells_rank", b"k_md_check", b"k_md_begin", b"k_md_finish", b"k_md_drift1",
           b"k_md_drift2", b"k_md_moments", b"k_md_forces", b"k_md_row", b"k_md_small")
A_SIGMA = 2.3925 / 0.5291772108 * 1.8                   # bohr
MASS = 18.01528 * 1822.888486209
U64 = ctypes.c_ulonglong


def _lib():
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.dynamics import load_md_library
    build.build_md()
    return load_md_library()


def _declared():
    text = open(os.path.join(ROOT, "include", "mw_md.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mw_md_\w+)\s*\(", text)))


def test_build_md_compiles_for_gfx950():
    from mc_water_ls_mw_amd import build
    lib = build.build_md(force=True)
    assert lib == build.MD_LIB and os.path.exists(lib)
    data = open(lib, "rb").read()
    assert b"__CLANG_OFFLOAD_BUNDLE__" in data and b"gfx950" in data
    for kernel in KERNELS:
        assert kernel in data, kernel
    header = os.path.join(ROOT, "include", "mw_md.h")
    shared = [os.path.join(build.CSRC, f) for f in ("mw_lib_host.h", "mw_lib_cells.h", "mw_lib_forces.h", "mw_common.hip.h")]
    assert sorted(build.MD_DEPS) == sorted([build.MD_SRC, header, *shared]) and all(os.path.exists(p) for p in build.MD_DEPS)
    for deps in (build.DEPS, build.SK_DEPS, build.BOO_DEPS, build.TET_DEPS, build.ADF_DEPS, build.RINGS_DEPS, build.QUENCH_DEPS, build.COMMS_DEPS):
        assert not any(p in deps for p in (build.MD_SRC, header))           # no other library moves with it
    assert os.path.basename(build.MD_SRC) == "mw_md.hip"


def test_the_force_layer_is_one_header_that_both_libraries_watch():
    """The moments, the entry force and the reductions live in mw_lib_forces.h and nowhere else; libmw_quench.so is rebuilt when it
    changes (QUENCH_BUILD_DEPS: QUENCH_DEPS, the library's own files, plus the shared header) and so is libmw_md.so."""
    from mc_water_ls_mw_amd import build
    assert build.LIB_FORCES in build.MD_DEPS and build.LIB_FORCES in build.QUENCH_BUILD_DEPS and set(build.QUENCH_DEPS) < set(build.QUENCH_BUILD_DEPS)
    assert build.LIB_FORCES not in build.DEPS                                # not a dependency of the engine
    for src in (build.MD_SRC, build.QUENCH_SRC):
        text = open(src).read()
        assert '#include "mw_lib_forces.h"' in text
        for word in ("struct Sums", "void triplet_grad", "void entry_force", "struct CellRegs", "double dpp_wave_max", "double block_reduce"):
            assert word not in text, (src, word)
    text = open(build.LIB_FORCES).read()
    for word in ("struct Sums", "void triplet_grad", "void entry_force", "struct CellRegs", "double dpp_wave_max", "double block_reduce"):
        assert text.count(word) == 1, word


def test_build_entry_builds_the_library():
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "mwbuild.build_md(" in text
    text = open(os.path.join(ROOT, "mc_water_ls_mw_amd", "build.py")).read()
    assert re.search(r"for builder in \(.*build_md\b", text)


def test_every_declared_name_is_exported_and_listed():
    L = _lib()
    from mc_water_ls_mw_amd import dynamics
    names = _declared()
    assert len(names) == 9 and sorted(dynamics.MD_ABI_SYMBOLS) == names
    for name in names:
        assert hasattr(L, name), name
    text = open(os.path.join(ROOT, "include", "mw_md.h")).read()
    assert re.search(r"#define\s+MW_MD_PLAN_FIELDS\s+10\b", text) and len(dynamics.PLAN_FIELDS) == 10
    assert re.search(r"#define\s+MW_MD_TRACE_FIELDS\s+4\b", text) and len(dynamics.TRACE_FIELDS) == 4
    assert re.search(r"#define\s+MW_MD_MAX_STEPS\s+100000000\b", text) and dynamics.MAX_STEPS == 100000000
    m = re.search(r"#define\s+MW_MD_MASS_WATER\s+\(([\d.]+) \* ([\d.]+)\)", text)
    assert (m.group(1), m.group(2)) == ("18.01528", "1822.888486209") and dynamics.MASS_WATER == 18.01528 * 1822.888486209 == MASS
    assert "18.01528 amu x 1822.888486209 electron masses per amu" in text
    assert abs(dynamics.FS - 41.341373335) < 1e-8 and abs(dynamics.KELVIN - 3.1668115634556e-6) < 1e-18


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not in this image")
def test_the_libraries_keep_their_prefixes_apart():
    from mc_water_ls_mw_amd import build
    others = [build.build(), build.build_sk(), build.build_boo(), build.build_tet(), build.build_adf(), build.build_rings(), build.build_quench()]
    build.build_md()

    def defined(lib):
        out = subprocess.run([READELF, "--dyn-syms", "-W", lib], capture_output=True, text=True, check=True).stdout
        rows = [ln.split() for ln in out.splitlines()]
        return {f[7].split("@")[0] for f in rows if len(f) == 8 and f[0].endswith(":") and f[6] != "UND" and f[7].startswith("mw_")}

    assert defined(build.MD_LIB) == set(_declared())
    for lib in others:
        assert not any(s.startswith("mw_md") for s in defined(lib))
        data = open(lib, "rb").read()
        assert b"mw_md_" not in data and b"k_md_" not in data, lib
    data = open(build.MD_LIB, "rb").read()
    for word in (b"k_boo_", b"mw_boo", b"mw_sk_", b"k_tet_", b"mw_tet", b"k_adf_", b"mw_adf", b"k_rings_", b"mw_rings", b"k_model_", b"mw_model_",
                 b"k_quench_", b"mw_quench"):
        assert word not in data, word
    # the engine's exported names are the recorded ones
    from mc_water_ls_mw_amd.energy import ABI_SYMBOLS
    assert defined(build.LIB) >= set(ABI_SYMBOLS) and not any(s.startswith(("mw_md", "mw_quench")) for s in defined(build.LIB))


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
            p = tmp_path / "md.co"
            p.write_bytes(data[i + o:i + o + s])
            return str(p)
    raise AssertionError("no gfx950 code object")


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not in this image")
def test_no_kernel_uses_a_private_segment_or_spills_vector_registers(tmp_path):
    """As in libmw_quench.so the moments live in registers and the cell in vector registers; no kernel has a private segment or
    spills a vector register, and the two passes of the general geometry keep four wavefronts per SIMD (<= 128 VGPRs)."""
    from mc_water_ls_mw_amd import build
    build.build_md()
    notes = subprocess.run([READELF, "--notes", _gfx950_code_object(build.MD_LIB, tmp_path)], capture_output=True, text=True, check=True).stdout
    seen = set()
    for blk in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.match(r"_ZN4mwmd\d+(k_md_[a-z0-9]+)(E|ILb[01]EEE)", name) or re.match(r"_ZN7mwcells\d+(k_cells_[a-z]+)(E)", name)
        assert m, name                                                       # the library holds no other kernel
        get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))     # noqa: E731
        print(m.group(1), m.group(2), "vgprs", get("vgpr_count"), "sgprs", get("sgpr_count"), "sgpr spills", get("sgpr_spill_count"), "lds", get("group_segment_fixed_size"))
        assert get("private_segment_fixed_size") == 0 and get("vgpr_spill_count") == 0, name
        if (m.group(1), m.group(2)) != ("k_md_small", "ILb1EEE"):           # (the thermostat's instance parks scalar registers in vector lanes)
            assert get("sgpr_spill_count") == 0, name
        if m.group(1) in ("k_md_moments", "k_md_forces"):
            assert get("vgpr_count") <= 128, (name, get("vgpr_count"))
        if m.group(1) == "k_md_small":
            assert get("vgpr_count") <= 256 and get("group_segment_fixed_size") == 4 * 13 * 64 * 8
        seen.add(m.group(1).encode())
    assert seen == set(KERNELS)


def _args(nboxes=2, nwater=4):
    cells = np.tile(np.eye(3).ravel() * 20.0, (max(nboxes, 1), 1))
    pos = np.arange(max(nboxes, 1) * max(nwater, 1) * 3, dtype=np.float64).reshape(max(nboxes, 1), max(nwater, 1), 3) * 0.7
    return cells, pos


def _run(L, nboxes=2, nwater=4, cells=None, pos=None, vel=None, pos_ref=None, nsteps=10, sample_every=1, dt=100.0, mass=MASS, kT=1e-3, gamma=1e-3,
         entry="mw_md_run"):
    """One run entry with outputs prefilled so that a write would show."""
    nb = min(max(nboxes, 1), 8)                                           # (counts out of range are rejected before anything is sized by them)
    size = nb * min(max(nwater, 1), 8)
    outs = [np.full(3 * size, -7.0), np.full(3 * size, -7.0), np.full(3 * size, -7.0), np.full(4 * 200 * nb, -7.0), np.full(2 * nb, -7, dtype=np.int32)]
    f = getattr(L, entry)
    ptr = lambda a: None if a is None else a.ctypes.data                   # noqa: E731
    rc_ = f(nboxes, nwater, ptr(cells), ptr(pos), ptr(vel), ptr(pos_ref), None, 1, 0, nsteps, sample_every, dt, mass, kT, gamma, *[o.ctypes.data for o in outs])
    clean = all(bool(np.all(o == -7)) for o in outs)
    return rc_, L.mw_md_last_error().decode(), clean


def test_calls_before_init_fail_with_not_initialised():
    L = _lib()
    if L.mw_md_is_initialised():
        pytest.skip("the library is live in this process")
    cells, pos = _args()
    for entry in ("mw_md_run", "mw_md_run_device"):
        rc_, msg, clean = _run(L, cells=cells, pos=pos, entry=entry)
        assert rc_ != 0 and "not initialised" in msg and entry in msg and clean, msg
    out = (ctypes.c_int * 10)()
    t = [ctypes.c_float(-1.0) for _ in range(4)]
    for name, call in (("mw_md_last", lambda: L.mw_md_last(out, 10)), ("mw_md_elapsed_ms", lambda: L.mw_md_elapsed_ms(*[ctypes.byref(v) for v in t]))):
        assert call() != 0, name
        msg = L.mw_md_last_error().decode()
        assert "not initialised" in msg and name in msg, msg
    assert not any(out) and all(v.value == -1.0 for v in t)
    assert L.mw_md_finalize() == 0                                  # nothing to undo is not an error
    from mc_water_ls_mw_amd import dynamics
    with pytest.raises(dynamics.MwError, match="not initialised"):
        dynamics.md_last()


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
        (dict(cells=narrow), r"a_sigma.*box 1\b"), (dict(cells=just_narrow), r"a_sigma.*box 1\b"), (dict(cells=singular), r"cells.*box 1\b"),
        (dict(pos=spoiled(pos, 1, nan)), r"\bpos\b.*box 1\b"), (dict(pos=spoiled(pos, 0, inf)), r"\bpos\b.*box 0\b"),
        (dict(vel=spoiled(pos, 1, nan)), r"\bvel\b.*box 1\b"), (dict(vel=spoiled(pos, 1, -inf)), r"\bvel\b.*box 1\b"),
        (dict(pos_ref=spoiled(pos, 1, nan)), r"\bpos_ref\b.*box 1\b"),
    ]
    for change, pattern in cases:
        kw = dict(cells=cells, pos=pos)
        kw.update(change)
        rc_, msg, clean = _run(L, **kw)
        assert rc_ != 0 and re.search(pattern, msg) and "mw_md_run" in msg and "not initialised" not in msg and clean, (change, msg)
    # with good arguments -- the bounds themselves included -- the next thing a call without a device meets is the state
    import torch
    if not torch.cuda.is_available() and not L.mw_md_is_initialised():
        wide = cells.copy()
        wide[1, 0] = A_SIGMA * (1.0 + 1e-9) * (1.0 + 1e-15)
        for kw in (dict(), dict(nsteps=0), dict(nsteps=100000000, sample_every=100000000), dict(kT=0.0, gamma=0.0), dict(cells=wide), dict(vel=pos, pos_ref=pos)):
            full = dict(cells=cells, pos=pos)
            full.update(kw)
            rc_, msg, clean = _run(L, **full)
            assert rc_ != 0 and "not initialised" in msg and clean, msg
    # the device-pointer entry checks what it can see from the host before anything else
    for kw, pattern in ((dict(nboxes=0), "nboxes"), (dict(cells=None), "cells"), (dict(dt=nan), r"\bdt\b"), (dict(nsteps=-5), "nsteps"), (dict(gamma=-1.0), "gamma"),
                        (dict(sample_every=0), "sample_every")):
        full = dict(cells=cells, pos=pos)
        full.update(kw)
        rc_, msg, clean = _run(L, entry="mw_md_run_device", **full)
        assert rc_ != 0 and re.search(pattern, msg) and "mw_md_run_device" in msg and clean, msg


def test_init_without_a_device_fails_with_its_message():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device behaviour is checked on the CPU box")
    L = _lib()
    assert L.mw_md_init(0) != 0
    msg = L.mw_md_last_error().decode()
    assert "no HIP device" in msg and "mw_md_init" in msg
    assert not L.mw_md_is_initialised()
    from mc_water_ls_mw_amd import dynamics
    with pytest.raises(dynamics.MwError, match="no HIP device"):
        dynamics.molecular_dynamics(np.eye(3) * 20.0, np.zeros((4, 3)), 1, 1.0)


def test_the_diagnostic_switches_are_checked_by_init():
    """MW_MD_SLICE is read before the device is looked for, in a fresh process each."""
    _lib()
    code = ("import sys; from mc_water_ls_mw_amd.dynamics import load_md_library; L = load_md_library(); rc = L.mw_md_init(0); "
            "print(rc != 0, L.mw_md_last_error().decode())")
    for env in (dict(MW_MD_SLICE="0"), dict(MW_MD_SLICE="257"), dict(MW_MD_SLICE="x")):
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120, env=dict(os.environ, **env))
        assert out.returncode == 0 and out.stdout.startswith("True") and "MW_MD_SLICE" in out.stdout and "mw_md_init" in out.stdout, (out.stdout, out.stderr)


def test_plan_matches_the_python_arithmetic():
    _lib()
    from mc_water_ls_mw_amd.dynamics import MwError, PLAN_FIELDS, load_md_library, md_plan
    if load_md_library().mw_md_is_initialised():
        pytest.skip("the library is live in this process: its budget may not be the default one")
    budget = 256 << 20
    h = load_golden("ih4096_t015")["h"]
    a16 = lambda v: (v + 15) // 16 * 16                                      # noqa: E731
    vol = abs(np.linalg.det(h))
    w = np.array([vol / np.linalg.norm(np.cross(h[(k + 1) % 3], h[(k + 2) % 3])) for k in range(3)])
    g = np.floor(w / (A_SIGMA * (1.0 + 1e-9))).astype(int)
    for n in (48, 64, 65, 96, 1536):
        small = n <= 64
        # x, v, F, the row (4 doubles) and the ints (4) for both; the general geometry adds the sort (sorted and unsorted fractional
        # positions, three index arrays, two cell tables), moments and energy in cell order and the partial sums of its workgroups
        per_box = 3 * a16(24 * n) + 32 + 16
        if not small:
            per_box += 2 * a16(24 * n) + 3 * a16(4 * n) + 2 * a16(4 * (2 * n + 1)) + a16(80 * n) + a16(8 * n) + a16(8 * 4 * (-(-n // 256)))
        for nboxes in (1, 200, 3000000):
            p = md_plan(n, h, nboxes)
            assert set(p) == set(PLAN_FIELDS)
            most = min(budget // per_box, (1 << 20) if small else 65535, nboxes)
            assert p["scratch_bytes_per_box"] == per_box and p["small"] == small, (n, p)
            assert p["boxes_per_chunk"] == most and p["chunks"] == -(-nboxes // most), (n, nboxes, p)
            assert p["boxes_per_workgroup"] == (4 if small else 0) and p["steps_per_launch"] == (64 if small else 1)
            assert p["lds_bytes"] == (4 * 13 * 64 * 8 if small else 4 * 4 * 8)
            gg = list(g)
            while gg[0] * gg[1] * gg[2] > max(2 * n, 64):
                gg[int(np.argmax(gg))] -= 1
            assert [p["g1"], p["g2"], p["g3"]] == gg, (n, p, gg)
    with pytest.raises(MwError, match="one box.*does not fit"):
        md_plan(1 << 22, h * 16.0, 1)
    narrow = np.diag([40.0, 40.0, 8.0])
    for bad, pattern in (((0, h, 1), "nwater"), ((8, h, 0), "nboxes"), ((8, h * 0.0, 1), "cell"), ((8, narrow, 1), r"a_sigma.*box 0\b")):
        with pytest.raises(MwError, match=pattern):
            md_plan(*bad)


def test_dynamics_does_not_import_the_oracle():
    src = open(os.path.join(ROOT, "mc_water_ls_mw_amd", "dynamics.py")).read()
    assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M) and "oracle" not in src
    out = subprocess.run([sys.executable, "-c",
                          "import sys; import mc_water_ls_mw_amd.dynamics; print(int(any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules)))"],
                         capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "0", out.stderr


def test_maxwell_boltzmann_has_no_drift_and_the_right_width():
    from mc_water_ls_mw_amd.dynamics import KELVIN, MASS_WATER, maxwell_boltzmann
    v = maxwell_boltzmann(64, 96, 250.0 * KELVIN, seed=5)
    assert v.shape == (64, 96, 3) and np.abs(v.mean(axis=1)).max() < 1e-18
    var = (v * v).mean() * MASS_WATER / (250.0 * KELVIN)
    assert abs(var - 1.0) < 5.0 * np.sqrt(2.0 / v.size) + 1.0 / 96                 # (removing the drift takes one part in 96 away)
    assert np.array_equal(v, maxwell_boltzmann(64, 96, 250.0 * KELVIN, seed=5)) and not np.array_equal(v, maxwell_boltzmann(64, 96, 250.0 * KELVIN, seed=6))
    import md_ref
    assert np.array_equal(v, md_ref.maxwell_boltzmann(64, 96, 250.0 * md_ref.KELVIN, md_ref.MASS_WATER, 5))
