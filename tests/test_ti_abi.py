"""CPU: libmw_ti.so builds for gfx950, loads without a GPU, exports what include/mw_ti.h declares (and nothing of it leaks into the
other libraries, nor theirs into it), shares the cell and force layers with libmw_md.so through the headers, keeps its kernels free
of scratch memory and the small kernels at two wavefronts per SIMD, rejects bad arguments and uninitialised calls with messages
that name the entry and the argument and leaves the outputs alone, and reports the launch rules of mw_md_plan through mw_ti_plan."""
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
KERNELS = (b"k_cells_bin", b"k_cells_scan", b"k_cells_place", b"k_cells_rank", b"k_ti_check", b"k_ti_begin", b"k_ti_finish", b"k_ti_drift1",
           b"k_ti_drift2", b"k_ti_moments", b"k_ti_forces", b"k_ti_row", b"k_ti_small")
A_SIGMA = 2.3925 / 0.5291772108 * 1.8                   # bohr
MASS = 18.01528 * 1822.888486209


def _lib():
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.einstein import load_ti_library
    build.build_ti()
    return load_ti_library()


def _declared():
    text = open(os.path.join(ROOT, "include", "mw_ti.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mw_ti_\w+)\s*\(", text)))


def test_build_ti_compiles_for_gfx950():
    from mc_water_ls_mw_amd import build
    lib = build.build_ti(force=True)
    assert lib == build.TI_LIB and os.path.exists(lib)
    data = open(lib, "rb").read()
    assert b"__CLANG_OFFLOAD_BUNDLE__" in data and b"gfx950" in data
    for kernel in KERNELS:
        assert kernel in data, kernel
    header = os.path.join(ROOT, "include", "mw_ti.h")
    shared = [os.path.join(build.CSRC, f) for f in ("mw_lib_host.h", "mw_lib_cells.h", "mw_lib_forces.h", "mw_common.hip.h")]
    assert sorted(build.TI_DEPS) == sorted([build.TI_SRC, header, *shared]) and all(os.path.exists(p) for p in build.TI_DEPS)
    others = (build.DEPS, build.SK_DEPS, build.BOO_DEPS, build.TET_DEPS, build.ADF_DEPS, build.RINGS_DEPS, build.QUENCH_DEPS, build.QUENCH_BUILD_DEPS,
              build.MD_DEPS, build.NPT_DEPS, build.TCF_DEPS, build.HESS_DEPS, build.COMMS_DEPS)
    for deps in others:
        assert not any(p in deps for p in (build.TI_SRC, header))           # no other library moves with it
    sources = (build.SOURCES[0], build.SK_SRC, build.BOO_SRC, build.TET_SRC, build.ADF_SRC, build.RINGS_SRC, build.QUENCH_SRC, build.MD_SRC, build.NPT_SRC,
               build.TCF_SRC, build.HESS_SRC, build.COMMS_SRC)
    assert not any(p in build.TI_DEPS for p in sources)                      # and it moves with no other library's source
    assert os.path.basename(build.TI_SRC) == "mw_ti.hip"


def test_the_step_is_restated_and_the_force_layer_is_the_shared_header():
    from mc_water_ls_mw_amd import build
    text = open(build.TI_SRC).read()
    assert '#include "mw_lib_forces.h"' in text and '#include "mw_lib_cells.h"' in text and '#include "mw_lib_host.h"' in text
    for word in ("struct Sums", "void triplet_grad", "void entry_force", "struct CellRegs", "double dpp_wave_max", "double block_reduce"):
        assert word not in text, word
    assert "atomicAdd" not in text and "contract(off)" in text and "restated" in text
    assert "__builtin_fma(nlk, u0, oml * fx)" in text                        # the mixing as the header spells it


def test_build_entry_builds_the_library():
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "mwbuild.build_ti(" in text
    text = open(os.path.join(ROOT, "mc_water_ls_mw_amd", "build.py")).read()
    assert re.search(r"for builder in \(.*build_ti\b", text)


def test_every_declared_name_is_exported_and_listed():
    L = _lib()
    from mc_water_ls_mw_amd import dynamics, einstein
    names = _declared()
    assert len(names) == 9 and sorted(einstein.TI_ABI_SYMBOLS) == names
    for name in names:
        assert hasattr(L, name), name
    text = open(os.path.join(ROOT, "include", "mw_ti.h")).read()
    assert re.search(r"#define\s+MW_TI_PLAN_FIELDS\s+10\b", text) and len(dynamics.PLAN_FIELDS) == 10
    assert re.search(r"#define\s+MW_TI_TRACE_FIELDS\s+5\b", text) and len(einstein.TRACE_FIELDS) == 5
    assert re.search(r"#define\s+MW_TI_MAX_STEPS\s+100000000\b", text) and einstein.MAX_STEPS == 100000000 == dynamics.MAX_STEPS


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not in this image")
def test_the_libraries_keep_their_prefixes_apart():
    from mc_water_ls_mw_amd import build
    others = [build.build(), build.build_sk(), build.build_boo(), build.build_tet(), build.build_adf(), build.build_rings(), build.build_quench(),
              build.build_md(), build.build_npt(), build.build_tcf(), build.build_hess()]
    build.build_ti()

    def defined(lib):
        out = subprocess.run([READELF, "--dyn-syms", "-W", lib], capture_output=True, text=True, check=True).stdout
        rows = [ln.split() for ln in out.splitlines()]
        return {f[7].split("@")[0] for f in rows if len(f) == 8 and f[0].endswith(":") and f[6] != "UND" and f[7].startswith("mw_")}

    assert defined(build.TI_LIB) == set(_declared())
    for lib in others:
        assert not any(s.startswith("mw_ti_") for s in defined(lib))
        data = open(lib, "rb").read()
        assert b"mw_ti_" not in data and b"k_ti_" not in data, lib
    data = open(build.TI_LIB, "rb").read()
    for word in (b"k_boo_", b"mw_boo", b"mw_sk_", b"k_tet_", b"mw_tet", b"k_adf_", b"mw_adf", b"k_rings_", b"mw_rings", b"k_model_", b"mw_model_",
                 b"k_quench_", b"mw_quench", b"k_md_", b"mw_md_", b"k_npt_", b"mw_npt", b"k_tcf_", b"mw_tcf", b"k_hess_", b"mw_hess"):
        assert word not in data, word


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
            p = tmp_path / "ti.co"
            p.write_bytes(data[i + o:i + o + s])
            return str(p)
    raise AssertionError("no gfx950 code object")


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not in this image")
def test_no_kernel_uses_a_private_segment_or_spills_vector_registers(tmp_path):
    """As in libmw_md.so: no kernel has a private segment or spills a vector register, the two passes of the general geometry
    keep four wavefronts per SIMD (<= 128 VGPRs) and the small kernels two (<= 256), with the LDS of libmw_md.so's."""
    from mc_water_ls_mw_amd import build
    build.build_ti()
    notes = subprocess.run([READELF, "--notes", _gfx950_code_object(build.TI_LIB, tmp_path)], capture_output=True, text=True, check=True).stdout
    seen = set()
    for blk in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.match(r"_ZN4mwti\d+(k_ti_[a-z0-9]+)(E|ILb[01]EEE)", name) or re.match(r"_ZN7mwcells\d+(k_cells_[a-z]+)(E)", name)
        assert m, name                                                       # the library holds no other kernel
        get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))     # noqa: E731
        print(m.group(1), m.group(2), "vgprs", get("vgpr_count"), "sgprs", get("sgpr_count"), "sgpr spills", get("sgpr_spill_count"), "lds", get("group_segment_fixed_size"))
        assert get("private_segment_fixed_size") == 0 and get("vgpr_spill_count") == 0, name
        if m.group(1) != "k_ti_small":
            assert get("sgpr_spill_count") == 0, name
        if m.group(1) in ("k_ti_moments", "k_ti_forces"):
            assert get("vgpr_count") <= 128, (name, get("vgpr_count"))
        if m.group(1) == "k_ti_small":
            assert get("vgpr_count") <= 256 and get("group_segment_fixed_size") == 4 * 13 * 64 * 8
        seen.add(m.group(1).encode())
    assert seen == set(KERNELS)


def _args(nboxes=2, nwater=4):
    cells = np.tile(np.eye(3).ravel() * 20.0, (max(nboxes, 1), 1))
    pos = np.arange(max(nboxes, 1) * max(nwater, 1) * 3, dtype=np.float64).reshape(max(nboxes, 1), max(nwater, 1), 3) * 0.7
    return cells, pos


_DEFAULT = object()


def _run(L, nboxes=2, nwater=4, cells=None, pos=None, vel=None, sites=None, lambdas=_DEFAULT, springs=_DEFAULT, nsteps=10, sample_every=1, equil_steps=2,
         block_steps=3, dt=100.0, mass=MASS, kT=1e-3, gamma=1e-3, entry="mw_ti_run"):
    """One run entry with outputs prefilled so that a write would show."""
    nb = min(max(nboxes, 1), 8)                                           # (counts out of range are rejected before anything is sized by them)
    size = nb * min(max(nwater, 1), 8)
    if lambdas is _DEFAULT:
        lambdas = np.linspace(0.0, 1.0, nb)
    if springs is _DEFAULT:
        springs = np.full(nb, 0.02)
    outs = [np.full(3 * size, -7.0), np.full(3 * size, -7.0), np.full(3 * size, -7.0), np.full(5 * 200 * nb, -7.0), np.full(5 * 200 * nb, -7.0),
            np.full(2 * nb, -7, dtype=np.int32)]
    f = getattr(L, entry)
    ptr = lambda a: None if a is None else a.ctypes.data                   # noqa: E731
    rc_ = f(nboxes, nwater, ptr(cells), ptr(pos), ptr(vel), ptr(sites), ptr(lambdas), ptr(springs), None, 1, 0, nsteps, sample_every, equil_steps,
            block_steps, dt, mass, kT, gamma, *[o.ctypes.data for o in outs])
    clean = all(bool(np.all(o == -7)) for o in outs)
    return rc_, L.mw_ti_last_error().decode(), clean


def test_calls_before_init_fail_with_not_initialised():
    L = _lib()
    if L.mw_ti_is_initialised():
        pytest.skip("the library is live in this process")
    cells, pos = _args()
    for entry in ("mw_ti_run", "mw_ti_run_device"):
        rc_, msg, clean = _run(L, cells=cells, pos=pos, sites=pos, entry=entry)
        assert rc_ != 0 and "not initialised" in msg and entry in msg and clean, msg
    out = (ctypes.c_int * 10)()
    t = [ctypes.c_float(-1.0) for _ in range(4)]
    for name, call in (("mw_ti_last", lambda: L.mw_ti_last(out, 10)), ("mw_ti_elapsed_ms", lambda: L.mw_ti_elapsed_ms(*[ctypes.byref(v) for v in t]))):
        assert call() != 0, name
        msg = L.mw_ti_last_error().decode()
        assert "not initialised" in msg and name in msg, msg
    assert not any(out) and all(v.value == -1.0 for v in t)
    assert L.mw_ti_finalize() == 0                                  # nothing to undo is not an error
    from mc_water_ls_mw_amd import einstein
    with pytest.raises(einstein.MwError, match="not initialised"):
        einstein.ti_last()


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

    arr = lambda *v: np.array(v, dtype=np.float64)                          # noqa: E731
    cases = [
        (dict(nboxes=0), "nboxes"), (dict(nboxes=(1 << 24) + 1), "nboxes"), (dict(nwater=0), "nwater"), (dict(nwater=(1 << 22) + 1), "nwater"),
        (dict(cells=None), "cells"), (dict(sites=None), "sites"), (dict(lambdas=None), "lambdas"), (dict(springs=None), "springs"),
        (dict(nsteps=-1), "nsteps"), (dict(nsteps=100000001), "nsteps"), (dict(sample_every=0), "sample_every"), (dict(sample_every=-3), "sample_every"),
        (dict(equil_steps=-1), "equil_steps"), (dict(block_steps=-1), "block_steps"),
        (dict(dt=0.0), r"\bdt\b"), (dict(dt=-1.0), r"\bdt\b"), (dict(dt=nan), r"\bdt\b"), (dict(dt=inf), r"\bdt\b"),
        (dict(mass=0.0), "mass"), (dict(mass=-1.0), "mass"), (dict(mass=nan), "mass"), (dict(mass=inf), "mass"),
        (dict(kT=-1e-9), "kT"), (dict(kT=nan), "kT"), (dict(kT=inf), "kT"),
        (dict(gamma=-1e-9), "gamma"), (dict(gamma=nan), "gamma"), (dict(gamma=inf), "gamma"),
        (dict(lambdas=arr(0.5, 1.0000001)), r"lambdas.*box 1\b"), (dict(lambdas=arr(-1e-12, 0.5)), r"lambdas.*box 0\b"), (dict(lambdas=arr(0.5, nan)), r"lambdas.*box 1\b"),
        (dict(lambdas=arr(inf, 0.5)), r"lambdas.*box 0\b"),
        (dict(springs=arr(0.02, 0.0)), r"springs.*box 1\b"), (dict(springs=arr(-0.02, 0.02)), r"springs.*box 0\b"), (dict(springs=arr(0.02, nan)), r"springs.*box 1\b"),
        (dict(springs=arr(0.02, inf)), r"springs.*box 1\b"),
        (dict(cells=narrow), r"a_sigma.*box 1\b"), (dict(cells=just_narrow), r"a_sigma.*box 1\b"), (dict(cells=singular), r"cells.*box 1\b"),
        (dict(cells=spoiled(cells.reshape(2, 3, 3), 1, nan).reshape(2, 9)), r"cells.*box 1\b"),
        (dict(pos=spoiled(pos, 1, nan)), r"\bpos\b.*box 1\b"), (dict(pos=spoiled(pos, 0, inf)), r"\bpos\b.*box 0\b"),
        (dict(vel=spoiled(pos, 1, nan)), r"\bvel\b.*box 1\b"), (dict(vel=spoiled(pos, 1, -inf)), r"\bvel\b.*box 1\b"),
        (dict(sites=spoiled(pos, 1, nan)), r"\bsites\b.*box 1\b"), (dict(sites=spoiled(pos, 0, -inf)), r"\bsites\b.*box 0\b"),
    ]
    for change, pattern in cases:
        kw = dict(cells=cells, pos=pos, sites=pos)
        kw.update(change)
        rc_, msg, clean = _run(L, **kw)
        assert rc_ != 0 and re.search(pattern, msg) and "mw_ti_run" in msg and "not initialised" not in msg and clean, (change, msg)
    # with good arguments -- the bounds themselves included -- the next thing a call without a device meets is the state
    import torch
    if not torch.cuda.is_available() and not L.mw_ti_is_initialised():
        wide = cells.copy()
        wide[1, 0] = A_SIGMA * (1.0 + 1e-9) * (1.0 + 1e-15)
        for kw in (dict(), dict(nsteps=0), dict(nsteps=100000000, sample_every=100000000), dict(kT=0.0, gamma=0.0), dict(cells=wide), dict(vel=pos), dict(pos=None),
                   dict(lambdas=arr(0.0, 1.0)), dict(springs=arr(1e-300, 1e300)), dict(equil_steps=0, block_steps=0), dict(equil_steps=1 << 30, block_steps=1 << 30)):
            full = dict(cells=cells, pos=pos, sites=pos)
            full.update(kw)
            rc_, msg, clean = _run(L, **full)
            assert rc_ != 0 and "not initialised" in msg and clean, msg
    # the device-pointer entry checks what it can see from the host before anything else
    for kw, pattern in ((dict(nboxes=0), "nboxes"), (dict(cells=None), "cells"), (dict(sites=None), "sites"), (dict(lambdas=None), "lambdas"), (dict(springs=None), "springs"),
                        (dict(dt=nan), r"\bdt\b"), (dict(nsteps=-5), "nsteps"), (dict(gamma=-1.0), "gamma"), (dict(sample_every=0), "sample_every"),
                        (dict(equil_steps=-2), "equil_steps"), (dict(block_steps=-2), "block_steps")):
        full = dict(cells=cells, pos=pos, sites=pos)
        full.update(kw)
        rc_, msg, clean = _run(L, entry="mw_ti_run_device", **full)
        assert rc_ != 0 and re.search(pattern, msg) and "mw_ti_run_device" in msg and clean, msg


def test_init_without_a_device_fails_with_its_message():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device behaviour is checked on the CPU box")
    L = _lib()
    assert L.mw_ti_init(0) != 0
    msg = L.mw_ti_last_error().decode()
    assert "no HIP device" in msg and "mw_ti_init" in msg
    assert not L.mw_ti_is_initialised()
    from mc_water_ls_mw_amd import einstein
    with pytest.raises(einstein.MwError, match="no HIP device"):
        einstein.einstein_md(np.eye(3) * 20.0, np.zeros((4, 3)), 0.5, 0.02, 1, 1.0)


def test_the_diagnostic_switches_are_checked_by_init():
    """MW_TI_SLICE is read before the device is looked for, in a fresh process each."""
    _lib()
    code = ("import sys; from mc_water_ls_mw_amd.einstein import load_ti_library; L = load_ti_library(); rc = L.mw_ti_init(0); "
            "print(rc != 0, L.mw_ti_last_error().decode())")
    for env in (dict(MW_TI_SLICE="0"), dict(MW_TI_SLICE="257"), dict(MW_TI_SLICE="x")):
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120, env=dict(os.environ, **env))
        assert out.returncode == 0 and out.stdout.startswith("True") and "MW_TI_SLICE" in out.stdout and "mw_ti_init" in out.stdout, (out.stdout, out.stderr)


def test_plan_matches_mw_md_plan_and_the_python_arithmetic():
    """The fields of mw_md_plan for the same inputs: geometry, grid, boxes per workgroup and steps per launch are equal; the scratch
    of a box is the molecular dynamics' plus a fifth row double, the five block accumulators and three more partial sums per
    workgroup; the chunking follows from it by the same rule."""
    _lib()
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.dynamics import load_md_library, md_plan
    from mc_water_ls_mw_amd.einstein import MwError, load_ti_library, ti_plan
    from mc_water_ls_mw_amd.dynamics import PLAN_FIELDS
    build.build_md()
    if load_ti_library().mw_ti_is_initialised() or load_md_library().mw_md_is_initialised():
        pytest.skip("a library is live in this process: its budget may not be the default one")
    budget = 256 << 20
    a16 = lambda v: (v + 15) // 16 * 16                                      # noqa: E731
    cells = (load_golden("ih4096_t015")["h"], np.array([[41.0, 0.0, 0.0], [9.0, 37.0, 0.0], [-6.0, 11.0, 45.0]]))
    for h in cells:
        for n in (48, 64, 65, 96, 1536):
            small = n <= 64
            extra = (a16(8 * 5) - a16(8 * 4)) + a16(8 * 5)
            if not small:
                extra += a16(8 * 7 * (-(-n // 256))) - a16(8 * 4 * (-(-n // 256)))
            for nboxes in (1, 200, 3000000):
                p, q = ti_plan(n, h, nboxes), md_plan(n, h, nboxes)
                assert set(p) == set(PLAN_FIELDS) == set(q)
                for f in ("small", "g1", "g2", "g3", "boxes_per_workgroup", "steps_per_launch"):
                    assert p[f] == q[f], (n, nboxes, f)
                assert p["scratch_bytes_per_box"] == q["scratch_bytes_per_box"] + extra, (n, p, q)
                most = min(budget // p["scratch_bytes_per_box"], (1 << 20) if small else 65535, nboxes)
                assert p["boxes_per_chunk"] == most and p["chunks"] == -(-nboxes // most), (n, nboxes, p)
                assert p["lds_bytes"] == (4 * 13 * 64 * 8 if small else 4 * 7 * 8)
    h = cells[0]
    with pytest.raises(MwError, match="one box.*does not fit"):
        ti_plan(1 << 22, h * 16.0, 1)
    narrow = np.diag([40.0, 40.0, 8.0])
    for bad, pattern in (((0, h, 1), "nwater"), ((8, h, 0), "nboxes"), ((8, h * 0.0, 1), "cell"), ((8, narrow, 1), r"a_sigma.*box 0\b")):
        with pytest.raises(MwError, match=pattern):
            ti_plan(*bad)


def test_einstein_does_not_import_the_oracle():
    src = open(os.path.join(ROOT, "mc_water_ls_mw_amd", "einstein.py")).read()
    assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M) and "oracle" not in src
    out = subprocess.run([sys.executable, "-c",
                          "import sys; import mc_water_ls_mw_amd.einstein; print(int(any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules)))"],
                         capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "0", out.stderr
