"""CPU: libmw_quench.so builds for gfx950, loads without a GPU, exports what include/mw_quench.h declares (and nothing of it
leaks into the other libraries), keeps its kernels free of scratch memory and spills, rejects bad arguments and uninitialised
calls with messages that name the argument and leaves the outputs alone, and reports its launch rules through
mw_quench_plan."""
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
KERNELS = (b"k_cells_bin", b"k_cells_scan", b"k_cells_place", b"k_cells_rank", b"k_quench_begin", b"k_quench_moments", b"k_quench_forces",
           b"k_quench_decide", b"k_quench_step", b"k_quench_move", b"k_quench_small", b"k_quench_finish")
A_SIGMA = 2.3925 / 0.5291772108 * 1.8                   # bohr
DEFAULTS = (20.0, 200.0, 0.2, 0.1, 0.99, 1.1, 0.5, 5.0)


def _lib():
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.quench import load_quench_library
    build.build_quench()
    return load_quench_library()


def _declared():
    text = open(os.path.join(ROOT, "include", "mw_quench.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mw_quench_\w+)\s*\(", text)))


def test_build_quench_compiles_for_gfx950():
    from mc_water_ls_mw_amd import build
    lib = build.build_quench(force=True)
    assert lib == build.QUENCH_LIB and os.path.exists(lib)
    data = open(lib, "rb").read()
    assert b"__CLANG_OFFLOAD_BUNDLE__" in data and b"gfx950" in data
    for kernel in KERNELS:
        assert kernel in data, kernel
    header = os.path.join(ROOT, "include", "mw_quench.h")
    shared = [os.path.join(build.CSRC, f) for f in ("mw_lib_host.h", "mw_lib_cells.h", "mw_common.hip.h")]
    assert sorted(build.QUENCH_DEPS) == sorted([build.QUENCH_SRC, header, *shared]) and all(os.path.exists(p) for p in build.QUENCH_DEPS)
    for deps in (build.DEPS, build.SK_DEPS, build.BOO_DEPS, build.TET_DEPS, build.ADF_DEPS, build.RINGS_DEPS, build.COMMS_DEPS):   # no other library moves with it
        assert not any(p in deps for p in (build.QUENCH_SRC, header))
    assert os.path.basename(build.QUENCH_SRC) == "mw_quench.hip" and not any("quench" in f for f in os.listdir(build.CSRC) if f.endswith(".hip.h"))


def test_build_entry_builds_seven_libraries():
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert len(re.findall(r"mwbuild\.build(?:_\w+)?\(\)", text)) == 8 and "mwbuild.build_quench()" in text      # the engine, the exchange layer and six device libraries
    text = open(os.path.join(ROOT, "mc_water_ls_mw_amd", "build.py")).read()
    assert re.search(r"for builder in \(.*build_quench\)", text)


def test_every_declared_name_is_exported_and_listed():
    L = _lib()
    from mc_water_ls_mw_amd.quench import FIRE_DEFAULTS, QUENCH_ABI_SYMBOLS
    names = _declared()
    assert len(names) == 9 and sorted(QUENCH_ABI_SYMBOLS) == names
    for name in names:
        assert hasattr(L, name), name
    text = open(os.path.join(ROOT, "include", "mw_quench.h")).read()
    assert re.search(r"#define\s+MW_QUENCH_PLAN_FIELDS\s+9\b", text) and re.search(r"#define\s+MW_QUENCH_MAX_ITER\s+1000000\b", text)
    m = re.search(r"#define\s+MW_QUENCH_FIRE_DEFAULTS\s+\{([^}]*)\}", text)
    assert tuple(float(v) for v in m.group(1).split(",")) == FIRE_DEFAULTS == DEFAULTS


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not in this image")
def test_the_libraries_keep_their_prefixes_apart():
    from mc_water_ls_mw_amd import build
    others = [build.build(), build.build_sk(), build.build_boo(), build.build_tet(), build.build_adf(), build.build_rings()]
    build.build_quench()

    def defined(lib):
        out = subprocess.run([READELF, "--dyn-syms", "-W", lib], capture_output=True, text=True, check=True).stdout
        rows = [ln.split() for ln in out.splitlines()]
        return {f[7].split("@")[0] for f in rows if len(f) == 8 and f[0].endswith(":") and f[6] != "UND" and f[7].startswith("mw_")}

    assert defined(build.QUENCH_LIB) == set(_declared())
    for lib in others:
        assert not any(s.startswith("mw_quench") for s in defined(lib))
        data = open(lib, "rb").read()
        assert b"mw_quench" not in data and b"k_quench_" not in data, lib
    data = open(build.QUENCH_LIB, "rb").read()
    for word in (b"k_boo_", b"mw_boo", b"mw_sk_", b"k_tet_", b"mw_tet", b"k_adf_", b"mw_adf", b"k_rings_", b"mw_rings", b"k_model_", b"mw_model_"):
        assert word not in data, word
    for f in os.listdir(build.CSRC):
        if f != "mw_quench.hip":
            assert "mw_quench" not in open(os.path.join(build.CSRC, f)).read(), f


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
            p = tmp_path / "quench.co"
            p.write_bytes(data[i + o:i + o + s])
            return str(p)
    raise AssertionError("no gfx950 code object")


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not in this image")
def test_no_kernel_uses_a_private_segment_or_spills(tmp_path):
    """The moments of a molecule and of its neighbour live in registers, the cell in vector registers (CellRegs): a
    runtime-indexed array would show as a private segment, a shortage of either kind of register as spills.  The two passes of
    the general geometry keep four wavefronts per SIMD (<= 128 VGPRs)."""
    from mc_water_ls_mw_amd import build
    build.build_quench()
    notes = subprocess.run([READELF, "--notes", _gfx950_code_object(build.QUENCH_LIB, tmp_path)], capture_output=True, text=True, check=True).stdout
    seen = set()
    for blk in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.match(r"_ZN8mwquench\d+(k_quench_[a-z]+)E", name) or re.match(r"_ZN7mwcells\d+(k_cells_[a-z]+)E", name)
        assert m, name                                                       # the library holds no other kernel
        get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))     # noqa: E731
        print(m.group(1), "vgprs", get("vgpr_count"), "sgprs", get("sgpr_count"), "lds", get("group_segment_fixed_size"))
        assert get("private_segment_fixed_size") == 0 and get("vgpr_spill_count") == 0 and get("sgpr_spill_count") == 0, name
        if m.group(1) in ("k_quench_moments", "k_quench_forces"):
            assert get("vgpr_count") <= 128, (name, get("vgpr_count"))
        if m.group(1) == "k_quench_small":
            assert get("vgpr_count") <= 256 and get("group_segment_fixed_size") == 4 * 13 * 64 * 8
        seen.add(m.group(1).encode())
    assert seen == set(KERNELS)


def _args(nboxes=2, nwater=4):
    cells = np.tile(np.eye(3).ravel() * 20.0, (max(nboxes, 1), 1))
    pos = np.arange(max(nboxes, 1) * max(nwater, 1) * 3, dtype=np.float64) * 0.7
    return cells, pos


def _compute(L, nboxes, nwater, cells, pos, ftol=1e-8, max_iter=100, fire=None, entry="mw_quench_compute"):
    """One compute entry with outputs prefilled so that a write would show."""
    size = max(nboxes, 1) * max(nwater, 1)
    pos_out, forces = np.full(3 * size, -7.0), np.full(3 * size, -7.0)
    stats, iters = np.full(6 * max(nboxes, 1), -7.0), np.full(2 * max(nboxes, 1), -7, dtype=np.int32)
    fire = None if fire is None else np.ascontiguousarray(fire, dtype=np.float64)
    rc_ = getattr(L, entry)(nboxes, nwater, None if cells is None else cells.ctypes.data, None if pos is None else pos.ctypes.data, ftol, max_iter,
                            None if fire is None else fire.ctypes.data, pos_out.ctypes.data, forces.ctypes.data, stats.ctypes.data, iters.ctypes.data)
    clean = bool(np.all(pos_out == -7.0) and np.all(forces == -7.0) and np.all(stats == -7.0) and np.all(iters == -7))
    return rc_, L.mw_quench_last_error().decode(), clean


def test_calls_before_init_fail_with_not_initialised():
    L = _lib()
    if L.mw_quench_is_initialised():
        pytest.skip("the library is live in this process")
    cells, pos = _args()
    for entry in ("mw_quench_compute", "mw_quench_compute_device"):
        rc_, msg, clean = _compute(L, 2, 4, cells, pos, entry=entry)
        assert rc_ != 0 and "not initialised" in msg and entry in msg and clean, msg
    out = (ctypes.c_int * 9)()
    t = [ctypes.c_float(-1.0) for _ in range(4)]
    for name, call in (("mw_quench_last", lambda: L.mw_quench_last(out, 9)),
                       ("mw_quench_elapsed_ms", lambda: L.mw_quench_elapsed_ms(*[ctypes.byref(v) for v in t]))):
        assert call() != 0, name
        msg = L.mw_quench_last_error().decode()
        assert "not initialised" in msg and name in msg, msg
    assert not any(out) and all(v.value == -1.0 for v in t)
    assert L.mw_quench_finalize() == 0                              # nothing to undo is not an error
    from mc_water_ls_mw_amd import quench
    with pytest.raises(quench.MwError, match="not initialised"):
        quench.quench_last()


def test_argument_validation_needs_no_device():
    L = _lib()
    cells, pos = _args(2, 4)
    singular = cells.copy()
    singular[1, 3:6] = singular[1, 0:3]
    nan_cell = cells.copy()
    nan_cell[0, 4] = np.nan
    narrow = cells.copy()
    narrow[1, 8] = 8.0                                              # box 1 is 8 bohr wide along z: below a sigma = 8.138 bohr
    just_narrow = cells.copy()
    just_narrow[1, 0] = A_SIGMA * (1.0 + 0.5e-9)
    nan, inf = float("nan"), float("inf")

    def fire(k, v):
        f = list(DEFAULTS)
        f[k] = v
        return f

    cases = [
        (dict(nboxes=0), "nboxes"), (dict(nboxes=(1 << 24) + 1), "nboxes"), (dict(nwater=0), "nwater"), (dict(nwater=(1 << 22) + 1), "nwater"),
        (dict(cells=None), "cells"), (dict(pos=None), "pos"),
        (dict(ftol=0.0), "ftol"), (dict(ftol=-1.0), "ftol"), (dict(ftol=nan), "ftol"), (dict(ftol=inf), "ftol"),
        (dict(max_iter=-1), "max_iter"), (dict(max_iter=1000001), "max_iter"),
        (dict(cells=narrow), r"a_sigma.*box 1\b"), (dict(cells=just_narrow), r"a_sigma.*box 1\b"),
        (dict(cells=singular), r"cells.*box 1\b"), (dict(cells=nan_cell), r"cells.*box 0\b"),
        (dict(fire=fire(5, 1.0)), r"fire\[5\].*f_inc"), (dict(fire=fire(5, 0.9)), r"fire\[5\].*f_inc"),
        (dict(fire=fire(6, 1.0)), r"fire\[6\].*f_dec"), (dict(fire=fire(6, 1.5)), r"fire\[6\].*f_dec"),
        (dict(fire=fire(4, 1.0)), r"fire\[4\].*f_alpha"), (dict(fire=fire(3, 1.5)), r"fire\[3\].*alpha0"),
    ]
    names = ("dt0", "dtmax", "maxstep", "alpha0", "f_alpha", "f_inc", "f_dec", "n_min")
    for k, name in enumerate(names):                                # every fire field: zero, negative, NaN and inf
        cases += [(dict(fire=fire(k, v)), r"fire\[%d\] \(%s\)" % (k, name)) for v in (0.0, -1.0, nan, inf)]
    for change, pattern in cases:
        kw = dict(nboxes=2, nwater=4, cells=cells, pos=pos, ftol=1e-8, max_iter=100, fire=None)
        kw.update(change)
        rc_, msg, clean = _compute(L, **kw)
        assert rc_ != 0 and re.search(pattern, msg) and "mw_quench_compute" in msg and "not initialised" not in msg and clean, (change, msg)
    # with good arguments -- the bounds themselves included -- the next thing a call without a device meets is the state
    import torch
    if not torch.cuda.is_available() and not L.mw_quench_is_initialised():
        wide = cells.copy()
        wide[1, 0] = A_SIGMA * (1.0 + 1e-9) * (1.0 + 1e-15)
        for kw in (dict(), dict(max_iter=0), dict(max_iter=1000000), dict(fire=DEFAULTS), dict(fire=fire(3, 1.0)), dict(cells=wide)):
            rc_, msg, clean = _compute(L, 2, 4, kw.pop("cells", cells), pos, **kw)
            assert rc_ != 0 and "not initialised" in msg and clean, msg
    # the device-pointer entry checks what it can see from the host before anything else
    for kw, pattern in ((dict(nboxes=0), "nboxes"), (dict(cells=None), "cells"), (dict(ftol=nan), "ftol"), (dict(max_iter=-5), "max_iter"),
                        (dict(fire=fire(1, inf)), r"fire\[1\]")):
        full = dict(nboxes=2, nwater=4, cells=cells, pos=pos, ftol=1e-8, max_iter=100, fire=None)
        full.update(kw)
        rc_, msg, clean = _compute(L, entry="mw_quench_compute_device", **full)
        assert rc_ != 0 and re.search(pattern, msg) and "mw_quench_compute_device" in msg and clean, msg


def test_init_without_a_device_fails_with_its_message():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device behaviour is checked on the CPU box")
    L = _lib()
    assert L.mw_quench_init(0) != 0
    msg = L.mw_quench_last_error().decode()
    assert "no HIP device" in msg and "mw_quench_init" in msg
    assert not L.mw_quench_is_initialised()
    from mc_water_ls_mw_amd import quench
    with pytest.raises(quench.MwError, match="no HIP device"):
        quench.inherent_structures(np.eye(3) * 20.0, np.zeros((4, 3)))


def test_the_diagnostic_switches_are_checked_by_init():
    """MW_QUENCH_LOOK and MW_QUENCH_SLICE are read before the device is looked for, in a fresh process each."""
    _lib()
    code = ("import sys; from mc_water_ls_mw_amd.quench import load_quench_library; L = load_quench_library(); rc = L.mw_quench_init(0); "
            "print(rc != 0, L.mw_quench_last_error().decode())")
    for env, word in ((dict(MW_QUENCH_LOOK="0"), "MW_QUENCH_LOOK"), (dict(MW_QUENCH_LOOK="4097"), "MW_QUENCH_LOOK"), (dict(MW_QUENCH_SLICE="x"), "MW_QUENCH_SLICE"),
                      (dict(MW_QUENCH_SLICE="257"), "MW_QUENCH_SLICE")):
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120, env=dict(os.environ, **env))
        assert out.returncode == 0 and out.stdout.startswith("True") and word in out.stdout and "mw_quench_init" in out.stdout, (out.stdout, out.stderr)


def test_plan_reports_the_launch_rules():
    _lib()
    from mc_water_ls_mw_amd.quench import MwError, PLAN_FIELDS, load_quench_library, quench_plan
    if load_quench_library().mw_quench_is_initialised():
        pytest.skip("the library is live in this process: its budget may not be the default one")
    budget = 256 << 20
    h = load_golden("ih4096_t015")["h"]
    p = quench_plan(4096, h, 8)
    assert set(p) == set(PLAN_FIELDS)
    per_box = p["scratch_bytes_per_box"]
    # the sort (sorted and unsorted fractional positions, three index arrays, two cell tables), moments and energy in cell order,
    # the partial sums of 16 workgroups, x, v and F, and the scalars
    assert per_box == 4096 * (24 + 24 + 12) + 2 * 4 * (2 * 4096 + 1 + 3) + 4096 * (80 + 8) + 16 * 5 * 8 + 3 * 4096 * 24 + 64 + 32 + 16
    assert 8 * per_box <= budget and p["boxes_per_chunk"] == 8 and p["chunks"] == 1 and not p["small"] and p["boxes_per_workgroup"] == 0
    p = quench_plan(4096, h, 1024)
    assert p["boxes_per_chunk"] == budget // per_box and 1 < p["boxes_per_chunk"] < 1024 and p["chunks"] == -(-1024 // p["boxes_per_chunk"])
    with pytest.raises(MwError, match="one box.*does not fit"):
        quench_plan(1 << 22, h * 16.0, 1)
    # the grid of a sigma: floor(w_k / (a sigma (1 + 1e-9))) cells per axis
    vol = abs(np.linalg.det(h))
    w = np.array([vol / np.linalg.norm(np.cross(h[(k + 1) % 3], h[(k + 2) % 3])) for k in range(3)])
    g = np.floor(w / (A_SIGMA * (1.0 + 1e-9))).astype(int)
    p = quench_plan(4096, h, 1)
    assert (p["g1"], p["g2"], p["g3"]) == tuple(g) and g.prod() <= 2 * 4096
    # the geometry switches with nwater alone, at 64
    for n, small in ((1, True), (48, True), (64, True), (65, False), (1536, False)):
        p = quench_plan(n, h, 200)
        assert p["small"] == small and p["chunks"] == 1, (n, p)
        if small:
            assert p["boxes_per_workgroup"] == 4 and p["lds_bytes"] == 4 * 13 * 64 * 8
            assert p["scratch_bytes_per_box"] == 3 * ((24 * n + 15) // 16 * 16) + 64 + 32 + 16     # x, v, F and the scalars, carried from launch to launch
    assert quench_plan(48, h, (1 << 20) + 1)["chunks"] >= 2
    narrow = np.diag([40.0, 40.0, 8.0])
    for bad, pattern in (((0, h, 1), "nwater"), ((8, h, 0), "nboxes"), ((8, h * 0.0, 1), "cell"), ((8, narrow, 1), r"a_sigma.*box 0\b")):
        with pytest.raises(MwError, match=pattern):
            quench_plan(*bad)


def test_quench_does_not_import_the_oracle():
    src = open(os.path.join(ROOT, "mc_water_ls_mw_amd", "quench.py")).read()
    assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M) and "oracle" not in src
    out = subprocess.run([sys.executable, "-c",
                          "import sys; import mc_water_ls_mw_amd.quench; print(int(any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules)))"],
                         capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "0", out.stderr
