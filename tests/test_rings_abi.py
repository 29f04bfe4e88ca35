"""CPU: libmw_rings.so builds for gfx950, loads without a GPU, exports what include/mw_rings.h declares (and nothing of it
leaks into the other libraries), keeps its kernels free of scratch memory, rejects bad arguments and uninitialised calls with
messages that name the argument, and reports its launch rules through mw_rings_plan."""
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
KERNELS = (b"k_cells_bin", b"k_cells_scan", b"k_cells_place", b"k_cells_rank", b"k_ring_adj", b"k_ring_small", b"k_ring_rows", b"k_ring_walk",
           b"k_ring_offsets")
ANG_TO_BOHR = 1.0 / 0.5291772108


def _lib():
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.rings import load_rings_library
    build.build_rings()
    return load_rings_library()


def _declared():
    text = open(os.path.join(ROOT, "include", "mw_rings.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mw_rings_\w+)\s*\(", text)))


def test_build_rings_compiles_for_gfx950():
    from mc_water_ls_mw_amd import build
    lib = build.build_rings(force=True)
    assert lib == build.RINGS_LIB and os.path.exists(lib)
    data = open(lib, "rb").read()
    assert b"__CLANG_OFFLOAD_BUNDLE__" in data and b"gfx950" in data
    for kernel in KERNELS:
        assert kernel in data, kernel
    header = os.path.join(ROOT, "include", "mw_rings.h")
    shared = os.path.join(build.CSRC, "mw_lib_host.h")                          # the host layer the device libraries include
    common = os.path.join(build.CSRC, "mw_common.hip.h")
    cells = os.path.join(build.CSRC, "mw_lib_cells.h")                          # the cell grid, sort and walks; not a .hip.h, so not libmw_hip.so's
    assert set(build.RINGS_DEPS) == {build.RINGS_SRC, header, shared, cells, common} and all(os.path.exists(p) for p in build.RINGS_DEPS)
    assert cells not in build.DEPS and cells not in build.SK_DEPS
    for deps in (build.DEPS, build.SK_DEPS, build.BOO_DEPS, build.TET_DEPS, build.ADF_DEPS, build.COMMS_DEPS):   # no other library moves with it
        assert not any(p in deps for p in (build.RINGS_SRC, header))
    assert os.path.basename(build.RINGS_SRC) == "mw_rings.hip" and not any("ring" in f for f in os.listdir(build.CSRC) if f.endswith(".hip.h"))


def test_every_declared_name_is_exported_and_listed():
    L = _lib()
    from mc_water_ls_mw_amd.rings import PLAN_FIELDS, RING_SIZES, RINGS_ABI_SYMBOLS, RINGS_DEG
    from mc_water_ls_mw_amd import tetrahedral
    names = _declared()
    assert len(names) == 9 and sorted(RINGS_ABI_SYMBOLS) == names
    for name in names:
        assert hasattr(L, name), name
    text = open(os.path.join(ROOT, "include", "mw_rings.h")).read()
    assert re.search(r"#define\s+MW_RINGS_DEG\s+8\b", text) and re.search(r"#define\s+MW_RINGS_PLAN_FIELDS\s+9\b", text) and RINGS_DEG == 8
    assert re.search(r"#define\s+MW_RINGS_SIZES\s+5\b", text) and re.search(r"#define\s+MW_RINGS_MAX\s+7\b", text) and RING_SIZES == (3, 4, 5, 6, 7)
    assert PLAN_FIELDS == tetrahedral.PLAN_FIELDS                              # the same nine fields in the same order


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not in this image")
def test_the_library_defines_its_abi_and_nothing_else_named_mw():
    from mc_water_ls_mw_amd import build
    others = (build.build(), build.build_sk(), build.build_boo(), build.build_tet(), build.build_adf())
    build.build_rings()

    def defined(lib):
        out = subprocess.run([READELF, "--dyn-syms", "-W", lib], capture_output=True, text=True, check=True).stdout
        rows = [ln.split() for ln in out.splitlines()]
        return {f[7].split("@")[0] for f in rows if len(f) == 8 and f[0].endswith(":") and f[6] != "UND" and f[7].startswith("mw_")}

    assert defined(build.RINGS_LIB) == set(_declared())
    for lib in others:
        data = open(lib, "rb").read()
        assert not any(s.startswith("mw_rings") for s in defined(lib))
        assert b"mw_rings" not in data and b"k_ring" not in data, lib
    data = open(build.RINGS_LIB, "rb").read()
    for other in (b"k_adf_", b"mw_adf", b"k_tet_", b"mw_tet", b"k_boo_", b"mw_boo", b"mw_sk_"):
        assert other not in data, other
    for f in ("mw_kernels.hip.h", "mw_api.hip", "mw_boo.hip", "mw_sk.hip", "mw_tet.hip", "mw_adf.hip"):
        assert "mw_rings" not in open(os.path.join(ROOT, "mc_water_ls_mw_amd", "csrc", f)).read()


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
            p = tmp_path / "rings.co"
            p.write_bytes(data[i + o:i + o + s])
            return str(p)
    raise AssertionError("no gfx950 code object")


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not in this image")
def test_no_kernel_uses_scratch_memory_or_spills(tmp_path):
    """The stack of the walk lives in LDS and the eight codes of a row in registers under compile-time indices: a runtime-indexed
    array would show as a private segment, a register shortage as spills.  Every kernel keeps eight wavefronts per SIMD
    (<= 64 VGPRs), and the walk's LDS is what mw_rings_plan reports."""
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.rings import rings_plan
    build.build_rings()
    notes = subprocess.run([READELF, "--notes", _gfx950_code_object(build.RINGS_LIB, tmp_path)], capture_output=True, text=True, check=True).stdout
    seen = set()
    for blk in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.match(r"_ZN7mwrings\d+(k_ring_[a-z0-9]+)(ILb[01]EE)?E", name) or re.match(r"_ZN7mwcells\d+(k_cells_[a-z]+)E", name)
        assert m, name                                                       # the library holds no other kernel
        get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))     # noqa: E731
        assert get("private_segment_fixed_size") == 0 and get("vgpr_spill_count") == 0 and get("sgpr_spill_count") == 0, name
        assert get("vgpr_count") <= 64, (name, get("vgpr_count"))
        if m.group(1) == "k_ring_walk":
            assert get("group_segment_fixed_size") == rings_plan(100, np.eye(3) * 40.0)["lds_bytes"] == 2 * 4 * 7 * 128 + 4 * 12, name
        seen.add(m.group(1).encode())
    assert seen == set(KERNELS)


def _args(nboxes=2, nwater=4):
    cells = np.tile(np.eye(3).ravel() * 20.0, (max(nboxes, 1), 1))
    pos = np.arange(max(nboxes, 1) * max(nwater, 1) * 3, dtype=np.float64) * 0.7
    return cells, pos


def _compute(L, nboxes=2, nwater=4, cells=None, pos=None, rc=10.0, list_cap=3, entry="mw_rings_compute"):
    """One compute entry with outputs prefilled so that a write would show."""
    nb, n = min(max(nboxes, 1), 2), min(max(nwater, 1), 4)                   # (a call that would write more is rejected on its sizes)
    hist, closed, summary = np.full(nb * 5, -7, dtype=np.int64), np.full(nb * 5, -7, dtype=np.int64), np.full(nb * 4, -7, dtype=np.int64)
    member, counts, rings = np.full(nb * n * 5, -7, dtype=np.int32), np.full(nb * n, -7, dtype=np.int32), np.full(nb * 3 * 8, -7, dtype=np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data                       # noqa: E731
    rc_ = getattr(L, entry)(nboxes, nwater, ptr(cells), ptr(pos), rc, list_cap, hist.ctypes.data, closed.ctypes.data, member.ctypes.data,
                            counts.ctypes.data, summary.ctypes.data, rings.ctypes.data)
    clean = all(bool(np.all(a == -7)) for a in (hist, closed, summary, member, counts, rings))
    return rc_, L.mw_rings_last_error().decode(), clean


def test_calls_before_init_fail_with_not_initialised():
    L = _lib()
    if L.mw_rings_is_initialised():
        pytest.skip("the library is live in this process")
    cells, pos = _args()
    for entry in ("mw_rings_compute", "mw_rings_compute_device"):
        rc_, msg, clean = _compute(L, cells=cells, pos=pos, entry=entry)
        assert rc_ != 0 and "not initialised" in msg and entry in msg and clean, msg
    out = (ctypes.c_int * 9)()
    t = [ctypes.c_float(-1.0) for _ in range(3)]
    for name, call in (("mw_rings_last", lambda: L.mw_rings_last(out, 9)),
                       ("mw_rings_elapsed_ms", lambda: L.mw_rings_elapsed_ms(*[ctypes.byref(v) for v in t]))):
        assert call() != 0, name
        msg = L.mw_rings_last_error().decode()
        assert "not initialised" in msg and name in msg, msg
    assert not any(out) and all(v.value == -1.0 for v in t)
    assert L.mw_rings_finalize() == 0                               # nothing to undo is not an error
    from mc_water_ls_mw_amd import rings
    with pytest.raises(rings.MwError, match="not initialised"):
        rings.rings_last()


def test_argument_validation_needs_no_device():
    L = _lib()
    cells, pos = _args(2, 4)
    singular = cells.copy()
    singular[1, 3:6] = singular[1, 0:3]
    nan_cell = cells.copy()
    nan_cell[0, 4] = np.nan
    narrow = cells.copy()
    narrow[1, 8] = 8.0                                              # box 1 is 8 bohr wide along z
    nan, inf = float("nan"), float("inf")
    cases = [
        (dict(nboxes=0), "nboxes"), (dict(nboxes=(1 << 24) + 1), "nboxes"), (dict(nwater=0), "nwater"), (dict(nwater=(1 << 22) + 1), "nwater"),
        (dict(cells=None), "cells"), (dict(pos=None), "pos"),
        (dict(rc=0.0), "r_cut"), (dict(rc=-1.0), "r_cut"), (dict(rc=nan), "r_cut"), (dict(rc=inf), "r_cut"),
        (dict(rc=20.0), r"r_cut.*box 0\b"), (dict(rc=20.0 / (1.0 + 0.5e-9)), r"r_cut.*box 0\b"), (dict(cells=narrow), r"r_cut.*box 1\b"),
        (dict(cells=singular), r"cells.*box 1\b"), (dict(cells=nan_cell), r"cells.*box 0\b"),
        (dict(list_cap=-1), "list_cap"),
    ]
    for change, pattern in cases:
        kw = dict(nboxes=2, nwater=4, cells=cells, pos=pos)
        kw.update(change)
        for entry in ("mw_rings_compute", "mw_rings_compute_device"):
            if entry.endswith("device") and ("box" in pattern):
                continue                                                  # (the device entry reads its cells once the library is live)
            rc_, msg, clean = _compute(L, entry=entry, **kw)
            assert rc_ != 0 and re.search(pattern, msg) and entry in msg and "not initialised" not in msg and clean, (change, msg)
    # with good arguments the next thing a call without a device meets is the state
    import torch
    if not torch.cuda.is_available() and not L.mw_rings_is_initialised():
        for kw in (dict(), dict(list_cap=0), dict(nwater=1)):
            rc_, msg, clean = _compute(L, cells=cells, pos=pos, **kw)
            assert rc_ != 0 and "not initialised" in msg and clean, msg
    # the widest supported radius passes (mw_rings_plan applies the same checks and needs no device)
    out = (ctypes.c_int * 9)()
    assert L.mw_rings_plan(4, cells.ctypes.data, 20.0 / (1.0 + 1e-9) * (1.0 - 1e-15), 2, out, 9) == 0, L.mw_rings_last_error().decode()
    assert list(out)[2:6] == [1, 1, 1, 1]
    assert L.mw_rings_plan(4, cells.ctypes.data, 20.0 / (1.0 + 0.5e-9), 2, out, 9) != 0 and "r_cut" in L.mw_rings_last_error().decode()


def test_init_without_a_device_fails_with_its_message():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device behaviour is checked on the CPU box")
    L = _lib()
    assert L.mw_rings_init(0) != 0
    msg = L.mw_rings_last_error().decode()
    assert "no HIP device" in msg and "mw_rings_init" in msg
    assert not L.mw_rings_is_initialised()
    from mc_water_ls_mw_amd import rings
    with pytest.raises(rings.MwError, match="no HIP device"):
        rings.ring_statistics(np.eye(3) * 20.0, np.zeros((4, 3)))


def _widths(h):
    vol = abs(np.linalg.det(h))
    return np.array([vol / np.linalg.norm(np.cross(h[(k + 1) % 3], h[(k + 2) % 3])) for k in range(3)])


def _up16(v):
    return (v + 15) & ~15


def _scratch(n):
    """the entry counts, the first 8 codes, the sorted rows and the ring counts of the 8 lanes of every molecule; in the general
    geometry also sorted and unsorted fractional positions, three index arrays and two cell tables"""
    rows = _up16(4 * n) + 3 * 32 * n
    return rows if n <= 64 else rows + 2 * _up16(24 * n) + 3 * _up16(4 * n) + 2 * _up16(4 * (max(64, 2 * n) + 1))


def test_plan_reports_the_launch_rules():
    _lib()
    from adf_ref import cell_grid
    from mc_water_ls_mw_amd.rings import MwError, PLAN_FIELDS, load_rings_library, rings_plan
    if load_rings_library().mw_rings_is_initialised():
        pytest.skip("the library is live in this process: its budget may not be the default one")
    budget = 256 << 20
    h = load_golden("ih4096_t015")["h"]
    p = rings_plan(4096, h, 3.5, 8)
    assert set(p) == set(PLAN_FIELDS)
    per_box = p["scratch_bytes_per_box"]
    assert per_box == _scratch(4096) == 4096 * (24 + 24 + 12 + 4 + 96) + 2 * 4 * (2 * 4096 + 1 + 3)
    assert 8 * per_box <= budget and p["boxes_per_chunk"] == 8 and p["chunks"] == 1 and not p["small"] and p["boxes_per_workgroup"] == 0
    assert p["lds_bytes"] == 2 * 4 * 7 * 128 + 4 * 12
    p = rings_plan(4096, h, 3.5, 2048)
    assert p["boxes_per_chunk"] == budget // per_box and 1 < p["boxes_per_chunk"] < 2048 and p["chunks"] == -(-2048 // p["boxes_per_chunk"])
    with pytest.raises(MwError, match="one box.*does not fit"):
        rings_plan(1 << 22, h * 16.0, 3.5, 1)
    # the grid: floor(w_k / (r_cut (1 + 1e-9))) cells per axis
    for rc_ang in (3.5, 4.8, 9.0):
        g = np.floor(_widths(h) / (rc_ang * ANG_TO_BOHR * (1.0 + 1e-9))).astype(int)
        p = rings_plan(4096, h, rc_ang, 1)
        assert (p["g1"], p["g2"], p["g3"]) == tuple(g) == cell_grid(h, rc_ang * ANG_TO_BOHR, 4096) and g.prod() <= 2 * 4096, (rc_ang, p)
    # ... lowered from the largest until it fits max(64, 2 nwater) cells
    big = np.diag([400.0, 300.0, 100.0])
    p = rings_plan(100, big, 3.5, 1)
    assert [p["g1"], p["g2"], p["g3"]] == [5, 6, 6] == list(cell_grid(big, 3.5 * ANG_TO_BOHR, 100)), p    # ties lower the first axis
    z = load_golden("ih8_small")
    w = _widths(z["h"]).min() / ANG_TO_BOHR
    p = rings_plan(8, z["h"], 0.9999 * w, 3)
    assert (p["g1"], p["g2"], p["g3"]) == (1, 1, 1) and p["small"]
    with pytest.raises(MwError, match=r"r_cut.*box 0\b"):
        rings_plan(8, z["h"], 1.0001 * w, 3)
    # the geometry switches with nwater alone, at 64
    for n, small in ((1, True), (48, True), (64, True), (65, False), (1536, False)):
        p = rings_plan(n, h, 3.5, 200)
        assert p["small"] == small and p["chunks"] == 1 and p["scratch_bytes_per_box"] == _scratch(n), (n, p)
        assert p["boxes_per_workgroup"] == (1 if small else 0)
    p = rings_plan(48, h, 3.5, 1 << 17)                                    # at most 65535 boxes per chunk (the grid's second axis)
    assert p["boxes_per_chunk"] == min(65535, budget // _scratch(48)) and p["chunks"] == -(-(1 << 17) // p["boxes_per_chunk"]) > 1
    for bad, pattern in (((0, h, 3.5, 1), "nwater"), ((8, h, 3.5, 0), "nboxes"), ((8, h, -1.0, 1), "r_cut"), ((8, h * 0.0, 3.5, 1), "cell")):
        with pytest.raises(MwError, match=pattern):
            rings_plan(*bad)


def test_rings_does_not_import_the_oracle():
    src = open(os.path.join(ROOT, "mc_water_ls_mw_amd", "rings.py")).read()
    assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M) and "oracle" not in src
    out = subprocess.run([sys.executable, "-c",
                          "import sys; import mc_water_ls_mw_amd.rings; print(int(any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules)))"],
                         capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "0", out.stderr
