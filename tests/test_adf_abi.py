"""CPU: libmw_adf.so builds for gfx950, loads without a GPU, exports what include/mw_adf.h declares (and nothing of it leaks
into the other libraries), keeps its kernels free of scratch memory, rejects bad arguments and uninitialised calls with
messages that name the argument, and reports its launch rules through mw_adf_plan."""
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
KERNELS = (b"k_cells_bin", b"k_cells_scan", b"k_cells_place", b"k_cells_rank", b"k_adf_angles", b"k_adf_small")
ANG_TO_BOHR = 1.0 / 0.5291772108


def _lib():
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.angles import load_adf_library
    build.build_adf()
    return load_adf_library()


def _declared():
    text = open(os.path.join(ROOT, "include", "mw_adf.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mw_adf_\w+)\s*\(", text)))


def test_build_adf_compiles_for_gfx950():
    from mc_water_ls_mw_amd import build
    lib = build.build_adf(force=True)
    assert lib == build.ADF_LIB and os.path.exists(lib)
    data = open(lib, "rb").read()
    assert b"__CLANG_OFFLOAD_BUNDLE__" in data and b"gfx950" in data
    for kernel in KERNELS:
        assert kernel in data, kernel
    header = os.path.join(ROOT, "include", "mw_adf.h")
    shared = os.path.join(build.CSRC, "mw_lib_host.h")                          # the host layer the device libraries include
    assert set(build.ADF_DEPS) >= {build.ADF_SRC, header, shared} and all(os.path.exists(p) for p in build.ADF_DEPS)
    cells = os.path.join(build.CSRC, "mw_lib_cells.h")                          # the cell grid, sort and walks; not a .hip.h, so not libmw_hip.so's
    assert cells in build.ADF_DEPS and cells not in build.DEPS and cells not in build.SK_DEPS
    for deps in (build.DEPS, build.SK_DEPS, build.BOO_DEPS, build.TET_DEPS, build.COMMS_DEPS):   # no other library moves with it
        assert not any(p in deps for p in (build.ADF_SRC, header))
    assert os.path.basename(build.ADF_SRC) == "mw_adf.hip" and not any("adf" in f for f in os.listdir(build.CSRC) if f.endswith(".hip.h"))


def test_every_declared_name_is_exported_and_listed():
    L = _lib()
    from mc_water_ls_mw_amd.angles import ADF_ABI_SYMBOLS, ADF_KEEP, PLAN_FIELDS
    from mc_water_ls_mw_amd import tetrahedral
    names = _declared()
    assert len(names) == 9 and sorted(ADF_ABI_SYMBOLS) == names
    for name in names:
        assert hasattr(L, name), name
    text = open(os.path.join(ROOT, "include", "mw_adf.h")).read()
    assert re.search(r"#define\s+MW_ADF_KEEP\s+32\b", text) and re.search(r"#define\s+MW_ADF_PLAN_FIELDS\s+9\b", text) and ADF_KEEP == 32
    assert PLAN_FIELDS == tetrahedral.PLAN_FIELDS                              # the same nine fields in the same order


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not in this image")
def test_the_library_defines_its_abi_and_nothing_else_named_mw():
    from mc_water_ls_mw_amd import build
    build.build()
    build.build_sk()
    build.build_boo()
    build.build_tet()
    build.build_adf()

    def defined(lib):
        out = subprocess.run([READELF, "--dyn-syms", "-W", lib], capture_output=True, text=True, check=True).stdout
        rows = [ln.split() for ln in out.splitlines()]
        return {f[7].split("@")[0] for f in rows if len(f) == 8 and f[0].endswith(":") and f[6] != "UND" and f[7].startswith("mw_")}

    assert defined(build.ADF_LIB) == set(_declared())
    for lib in (build.LIB, build.SK_LIB, build.BOO_LIB, build.TET_LIB):
        assert not any(s.startswith("mw_adf") for s in defined(lib))
        assert b"mw_adf" not in open(lib, "rb").read() and b"k_adf_" not in open(lib, "rb").read()
    data = open(build.ADF_LIB, "rb").read()
    assert b"k_tet_" not in data and b"mw_tet" not in data and b"k_boo_" not in data and b"mw_boo" not in data and b"mw_sk_" not in data
    for f in ("mw_kernels.hip.h", "mw_api.hip", "mw_boo.hip", "mw_sk.hip", "mw_tet.hip"):
        assert "mw_adf" not in open(os.path.join(ROOT, "mc_water_ls_mw_amd", "csrc", f)).read()


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
            p = tmp_path / "adf.co"
            p.write_bytes(data[i + o:i + o + s])
            return str(p)
    raise AssertionError("no gfx950 code object")


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not in this image")
def test_no_kernel_uses_scratch_memory_or_spills(tmp_path):
    """The kept entries live in LDS and eight unit vectors in registers under compile-time indices: a runtime-indexed array
    would show as a private segment, a register shortage as spills.  Also the two angle kernels keep at least four
    wavefronts per SIMD (<= 128 VGPRs) and declare no static LDS (theirs is sized per call)."""
    from mc_water_ls_mw_amd import build
    build.build_adf()
    notes = subprocess.run([READELF, "--notes", _gfx950_code_object(build.ADF_LIB, tmp_path)], capture_output=True, text=True, check=True).stdout
    seen = set()
    for blk in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.match(r"_ZN5mwadf\d+(k_adf_[a-z0-9]+)E", name) or re.match(r"_ZN7mwcells\d+(k_cells_[a-z]+)E", name)
        assert m, name                                                       # the library holds no other kernel
        get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))     # noqa: E731
        assert get("private_segment_fixed_size") == 0 and get("vgpr_spill_count") == 0 and get("sgpr_spill_count") == 0, name
        if m.group(1) in ("k_adf_angles", "k_adf_small"):
            assert get("vgpr_count") <= 128, (name, get("vgpr_count"))
            assert get("group_segment_fixed_size") == 0, name
        seen.add(m.group(1).encode())
    assert seen == set(KERNELS)


def _args(nboxes=2, nwater=4):
    cells = np.tile(np.eye(3).ravel() * 20.0, (max(nboxes, 1), 1))
    pos = np.arange(max(nboxes, 1) * max(nwater, 1) * 3, dtype=np.float64) * 0.7
    return cells, pos


EDGES = np.linspace(-1.0, 1.0, 11)


def _compute(L, nboxes=2, nwater=4, cells=None, pos=None, rc=10.0, nbins=10, edges=EDGES, ngroups=1, group=None, entry="mw_adf_compute"):
    """One compute entry with outputs prefilled so that a write would show."""
    nb, n = min(max(nboxes, 1), 2), min(max(nwater, 1), 4)                   # (a call that would write more is rejected on its sizes)
    hist = np.full(nb * 8 * 1024, -7, dtype=np.int64)
    counts, summary = np.full(nb * n, -7, dtype=np.int32), np.full(nb * 8 * 4, -7, dtype=np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data                       # noqa: E731
    rc_ = getattr(L, entry)(nboxes, nwater, ptr(cells), ptr(pos), rc, nbins, ptr(edges), ngroups, ptr(group), hist.ctypes.data,
                            counts.ctypes.data, summary.ctypes.data)
    clean = bool(np.all(hist == -7) and np.all(counts == -7) and np.all(summary == -7))
    return rc_, L.mw_adf_last_error().decode(), clean


def test_calls_before_init_fail_with_not_initialised():
    L = _lib()
    if L.mw_adf_is_initialised():
        pytest.skip("the library is live in this process")
    cells, pos = _args()
    for entry in ("mw_adf_compute", "mw_adf_compute_device"):
        rc_, msg, clean = _compute(L, cells=cells, pos=pos, entry=entry)
        assert rc_ != 0 and "not initialised" in msg and entry in msg and clean, msg
    out = (ctypes.c_int * 9)()
    t = [ctypes.c_float(-1.0) for _ in range(3)]
    for name, call in (("mw_adf_last", lambda: L.mw_adf_last(out, 9)),
                       ("mw_adf_elapsed_ms", lambda: L.mw_adf_elapsed_ms(*[ctypes.byref(v) for v in t]))):
        assert call() != 0, name
        msg = L.mw_adf_last_error().decode()
        assert "not initialised" in msg and name in msg, msg
    assert not any(out) and all(v.value == -1.0 for v in t)
    assert L.mw_adf_finalize() == 0                                 # nothing to undo is not an error
    from mc_water_ls_mw_amd import angles
    with pytest.raises(angles.MwError, match="not initialised"):
        angles.adf_last()


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

    def edges_with(m, v):
        e = EDGES.copy()
        e[m] = v
        return e

    good_group = np.array([[0, 1, -1, 2], [2, 2, 0, -1]], dtype=np.int32)
    bad_group = good_group.copy()
    bad_group[1, 2] = 3
    low_group = good_group.copy()
    low_group[0, 3] = -2
    cases = [
        (dict(nboxes=0), "nboxes"), (dict(nboxes=(1 << 24) + 1), "nboxes"), (dict(nwater=0), "nwater"), (dict(nwater=(1 << 22) + 1), "nwater"),
        (dict(cells=None), "cells"), (dict(pos=None), "pos"),
        (dict(rc=0.0), "r_cut"), (dict(rc=-1.0), "r_cut"), (dict(rc=nan), "r_cut"), (dict(rc=inf), "r_cut"),
        (dict(rc=20.0), r"r_cut.*box 0\b"), (dict(rc=20.0 / (1.0 + 0.5e-9)), r"r_cut.*box 0\b"), (dict(cells=narrow), r"r_cut.*box 1\b"),
        (dict(cells=singular), r"cells.*box 1\b"), (dict(cells=nan_cell), r"cells.*box 0\b"),
        (dict(nbins=0), "nbins"), (dict(nbins=-3), "nbins"), (dict(nbins=1025, edges=np.linspace(-1.0, 1.0, 1026)), "nbins"),
        (dict(edges=None), "edges"),
        (dict(edges=edges_with(4, EDGES[3])), r"edges\[3\].*edges\[4\]"), (dict(edges=edges_with(4, EDGES[6])), r"edges\[4\].*edges\[5\]"),
        (dict(edges=edges_with(5, nan)), r"edges\[5\].*finite"), (dict(edges=edges_with(10, inf)), r"edges\[10\].*finite"),
        (dict(edges=edges_with(0, -1.0 - 1e-15)), r"edges\[0\].*-1"), (dict(edges=edges_with(10, 1.0 + 1e-15)), r"edges\[10\].*above 1"),
        (dict(ngroups=0), "ngroups"), (dict(ngroups=9, group=good_group), "ngroups"),
        (dict(ngroups=3), r"group is NULL.*ngroups"),
        (dict(ngroups=3, group=bad_group), r"group = 3 of molecule 2 of box 1\b"),
        (dict(ngroups=3, group=low_group), r"group = -2 of molecule 3 of box 0\b"),
        (dict(ngroups=2, group=good_group), r"group = 2 of molecule 3 of box 0\b"),
    ]
    for change, pattern in cases:
        kw = dict(nboxes=2, nwater=4, cells=cells, pos=pos)
        kw.update(change)
        rc_, msg, clean = _compute(L, **kw)
        assert rc_ != 0 and re.search(pattern, msg) and "mw_adf_compute" in msg and "not initialised" not in msg and clean, (change, msg)
    # with good arguments the next thing a call without a device meets is the state
    import torch
    if not torch.cuda.is_available() and not L.mw_adf_is_initialised():
        for kw in (dict(), dict(ngroups=3, group=good_group), dict(nbins=1, edges=np.array([-0.5, 0.25])),
                   dict(nbins=1024, edges=np.linspace(-1.0, 1.0, 1025), ngroups=8, group=good_group)):
            rc_, msg, clean = _compute(L, cells=cells, pos=pos, **kw)
            assert rc_ != 0 and "not initialised" in msg and clean, msg
    # the widest supported radius passes (mw_adf_plan applies the same checks and needs no device)
    out = (ctypes.c_int * 9)()
    L.mw_adf_plan.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                              ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    assert L.mw_adf_plan(4, cells.ctypes.data, 20.0 / (1.0 + 1e-9) * (1.0 - 1e-15), 10, 1, 2, out, 9) == 0, L.mw_adf_last_error().decode()
    assert list(out)[2:6] == [1, 1, 1, 1]
    assert L.mw_adf_plan(4, cells.ctypes.data, 20.0 / (1.0 + 0.5e-9), 10, 1, 2, out, 9) != 0 and "r_cut" in L.mw_adf_last_error().decode()
    # the device-pointer entry checks what it can see from the host before anything else
    for kw, pattern in ((dict(nboxes=0), "nboxes"), (dict(cells=None), "cells"), (dict(rc=nan), "r_cut"), (dict(nbins=0), "nbins"),
                        (dict(edges=edges_with(2, 0.9)), r"edges\[2\]"), (dict(ngroups=2), r"group is NULL")):
        full = dict(nboxes=2, nwater=4, cells=cells, pos=pos)
        full.update(kw)
        rc_, msg, clean = _compute(L, entry="mw_adf_compute_device", **full)
        assert rc_ != 0 and re.search(pattern, msg) and "mw_adf_compute_device" in msg and clean, msg


def test_init_without_a_device_fails_with_its_message():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device behaviour is checked on the CPU box")
    L = _lib()
    assert L.mw_adf_init(0) != 0
    msg = L.mw_adf_last_error().decode()
    assert "no HIP device" in msg and "mw_adf_init" in msg
    assert not L.mw_adf_is_initialised()
    from mc_water_ls_mw_amd import angles
    with pytest.raises(angles.MwError, match="no HIP device"):
        angles.angle_counts(np.eye(3) * 20.0, np.zeros((4, 3)))


def _widths(h):
    vol = abs(np.linalg.det(h))
    return np.array([vol / np.linalg.norm(np.cross(h[(k + 1) % 3], h[(k + 2) % 3])) for k in range(3)])


def _up16(v):
    return (v + 15) & ~15


def _lds(small, nbins, ngroups):
    """edges | the box (small) | 32 entries of every lane (64 lanes small, 128 general) | the histograms | the totals"""
    return _up16(8 * (nbins + 1)) + (3 * 64 * 8 if small else 0) + 4 * 32 * (64 if small else 128) + _up16(4 * ngroups * nbins) + 16 * ngroups


def test_plan_reports_the_launch_rules():
    _lib()
    from adf_ref import cell_grid
    from mc_water_ls_mw_amd.angles import MwError, PLAN_FIELDS, adf_plan, load_adf_library
    if load_adf_library().mw_adf_is_initialised():
        pytest.skip("the library is live in this process: its budget may not be the default one")
    budget = 256 << 20
    h = load_golden("ih4096_t015")["h"]
    p = adf_plan(4096, h, 3.5, 90, 1, 8)
    assert set(p) == set(PLAN_FIELDS)
    per_box = p["scratch_bytes_per_box"]
    # sorted and unsorted fractional positions, three index arrays, two cell tables; the histogram and the totals of the box
    assert per_box == 4096 * (24 + 24 + 12) + 2 * 4 * (2 * 4096 + 1 + 3) + 8 * 90 + 32
    assert 8 * per_box <= budget and p["boxes_per_chunk"] == 8 and p["chunks"] == 1 and not p["small"] and p["boxes_per_workgroup"] == 0
    assert p["lds_bytes"] == _lds(False, 90, 1)
    p = adf_plan(4096, h, 3.5, 90, 1, 2048)
    assert p["boxes_per_chunk"] == budget // per_box and 1 < p["boxes_per_chunk"] < 2048 and p["chunks"] == -(-2048 // p["boxes_per_chunk"])
    q = adf_plan(4096, h, 3.5, 1024, 8, 2048)
    assert q["scratch_bytes_per_box"] == per_box - (8 * 90 + 32) + 8 * 8 * 1024 + 32 * 8 and q["boxes_per_chunk"] == budget // q["scratch_bytes_per_box"]
    assert q["lds_bytes"] == _lds(False, 1024, 8) <= 64 * 1024
    with pytest.raises(MwError, match="one box.*does not fit"):
        adf_plan(1 << 22, h * 16.0, 3.5, 90, 1, 1)
    # the grid: floor(w_k / (r_cut (1 + 1e-9))) cells per axis
    for rc_ang in (3.5, 4.8, 9.0):
        g = np.floor(_widths(h) / (rc_ang * ANG_TO_BOHR * (1.0 + 1e-9))).astype(int)
        p = adf_plan(4096, h, rc_ang, 90, 1, 1)
        assert (p["g1"], p["g2"], p["g3"]) == tuple(g) == cell_grid(h, rc_ang * ANG_TO_BOHR, 4096) and g.prod() <= 2 * 4096, (rc_ang, p)
    # ... lowered from the largest until it fits max(64, 2 nwater) cells
    big = np.diag([400.0, 300.0, 100.0])
    p = adf_plan(100, big, 3.5, 90, 1, 1)
    assert [p["g1"], p["g2"], p["g3"]] == [5, 6, 6] == list(cell_grid(big, 3.5 * ANG_TO_BOHR, 100)), p    # ties lower the first axis
    z = load_golden("ih8_small")
    w = _widths(z["h"]).min() / ANG_TO_BOHR
    p = adf_plan(8, z["h"], 0.9999 * w, 90, 1, 3)
    assert (p["g1"], p["g2"], p["g3"]) == (1, 1, 1) and p["small"]
    with pytest.raises(MwError, match=r"r_cut.*box 0\b"):
        adf_plan(8, z["h"], 1.0001 * w, 90, 1, 3)
    # the geometry switches with nwater alone, at 64
    for n, small in ((1, True), (48, True), (64, True), (65, False), (1536, False)):
        p = adf_plan(n, h, 3.5, 90, 6, 200)
        assert p["small"] == small and p["chunks"] == 1 and p["lds_bytes"] == _lds(small, 90, 6), (n, p)
        if small:
            assert p["boxes_per_workgroup"] == 1 and p["scratch_bytes_per_box"] == 8 * 6 * 90 + 32 * 6
    assert adf_plan(48, h, 3.5, 1, 1, (1 << 20) + 1)["chunks"] == 2         # at most 2^20 boxes per chunk
    p = adf_plan(48, h, 3.5, 1024, 8, 1 << 16)                             # the small geometry's chunks hold their histograms too
    assert p["boxes_per_chunk"] == budget // (8 * 8 * 1024 + 32 * 8) and p["chunks"] == -(-(1 << 16) // p["boxes_per_chunk"]) > 1
    for bad, pattern in (((0, h, 3.5, 90, 1, 1), "nwater"), ((8, h, 3.5, 90, 1, 0), "nboxes"), ((8, h, -1.0, 90, 1, 1), "r_cut"),
                         ((8, h * 0.0, 3.5, 90, 1, 1), "cell"), ((8, h, 3.5, 0, 1, 1), "nbins"), ((8, h, 3.5, 90, 9, 1), "ngroups")):
        with pytest.raises(MwError, match=pattern):
            adf_plan(*bad)


def test_angles_does_not_import_the_oracle():
    src = open(os.path.join(ROOT, "mc_water_ls_mw_amd", "angles.py")).read()
    assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M) and "oracle" not in src
    out = subprocess.run([sys.executable, "-c",
                          "import sys; import mc_water_ls_mw_amd.angles; print(int(any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules)))"],
                         capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "0", out.stderr
