"""CPU: libmw_tet.so builds for gfx950, loads without a GPU, exports what include/mw_tet.h declares (and nothing of it leaks
into the other libraries), keeps its kernels free of scratch memory, rejects bad arguments and uninitialised calls with
messages that name the argument, and reports its launch rules through mw_tet_plan."""
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
KERNELS = (b"k_cells_bin", b"k_cells_scan", b"k_cells_place", b"k_cells_rank", b"k_tet_select", b"k_tet_summary", b"k_tet_small")
ANG_TO_BOHR = 1.0 / 0.5291772108


def _lib():
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.tetrahedral import load_tet_library
    build.build_tet()
    return load_tet_library()


def _declared():
    text = open(os.path.join(ROOT, "include", "mw_tet.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mw_tet_\w+)\s*\(", text)))


def test_build_tet_compiles_for_gfx950():
    from mc_water_ls_mw_amd import build
    lib = build.build_tet(force=True)
    assert lib == build.TET_LIB and os.path.exists(lib)
    data = open(lib, "rb").read()
    assert b"__CLANG_OFFLOAD_BUNDLE__" in data and b"gfx950" in data
    for kernel in KERNELS:
        assert kernel in data, kernel
    header = os.path.join(ROOT, "include", "mw_tet.h")
    shared = os.path.join(build.CSRC, "mw_lib_host.h")                          # the host layer the device libraries include
    assert set(build.TET_DEPS) >= {build.TET_SRC, header, shared} and all(os.path.exists(p) for p in build.TET_DEPS)
    for deps in (build.DEPS, build.SK_DEPS, build.BOO_DEPS, build.COMMS_DEPS):   # no other library moves with it
        assert not any(p in deps for p in (build.TET_SRC, header))
    assert shared not in build.DEPS
    cells = os.path.join(build.CSRC, "mw_lib_cells.h")                          # the cell grid, sort and walks; not a .hip.h, so not libmw_hip.so's
    assert cells in build.TET_DEPS and cells not in build.DEPS and cells not in build.SK_DEPS
    assert os.path.basename(build.TET_SRC) == "mw_tet.hip" and not any("tet" in f for f in os.listdir(build.CSRC) if f.endswith(".hip.h"))


def test_every_declared_name_is_exported_and_listed():
    L = _lib()
    from mc_water_ls_mw_amd.tetrahedral import TET_ABI_SYMBOLS
    names = _declared()
    assert len(names) == 9 and sorted(TET_ABI_SYMBOLS) == names
    for name in names:
        assert hasattr(L, name), name
    text = open(os.path.join(ROOT, "include", "mw_tet.h")).read()
    assert re.search(r"#define\s+MW_TET_KEEP\s+16\b", text) and re.search(r"#define\s+MW_TET_PLAN_FIELDS\s+9\b", text)


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not in this image")
def test_the_four_libraries_keep_their_prefixes_apart():
    from mc_water_ls_mw_amd import build
    build.build()
    build.build_sk()
    build.build_boo()
    build.build_tet()

    def defined(lib):
        out = subprocess.run([READELF, "--dyn-syms", "-W", lib], capture_output=True, text=True, check=True).stdout
        rows = [ln.split() for ln in out.splitlines()]
        return {f[7].split("@")[0] for f in rows if len(f) == 8 and f[0].endswith(":") and f[6] != "UND" and f[7].startswith("mw_")}

    assert defined(build.TET_LIB) == set(_declared())
    for lib in (build.LIB, build.SK_LIB, build.BOO_LIB):
        assert not any(s.startswith("mw_tet") for s in defined(lib))
        assert b"mw_tet" not in open(lib, "rb").read() and b"k_tet_" not in open(lib, "rb").read()
    data = open(build.TET_LIB, "rb").read()
    assert b"k_boo_" not in data and b"mw_boo" not in data and b"mw_sk_" not in data
    for f in ("mw_kernels.hip.h", "mw_api.hip", "mw_boo.hip", "mw_sk.hip"):
        assert "mw_tet" not in open(os.path.join(ROOT, "mc_water_ls_mw_amd", "csrc", f)).read()


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
            p = tmp_path / "tet.co"
            p.write_bytes(data[i + o:i + o + s])
            return str(p)
    raise AssertionError("no gfx950 code object")


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not in this image")
def test_no_kernel_uses_scratch_memory_or_spills(tmp_path):
    """The 16 nearest are held in registers: a runtime-indexed array would show as a private segment, a register shortage as
    spills.  Also the selection keeps at least four wavefronts per SIMD (<= 128 VGPRs)."""
    from mc_water_ls_mw_amd import build
    build.build_tet()
    notes = subprocess.run([READELF, "--notes", _gfx950_code_object(build.TET_LIB, tmp_path)], capture_output=True, text=True, check=True).stdout
    seen = set()
    for blk in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.match(r"_ZN5mwtet\d+(k_tet_[a-z0-9]+)E", name) or re.match(r"_ZN7mwcells\d+(k_cells_[a-z]+)E", name)
        assert m, name                                                       # the library holds no other kernel
        get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))     # noqa: E731
        assert get("private_segment_fixed_size") == 0 and get("vgpr_spill_count") == 0 and get("sgpr_spill_count") == 0, name
        if m.group(1) in ("k_tet_select", "k_tet_small"):
            assert get("vgpr_count") <= 128, (name, get("vgpr_count"))
        seen.add(m.group(1).encode())
    assert seen == set(KERNELS)


def _args(nboxes=2, nwater=4):
    cells = np.tile(np.eye(3).ravel() * 20.0, (max(nboxes, 1), 1))
    pos = np.arange(max(nboxes, 1) * max(nwater, 1) * 3, dtype=np.float64) * 0.7
    return cells, pos


def _compute(L, nboxes, nwater, cells, pos, rs, rl, entry="mw_tet_compute"):
    """One compute entry with outputs prefilled so that a write would show."""
    size = max(nboxes, 1) * max(nwater, 1)
    order, near = np.full(4 * size, -7.0), np.full(4 * size, -7, dtype=np.int32)
    counts, summary = np.full(2 * size, -7, dtype=np.int32), np.full(8 * max(nboxes, 1), -7.0)
    rc_ = getattr(L, entry)(nboxes, nwater, None if cells is None else cells.ctypes.data, None if pos is None else pos.ctypes.data,
                            rs, rl, order.ctypes.data, near.ctypes.data, counts.ctypes.data, summary.ctypes.data)
    clean = bool(np.all(order == -7.0) and np.all(near == -7) and np.all(counts == -7) and np.all(summary == -7.0))
    return rc_, L.mw_tet_last_error().decode(), clean


def test_calls_before_init_fail_with_not_initialised():
    L = _lib()
    if L.mw_tet_is_initialised():
        pytest.skip("the library is live in this process")
    cells, pos = _args()
    for entry in ("mw_tet_compute", "mw_tet_compute_device"):
        rc_, msg, clean = _compute(L, 2, 4, cells, pos, 10.0, 7.0, entry)
        assert rc_ != 0 and "not initialised" in msg and entry in msg and clean, msg
    out = (ctypes.c_int * 9)()
    t = [ctypes.c_float(-1.0) for _ in range(3)]
    for name, call in (("mw_tet_last", lambda: L.mw_tet_last(out, 9)),
                       ("mw_tet_elapsed_ms", lambda: L.mw_tet_elapsed_ms(*[ctypes.byref(v) for v in t]))):
        assert call() != 0, name
        msg = L.mw_tet_last_error().decode()
        assert "not initialised" in msg and name in msg, msg
    assert not any(out) and all(v.value == -1.0 for v in t)
    assert L.mw_tet_finalize() == 0                                 # nothing to undo is not an error
    from mc_water_ls_mw_amd import tetrahedral
    with pytest.raises(tetrahedral.MwError, match="not initialised"):
        tetrahedral.tet_last()


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
        (dict(rs=0.0), "r_search"), (dict(rs=-1.0), "r_search"), (dict(rs=nan), "r_search"), (dict(rs=inf), "r_search"),
        (dict(rl=0.0), "r_lsi"), (dict(rl=-1.0), "r_lsi"), (dict(rl=nan), "r_lsi"), (dict(rl=inf), "r_lsi"),
        (dict(rl=10.0 * (1.0 + 1e-15)), r"r_lsi.*r_search"), (dict(rs=6.0), r"r_lsi.*r_search"),
        (dict(rs=20.0), r"r_search.*box 0\b"), (dict(rs=20.0 / (1.0 + 0.5e-9)), r"r_search.*box 0\b"), (dict(cells=narrow), r"r_search.*box 1\b"),
        (dict(cells=singular), r"cells.*box 1\b"), (dict(cells=nan_cell), r"cells.*box 0\b"),
    ]
    for change, pattern in cases:
        kw = dict(nboxes=2, nwater=4, cells=cells, pos=pos, rs=10.0, rl=7.0)
        kw.update(change)
        rc_, msg, clean = _compute(L, kw["nboxes"], kw["nwater"], kw["cells"], kw["pos"], kw["rs"], kw["rl"])
        assert rc_ != 0 and re.search(pattern, msg) and "mw_tet_compute" in msg and "not initialised" not in msg and clean, (change, msg)
    # r_lsi = r_search is inside the range: with good arguments the next thing a call without a device meets is the state
    import torch
    if not torch.cuda.is_available() and not L.mw_tet_is_initialised():
        rc_, msg, clean = _compute(L, 2, 4, cells, pos, 10.0, 10.0)
        assert rc_ != 0 and "not initialised" in msg and clean, msg
    # the widest supported radius passes (mw_tet_plan applies the same checks and needs no device)
    out = (ctypes.c_int * 9)()
    assert L.mw_tet_plan(4, cells.ctypes.data, 20.0 / (1.0 + 1e-9) * (1.0 - 1e-15), 2, out, 9) == 0, L.mw_tet_last_error().decode()
    assert list(out)[2:6] == [1, 1, 1, 1]
    assert L.mw_tet_plan(4, cells.ctypes.data, 20.0 / (1.0 + 0.5e-9), 2, out, 9) != 0 and "r_search" in L.mw_tet_last_error().decode()
    # the device-pointer entry checks what it can see from the host before anything else
    for kw, pattern in ((dict(nboxes=0), "nboxes"), (dict(cells=None), "cells"), (dict(rs=nan), "r_search"), (dict(rl=nan), "r_lsi"),
                        (dict(rl=11.0), r"r_lsi.*r_search")):
        full = dict(nboxes=2, nwater=4, cells=cells, pos=pos, rs=10.0, rl=7.0)
        full.update(kw)
        rc_, msg, clean = _compute(L, full["nboxes"], full["nwater"], full["cells"], full["pos"], full["rs"], full["rl"], "mw_tet_compute_device")
        assert rc_ != 0 and re.search(pattern, msg) and "mw_tet_compute_device" in msg and clean, msg


def test_init_without_a_device_fails_with_its_message():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device behaviour is checked on the CPU box")
    L = _lib()
    assert L.mw_tet_init(0) != 0
    msg = L.mw_tet_last_error().decode()
    assert "no HIP device" in msg and "mw_tet_init" in msg
    assert not L.mw_tet_is_initialised()
    from mc_water_ls_mw_amd import tetrahedral
    with pytest.raises(tetrahedral.MwError, match="no HIP device"):
        tetrahedral.tetrahedral_order(np.eye(3) * 20.0, np.zeros((4, 3)))


def _widths(h):
    vol = abs(np.linalg.det(h))
    return np.array([vol / np.linalg.norm(np.cross(h[(k + 1) % 3], h[(k + 2) % 3])) for k in range(3)])


def test_plan_reports_the_launch_rules():
    _lib()
    from mc_water_ls_mw_amd.tetrahedral import MwError, PLAN_FIELDS, load_tet_library, tet_plan
    if load_tet_library().mw_tet_is_initialised():
        pytest.skip("the library is live in this process: its budget may not be the default one")
    budget = 256 << 20
    h = load_golden("ih4096_t015")["h"]
    p = tet_plan(4096, h, 5.5, 8)
    assert set(p) == set(PLAN_FIELDS)
    per_box = p["scratch_bytes_per_box"]
    # sorted and unsorted fractional positions, three index arrays and the four values per molecule, two cell tables
    assert per_box == 4096 * (24 + 24 + 12 + 32) + 2 * 4 * (2 * 4096 + 1 + 3)
    assert 8 * per_box <= budget and p["boxes_per_chunk"] == 8 and p["chunks"] == 1 and not p["small"] and p["boxes_per_workgroup"] == 0
    p = tet_plan(4096, h, 5.5, 1024)
    assert p["boxes_per_chunk"] == budget // per_box and 1 < p["boxes_per_chunk"] < 1024 and p["chunks"] == -(-1024 // p["boxes_per_chunk"])
    with pytest.raises(MwError, match="one box.*does not fit"):
        tet_plan(1 << 22, h * 16.0, 5.5, 1)
    # the grid: floor(w_k / (r_search (1 + 1e-9))) cells per axis
    for rs_ang in (3.5, 5.5, 9.0):
        g = np.floor(_widths(h) / (rs_ang * ANG_TO_BOHR * (1.0 + 1e-9))).astype(int)
        p = tet_plan(4096, h, rs_ang, 1)
        assert (p["g1"], p["g2"], p["g3"]) == tuple(g) and g.prod() <= 2 * 4096, (rs_ang, p)
    # ... lowered from the largest until it fits max(64, 2 nwater) cells
    big = np.diag([400.0, 300.0, 100.0])
    p = tet_plan(100, big, 3.5, 1)
    assert [p["g1"], p["g2"], p["g3"]] == [5, 6, 6], p                  # (6, 6, 6) is 216 cells; ties lower the first axis
    z = load_golden("ih8_small")
    w = _widths(z["h"]).min() / ANG_TO_BOHR
    p = tet_plan(8, z["h"], 0.9999 * w, 3)
    assert (p["g1"], p["g2"], p["g3"]) == (1, 1, 1) and p["small"]
    with pytest.raises(MwError, match=r"r_search.*box 0\b"):
        tet_plan(8, z["h"], 1.0001 * w, 3)
    # the geometry switches with nwater alone, at 64
    for n, small in ((1, True), (48, True), (64, True), (65, False), (1536, False)):
        p = tet_plan(n, h, 5.5, 200)
        assert p["small"] == small and p["chunks"] == 1, (n, p)
        if small:
            assert p["boxes_per_workgroup"] == 4 and p["scratch_bytes_per_box"] == 0 and p["lds_bytes"] == 4 * 3 * 64 * 8
    assert tet_plan(48, h, 5.5, (1 << 20) + 1)["chunks"] == 2
    for bad, pattern in (((0, h, 5.5, 1), "nwater"), ((8, h, 5.5, 0), "nboxes"), ((8, h, -1.0, 1), "r_search"), ((8, h * 0.0, 5.5, 1), "cell")):
        with pytest.raises(MwError, match=pattern):
            tet_plan(*bad)


def test_tetrahedral_does_not_import_the_oracle():
    src = open(os.path.join(ROOT, "mc_water_ls_mw_amd", "tetrahedral.py")).read()
    assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M) and "oracle" not in src
    out = subprocess.run([sys.executable, "-c",
                          "import sys; import mc_water_ls_mw_amd.tetrahedral; print(int(any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules)))"],
                         capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "0", out.stderr
