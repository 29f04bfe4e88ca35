"""CPU: libmw_boo.so builds for gfx950, loads without a GPU, exports what include/mw_boo.h declares (and nothing of it leaks
into libmw_hip.so or libmw_sk.so), rejects bad arguments and uninitialised calls with messages that name the argument, and
reports its launch rules through mw_boo_plan."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
KERNELS = (b"k_cells_bin", b"k_cells_scan", b"k_cells_place", b"k_cells_rank", b"k_boo_pass1", b"k_boo_pass2", b"k_boo_summary", b"k_boo_small")
ANG_TO_BOHR = 1.0 / 0.5291772108


def _lib():
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.bondorder import load_boo_library
    build.build_boo()
    return load_boo_library()


def _declared():
    text = open(os.path.join(ROOT, "include", "mw_boo.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mw_boo_\w+)\s*\(", text)))


def test_build_boo_compiles_for_gfx950():
    from mc_water_ls_mw_amd import build
    lib = build.build_boo(force=True)
    assert lib == build.BOO_LIB and os.path.exists(lib)
    data = open(lib, "rb").read()
    assert b"__CLANG_OFFLOAD_BUNDLE__" in data and b"gfx950" in data
    for kernel in KERNELS:
        assert kernel in data, kernel
    header = os.path.join(ROOT, "include", "mw_boo.h")
    assert set(build.BOO_DEPS) >= {build.BOO_SRC, header} and all(os.path.exists(p) for p in build.BOO_DEPS)
    assert not any(p in build.DEPS for p in (build.BOO_SRC, header))             # libmw_hip.so does not move with it
    assert not any(p in build.SK_DEPS for p in (build.BOO_SRC, header))
    shared = os.path.join(build.CSRC, "mw_lib_host.h")                          # the host layer both device libraries include
    assert shared in build.SK_DEPS and shared in build.BOO_DEPS and shared not in build.DEPS
    cells = os.path.join(build.CSRC, "mw_lib_cells.h")                          # the cell grid, sort and walks; not a .hip.h, so not libmw_hip.so's
    assert cells in build.BOO_DEPS and cells not in build.DEPS and cells not in build.SK_DEPS
    assert os.path.basename(build.BOO_SRC) == "mw_boo.hip" and not any("boo" in f for f in os.listdir(build.CSRC) if f.endswith(".hip.h"))


def test_every_declared_name_is_exported_and_listed():
    L = _lib()
    from mc_water_ls_mw_amd.bondorder import BOO_ABI_SYMBOLS
    names = _declared()
    assert len(names) == 9 and sorted(BOO_ABI_SYMBOLS) == names
    for name in names:
        assert hasattr(L, name), name


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not in this image")
def test_the_three_libraries_keep_their_prefixes_apart():
    from mc_water_ls_mw_amd import build
    build.build()
    build.build_sk()
    build.build_boo()

    def defined(lib):
        out = subprocess.run([READELF, "--dyn-syms", "-W", lib], capture_output=True, text=True, check=True).stdout
        rows = [ln.split() for ln in out.splitlines()]
        return {f[7].split("@")[0] for f in rows if len(f) == 8 and f[0].endswith(":") and f[6] != "UND" and f[7].startswith("mw_")}

    assert defined(build.BOO_LIB) == set(_declared())
    for lib in (build.LIB, build.SK_LIB):
        assert not any(s.startswith("mw_boo") for s in defined(lib))
        assert b"mw_boo" not in open(lib, "rb").read() and b"k_boo_" not in open(lib, "rb").read()
    for f in ("mw_kernels.hip.h", "mw_api.hip"):
        assert "mw_boo" not in open(os.path.join(ROOT, "mc_water_ls_mw_amd", "csrc", f)).read()


def _args(nboxes=2, nwater=4):
    cells = np.tile(np.eye(3).ravel() * 20.0, (max(nboxes, 1), 1))
    pos = np.arange(max(nboxes, 1) * max(nwater, 1) * 3, dtype=np.float64) * 0.7
    return cells, pos


def _compute(L, nboxes, nwater, cells, pos, rc, thr, entry="mw_boo_compute"):
    """One compute entry with outputs prefilled so that a write would show."""
    size = max(nboxes, 1) * max(nwater, 1)
    q, nn, summary = np.full(4 * size, -7.0), np.full(2 * size, -7, dtype=np.int32), np.full(4 * max(nboxes, 1), -7.0)
    rc_ = getattr(L, entry)(nboxes, nwater, None if cells is None else cells.ctypes.data, None if pos is None else pos.ctypes.data,
                            rc, thr, q.ctypes.data, nn.ctypes.data, summary.ctypes.data)
    return rc_, L.mw_boo_last_error().decode(), bool(np.all(q == -7.0) and np.all(nn == -7) and np.all(summary == -7.0))


def test_calls_before_init_fail_with_not_initialised():
    L = _lib()
    if L.mw_boo_is_initialised():
        pytest.skip("the library is live in this process")
    cells, pos = _args()
    for entry in ("mw_boo_compute", "mw_boo_compute_device"):
        rc_, msg, clean = _compute(L, 2, 4, cells, pos, 6.0, 0.5, entry)
        assert rc_ != 0 and "not initialised" in msg and entry in msg and clean, msg
    out = (ctypes.c_int * 9)()
    t = [ctypes.c_float(-1.0) for _ in range(4)]
    for name, call in (("mw_boo_last", lambda: L.mw_boo_last(out, 9)),
                       ("mw_boo_elapsed_ms", lambda: L.mw_boo_elapsed_ms(*[ctypes.byref(v) for v in t]))):
        assert call() != 0, name
        msg = L.mw_boo_last_error().decode()
        assert "not initialised" in msg and name in msg, msg
    assert not any(out) and all(v.value == -1.0 for v in t)
    assert L.mw_boo_finalize() == 0                                 # nothing to undo is not an error
    from mc_water_ls_mw_amd import bondorder
    with pytest.raises(bondorder.MwError, match="not initialised"):
        bondorder.boo_last()


def test_argument_validation_needs_no_device():
    L = _lib()
    cells, pos = _args(2, 4)
    singular = cells.copy()
    singular[1, 3:6] = singular[1, 0:3]
    nan_cell = cells.copy()
    nan_cell[0, 4] = np.nan
    narrow = cells.copy()
    narrow[1, 8] = 5.0                                              # box 1 is 5 bohr wide along z
    cases = [
        (dict(nboxes=0), "nboxes"), (dict(nboxes=(1 << 24) + 1), "nboxes"), (dict(nwater=0), "nwater"), (dict(nwater=(1 << 22) + 1), "nwater"),
        (dict(cells=None), "cells"), (dict(pos=None), "pos"),
        (dict(rc=0.0), r"\brc\b"), (dict(rc=-1.0), r"\brc\b"), (dict(rc=float("nan")), r"\brc\b"), (dict(rc=float("inf")), r"\brc\b"),
        (dict(rc=20.0), r"\brc\b.*box 0\b"), (dict(rc=20.0 / (1.0 + 0.5e-9)), r"\brc\b.*box 0\b"), (dict(rc=6.0, cells=narrow), r"\brc\b.*box 1\b"),
        (dict(cells=singular), r"cells.*box 1\b"), (dict(cells=nan_cell), r"cells.*box 0\b"),
        (dict(thr=1.5), "threshold"), (dict(thr=-1.0001), "threshold"), (dict(thr=float("nan")), "threshold"),
    ]
    for change, pattern in cases:
        kw = dict(nboxes=2, nwater=4, cells=cells, pos=pos, rc=6.0, thr=0.5)
        kw.update(change)
        rc_, msg, clean = _compute(L, kw["nboxes"], kw["nwater"], kw["cells"], kw["pos"], kw["rc"], kw["thr"])
        assert rc_ != 0 and re.search(pattern, msg) and "mw_boo_compute" in msg and "not initialised" not in msg and clean, (change, msg)
    # the widest supported cutoff passes (mw_boo_plan applies the same checks and needs no device)
    out = (ctypes.c_int * 9)()
    assert L.mw_boo_plan(4, cells.ctypes.data, 20.0 / (1.0 + 1e-9) * (1.0 - 1e-15), 2, out, 9) == 0, L.mw_boo_last_error().decode()
    assert list(out)[2:6] == [1, 1, 1, 1]
    assert L.mw_boo_plan(4, cells.ctypes.data, 20.0 / (1.0 + 0.5e-9), 2, out, 9) != 0 and "rc" in L.mw_boo_last_error().decode()
    # the device-pointer entry checks what it can see from the host before anything else
    for kw, pattern in ((dict(nboxes=0), "nboxes"), (dict(cells=None), "cells"), (dict(rc=float("nan")), r"\brc\b"), (dict(thr=2.0), "threshold")):
        full = dict(nboxes=2, nwater=4, cells=cells, pos=pos, rc=6.0, thr=0.5)
        full.update(kw)
        rc_, msg, clean = _compute(L, full["nboxes"], full["nwater"], full["cells"], full["pos"], full["rc"], full["thr"], "mw_boo_compute_device")
        assert rc_ != 0 and re.search(pattern, msg) and "mw_boo_compute_device" in msg and clean, msg


def test_init_without_a_device_fails_with_its_message():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device behaviour is checked on the CPU box")
    L = _lib()
    assert L.mw_boo_init(0) != 0
    msg = L.mw_boo_last_error().decode()
    assert "no HIP device" in msg and "mw_boo_init" in msg
    assert not L.mw_boo_is_initialised()
    from mc_water_ls_mw_amd import bondorder
    with pytest.raises(bondorder.MwError, match="no HIP device"):
        bondorder.bond_order(np.eye(3) * 20.0, np.zeros((4, 3)))


def _widths(h):
    vol = abs(np.linalg.det(h))
    return np.array([vol / np.linalg.norm(np.cross(h[(k + 1) % 3], h[(k + 2) % 3])) for k in range(3)])


def test_plan_reports_the_launch_rules():
    _lib()
    from mc_water_ls_mw_amd.bondorder import MwError, PLAN_FIELDS, boo_plan, load_boo_library
    if load_boo_library().mw_boo_is_initialised():
        pytest.skip("the library is live in this process: its budget may not be the default one")
    budget = 256 << 20
    h = load_golden("ih4096_t015")["h"]
    p = boo_plan(4096, h, 3.5, 8)
    assert set(p) == set(PLAN_FIELDS)
    per_box = p["scratch_bytes_per_box"]
    # sorted and unsorted fractional positions, three index arrays, 24 doubles and (qbar4, qbar6) per molecule, two cell tables
    assert per_box == 4096 * (24 + 24 + 12 + 192 + 16) + 2 * 4 * (2 * 4096 + 1 + 3)
    assert 8 * per_box <= budget and p["boxes_per_chunk"] == 8 and p["chunks"] == 1 and not p["small"] and p["boxes_per_workgroup"] == 0
    p = boo_plan(4096, h, 3.5, 512)
    assert p["boxes_per_chunk"] == budget // per_box and 1 < p["boxes_per_chunk"] < 512 and p["chunks"] == -(-512 // p["boxes_per_chunk"])
    with pytest.raises(MwError, match="one box.*does not fit"):
        boo_plan(1 << 22, h * 16.0, 3.5, 1)
    # the grid: floor(w_k / (rc (1 + 1e-9))) cells per axis
    for rc_ang in (3.5, 5.0, 9.0):
        g = np.floor(_widths(h) / (rc_ang * ANG_TO_BOHR * (1.0 + 1e-9))).astype(int)
        p = boo_plan(4096, h, rc_ang, 1)
        assert (p["g1"], p["g2"], p["g3"]) == tuple(g) and g.prod() <= 2 * 4096, (rc_ang, p)
    # ... lowered from the largest until it fits max(64, 2 nwater) cells
    big = np.diag([400.0, 300.0, 100.0])
    p = boo_plan(100, big, 3.5, 1)
    g = [p["g1"], p["g2"], p["g3"]]
    assert g == [5, 6, 6], p                                          # (6, 6, 6) is 216 cells; ties lower the first axis
    z = load_golden("ih8_small")
    w = _widths(z["h"]).min() / ANG_TO_BOHR
    p = boo_plan(8, z["h"], 0.9999 * w, 3)
    assert (p["g1"], p["g2"], p["g3"]) == (1, 1, 1) and p["small"]
    with pytest.raises(MwError, match=r"\brc\b.*box 0\b"):
        boo_plan(8, z["h"], 1.0001 * w, 3)
    # the geometry switches with nwater alone
    for n, small in ((1, True), (48, True), (64, True), (65, False), (1536, False)):
        p = boo_plan(n, h, 3.5, 200)
        assert p["small"] == small and p["chunks"] == 1, (n, p)
        if small:
            assert p["boxes_per_workgroup"] == 4 and p["scratch_bytes_per_box"] == 0 and p["lds_bytes"] == 4 * 27 * 64 * 8
    assert boo_plan(48, h, 3.5, (1 << 20) + 1)["chunks"] == 2
    for bad, pattern in (((0, h, 3.5, 1), "nwater"), ((8, h, 3.5, 0), "nboxes"), ((8, h, -1.0, 1), r"\brc\b"), ((8, h * 0.0, 3.5, 1), "cell")):
        with pytest.raises(MwError, match=pattern):
            boo_plan(*bad)


def test_bondorder_does_not_import_the_oracle():
    src = open(os.path.join(ROOT, "mc_water_ls_mw_amd", "bondorder.py")).read()
    assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M) and "oracle" not in src
    out = subprocess.run([sys.executable, "-c",
                          "import sys; import mc_water_ls_mw_amd.bondorder; print(int(any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules)))"],
                         capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "0", out.stderr
