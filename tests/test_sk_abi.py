"""CPU: libmw_sk.so builds for gfx950, loads without a GPU, exports what include/mw_sk.h declares (and nothing of it leaks
into libmw_hip.so), rejects bad arguments and uninitialised calls with messages that name the argument, and reports its
launch rules through mw_sk_plan."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)


def _lib():
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.structure import load_sk_library
    build.build_sk()
    return load_sk_library()


def _declared():
    text = open(os.path.join(ROOT, "include", "mw_sk.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mw_sk_\w+)\s*\(", text)))


def test_build_sk_compiles_for_gfx950():
    from mc_water_ls_mw_amd import build
    lib = build.build_sk(force=True)
    assert lib == build.SK_LIB and os.path.exists(lib)
    data = open(lib, "rb").read()
    assert b"__CLANG_OFFLOAD_BUNDLE__" in data and b"gfx950" in data
    for kernel in (b"k_sk_phasors", b"k_sk_sum", b"k_sk_finish", b"k_sk_mean"):
        assert kernel in data, kernel
    assert set(build.SK_DEPS) >= {build.SK_SRC, os.path.join(ROOT, "include", "mw_sk.h")}
    assert all(os.path.exists(p) for p in build.SK_DEPS)
    assert not any(p in build.DEPS for p in (build.SK_SRC, os.path.join(ROOT, "include", "mw_sk.h")))   # libmw_hip.so does not move with it


def test_every_declared_name_is_exported_and_listed():
    L = _lib()
    from mc_water_ls_mw_amd.structure import SK_ABI_SYMBOLS
    names = _declared()
    assert len(names) == 10 and sorted(SK_ABI_SYMBOLS) == names
    for name in names:
        assert hasattr(L, name), name


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not in this image")
def test_the_two_libraries_keep_their_prefixes_apart():
    from mc_water_ls_mw_amd import build
    build.build()
    build.build_sk()

    def defined(lib):
        out = subprocess.run([READELF, "--dyn-syms", "-W", lib], capture_output=True, text=True, check=True).stdout
        rows = [ln.split() for ln in out.splitlines()]
        return {f[7].split("@")[0] for f in rows if len(f) == 8 and f[0].endswith(":") and f[6] != "UND" and f[7].startswith("mw_")}

    sk, hip = defined(build.SK_LIB), defined(build.LIB)
    assert sk == set(_declared())
    assert not any(s.startswith("mw_sk_") for s in hip)
    src = open(os.path.join(ROOT, "mc_water_ls_mw_amd", "csrc", "mw_kernels.hip.h")).read() + \
        open(os.path.join(ROOT, "mc_water_ls_mw_amd", "csrc", "mw_api.hip")).read()
    assert "mw_sk" not in src


def _args(nboxes=1, nwater=4, M=3):
    cells = np.tile(np.eye(3).ravel() * 10.0, (max(nboxes, 1), 1))
    pos = np.arange(max(nboxes, 1) * max(nwater, 1) * 3, dtype=np.float64) * 0.1
    nvec = np.array([[1, 0, 0], [0, -2, 0], [3, 3, 3]] * max(1, -(-max(M, 1) // 3)), dtype=np.int32)[:max(M, 1)].copy()
    return cells, pos, nvec


def _entries(L, nboxes, nwater, cells, pos, M, nvec, ngroups=1):
    """Every compute entry on the same arguments, with outputs prefilled so that a write would show."""
    cp = None if cells is None else cells.ctypes.data_as(_dp)
    pp = None if pos is None else pos.ctypes.data_as(_dp)
    vp = None if nvec is None else nvec.ctypes.data_as(_ip)
    size = max(nboxes, 1) * max(M, 1)
    rho, S, mean = np.full(2 * size, -7.0), np.full(size, -7.0), np.full(size, -7.0)
    calls = {"mw_sk_compute": lambda: L.mw_sk_compute(nboxes, nwater, cp, pp, M, vp, rho.ctypes.data_as(_dp), S.ctypes.data_as(_dp)),
             "mw_sk_mean": lambda: L.mw_sk_mean(nboxes, nwater, cp, pp, M, vp, ngroups, mean.ctypes.data_as(_dp))}
    return calls, (rho, S, mean)


def test_calls_before_init_fail_with_not_initialised():
    L = _lib()
    if L.mw_sk_is_initialised():
        pytest.skip("the library is live in this process")
    cells, pos, nvec = _args()
    calls, outs = _entries(L, 1, 4, cells, pos, 3, nvec)
    calls["mw_sk_compute_device"] = lambda: L.mw_sk_compute_device(1, 4, cells.ctypes.data_as(_dp), pos.ctypes.data_as(_dp), 3,
                                                                   nvec.ctypes.data_as(_ip), None, None)
    out = (ctypes.c_int * 9)()
    a, b = ctypes.c_float(-1.0), ctypes.c_float(-1.0)
    calls["mw_sk_last"] = lambda: L.mw_sk_last(out, 9)
    calls["mw_sk_elapsed_ms"] = lambda: L.mw_sk_elapsed_ms(ctypes.byref(a), ctypes.byref(b))
    for name, call in calls.items():
        assert call() != 0, name
        msg = L.mw_sk_last_error().decode()
        assert "not initialised" in msg and name in msg, msg
    assert all(np.all(o == -7.0) for o in outs) and a.value == -1.0 and not any(out)
    assert L.mw_sk_finalize() == 0                                  # nothing to undo is not an error
    from mc_water_ls_mw_amd import structure
    with pytest.raises(structure.MwError, match="not initialised"):
        structure.sk_last()


def test_argument_validation_needs_no_device():
    L = _lib()
    cells, pos, nvec = _args(2, 4, 3)
    big = nvec.copy()
    big[2, 1] = -256
    singular = cells.copy()
    singular[1, 3:6] = singular[1, 0:3]
    nan_cell = cells.copy()
    nan_cell[0, 4] = np.nan
    cases = [
        (dict(nboxes=0), "nboxes"), (dict(nwater=0), "nwater"), (dict(nwater=(1 << 22) + 1), "nwater"),
        (dict(M=0), r"\bM\b"), (dict(M=(1 << 20) + 1), r"\bM\b"),
        (dict(cells=None), "cells"), (dict(pos=None), "pos"), (dict(nvec=None), "nvec"),
        (dict(nvec=big), r"nvec.*vector 2\b.*255"), (dict(cells=singular), r"cells.*box 1\b"), (dict(cells=nan_cell), r"cells.*box 0\b"),
    ]
    for change, pattern in cases:
        kw = dict(nboxes=2, nwater=4, cells=cells, pos=pos, M=3, nvec=nvec)
        kw.update(change)
        calls, outs = _entries(L, kw["nboxes"], kw["nwater"], kw["cells"], kw["pos"], kw["M"], kw["nvec"])
        for name, call in calls.items():
            assert call() != 0, (name, change)
            msg = L.mw_sk_last_error().decode()
            assert re.search(pattern, msg) and name in msg and "not initialised" not in msg, (name, change, msg)
        assert all(np.all(o == -7.0) for o in outs), change
    calls, outs = _entries(L, 3, 4, *_args(3, 4, 3)[:2], 3, nvec, ngroups=2)
    assert calls["mw_sk_mean"]() != 0 and "ngroups" in L.mw_sk_last_error().decode()
    calls, outs = _entries(L, 2, 4, cells, pos, 3, nvec, ngroups=0)
    assert calls["mw_sk_mean"]() != 0 and "ngroups" in L.mw_sk_last_error().decode()
    assert L.mw_sk_mean(2, 4, cells.ctypes.data_as(_dp), pos.ctypes.data_as(_dp), 3, nvec.ctypes.data_as(_ip), 1, None) != 0
    assert "S_mean" in L.mw_sk_last_error().decode()
    # the device-pointer entry checks what it can see from the host before anything else
    assert L.mw_sk_compute_device(0, 4, None, None, 3, None, None, None) != 0 and "nboxes" in L.mw_sk_last_error().decode()
    assert L.mw_sk_compute_device(1, 4, None, None, 3, None, None, None) != 0 and "cells" in L.mw_sk_last_error().decode()


def test_init_without_a_device_fails_with_its_message():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device behaviour is checked on the CPU box")
    L = _lib()
    assert L.mw_sk_init(0) != 0
    msg = L.mw_sk_last_error().decode()
    assert "no HIP device" in msg and "mw_sk_init" in msg
    assert not L.mw_sk_is_initialised()
    from mc_water_ls_mw_amd import structure
    z = np.eye(3) * 10.0
    with pytest.raises(structure.MwError, match="no HIP device"):
        structure.structure_factor(z, np.zeros((4, 3)), np.array([[1, 0, 0]]))


def test_plan_reports_the_launch_rules():
    _lib()
    from mc_water_ls_mw_amd.structure import MwError, PLAN_FIELDS, load_sk_library, sk_plan
    if load_sk_library().mw_sk_is_initialised():
        pytest.skip("the library is live in this process: its budget may not be the default one")
    budget = 256 << 20
    # everything fits: one chunk
    p = sk_plan(4096, (24, 24, 24), 10000, 8)
    assert set(p) == set(PLAN_FIELDS)
    per_box = 4096 * 75 * 16 + p["segments"] * 10000 * 16
    assert 8 * per_box <= budget and p["boxes_per_chunk"] == 8 and p["chunks"] == 1
    assert p["segments"] == -(-4096 // p["segment_length"]) and not p["small"]
    assert p["kvec_per_workgroup"] == 256 * p["kvec_per_lane"]
    assert p["lds_bytes"] == 75 * (p["tile"] + 1) * 16 <= 64 * 1024
    # it does not: ceil(nboxes / boxes_per_chunk) chunks of as many boxes as fit
    p = sk_plan(4096, (24, 24, 24), 10000, 512)
    assert p["boxes_per_chunk"] == budget // per_box and 1 < p["boxes_per_chunk"] < 512
    assert p["chunks"] == -(-512 // p["boxes_per_chunk"])
    # one box that does not fit is an error that says so
    with pytest.raises(MwError, match="one box.*does not fit"):
        sk_plan(1 << 22, (255, 255, 255), 1000, 1)
    # the small-box geometry: tables in the sum kernel's LDS, one segment, no table scratch
    for n, small in ((1, True), (48, True), (63, True), (64, True), (65, False), (1536, False)):
        p = sk_plan(n, (14, 7, 14), 3000, 4)
        assert p["small"] == small and p["chunks"] == 1, (n, p)
        if small:
            assert p["segments"] == 1 and p["tile"] == n and p["lds_bytes"] == 38 * (n | 1) * 16
    # ... only while those tables fit a workgroup's LDS: the bits do not depend on the choice (tests/test_gpu_sk.py)
    assert not sk_plan(64, (255, 0, 0), 100, 1)["small"] and sk_plan(64, (59, 0, 0), 100, 1)["small"]
    # the molecule tile shrinks as the tables get taller; the segments never move with anything but nwater
    tiles = [sk_plan(5000, (m, m, m), 100, 1) for m in (10, 40, 100, 255)]
    assert [t["tile"] for t in tiles] == [32, 32, 8, 4] and {t["segments"] for t in tiles} == {5}
    assert all(t["lds_bytes"] <= 64 * 1024 for t in tiles)
    for bad, pattern in (((0, (1, 1, 1), 1, 1), "nwater"), ((8, (1, 256, 1), 1, 1), "nmax"), ((8, (1, -1, 1), 1, 1), "nmax"),
                         ((8, (1, 1, 1), 0, 1), r"\bM\b"), ((8, (1, 1, 1), 1, 0), "nboxes")):
        with pytest.raises(MwError, match=pattern):
            sk_plan(*bad)


def test_structure_does_not_import_the_oracle():
    src = open(os.path.join(ROOT, "mc_water_ls_mw_amd", "structure.py")).read()
    assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M) and "oracle" not in src
    out = subprocess.run([sys.executable, "-c",
                          "import sys; import mc_water_ls_mw_amd.structure; print(int(any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules)))"],
                         capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "0", out.stderr
