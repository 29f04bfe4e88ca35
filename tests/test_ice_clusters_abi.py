"""CPU: the ice-cluster entries of the C ABI are exported, listed in ABI_SYMBOLS, and fail with a message before mw_init;
mw_ice_clusters_plan is host arithmetic; the Fortran module's compute_ice_clusters compiles and binds mw_ice_clusters where
the reference's host modules are built."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NAMES = ("mw_ice_clusters", "mw_ice_clusters_batch", "mw_ice_clusters_launch", "mw_ice_clusters_plan", "mw_ice_clusters_last")


def _lib():
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.energy import load_library
    build.build()
    return load_library()


def test_cluster_entries_are_exported_and_listed():
    L = _lib()
    from mc_water_ls_mw_amd.energy import ABI_SYMBOLS
    header = open(os.path.join(ROOT, "include", "mw_energy.h")).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in ABI_SYMBOLS, name
        assert f"int {name}(" in header, name


def test_cluster_entries_fail_with_a_message_before_init():
    L = _lib()
    if L.mw_is_initialised():
        pytest.skip("engine is live in this process")
    label, summary = np.full(48, -7, dtype=np.int32), np.full(4, -7, dtype=np.int32)
    lp = label.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    sp = summary.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    rc = ctypes.c_double(6.614)
    calls = [lambda: L.mw_ice_clusters(1, rc, 0b1110, lp, sp),
             lambda: L.mw_ice_clusters_batch(1, 1, rc, 0b1110, lp, sp),
             lambda: L.mw_ice_clusters_launch(1, 1, rc, 0b1110, -1),
             lambda: L.mw_ice_clusters_last(sp)]
    for call in calls:
        assert call() != 0
        assert b"not initialised" in L.mw_last_error()
    assert np.all(label == -7) and np.all(summary == -7)


def test_python_methods_raise_before_init():
    from mc_water_ls_mw_amd.energy import (ICE_CLASS_NAMES, ICE_CLUSTER_DEFAULT, EnergyModule, MwError, cluster_sizes,
                                           ice_cluster_mask)
    assert ICE_CLUSTER_DEFAULT == ("cubic", "hexagonal", "interfacial ice")
    assert ice_cluster_mask() == 0b1110 and ice_cluster_mask(ICE_CLUSTER_DEFAULT) == 0b1110
    assert ice_cluster_mask(ICE_CLASS_NAMES[1:]) == 0b111110 and ice_cluster_mask("hexagonal ice") == 0b100
    assert ice_cluster_mask(("clathrate", "interfacial clathrate")) == 0b110000 and ice_cluster_mask(0b110) == 0b110
    with pytest.raises(MwError, match="ice class"):
        ice_cluster_mask(("cubic", "amorphous"))
    assert list(cluster_sizes([0, 1, 1, 4, 0, 4, 4, 8])) == [3, 2, 1] and len(cluster_sizes(np.zeros(5, dtype=np.int32))) == 0
    em = EnergyModule(48, 2)
    if em.L.mw_is_initialised():
        pytest.skip("engine is live in this process")
    with pytest.raises(MwError, match="not initialised"):
        em.ice_clusters_batch()
    with pytest.raises(MwError, match="not initialised"):
        em.ice_clusters_launch(1, 2)
    with pytest.raises(MwError, match="not initialised"):
        em.ice_clusters_last()
    with pytest.raises(MwError, match="outside"):
        em.ice_clusters_batch(2, 2)
    with pytest.raises(MwError, match="outside"):
        em.ice_clusters(3)


def test_the_plan_is_host_arithmetic_and_monotone():
    L = _lib()
    from mc_water_ls_mw_amd.energy import MwError, ice_clusters_plan
    out = (ctypes.c_int * 4)()
    assert L.mw_ice_clusters_plan(0, out) != 0 and b"nwater" in L.mw_last_error()
    with pytest.raises(MwError, match="nwater"):
        ice_clusters_plan(-3)
    limit = ice_clusters_plan(48)["lds_max_nwater"]
    # 8 B per molecule in 160 KiB less the kernel's static LDS (at most 2 KiB, as the rest of the engine reserves)
    assert (160 * 1024 - 2048) // 8 <= limit <= 160 * 1024 // 8
    prev = None
    for n in (1, 32, 48, 63, 64, 65, 160, 512, 1000, 1024, 1025, 4096, limit - 1, limit, limit + 1, 32768, 1 << 20):
        p = ice_clusters_plan(n)
        assert p["lds_max_nwater"] == limit
        assert p["lds"] == (n <= limit)
        assert p["threads"] % 64 == 0 and 64 <= p["threads"] <= 1024 and (p["threads"] >= n or p["threads"] == 1024)
        assert p["lds_bytes"] == ((8 * n + 15) // 16 * 16 if p["lds"] else 0) and p["lds_bytes"] <= 160 * 1024
        if prev is not None:
            assert p["lds"] <= prev["lds"] and p["threads"] >= prev["threads"]          # never re-admitted, never fewer threads
            assert not p["lds"] or p["lds_bytes"] >= prev["lds_bytes"]
        prev = p


REF = os.path.join(ROOT, "oracle", "_ref")
SRC = os.path.join(ROOT, "mc_water_ls_mw_amd", "fortran", "energy_hip.F90")
FC = shutil.which("amdflang") or "/opt/rocm/llvm/bin/amdflang"
NM = shutil.which("nm") or shutil.which("llvm-nm")


@pytest.mark.skipif(not all(os.path.exists(os.path.join(REF, m + ".mod")) for m in ("constants", "userparams", "util", "model")),
                    reason="the reference's host modules are not built here (oracle/_ref/)")
@pytest.mark.skipif(not os.path.exists(FC) or NM is None, reason="no Fortran compiler / nm in this image")
def test_compute_ice_clusters_compiles_and_binds_the_c_entry(tmp_path):
    obj = tmp_path / "energy_hip.o"
    subprocess.run([FC, "-O2", "-fPIC", "-I", REF, "-module-dir", str(tmp_path), "-c", SRC, "-o", str(obj)],
                   check=True, capture_output=True, text=True)
    syms = subprocess.run([NM, str(obj)], check=True, capture_output=True, text=True).stdout
    assert "compute_ice_clusters" in syms.lower()
    assert any(line.split()[-1] == "mw_ice_clusters" and line.split()[-2] == "U" for line in syms.splitlines() if line.split())
