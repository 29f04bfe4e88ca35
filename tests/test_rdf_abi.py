"""CPU: the pair-distance histogram entries of the C ABI are exported, listed in ABI_SYMBOLS, and fail with a message before
mw_init; the dispatch family is where the header says; the Fortran module's compute_rdf compiles and binds mw_rdf where the
reference's host modules are built."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NAMES = ("mw_rdf", "mw_rdf_batch", "mw_rdf_launch")


def _lib():
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.energy import load_library
    build.build()
    return load_library()


def test_rdf_entries_are_exported_and_listed():
    L = _lib()
    from mc_water_ls_mw_amd.energy import ABI_SYMBOLS
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in ABI_SYMBOLS, name


def test_rdf_entries_fail_with_a_message_before_init():
    L = _lib()
    if L.mw_is_initialised():
        pytest.skip("engine is live in this process")
    hist = np.zeros(200, dtype=np.int64)
    hp = hist.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong))
    r = ctypes.c_double(18.9)
    calls = [lambda: L.mw_rdf(1, r, 200, hp),
             lambda: L.mw_rdf_batch(1, 1, r, 200, hp),
             lambda: L.mw_rdf_launch(1, 1, r, 200, -1)]
    for call in calls:
        assert call() != 0
        assert b"not initialised" in L.mw_last_error()
    assert not hist.any()


def test_python_methods_raise_before_init():
    from mc_water_ls_mw_amd.energy import EnergyModule, MwError
    em = EnergyModule(48, 2)
    if em.L.mw_is_initialised():
        pytest.skip("engine is live in this process")
    with pytest.raises(MwError, match="not initialised"):
        em.rdf_counts(1, 10.0, 200)
    with pytest.raises(MwError, match="not initialised"):
        em.rdf_counts_batch(r_max_ang=10.0, nbins=200)
    with pytest.raises(MwError, match="not initialised"):
        em.rdf_launch(1, 2, 10.0, 200)
    with pytest.raises(MwError, match="not initialised"):
        em.rdf(1)
    with pytest.raises(MwError, match="outside"):
        em.rdf_counts_batch(2, 2, 10.0, 200)
    with pytest.raises(MwError, match="outside"):
        em.rdf_counts(3, 10.0, 200)


def test_the_dispatch_family_is_where_the_header_says():
    L = _lib()
    from mc_water_ls_mw_amd.energy import DISPATCH_FIELDS
    text = open(os.path.join(ROOT, "include", "mw_energy.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+MW_DISPATCH_(\w+)\s+(\d+)", text)}
    assert defs["RDF"] == 5 and defs["FAMILIES"] == 6
    assert list(DISPATCH_FIELDS).index("rdf") == defs["RDF"] and len(DISPATCH_FIELDS) == defs["FAMILIES"]
    assert DISPATCH_FIELDS["rdf"][:3] == ("ivcap", "boxes", "small") and DISPATCH_FIELDS["rdf"][-1] == "images"
    assert len(DISPATCH_FIELDS["rdf"]) <= defs["FIELDS"]
    for fam in ("build", "energy", "moves", "forces", "ice"):
        assert list(DISPATCH_FIELDS).index(fam) == defs[fam.upper()]
    out = (ctypes.c_int * 6)()
    assert L.mw_last_dispatch(defs["FAMILIES"], out, 6) != 0                 # one past the last family


REF = os.path.join(ROOT, "oracle", "_ref")
SRC = os.path.join(ROOT, "mc_water_ls_mw_amd", "fortran", "energy_hip.F90")
FC = shutil.which("amdflang") or "/opt/rocm/llvm/bin/amdflang"
NM = shutil.which("nm") or shutil.which("llvm-nm")


@pytest.mark.skipif(not all(os.path.exists(os.path.join(REF, m + ".mod")) for m in ("constants", "userparams", "util", "model")),
                    reason="the reference's host modules are not built here (oracle/_ref/)")
@pytest.mark.skipif(not os.path.exists(FC) or NM is None, reason="no Fortran compiler / nm in this image")
def test_compute_rdf_compiles_and_binds_the_c_entry(tmp_path):
    obj = tmp_path / "energy_hip.o"
    subprocess.run([FC, "-O2", "-fPIC", "-I", REF, "-module-dir", str(tmp_path), "-c", SRC, "-o", str(obj)],
                   check=True, capture_output=True, text=True)
    syms = subprocess.run([NM, str(obj)], check=True, capture_output=True, text=True).stdout
    assert "compute_rdf" in syms.lower()
    assert any(line.split()[-1] == "mw_rdf" and line.split()[-2] == "U" for line in syms.splitlines() if line.split())
