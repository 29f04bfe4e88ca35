"""CPU: the Fortran module's force routine (fortran/energy_hip.F90, compute_model_forces) compiles against the host
modules it uses and binds mw_model_forces.  Those modules (constants, userparams, util, model) are the reference's own,
built by oracle/Makefile into oracle/_ref/ where the reference's sources are at hand; elsewhere this skips."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

REF = os.path.join(ROOT, "oracle", "_ref")
SRC = os.path.join(ROOT, "mc_water_ls_mw_amd", "fortran", "energy_hip.F90")
FC = shutil.which("amdflang") or "/opt/rocm/llvm/bin/amdflang"
NM = shutil.which("nm") or shutil.which("llvm-nm")


@pytest.mark.skipif(not all(os.path.exists(os.path.join(REF, m + ".mod")) for m in ("constants", "userparams", "util", "model")),
                    reason="the reference's host modules are not built here (oracle/_ref/)")
@pytest.mark.skipif(not os.path.exists(FC) or NM is None, reason="no Fortran compiler / nm in this image")
def test_compute_model_forces_compiles_and_binds_the_c_entry(tmp_path):
    obj = tmp_path / "energy_hip.o"
    subprocess.run([FC, "-O2", "-fPIC", "-I", REF, "-module-dir", str(tmp_path), "-c", SRC, "-o", str(obj)],
                   check=True, capture_output=True, text=True)
    syms = subprocess.run([NM, str(obj)], check=True, capture_output=True, text=True).stdout
    assert "compute_model_forces" in syms.lower()
    assert any(line.split()[-1] == "mw_model_forces" and line.split()[-2] == "U" for line in syms.splitlines() if line.split())
