"""CPU: the set of mw_* symbols libmw_hip.so defines is the recorded one (tests/golden/exported_symbols.txt).  test_abi.py holds
the library to what include/mw_energy.h declares; this holds it to what it exported before its host code was split over the
mw_host_*.hip.h headers -- an entry point that loses its extern "C", or a helper that gains one, shows up here."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not in this image")
def test_defined_dynamic_symbols_are_the_recorded_ones():
    from mc_water_ls_mw_amd import build as mwbuild
    mwbuild.build()
    lib = os.path.join(ROOT, "mc_water_ls_mw_amd", "libmw_hip.so")
    out = subprocess.run([READELF, "--dyn-syms", "-W", lib], capture_output=True, text=True, check=True).stdout
    have = set()
    for line in out.splitlines():
        f = line.split()          # Num: Value Size Type Bind Vis Ndx Name
        if len(f) == 8 and f[0].endswith(":") and f[6] != "UND" and f[7].startswith("mw_"):
            have.add(f[7].split("@")[0])
    want = set(open(os.path.join(GOLDEN, "exported_symbols.txt")).read().split())
    assert len(want) >= 80
    assert have == want, (sorted(have - want), sorted(want - have))
