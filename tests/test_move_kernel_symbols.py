"""CPU: counting on demand adds run-time mode bits, not kernels.  The set of kernel symbols of the move
family is the one tests/test_code_object.py pins (its lists of wanted names live inside its tests, which the suite runs): every
kernel its module-level table of LDS-staged builds names is found exactly once, with no further k_move_* symbol besides the build
that gathers through L2 and the fallback.  Names only."""
import os
import re
import subprocess

import pytest

import test_code_object as pinned

pytestmark = pytest.mark.skipif(not os.path.exists(pinned.READELF), reason="llvm-readelf not in this image")


def _kernel_names(tmp_path):
    from mc_water_ls_mw_amd import build as mwbuild
    mwbuild.build()
    notes = subprocess.run([pinned.READELF, "--notes", pinned._gfx950_code_object(tmp_path)], capture_output=True, text=True, check=True).stdout
    return [re.search(r"\.name:\s+(\S+)", blk).group(1) for blk in notes.split("- .agpr_count")[1:]]


def test_no_kernel_was_added_to_the_move_family(tmp_path):
    names = _kernel_names(tmp_path)
    for prefix in pinned._LDS_KERNELS:
        assert sum(n.startswith(prefix) for n in names) == 1, prefix
    move = [n for n in names if re.match(r"_ZN2mw\d+k_move", n)]
    lds_builds = [p for p in pinned._LDS_KERNELS if "k_move_energy" in p]
    # the three LDS-staged builds of the table, the build that gathers through L2, and the fallback
    assert len(move) == len(lds_builds) + 2 and sum(n.startswith("_ZN2mw15k_move_fallback") for n in move) == 1, move
    assert len(names) == len(set(names))
