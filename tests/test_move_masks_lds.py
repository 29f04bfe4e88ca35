"""CPU: the row-slot masks of the move kernel's moment path (mw_move_energy.hip.h, mode bit 6) take no LDS of their own.  The table
of kMoveChunk words lies behind the sixteen wavefronts' queues inside the sixteen scratch blocks the launch has always asked for --
the dynamic request, move_lds_bytes, is pinned by test_code_object.py -- so what is left to hold is the kernel's STATIC LDS: no
larger than the 816 bytes it had before the masks (llvm-readelf --notes, .group_segment_fixed_size of the built code object)."""
import os
import re
import subprocess

import pytest

import test_code_object as pinned

pytestmark = pytest.mark.skipif(not os.path.exists(pinned.READELF), reason="llvm-readelf not in this image")

MOMENT_BUILD = "_ZN2mw13k_move_energyILb1ELi2ELb0ELb1EE"      # k_move_energy<true, kLayoutSoA, false, true>
STATIC_LDS_BEFORE = 816


def test_the_moment_build_has_no_more_static_lds_than_before_the_masks(tmp_path):
    from mc_water_ls_mw_amd import build as mwbuild
    mwbuild.build()
    notes = subprocess.run([pinned.READELF, "--notes", pinned._gfx950_code_object(tmp_path)], capture_output=True, text=True, check=True).stdout
    found = [blk for blk in notes.split("- .agpr_count")[1:] if re.search(r"\.name:\s+" + MOMENT_BUILD, blk)]
    assert len(found) == 1
    lds = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", found[0]).group(1))
    print("static LDS of the moment build", lds)
    assert lds <= STATIC_LDS_BEFORE
