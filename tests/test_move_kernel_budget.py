"""CPU: what the compiler made of k_move_energy, from the metadata of the built code object.  Every instantiation runs four
wavefronts per SIMD beside 155 KiB of LDS -- at most 128 vector registers -- and none may touch scratch memory; the static LDS of
each is what it was before the request loop was rearranged (the moment path's pair table and count sums: 816 bytes; the others 16)."""
import os
import re
import subprocess

import pytest

import test_code_object as pinned

pytestmark = pytest.mark.skipif(not os.path.exists(pinned.READELF), reason="llvm-readelf not in this image")

#: template arguments <LDSPOS, LAYOUT, SELFIMG, MOMPATH, ...> as mangled -> static LDS in bytes
STATIC_LDS = {"Lb1ELi2ELb1ELb0E": 16, "Lb1ELi2ELb0ELb0E": 16, "Lb1ELi2ELb0ELb1E": 816, "Lb0ELi2ELb1ELb0E": 16}


def test_move_energy_kernels_keep_registers_scratch_and_static_lds(tmp_path):
    from mc_water_ls_mw_amd import build as mwbuild
    mwbuild.build()
    notes = subprocess.run([pinned.READELF, "--notes", pinned._gfx950_code_object(tmp_path)], capture_output=True, text=True, check=True).stdout
    seen = set()
    for blk in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.match(r"_ZN2mw13k_move_energyI((?:L[bi]\d+E){4})", name)
        if not m:
            continue
        get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))     # noqa: E731
        print(name[:48], "vgpr", get("vgpr_count"), "scratch", get("private_segment_fixed_size"), "lds", get("group_segment_fixed_size"))
        assert get("private_segment_fixed_size") == 0 and get("vgpr_spill_count") == 0, name
        assert get("vgpr_count") <= 128, (name, get("vgpr_count"))
        assert get("group_segment_fixed_size") == STATIC_LDS[m.group(1)], (name, get("group_segment_fixed_size"))
        seen.add(m.group(1))
    assert seen == set(STATIC_LDS)
