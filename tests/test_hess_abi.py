"""CPU: libmw_hess.so builds for gfx950, loads without a GPU, exports what include/mw_hess.h declares (and nothing of it leaks
into the other libraries, nor theirs into it), keeps its kernels free of scratch memory and within the LDS its plan reports,
rejects bad arguments and uninitialised calls with messages that name the entry and the argument and leaves the outputs alone,
and reports its launch rules through mw_hess_plan."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
KERNELS = (b"k_hess_moments", b"k_hess_forces", b"k_hess_ef", b"k_hess_gather", b"k_hess_dmoments", b"k_hess_apply", b"k_hess_jsum", b"k_hess_clear", b"k_hess_rows")
RC = 1.8 * 2.3925 / 0.5291772108                                     # a sigma, bohr
ENTRIES = ("mw_hess_matvec", "mw_hess_matvec_device", "mw_hess_dense", "mw_hess_dense_device")


def _lib():
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.phonons import load_hess_library
    build.build_hess()
    return load_hess_library()


def _header():
    return open(os.path.join(ROOT, "include", "mw_hess.h")).read()


def _declared():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return sorted(set(re.findall(r"\b(mw_hess_\w+)\s*\(", text)))


def _define(name):
    return int(re.search(r"#define\s+" + name + r"\s+(\d+)", _header()).group(1))


def test_build_hess_compiles_for_gfx950():
    from mc_water_ls_mw_amd import build
    lib = build.build_hess(force=True)
    assert lib == build.HESS_LIB and os.path.exists(lib)
    data = open(lib, "rb").read()
    assert b"__CLANG_OFFLOAD_BUNDLE__" in data and b"gfx950" in data
    for kernel in KERNELS:
        assert kernel in data, kernel
    header = os.path.join(ROOT, "include", "mw_hess.h")
    common = os.path.join(build.CSRC, "mw_common.hip.h")
    assert sorted(build.HESS_DEPS) == sorted([build.HESS_SRC, header, build.LIB_HOST, build.LIB_CELLS, build.LIB_FORCES, common])
    assert all(os.path.exists(p) for p in build.HESS_DEPS)
    for deps in (build.DEPS, build.SK_DEPS, build.BOO_DEPS, build.TET_DEPS, build.ADF_DEPS, build.RINGS_DEPS, build.QUENCH_BUILD_DEPS, build.MD_DEPS,
                 build.NPT_DEPS, build.TCF_DEPS, build.COMMS_DEPS):
        assert not any(p in deps for p in (build.HESS_SRC, header))          # no other library moves with it
    assert os.path.basename(build.HESS_SRC) == "mw_hess.hip" and not any("hess" in f for f in os.listdir(build.CSRC) if f.endswith(".hip.h"))
    text = open(build.HESS_SRC).read()
    for inc in ('#include "mw_lib_host.h"', '#include "mw_lib_cells.h"', '#include "mw_lib_forces.h"', '#include "mw_common.hip.h"'):
        assert inc in text, inc
    assert "#pragma clang fp contract(off)" in text and text.index("#pragma clang fp contract(off)") < text.index('#include "mw_lib_host.h"')
    assert not re.search(r"atomic(Add|Max|Min|Exch|CAS)\s*\(", text) and "unsafeAtomicAdd" not in text       # none at all of its own
    assert "namespace mwhess" in text


def test_build_entry_builds_the_library():
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "mwbuild.build_hess(" in text
    text = open(os.path.join(ROOT, "mc_water_ls_mw_amd", "build.py")).read()
    assert re.search(r"for builder in \(.*build_hess\b", text)


def test_every_declared_name_is_exported_and_listed():
    L = _lib()
    from mc_water_ls_mw_amd import phonons
    names = _declared()
    assert len(names) == 11 and sorted(phonons.HESS_ABI_SYMBOLS) == names
    for name in names:
        assert hasattr(L, name), name
    assert _define("MW_HESS_PLAN_FIELDS") == len(phonons.PLAN_FIELDS) == 8
    assert (_define("MW_HESS_MAX_VEC"), _define("MW_HESS_VEC_GROUP"), _define("MW_HESS_MAX_DENSE_WATER")) == \
        (phonons.MAX_VEC, phonons.VEC_GROUP, phonons.MAX_DENSE_WATER) == (1024, 32, 8192)


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not in this image")
def test_the_libraries_keep_their_prefixes_apart():
    from mc_water_ls_mw_amd import build
    others = [build.build(), build.build_sk(), build.build_boo(), build.build_tet(), build.build_adf(), build.build_rings(), build.build_quench(),
              build.build_md(), build.build_npt(), build.build_tcf()]
    build.build_hess()

    def defined(lib):
        out = subprocess.run([READELF, "--dyn-syms", "-W", lib], capture_output=True, text=True, check=True).stdout
        rows = [ln.split() for ln in out.splitlines()]
        return {f[7].split("@")[0] for f in rows if len(f) == 8 and f[0].endswith(":") and f[6] != "UND" and f[7].startswith("mw_")}

    assert defined(build.HESS_LIB) == set(_declared())
    for lib in others:
        assert not any(s.startswith("mw_hess") for s in defined(lib))
        data = open(lib, "rb").read()
        assert b"mw_hess" not in data and b"k_hess_" not in data and b"mwhess" not in data, lib
    data = open(build.HESS_LIB, "rb").read() + open(build.HESS_SRC, "rb").read()
    for word in (b"k_boo_", b"mw_boo", b"mw_sk_", b"k_sk_", b"k_tet_", b"mw_tet", b"k_adf_", b"mw_adf", b"k_rings_", b"mw_rings", b"k_model_", b"mw_model_",
                 b"k_quench_", b"mw_quench", b"k_md_", b"mw_md", b"k_npt_", b"mw_npt", b"k_tcf_", b"mw_tcf"):
        assert word not in data, word
    for name in os.listdir(build.CSRC):
        if name != "mw_hess.hip":
            text = open(os.path.join(build.CSRC, name), "rb").read()
            assert b"mw_hess" not in text and b"k_hess_" not in text, name


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
            p = tmp_path / "hess.co"
            p.write_bytes(data[i + o:i + o + s])
            return str(p)
    raise AssertionError("no gfx950 code object")


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not in this image")
def test_no_kernel_uses_a_private_segment_or_spills_vector_registers(tmp_path):
    """Every sum of a molecule lives in registers: no kernel (the shared counting sort's included) has a private segment or spills
    a vector register, and the LDS of each is within what the plan reports."""
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.phonons import hess_plan
    build.build_hess()
    plan = hess_plan(96, np.eye(3) * 30.0, nvec=3)
    notes = subprocess.run([READELF, "--notes", _gfx950_code_object(build.HESS_LIB, tmp_path)], capture_output=True, text=True, check=True).stdout
    seen, most = set(), 0
    for blk in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.match(r"_ZN6mwhess\d+(k_hess_[a-z]+)E", name) or re.match(r"_ZN7mwcells\d+(k_cells_[a-z]+)E", name)
        assert m, name                                                       # the library holds no other kernel
        get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))     # noqa: E731
        print(m.group(1), "vgprs", get("vgpr_count"), "agprs", int(re.match(r":\s+(\d+)", blk).group(1)), "sgprs", get("sgpr_count"), "sgpr spills",
              get("sgpr_spill_count"), "lds", get("group_segment_fixed_size"))
        assert get("private_segment_fixed_size") == 0 and get("vgpr_spill_count") == 0, name
        assert get("group_segment_fixed_size") <= plan["lds_bytes"], name
        most = max(most, get("group_segment_fixed_size"))
        seen.add(m.group(1).encode())
    assert set(KERNELS) <= seen and most == plan["lds_bytes"]


def _call(L, entry="mw_hess_matvec", nboxes=2, nwater=4, cells=0, pos=0, nvec=3, vecs=0, out=0, ef=0):
    """One compute entry with outputs prefilled so that a write would show.  0 for a good array, None for NULL."""
    nb, n, nv = min(max(nboxes, 1), 4), min(max(nwater, 1), 8), min(max(nvec, 1), 4)
    good_cells = np.tile(np.eye(3) * 20.0, (nb, 1, 1))
    good_pos = np.arange(nb * n * 3, dtype=np.float64).reshape(nb, n, 3) * 0.7
    good_vecs = np.ones((nb, nv, n, 3))
    cells = good_cells if isinstance(cells, int) else cells
    pos = good_pos if isinstance(pos, int) else pos
    vecs = good_vecs if isinstance(vecs, int) else vecs
    out_buf, ef_buf = np.full(4096, -7.0), np.full(64, -7.0)
    ptr = lambda a: None if a is None else a.ctypes.data                     # noqa: E731
    p_out = None if out is None else out_buf.ctypes.data
    p_ef = None if ef is None else ef_buf.ctypes.data
    f = getattr(L, entry)
    if "matvec" in entry:
        rc_ = f(nboxes, nwater, ptr(cells), ptr(pos), nvec, ptr(vecs), p_out, p_ef)
    else:
        rc_ = f(nboxes, nwater, ptr(cells), ptr(pos), p_out, p_ef)
    clean = bool(np.all(out_buf == -7.0) and np.all(ef_buf == -7.0))
    return rc_, L.mw_hess_last_error().decode(), clean


def test_calls_before_init_fail_with_not_initialised():
    L = _lib()
    if L.mw_hess_is_initialised():
        pytest.skip("the library is live in this process")
    for entry in ENTRIES:
        rc_, msg, clean = _call(L, entry)
        assert rc_ != 0 and "not initialised" in msg and entry in msg and clean, msg
    out = (ctypes.c_int * 8)()
    t = [ctypes.c_float(-1.0) for _ in range(4)]
    for name, call in (("mw_hess_last", lambda: L.mw_hess_last(out, 8)), ("mw_hess_elapsed_ms", lambda: L.mw_hess_elapsed_ms(*[ctypes.byref(v) for v in t]))):
        assert call() != 0, name
        msg = L.mw_hess_last_error().decode()
        assert "not initialised" in msg and name in msg, msg
    assert not any(out) and all(v.value == -1.0 for v in t)
    assert L.mw_hess_finalize() == 0                                # nothing to undo is not an error
    from mc_water_ls_mw_amd import phonons
    with pytest.raises(phonons.MwError, match="not initialised"):
        phonons.hess_last()


def test_argument_validation_needs_no_device():
    L = _lib()
    good = np.tile(np.eye(3) * 20.0, (2, 1, 1))

    def cell(box, k, value):
        c = good.copy()
        c[box].flat[k] = value
        return c

    narrow = good.copy()
    narrow[1] = np.diag([20.0, RC * (1.0 + 0.5e-9), 20.0])
    singular = good.copy()
    singular[1, 2] = singular[1, 0]
    cases = [
        (dict(nboxes=0), "nboxes"), (dict(nboxes=(1 << 24) + 1), "nboxes"), (dict(nwater=0), "nwater"), (dict(nwater=(1 << 22) + 1), "nwater"),
        (dict(cells=None), r"\bcells\b"), (dict(pos=None), r"\bpos\b"), (dict(out=None), r"\b(out|hess)\b"),
        (dict(cells=cell(0, 4, float("nan"))), r"cells.*box 0\b"), (dict(cells=cell(1, 0, float("inf"))), r"cells.*box 1\b"),
        (dict(cells=singular), r"cells.*box 1\b"), (dict(cells=narrow), r"a_sigma.*box 1\b"),
    ]
    for entry in ("mw_hess_matvec", "mw_hess_dense"):
        for change, pattern in cases:
            rc_, msg, clean = _call(L, entry, **change)
            assert rc_ != 0 and re.search(pattern, msg) and entry in msg and "not initialised" not in msg and clean, (entry, change, msg)
    bad_pos = np.arange(2 * 4 * 3, dtype=np.float64).reshape(2, 4, 3) * 0.7
    bad_pos[1, 2, 1] = float("nan")
    bad_vecs = np.ones((2, 3, 4, 3))
    bad_vecs[0, 2, 3, 0] = float("inf")
    for entry in ("mw_hess_matvec", "mw_hess_dense"):
        rc_, msg, clean = _call(L, entry, pos=bad_pos)
        assert rc_ != 0 and re.search(r"\bpos\b.*box 1\b", msg) and entry in msg and "not initialised" not in msg and clean, msg
    rc_, msg, clean = _call(L, "mw_hess_matvec", vecs=bad_vecs)
    assert rc_ != 0 and re.search(r"\bvecs\b.*box 0\b", msg) and "not initialised" not in msg and clean, msg
    for change, pattern in ((dict(nvec=0), "nvec"), (dict(nvec=1025), "nvec"), (dict(vecs=None), r"\bvecs\b")):
        rc_, msg, clean = _call(L, "mw_hess_matvec", **change)
        assert rc_ != 0 and re.search(pattern, msg) and "mw_hess_matvec" in msg and "not initialised" not in msg and clean, (change, msg)
    # the dense matrix: at most 8192 molecules, and through host pointers it has to fit the scratch budget (256 MiB: 1928 molecules do, 1929 do not)
    rc_, msg, clean = _call(L, "mw_hess_dense", nwater=8193)
    assert rc_ != 0 and re.search(r"nwater = 8193 outside 1\.\.8192", msg) and clean, msg
    if not L.mw_hess_is_initialised():
        rc_, msg, clean = _call(L, "mw_hess_dense", nboxes=1, nwater=4096, pos=np.zeros((1, 4096, 3)), cells=np.eye(3)[None] * 100.0)
        assert rc_ != 0 and re.search(r"mw_hess_dense: one box needs \d+ bytes.*matrix.*does not fit the budget.*MW_HESS_SCRATCH_MB", msg) and clean, msg
    # with good arguments -- the bounds themselves included -- the next thing a call without a device meets is the state
    import torch
    if not torch.cuda.is_available() and not L.mw_hess_is_initialised():
        for entry, kw in (("mw_hess_matvec", dict()), ("mw_hess_matvec", dict(nvec=1)), ("mw_hess_matvec", dict(ef=None)), ("mw_hess_dense", dict()),
                          ("mw_hess_dense", dict(ef=None)), ("mw_hess_dense", dict(nwater=1)),
                          ("mw_hess_matvec", dict(cells=np.tile(np.eye(3) * RC * (1.0 + 2e-9), (2, 1, 1))))):
            rc_, msg, clean = _call(L, entry, **kw)
            assert rc_ != 0 and "not initialised" in msg and clean, (kw, msg)
    # the device-pointer entries check what they can see from the host before anything else
    for entry in ("mw_hess_matvec_device", "mw_hess_dense_device"):
        for kw, pattern in ((dict(nboxes=0), "nboxes"), (dict(nwater=0), "nwater"), (dict(cells=None), "cells"), (dict(pos=None), r"\bpos\b"),
                            (dict(out=None), r"\b(out|hess)\b")):
            rc_, msg, clean = _call(L, entry, **kw)
            assert rc_ != 0 and re.search(pattern, msg) and entry in msg and clean, msg
    rc_, msg, clean = _call(L, "mw_hess_matvec_device", nvec=-1)
    assert rc_ != 0 and "nvec" in msg and clean, msg


def test_init_without_a_device_fails_with_its_message():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device behaviour is checked on the CPU box")
    L = _lib()
    assert L.mw_hess_init(0) != 0
    msg = L.mw_hess_last_error().decode()
    assert "no HIP device" in msg and "mw_hess_init" in msg
    assert not L.mw_hess_is_initialised()
    from mc_water_ls_mw_amd import phonons
    with pytest.raises(phonons.MwError, match="no HIP device"):
        phonons.hessian(np.eye(3) * 20.0, np.zeros((4, 3)))


def test_plan_matches_the_python_arithmetic():
    _lib()
    from mc_water_ls_mw_amd.phonons import MwError, PLAN_FIELDS, VEC_GROUP, hess_plan, load_hess_library
    if load_hess_library().mw_hess_is_initialised():
        pytest.skip("the library is live in this process: its budget may not be the default one")
    budget = 256 << 20
    a16 = lambda v: (v + 15) // 16 * 16                                      # noqa: E731

    def base(n):
        cap = max(2 * n, 64)
        tab = a16(4 * (cap + 1))
        sort = a16(24 * n) + a16(4 * n) + a16(4 * n) + 2 * tab + a16(4 * n) + a16(24 * n)
        return sort + a16(80 * n) + a16(8 * n) + a16(16 * -(-n // 256))

    for n, side in ((1, 20.0), (48, 25.0), (65, 9.0), (1536, 75.0), (4096, 100.0)):
        g = max(1, min(int(side // (RC * (1 + 1e-9))), 1024))
        while g ** 3 > max(2 * n, 64):
            g -= 1
        for nboxes in (1, 200, 100000):
            for nvec in (1, 3, 64, 1024):
                p = hess_plan(n, np.eye(3) * side, nboxes, nvec)
                assert set(p) == set(PLAN_FIELDS)
                per_vec = a16(24 * n) + a16(80 * n)
                group = min(nvec, VEC_GROUP, (budget - base(n)) // per_vec)
                per_box = base(n) + group * per_vec
                most = min(budget // per_box, 65535, nboxes)
                assert (p["vectors_per_group"], p["scratch_bytes_per_box"], p["boxes_per_chunk"], p["chunks"]) == (group, per_box, most, -(-nboxes // most)), (n, nboxes, nvec, p)
                assert (p["g1"], p["g2"], p["g3"]) == (g, g, g) and p["lds_bytes"] == 64 * (4 + 72)
            if n <= 1536:
                p = hess_plan(n, np.eye(3) * side, nboxes, dense=True)
                per_box = base(n) + a16(240 * n) + 72 * n * n
                most = min(budget // per_box, 65535, nboxes)
                assert (p["vectors_per_group"], p["scratch_bytes_per_box"], p["boxes_per_chunk"], p["chunks"]) == (0, per_box, most, -(-nboxes // most)), (n, nboxes, p)
    with pytest.raises(MwError, match="one box.*does not fit"):
        hess_plan(4096, np.eye(3) * 100.0, dense=True)
    assert hess_plan(1928, np.eye(3) * 100.0, dense=True)["boxes_per_chunk"] == 1       # the largest box whose matrix the default budget stages
    with pytest.raises(MwError, match="one box.*does not fit"):
        hess_plan(1929, np.eye(3) * 100.0, dense=True)
    with pytest.raises(MwError, match="one box.*does not fit"):
        hess_plan(1 << 22, np.eye(3) * 2000.0, nvec=4)
    for bad, pattern in (((0, np.eye(3) * 20.0), "nwater"), ((8, np.eye(3) * 20.0, 0), "nboxes"), ((8, np.eye(3) * 20.0, 1, 0), "nvec"),
                         ((8, np.eye(3) * 20.0, 1, 1025), "nvec"), ((8193, np.eye(3) * 200.0, 1, 1, True), "nwater"), ((8, np.eye(3) * 8.0), "a_sigma")):
        with pytest.raises(MwError, match=pattern):
            hess_plan(*bad)


def test_phonons_does_not_import_the_oracle():
    src = open(os.path.join(ROOT, "mc_water_ls_mw_amd", "phonons.py")).read()
    assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M) and "oracle" not in src
