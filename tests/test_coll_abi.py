"""CPU: libmw_coll.so builds for gfx950, loads without a GPU, exports what include/mw_coll.h declares (and nothing of it leaks
into the other libraries, nor theirs into it), keeps its kernels free of scratch memory and within the LDS its plan reports,
rejects bad arguments and uninitialised calls with messages that name the entry and the argument and leaves the outputs alone,
and reports its launch rules through mw_coll_plan."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
KERNELS = (b"k_coll_check", b"k_coll_phasors", b"k_coll_sum", b"k_coll_finish", b"k_coll_corr", b"k_coll_pairs", b"k_coll_pairs_small",
           b"k_coll_overlap", b"k_coll_overlap_sum")


def _lib():
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.collective import load_coll_library
    build.build_coll()
    return load_coll_library()


def _header():
    return open(os.path.join(ROOT, "include", "mw_coll.h")).read()


def _declared():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return sorted(set(re.findall(r"\b(mw_coll_\w+)\s*\(", text)))


def _define(name):
    return int(re.search(r"#define\s+" + name + r"\s+(\d+)", _header()).group(1))


def test_build_coll_compiles_for_gfx950():
    from mc_water_ls_mw_amd import build
    lib = build.build_coll(force=True)
    assert lib == build.COLL_LIB and os.path.exists(lib)
    data = open(lib, "rb").read()
    assert b"__CLANG_OFFLOAD_BUNDLE__" in data and b"gfx950" in data
    for kernel in KERNELS:
        assert kernel in data, kernel
    header = os.path.join(ROOT, "include", "mw_coll.h")
    assert sorted(build.COLL_DEPS) == sorted([build.COLL_SRC, header, build.LIB_HOST]) and all(os.path.exists(p) for p in build.COLL_DEPS)
    for deps in (build.DEPS, build.SK_DEPS, build.BOO_DEPS, build.TET_DEPS, build.ADF_DEPS, build.RINGS_DEPS, build.QUENCH_BUILD_DEPS, build.MD_DEPS,
                 build.NPT_DEPS, build.TCF_DEPS, build.HESS_DEPS, build.TI_DEPS, build.FLEX_DEPS, build.PIN_DEPS, build.NUC_DEPS, build.COMMS_DEPS):
        assert not any(p in deps for p in (build.COLL_SRC, header))        # no other library moves with it
    assert os.path.basename(build.COLL_SRC) == "mw_coll.hip" and build.LIB_CELLS not in build.COLL_DEPS
    text = open(build.COLL_SRC).read()
    assert "mw_lib_cells.h" not in text and '#include "mw_lib_host.h"' in text
    assert text.index("#pragma clang fp contract(off)") < text.index('#include "mw_lib_host.h"') < text.index("namespace mwcoll")
    assert not re.search(r"atomicAdd\s*\(\s*\(?\s*(double|float)", text) and "unsafeAtomicAdd" not in text


def test_build_entry_builds_the_library():
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "mwbuild.build_coll(" in text
    text = open(os.path.join(ROOT, "mc_water_ls_mw_amd", "build.py")).read()
    assert re.search(r"for builder in \(.*build_coll\b", text)


def test_every_declared_name_is_exported_and_listed():
    L = _lib()
    from mc_water_ls_mw_amd import collective
    names = _declared()
    assert len(names) == 9 and sorted(collective.COLL_ABI_SYMBOLS) == names
    for name in names:
        assert hasattr(L, name), name
    assert _define("MW_COLL_PLAN_FIELDS") == len(collective.PLAN_FIELDS) == 14
    assert (_define("MW_COLL_MAX_VECTORS"), _define("MW_COLL_MAX_COMPONENT"), _define("MW_COLL_MAX_BINS"), _define("MW_COLL_MAX_HIST_LAGS"),
            _define("MW_COLL_MAX_FRAMES")) == (collective.MAX_VECTORS, collective.MAX_COMPONENT, collective.MAX_BINS, collective.MAX_HIST_LAGS,
                                               collective.MAX_FRAMES) == (4096, 255, 4096, 64, 65536)
    # the flush rules the header states keep the 32-bit counters below 2^32
    assert _define("MW_COLL_FLUSH_TILES") * _define("MW_COLL_PAIR_TILE") ** 2 * 27 < 2 ** 32
    assert -(-_define("MW_COLL_MAX_FRAMES") // _define("MW_COLL_SLABS")) * 64 * 64 * 27 < 2 ** 32
    for word in ("Out of scope", "move during the trajectory", "centre of mass", "distinct part of the overlap", "ultiple-tau", "tress correlations",
                 "Fortran binding"):
        assert word in _header(), word
    assert "mw_coll.h" in open(os.path.join(ROOT, "include", "mw_tcf.h")).read()


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not in this image")
def test_the_libraries_keep_their_prefixes_apart():
    from mc_water_ls_mw_amd import build
    others = [build.build(), build.build_sk(), build.build_boo(), build.build_tet(), build.build_adf(), build.build_rings(), build.build_quench(),
              build.build_md(), build.build_npt(), build.build_tcf(), build.build_hess(), build.build_ti(), build.build_flex(), build.build_pin(),
              build.build_nuc()]
    build.build_coll()

    def defined(lib):
        out = subprocess.run([READELF, "--dyn-syms", "-W", lib], capture_output=True, text=True, check=True).stdout
        rows = [ln.split() for ln in out.splitlines()]
        return {f[7].split("@")[0] for f in rows if len(f) == 8 and f[0].endswith(":") and f[6] != "UND" and f[7].startswith("mw_")}

    assert defined(build.COLL_LIB) == set(_declared())
    for lib in others:
        assert not any(s.startswith("mw_coll") for s in defined(lib))
        data = open(lib, "rb").read()
        assert b"mw_coll" not in data and b"k_coll_" not in data, lib
    data = open(build.COLL_LIB, "rb").read()
    for word in (b"k_boo_", b"mw_boo", b"mw_sk_", b"k_sk_", b"k_tet_", b"mw_tet", b"k_adf_", b"mw_adf", b"k_rings_", b"mw_rings", b"k_model_", b"mw_model_",
                 b"k_quench_", b"mw_quench", b"k_md_", b"mw_md", b"k_npt_", b"mw_npt", b"k_cells_", b"k_rdf_", b"k_tcf_", b"mw_tcf", b"k_hess_", b"mw_hess"):
        assert word not in data, word
    for name in os.listdir(build.CSRC):
        if name != "mw_coll.hip":
            text = open(os.path.join(build.CSRC, name), "rb").read()
            assert b"mw_coll" not in text and b"k_coll_" not in text, name


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
            p = tmp_path / "coll.co"
            p.write_bytes(data[i + o:i + o + s])
            return str(p)
    raise AssertionError("no gfx950 code object")


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not in this image")
def test_no_kernel_uses_a_private_segment_or_spills_vector_registers(tmp_path):
    """No kernel has a private segment or spills a vector register; the static LDS of every kernel (the pair tile's staged
    positions) is within what the plan reports for a call that uses it, and the pair kernels stay at or below 128 VGPRs."""
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.collective import coll_plan
    build.build_coll()
    plan = coll_plan(64, 300, nbins=1, nh=1)
    assert plan["lds_bytes"] == 4 * 1 + 3 * 256 * 8
    notes = subprocess.run([READELF, "--notes", _gfx950_code_object(build.COLL_LIB, tmp_path)], capture_output=True, text=True, check=True).stdout
    seen, sums = set(), 0
    for blk in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.match(r"_ZN6mwcoll\d+(k_coll_[a-z_]+?)(E|ILb[01]EEE)", name)
        assert m, name                                                       # the library holds no other kernel
        get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))     # noqa: E731
        print(m.group(1), m.group(2), "vgprs", get("vgpr_count"), "sgprs", get("sgpr_count"), "sgpr spills", get("sgpr_spill_count"), "lds", get("group_segment_fixed_size"))
        assert get("private_segment_fixed_size") == 0 and get("vgpr_spill_count") == 0, name
        assert get("group_segment_fixed_size") <= plan["lds_bytes"], name
        if m.group(1) == "k_coll_pairs":
            assert get("group_segment_fixed_size") == 3 * 256 * 8
        if m.group(1).startswith("k_coll_pairs"):
            assert get("vgpr_count") <= 128, (name, get("vgpr_count"))
        sums += m.group(1) == "k_coll_sum"
        seen.add(m.group(1).encode())
    assert seen == set(KERNELS) and sums == 2


def _call(L, entry="mw_coll_compute", nframes=6, nboxes=2, nwater=4, cells=0, pos=0, nlags=4, every=1, nvec=((1, 0, 0), (0, -2, 1)), r_max=3.0, nbins=8,
          hist_lags=(0, 3), a=0.5, outs="rho fkt gd qsum q2sum", M=None, nh=None):
    """One compute entry with outputs prefilled so that a write would show.  cells / pos: 0 for a good array, None for NULL."""
    shape = (min(max(nframes, 1), 8), min(max(nboxes, 1), 8), min(max(nwater, 1), 8), 3)
    good = np.arange(np.prod(shape), dtype=np.float64).reshape(shape) * 0.1
    good_cells = np.ascontiguousarray(np.broadcast_to(np.diag([10.0, 11.0, 12.0]), (shape[1], 3, 3)))
    pos = good if isinstance(pos, int) else pos
    cells = good_cells if isinstance(cells, int) else cells
    nv, hl = np.asarray(nvec, dtype=np.int32).reshape(-1, 3), np.asarray(hist_lags, dtype=np.int32)
    bufs = {k: np.full(8192, -7.0) for k in ("rho", "fkt")}
    bufs.update({k: np.full(8192, -7, dtype=np.int64) for k in ("gd", "qsum", "q2sum")})
    ptr = lambda v: None if v is None or v.size == 0 else v.ctypes.data      # noqa: E731
    want = outs.split()
    rc_ = getattr(L, entry)(nframes, nboxes, nwater, ptr(cells), ptr(pos), nlags, every, len(nv) if M is None else M, ptr(nv), r_max, nbins,
                            len(hl) if nh is None else nh, ptr(hl), a, *[bufs[k].ctypes.data if k in want else None for k in ("rho", "fkt", "gd", "qsum", "q2sum")])
    clean = all(bool(np.all(b == -7)) for b in bufs.values())
    return rc_, L.mw_coll_last_error().decode(), clean


def test_calls_before_init_fail_with_not_initialised():
    L = _lib()
    if L.mw_coll_is_initialised():
        pytest.skip("the library is live in this process")
    for entry in ("mw_coll_compute", "mw_coll_compute_device"):
        rc_, msg, clean = _call(L, entry)
        assert rc_ != 0 and "not initialised" in msg and entry in msg and clean, msg
    out = (ctypes.c_int * 14)()
    t = [ctypes.c_float(-1.0) for _ in range(4)]
    for name, call in (("mw_coll_last", lambda: L.mw_coll_last(out, 14)), ("mw_coll_elapsed_ms", lambda: L.mw_coll_elapsed_ms(*[ctypes.byref(v) for v in t]))):
        assert call() != 0, name
        msg = L.mw_coll_last_error().decode()
        assert "not initialised" in msg and name in msg, msg
    assert not any(out) and all(v.value == -1.0 for v in t)
    assert L.mw_coll_finalize() == 0                                # nothing to undo is not an error
    from mc_water_ls_mw_amd import collective
    with pytest.raises(collective.MwError, match="not initialised"):
        collective.coll_last()


def test_argument_validation_needs_no_device():
    L = _lib()
    nan, inf = float("nan"), float("inf")
    good = np.arange(6 * 2 * 4 * 3, dtype=np.float64).reshape(6, 2, 4, 3) * 0.1
    cells = np.ascontiguousarray(np.broadcast_to(np.diag([10.0, 11.0, 12.0]), (2, 3, 3)))

    def spoiled(frame, box, value):
        b = good.copy()
        b[frame, box, 2, 1] = value
        return b

    def flat(box):
        c = cells.copy()
        c[box, 2] = c[box, 1]
        return c

    def narrow(box):
        c = cells.copy()
        c[box] = np.diag([10.0, 1.9, 12.0])
        return c

    cases = [
        (dict(nframes=0), "nframes"), (dict(nframes=65537), "nframes"), (dict(nboxes=0), "nboxes"), (dict(nboxes=(1 << 24) + 1), "nboxes"),
        (dict(nwater=0), "nwater"), (dict(nwater=(1 << 22) + 1), "nwater"), (dict(nlags=0), "nlags"), (dict(nlags=7), "nlags"),
        (dict(every=0), "origin_every"), (dict(every=-2), "origin_every"), (dict(M=-1), r"\bM\b"), (dict(M=4097), r"\bM\b"),
        (dict(nbins=-1), "nbins"), (dict(nbins=4097), "nbins"), (dict(nh=-1), r"\bnh\b"), (dict(nh=65), r"\bnh\b"),
        (dict(cells=None), r"\bcells\b"), (dict(pos=None), r"\bpos\b"), (dict(nvec=(), M=2), "nvec is NULL"),
        (dict(nvec=((1, 0, 0), (0, 256, 0))), r"nvec.*component 1 of vector 1\b"), (dict(nvec=((-256, 0, 0),)), r"nvec.*component 0 of vector 0\b"),
        (dict(nvec=(), outs="rho gd"), r"\brho\b.*M = 0"), (dict(nvec=(), outs="fkt"), r"\bfkt\b.*M = 0"),
        (dict(hist_lags=(0, 4)), r"hist_lags\[1\]"), (dict(hist_lags=(-1, 2)), r"hist_lags\[0\]"), (dict(hist_lags=()), r"\bgd\b.*nh"),
        (dict(hist_lags=(), nh=2), "hist_lags is NULL"), (dict(nbins=0), r"\bgd\b.*nbins"),
        (dict(r_max=0.0), "r_max"), (dict(r_max=-1.0), "r_max"), (dict(r_max=nan), "r_max"), (dict(r_max=inf), "r_max"),
        (dict(r_max=15.1), r"r_max.*box 0\b"), (dict(r_max=3.0, cells=narrow(1)), r"r_max.*box 1\b"),
        (dict(a=-0.5), "overlap_a"), (dict(a=nan), "overlap_a"), (dict(a=inf), "overlap_a"), (dict(a=0.0), r"qsum.*overlap_a"),
        (dict(a=0.0, outs="q2sum"), r"q2sum.*overlap_a"),
        (dict(cells=flat(0)), r"cells.*box 0\b"), (dict(cells=flat(1)), r"cells.*box 1\b"),
        (dict(pos=spoiled(3, 1, nan)), r"\bpos\b.*frame 3 of box 1\b"), (dict(pos=spoiled(0, 0, inf)), r"\bpos\b.*frame 0 of box 0\b"),
    ]
    for change, pattern in cases:
        rc_, msg, clean = _call(L, **change)
        assert rc_ != 0 and re.search(pattern, msg) and "mw_coll_compute" in msg and "not initialised" not in msg and clean, (change, msg)
    # a count that could pass 2^62: 65536 origins x (2^22)^2 pairs x 27 images (nothing is read before the counts are checked)
    big = np.ascontiguousarray(np.diag([10.0, 11.0, 12.0])[None])
    rc_ = L.mw_coll_compute(65536, 1, 1 << 22, big.ctypes.data, good.ctypes.data, 1, 1, 0, None, 14.0, 8, 1, np.zeros(1, dtype=np.int32).ctypes.data, 0.0, None, None,
                            np.zeros(8, dtype=np.int64).ctypes.data, None, None)
    assert rc_ != 0 and re.search(r"gd.*2\^62", L.mw_coll_last_error().decode()), L.mw_coll_last_error().decode()
    # with good arguments -- the bounds themselves included -- the next thing a call without a device meets is the state
    import torch
    if not torch.cuda.is_available() and not L.mw_coll_is_initialised():
        for kw in (dict(), dict(nlags=6), dict(nlags=1, hist_lags=(0,)), dict(every=1 << 30), dict(nvec=(), outs="gd qsum q2sum"), dict(r_max=14.9),
                   dict(nbins=0, hist_lags=(), outs="rho fkt qsum"), dict(a=0.0, outs="rho fkt gd"), dict(outs=""), dict(r_max=nan, outs="fkt"),
                   dict(nvec=((255, -255, 0),), nbins=4096)):
            rc_, msg, clean = _call(L, **kw)
            assert rc_ != 0 and "not initialised" in msg and clean, (kw, msg)
    # the device-pointer entry checks what it can see from the host before anything else
    for kw, pattern in ((dict(nframes=0), "nframes"), (dict(pos=None), r"\bpos\b"), (dict(nlags=9), "nlags"), (dict(nvec=((300, 0, 0),)), "nvec"),
                        (dict(r_max=99.0), "r_max"), (dict(hist_lags=(9,)), "hist_lags"), (dict(a=-1.0), "overlap_a"), (dict(cells=flat(1)), "box 1")):
        rc_, msg, clean = _call(L, "mw_coll_compute_device", **kw)
        assert rc_ != 0 and re.search(pattern, msg) and "mw_coll_compute_device" in msg and clean, msg


def test_init_without_a_device_fails_with_its_message():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device behaviour is checked on the CPU box")
    L = _lib()
    assert L.mw_coll_init(0) != 0
    msg = L.mw_coll_last_error().decode()
    assert "no HIP device" in msg and "mw_coll_init" in msg
    assert not L.mw_coll_is_initialised()
    from mc_water_ls_mw_amd import collective
    with pytest.raises(collective.MwError, match="no HIP device"):
        collective.collective_correlations(np.diag([9.0, 9.0, 9.0]), np.zeros((3, 1, 4, 3)), nvec=[(1, 0, 0)])


def test_plan_matches_the_python_arithmetic():
    _lib()
    from mc_water_ls_mw_amd.collective import MwError, PLAN_FIELDS, coll_plan, load_coll_library
    from mc_water_ls_mw_amd.structure import sk_plan
    if load_coll_library().mw_coll_is_initialised():
        pytest.skip("the library is live in this process: its budget may not be the default one")
    budget = 256 << 20
    a16 = lambda v: (v + 15) // 16 * 16                                      # noqa: E731
    for nframes, n, nlags, every, M, nmax, nbins, nh, overlap in ((256, 48, 128, 1, 500, (5, 5, 5), 512, 4, True), (128, 4096, 64, 1, 500, (6, 6, 6), 512, 4, True),
                                                                  (16, 8, 16, 3, 0, (0, 0, 0), 4096, 2, False), (1, 1, 1, 1, 1, (0, 0, 0), 0, 0, True),
                                                                  (300, 200, 129, 7, 33, (255, 3, 0), 1, 64, True), (2, 8193, 2, 1, 3, (1, 2, 3), 0, 0, False)):
        o0 = (nframes - 1) // min(every, nframes) + 1
        sk = sk_plan(n, nmax, max(M, 1))
        tables = 0 if (sk["small"] or M == 0) else n * (sum(nmax) + 3) * 16
        unit = (tables + sk["segments"] * M * 16) if M else 0
        per_box = (a16(16 * M * nframes) if M else 0) + (a16(4 * nlags * o0) if overlap else 0)
        for nboxes in (1, 200, 3000000):
            p = coll_plan(nframes, n, nlags, every, M, nmax, nbins, nh, overlap, nboxes)
            assert set(p) == set(PLAN_FIELDS)
            keep = min(max(budget // 4, unit), unit * 65535)                 # what the mode pass keeps before the boxes are counted
            if keep + per_box > budget:
                keep = unit
            most = min((budget - keep) // per_box if per_box else 65535, 65535, nboxes)
            assert p["scratch_bytes_per_box"] == per_box and p["boxes_per_chunk"] == most and p["chunks"] == -(-nboxes // most), (n, nboxes, p)
            units = min(most * nframes, 65535)
            if unit:
                units = min(units, (budget - per_box * most) // unit)
            assert p["mode_units"] == units >= 1
            if M:                                                            # the mode pass follows the structure-factor library's rules
                assert (p["segments"], p["segment_molecules"], p["small"]) == (sk["segments"], sk["segment_length"], int(sk["small"]))
            assert (p["lag_block"], p["pair_tile"]) == (64, 256) and p["pair_small"] == (n <= 64) and p["pair_tiles"] == (1 if n <= 64 else -(-n // 256))
            assert p["slabs"] == min(o0, 32) and p["origins_per_slab"] == -(-o0 // p["slabs"]) and p["origins_per_slab"] <= 2048
            waves = 4 if 4 * (1536 + 4 * nbins) <= 65536 else 1
            pair = 0 if nbins == 0 else waves * (1536 + 4 * nbins) if n <= 64 else 4 * nbins + 6144
            assert p["lds_bytes"] == max(sk["lds_bytes"] if M else 0, pair) and p["lds_bytes"] <= 160 * 1024
    with pytest.raises(MwError, match="one box.*does not fit"):
        coll_plan(65536, 64, 65536, 1, 4096, (9, 9, 9), 0, 0, True)
    with pytest.raises(MwError, match="workgroups"):
        coll_plan(65536, 1 << 22, 1, 1, 0, (0, 0, 0), 0, 0, True)
    for bad, pattern in (((0, 8), "nframes"), ((8, 0), "nwater"), ((8, 8, 9), "nlags"), ((8, 8, 8, 0), "origin_every"), ((8, 8, 8, 1, 4097), r"\bM\b"),
                         ((8, 8, 8, 1, 1, (256, 0, 0)), "nmax"), ((8, 8, 8, 1, 0, (0, 0, 0), 4097), "nbins"), ((8, 8, 8, 1, 0, (0, 0, 0), 8, 65), r"\bnh\b"),
                         ((8, 8, 8, 1, 0, (0, 0, 0), 8, 1, False, 0), "nboxes")):
        with pytest.raises(MwError, match=pattern):
            coll_plan(*bad)


def test_a_chosen_output_must_be_possible_and_the_default_sets_take_what_the_lists_allow():
    from mc_water_ls_mw_amd import collective
    every = collective._wanted(collective.OUTPUTS, 0, 8, 2, 0.0)
    assert every == dict(rho=False, fkt=False, gd=True, qsum=False, q2sum=False)
    assert collective._wanted(("fkt", "gd", "qsum", "q2sum"), 3, 0, 2, 0.5) == dict(rho=False, fkt=True, gd=False, qsum=True, q2sum=True)
    assert collective._wanted(("gd",), 0, 8, 2, 0.0)["gd"] and not collective._wanted((), 3, 8, 2, 0.5)["fkt"]
    for outputs, args, word in ((("gd",), (3, 0, 2, 0.5), "nbins"), (("gd", "fkt"), (3, 8, 0, 0.5), "hist_lags"), (("rho",), (0, 8, 2, 0.5), "nvec"),
                                (("fkt", "qsum"), (3, 8, 2, 0.0), "overlap_a"), (("q2sum",), (3, 8, 2, 0.0), "overlap_a")):
        with pytest.raises(collective.MwError, match=word):
            collective._wanted(outputs, *args)
    with pytest.raises(collective.MwError, match="expected names"):
        collective._wanted(("rho", "S"), 3, 8, 2, 0.5)


def test_collective_does_not_import_the_oracle():
    src = open(os.path.join(ROOT, "mc_water_ls_mw_amd", "collective.py")).read()
    assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M) and "oracle" not in src
