"""CPU: libmw_tcf.so builds for gfx950, loads without a GPU, exports what include/mw_tcf.h declares (and nothing of it leaks into
the other libraries, nor theirs into it), keeps its kernels free of scratch memory and within the LDS its plan reports, rejects
bad arguments and uninitialised calls with messages that name the entry and the argument and leaves the outputs alone, and
reports its launch rules through mw_tcf_plan."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
KERNELS = (b"k_tcf_check", b"k_tcf_com", b"k_tcf_corr", b"k_tcf_reduce", b"k_tcf_hist")


def _lib():
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.timecorr import load_tcf_library
    build.build_tcf()
    return load_tcf_library()


def _header():
    return open(os.path.join(ROOT, "include", "mw_tcf.h")).read()


def _declared():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return sorted(set(re.findall(r"\b(mw_tcf_\w+)\s*\(", text)))


def _define(name):
    return int(re.search(r"#define\s+" + name + r"\s+(\d+)", _header()).group(1))


def test_build_tcf_compiles_for_gfx950():
    from mc_water_ls_mw_amd import build
    lib = build.build_tcf(force=True)
    assert lib == build.TCF_LIB and os.path.exists(lib)
    data = open(lib, "rb").read()
    assert b"__CLANG_OFFLOAD_BUNDLE__" in data and b"gfx950" in data
    for kernel in KERNELS:
        assert kernel in data, kernel
    header = os.path.join(ROOT, "include", "mw_tcf.h")
    assert sorted(build.TCF_DEPS) == sorted([build.TCF_SRC, header, build.LIB_HOST]) and all(os.path.exists(p) for p in build.TCF_DEPS)
    for deps in (build.DEPS, build.SK_DEPS, build.BOO_DEPS, build.TET_DEPS, build.ADF_DEPS, build.RINGS_DEPS, build.QUENCH_BUILD_DEPS, build.MD_DEPS,
                 build.NPT_DEPS, build.COMMS_DEPS):
        assert not any(p in deps for p in (build.TCF_SRC, header))          # no other library moves with it
    assert os.path.basename(build.TCF_SRC) == "mw_tcf.hip" and build.LIB_CELLS not in build.TCF_DEPS
    text = open(build.TCF_SRC).read()
    assert "mw_lib_cells.h" not in text and '#include "mw_lib_host.h"' in text and "#pragma clang fp contract(off)" in text
    assert not re.search(r"atomicAdd\s*\(\s*\(?\s*(double|float)", text) and "unsafeAtomicAdd" not in text


def test_build_entry_builds_the_library():
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "mwbuild.build_tcf(" in text
    text = open(os.path.join(ROOT, "mc_water_ls_mw_amd", "build.py")).read()
    assert re.search(r"for builder in \(.*build_tcf\b", text)


def test_every_declared_name_is_exported_and_listed():
    L = _lib()
    from mc_water_ls_mw_amd import timecorr
    names = _declared()
    assert len(names) == 9 and sorted(timecorr.TCF_ABI_SYMBOLS) == names
    for name in names:
        assert hasattr(L, name), name
    assert _define("MW_TCF_PLAN_FIELDS") == len(timecorr.PLAN_FIELDS) == 10
    assert (_define("MW_TCF_MAX_Q"), _define("MW_TCF_MAX_EDGES"), _define("MW_TCF_MAX_HIST_LAGS")) == (timecorr.MAX_Q, timecorr.MAX_EDGES,
                                                                                                      timecorr.MAX_HIST_LAGS) == (16, 1025, 64)
    assert re.search(r"#define\s+MW_TCF_REMOVE_COM\s+1u", _header()) and timecorr.REMOVE_COM == 1


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not in this image")
def test_the_libraries_keep_their_prefixes_apart():
    from mc_water_ls_mw_amd import build
    others = [build.build(), build.build_sk(), build.build_boo(), build.build_tet(), build.build_adf(), build.build_rings(), build.build_quench(),
              build.build_md(), build.build_npt()]
    build.build_tcf()

    def defined(lib):
        out = subprocess.run([READELF, "--dyn-syms", "-W", lib], capture_output=True, text=True, check=True).stdout
        rows = [ln.split() for ln in out.splitlines()]
        return {f[7].split("@")[0] for f in rows if len(f) == 8 and f[0].endswith(":") and f[6] != "UND" and f[7].startswith("mw_")}

    assert defined(build.TCF_LIB) == set(_declared())
    for lib in others:
        assert not any(s.startswith("mw_tcf") for s in defined(lib))
        data = open(lib, "rb").read()
        assert b"mw_tcf" not in data and b"k_tcf_" not in data, lib
    data = open(build.TCF_LIB, "rb").read() + open(build.TCF_SRC, "rb").read()
    for word in (b"k_boo_", b"mw_boo", b"mw_sk_", b"k_sk_", b"k_tet_", b"mw_tet", b"k_adf_", b"mw_adf", b"k_rings_", b"mw_rings", b"k_model_", b"mw_model_",
                 b"k_quench_", b"mw_quench", b"k_md_", b"mw_md", b"k_npt_", b"mw_npt", b"k_cells_"):
        assert word not in data, word
    for name in os.listdir(build.CSRC):
        if name != "mw_tcf.hip":
            text = open(os.path.join(build.CSRC, name), "rb").read()
            assert b"mw_tcf" not in text and b"k_tcf_" not in text, name


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
            p = tmp_path / "tcf.co"
            p.write_bytes(data[i + o:i + o + s])
            return str(p)
    raise AssertionError("no gfx950 code object")


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not in this image")
def test_no_kernel_uses_a_private_segment_or_spills_vector_registers(tmp_path):
    """The sums of a lag live in registers: no kernel has a private segment or spills a vector register; the correlation kernel's
    LDS is what the plan reports, at least two of its workgroups fit the 160 KiB of a CU, and it stays at or below 128 VGPRs."""
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.timecorr import tcf_plan
    build.build_tcf()
    plan = tcf_plan(64, 48, nq=4, nedges=1025)
    notes = subprocess.run([READELF, "--notes", _gfx950_code_object(build.TCF_LIB, tmp_path)], capture_output=True, text=True, check=True).stdout
    seen, instances = set(), 0
    for blk in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.match(r"_ZN5mwtcf\d+(k_tcf_[a-z]+)(E|ILi\d+EEE)", name)
        assert m, name                                                       # the library holds no other kernel
        get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))     # noqa: E731
        print(m.group(1), m.group(2), "vgprs", get("vgpr_count"), "sgprs", get("sgpr_count"), "sgpr spills", get("sgpr_spill_count"), "lds", get("group_segment_fixed_size"))
        assert get("private_segment_fixed_size") == 0 and get("vgpr_spill_count") == 0, name
        assert get("group_segment_fixed_size") <= plan["lds_bytes"], name
        if m.group(1) == "k_tcf_corr":
            instances += 1
            assert get("group_segment_fixed_size") == plan["lds_bytes"] and 2 * plan["lds_bytes"] <= 160 * 1024
            assert get("vgpr_count") <= 128, (name, get("vgpr_count"))
        seen.add(m.group(1).encode())
    assert seen == set(KERNELS) and instances == 3


def _call(L, entry="mw_tcf_compute", nframes=6, nboxes=2, nwater=4, pos=0, vel=0, nlags=4, every=1, q=(0.5, 1.5), edges2=(0.1, 0.4, 0.9), hist_lags=(0, 3),
          flags=0, outs="msd mqd vacf fs hist", nq=None, nedges=None, nh=None):
    """One compute entry with outputs prefilled so that a write would show.  pos / vel: 0 for a good array, None for NULL."""
    shape = (min(max(nframes, 1), 8), min(max(nboxes, 1), 8), min(max(nwater, 1), 8), 3)
    good = np.arange(np.prod(shape), dtype=np.float64).reshape(shape) * 0.1
    pos = good if isinstance(pos, int) else pos
    vel = good if isinstance(vel, int) else vel
    q, e2, hl = np.asarray(q, dtype=np.float64), np.asarray(edges2, dtype=np.float64), np.asarray(hist_lags, dtype=np.int32)
    bufs = {k: np.full(4096, -7.0) for k in ("msd", "mqd", "vacf", "fs")}
    bufs["hist"] = np.full(4096, -7, dtype=np.int64)
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data      # noqa: E731
    want = outs.split()
    rc_ = getattr(L, entry)(nframes, nboxes, nwater, ptr(pos), ptr(vel), nlags, every, len(q) if nq is None else nq, ptr(q),
                            len(e2) if nedges is None else nedges, ptr(e2), len(hl) if nh is None else nh, ptr(hl), flags,
                            *[bufs[k].ctypes.data if k in want else None for k in ("msd", "mqd", "vacf", "fs", "hist")])
    clean = all(bool(np.all(b == -7)) for b in bufs.values())
    return rc_, L.mw_tcf_last_error().decode(), clean


def test_calls_before_init_fail_with_not_initialised():
    L = _lib()
    if L.mw_tcf_is_initialised():
        pytest.skip("the library is live in this process")
    for entry in ("mw_tcf_compute", "mw_tcf_compute_device"):
        rc_, msg, clean = _call(L, entry)
        assert rc_ != 0 and "not initialised" in msg and entry in msg and clean, msg
    out = (ctypes.c_int * 10)()
    t = [ctypes.c_float(-1.0) for _ in range(3)]
    for name, call in (("mw_tcf_last", lambda: L.mw_tcf_last(out, 10)), ("mw_tcf_elapsed_ms", lambda: L.mw_tcf_elapsed_ms(*[ctypes.byref(v) for v in t]))):
        assert call() != 0, name
        msg = L.mw_tcf_last_error().decode()
        assert "not initialised" in msg and name in msg, msg
    assert not any(out) and all(v.value == -1.0 for v in t)
    assert L.mw_tcf_finalize() == 0                                 # nothing to undo is not an error
    from mc_water_ls_mw_amd import timecorr
    with pytest.raises(timecorr.MwError, match="not initialised"):
        timecorr.tcf_last()


def test_argument_validation_needs_no_device():
    L = _lib()
    nan, inf = float("nan"), float("inf")
    good = np.arange(6 * 2 * 4 * 3, dtype=np.float64).reshape(6, 2, 4, 3) * 0.1

    def spoiled(frame, box, value):
        b = good.copy()
        b[frame, box, 2, 1] = value
        return b

    cases = [
        (dict(nframes=0), "nframes"), (dict(nframes=(1 << 20) + 1), "nframes"), (dict(nboxes=0), "nboxes"), (dict(nboxes=(1 << 24) + 1), "nboxes"),
        (dict(nwater=0), "nwater"), (dict(nwater=(1 << 22) + 1), "nwater"), (dict(nlags=0), "nlags"), (dict(nlags=7), "nlags"),
        (dict(every=0), "origin_every"), (dict(every=-2), "origin_every"), (dict(nq=-1), r"\bnq\b"), (dict(nq=17), r"\bnq\b"),
        (dict(nedges=1), "nedges"), (dict(nedges=1026), "nedges"), (dict(nedges=-1), "nedges"), (dict(nh=-1), r"\bnh\b"), (dict(nh=65), r"\bnh\b"),
        (dict(flags=2), "flags"), (dict(flags=1 << 31), "flags"), (dict(pos=None), r"\bpos\b"), (dict(vel=None), r"vacf.*vel"),
        (dict(q=(0.5, 0.0)), r"q\[1\]"), (dict(q=(-1.0, 0.5)), r"q\[0\]"), (dict(q=(0.5, nan)), r"q\[1\]"), (dict(q=(inf, 1.0)), r"q\[0\]"),
        (dict(q=(), outs="msd fs"), r"\bfs\b.*nq"), (dict(q=(), nq=2), r"\bq\b is NULL"),
        (dict(edges2=(0.1, 0.1, 0.9)), r"edges2\[0\].*ascending"), (dict(edges2=(0.1, 0.9, 0.4)), r"edges2\[1\].*ascending"),
        (dict(edges2=(0.1, nan, 0.9)), r"edges2\[1\]"), (dict(edges2=(0.1, 0.4, inf)), r"edges2\[2\]"), (dict(edges2=()), r"hist.*nedges"),
        (dict(edges2=(), nedges=3), "edges2 is NULL"),
        (dict(hist_lags=(0, 4)), r"hist_lags\[1\]"), (dict(hist_lags=(-1, 2)), r"hist_lags\[0\]"), (dict(hist_lags=()), r"hist.*nh"),
        (dict(hist_lags=(), nh=2), "hist_lags is NULL"),
        (dict(pos=spoiled(3, 1, nan)), r"\bpos\b.*frame 3 of box 1\b"), (dict(pos=spoiled(0, 0, inf)), r"\bpos\b.*frame 0 of box 0\b"),
        (dict(vel=spoiled(5, 1, -inf)), r"\bvel\b.*frame 5 of box 1\b"), (dict(vel=spoiled(2, 0, nan)), r"\bvel\b.*frame 2 of box 0\b"),
    ]
    for change, pattern in cases:
        rc_, msg, clean = _call(L, **change)
        assert rc_ != 0 and re.search(pattern, msg) and "mw_tcf_compute" in msg and "not initialised" not in msg and clean, (change, msg)
    # with good arguments -- the bounds themselves included -- the next thing a call without a device meets is the state
    import torch
    if not torch.cuda.is_available() and not L.mw_tcf_is_initialised():
        for kw in (dict(), dict(nlags=6), dict(nlags=1, hist_lags=(0,)), dict(every=1 << 30), dict(q=(), outs="msd"), dict(edges2=(), hist_lags=(), outs="msd mqd vacf fs"),
                   dict(vel=None, outs="msd mqd fs hist"), dict(flags=1), dict(outs=""), dict(hist_lags=(), outs="msd")):
            rc_, msg, clean = _call(L, **kw)
            assert rc_ != 0 and "not initialised" in msg and clean, (kw, msg)
    # the device-pointer entry checks what it can see from the host before anything else
    for kw, pattern in ((dict(nframes=0), "nframes"), (dict(pos=None), r"\bpos\b"), (dict(nlags=9), "nlags"), (dict(q=(0.0,)), r"q\[0\]"),
                        (dict(edges2=(2.0, 1.0)), "ascending"), (dict(hist_lags=(9,)), "hist_lags"), (dict(vel=None), "vel"), (dict(flags=4), "flags")):
        rc_, msg, clean = _call(L, "mw_tcf_compute_device", **kw)
        assert rc_ != 0 and re.search(pattern, msg) and "mw_tcf_compute_device" in msg and clean, msg


def test_init_without_a_device_fails_with_its_message():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the no-device behaviour is checked on the CPU box")
    L = _lib()
    assert L.mw_tcf_init(0) != 0
    msg = L.mw_tcf_last_error().decode()
    assert "no HIP device" in msg and "mw_tcf_init" in msg
    assert not L.mw_tcf_is_initialised()
    from mc_water_ls_mw_amd import timecorr
    with pytest.raises(timecorr.MwError, match="no HIP device"):
        timecorr.time_correlations(np.zeros((3, 1, 4, 3)))


def test_plan_matches_the_python_arithmetic():
    _lib()
    from mc_water_ls_mw_amd.timecorr import MwError, PLAN_FIELDS, load_tcf_library, tcf_plan
    if load_tcf_library().mw_tcf_is_initialised():
        pytest.skip("the library is live in this process: its budget may not be the default one")
    budget = 256 << 20
    tile, lb, chunk = _define("MW_TCF_TILE"), _define("MW_TCF_LAG_BLOCK"), _define("MW_TCF_ORIGIN_CHUNK")
    a16 = lambda v: (v + 15) // 16 * 16                                      # noqa: E731
    for nframes, n, nlags, nq, nedges, com in ((256, 48, 128, 4, 0, False), (1024, 4096, 512, 4, 101, True), (16, 8, 16, 16, 1025, True), (1, 1, 1, 0, 0, False),
                                               (300, 200, 129, 0, 2, False)):
        tiles, blocks = -(-n // tile), -(-nlags // lb)
        per_box = a16(8 * tiles * (3 + nq) * nlags) + (2 * a16(24 * nframes) if com else 0)
        for nboxes in (1, 200, 3000000):
            p = tcf_plan(nframes, n, nlags, nq, nedges, com, nboxes)
            assert set(p) == set(PLAN_FIELDS)
            most = min(budget // per_box, 65535, nboxes)
            assert p["scratch_bytes_per_box"] == per_box and p["boxes_per_chunk"] == most and p["chunks"] == -(-nboxes // most), (n, nboxes, p)
            assert (p["tile"], p["lag_block"], p["origin_chunk"], p["frame_window"]) == (tile, lb, chunk, lb + chunk - 1)
            assert (p["tiles"], p["lag_blocks"]) == (tiles, blocks)
            # rows of (molecule, component) over the origin chunk and the target window, each padded to an odd length
            assert p["lds_bytes"] == 8 * 3 * tile * ((chunk + 1) + (lb + chunk - 1 + 2)) and 2 * p["lds_bytes"] <= 160 * 1024
            assert a16(8 * nedges) + 4 * (nedges + 1) <= p["lds_bytes"]
    with pytest.raises(MwError, match="one box.*does not fit"):
        tcf_plan(1 << 20, 1 << 21, 1 << 18, 16)
    for bad, pattern in (((0, 8), "nframes"), ((8, 0), "nwater"), ((8, 8, 9), "nlags"), ((8, 8, 8, 17), r"\bnq\b"), ((8, 8, 8, 0, 1), "nedges"),
                         ((8, 8, 8, 0, 0, False, 0), "nboxes")):
        with pytest.raises(MwError, match=pattern):
            tcf_plan(*bad)


def test_timecorr_does_not_import_the_oracle():
    src = open(os.path.join(ROOT, "mc_water_ls_mw_amd", "timecorr.py")).read()
    assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M) and "oracle" not in src
