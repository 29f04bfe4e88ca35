"""CPU: libmw_nuc.so builds for gfx950, loads without a GPU, exports what include/mw_nuc.h declares and nothing else, keeps its
kernels free of private segments and vector-register spills, shares the harmonics with libmw_boo.so through one header, rejects
bad arguments and uninitialised calls with messages that name the entry, the argument and the first offending box and leaves
the outputs alone, and reports its launch rules through mw_nuc_plan without a device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from test_flex_abi import A_SIGMA, MASS, READELF, _gfx950_code_object

KERNELS = ("k_cells_bin", "k_cells_scan", "k_cells_place", "k_cells_rank", "k_nuc_check", "k_nuc_begin", "k_nuc_finish", "k_nuc_drift1", "k_nuc_drift2",
           "k_nuc_moments", "k_nuc_forces", "k_nuc_row", "k_nuc_baro", "k_nuc_scale", "k_nuc_q6", "k_nuc_conn", "k_nuc_clusters", "k_nuc_kick1", "k_nuc_latch")
N = 65


def _lib():
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.nucleation import load_nuc_library
    build.build_nuc()
    return load_nuc_library()


def _declared():
    text = open(os.path.join(ROOT, "include", "mw_nuc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mw_nuc_\w+)\s*\(", text)))


def test_build_nuc_compiles_for_gfx950_and_moves_with_no_other_library():
    from mc_water_ls_mw_amd import build
    lib = build.build_nuc(force=True)
    assert lib == build.NUC_LIB and os.path.exists(lib)
    data = open(lib, "rb").read()
    assert b"__CLANG_OFFLOAD_BUNDLE__" in data and b"gfx950" in data
    for kernel in KERNELS:
        assert kernel.encode() in data, kernel
    header = os.path.join(ROOT, "include", "mw_nuc.h")
    shared = [os.path.join(build.CSRC, f) for f in ("mw_lib_host.h", "mw_lib_cells.h", "mw_lib_forces.h", "mw_lib_harmonics.h", "mw_common.hip.h")]
    flex_h = os.path.join(ROOT, "include", "mw_flex.h")                        # its constants alone
    assert sorted(build.NUC_DEPS) == sorted([build.NUC_SRC, header, flex_h, *shared]) and all(os.path.exists(p) for p in build.NUC_DEPS)
    for deps in (build.DEPS, build.SK_DEPS, build.BOO_DEPS, build.TET_DEPS, build.ADF_DEPS, build.RINGS_DEPS, build.QUENCH_BUILD_DEPS, build.MD_DEPS,
                 build.NPT_DEPS, build.TCF_DEPS, build.HESS_DEPS, build.TI_DEPS, build.FLEX_DEPS, build.PIN_DEPS, build.COMMS_DEPS):
        assert not any(p in deps for p in (build.NUC_SRC, header))
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "mwbuild.build_nuc(" in text
    assert re.search(r"for builder in \(.*build_nuc\b", open(os.path.join(ROOT, "mc_water_ls_mw_amd", "build.py")).read())
    src = open(build.NUC_SRC).read()
    assert src.index("#pragma clang fp contract(off)") < src.index('#include "mw_lib_host.h"') < src.index('#include "mw_lib_harmonics.h"')
    assert "atomicAdd" not in src.split("namespace mwnuc")[1]                  # (the counting sort's integer atomicAdd lives in mw_lib_cells.h)


def test_the_harmonics_exist_once():
    """The l = 6 harmonics live in mw_lib_harmonics.h alone; both translation units include it and neither restates them."""
    from mc_water_ls_mw_amd import build
    shared = open(build.LIB_HARMONICS).read()
    assert "void harmonics(" in shared and "void unit_harmonics(" in shared and "k66 = 6.461695905544936e-05" in shared
    assert build.LIB_HARMONICS in build.BOO_DEPS and build.LIB_HARMONICS in build.NUC_DEPS
    for src in (build.BOO_SRC, build.NUC_SRC):
        text = open(src).read()
        assert '#include "mw_lib_harmonics.h"' in text and "void harmonics(" not in text and "k66" not in text and "10395.0" not in text, src


def test_every_declared_name_is_exported_and_listed():
    L = _lib()
    from mc_water_ls_mw_amd import flexcell, nucleation
    names = _declared()
    assert len(names) == 9 and sorted(nucleation.NUC_ABI_SYMBOLS) == names
    for name in names:
        assert hasattr(L, name), name
    text = open(os.path.join(ROOT, "include", "mw_nuc.h")).read()
    for word, value in (("PLAN_FIELDS", 12), ("TRACE_FIELDS", 18), ("MAX_STEPS", 100000000), ("MIN_WATER", 65), ("MAX_CONN", 64), ("REACHED_HI", 3),
                        ("REACHED_LO", 4)):
        assert re.search(r"#define\s+MW_NUC_%s\s+%d\b" % (word, value), text), word
    assert len(nucleation.TRACE_FIELDS) == 18 and nucleation.TRACE_FIELDS[:15] == flexcell.TRACE_FIELDS and len(nucleation.NUC_PLAN_FIELDS) == 12
    assert (nucleation.REACHED_HI, nucleation.REACHED_LO, nucleation.MIN_WATER, nucleation.MAX_CONN) == (3, 4, 65, 64)
    import nuc_ref
    assert nuc_ref.TRACE_FIELDS == 18 and (nuc_ref.REACHED_HI, nuc_ref.REACHED_LO) == (3, 4)


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not in this image")
def test_the_library_exports_its_own_names_alone_and_no_kernel_has_a_private_segment(tmp_path):
    """The counts are printed.  The force pass and the moment pass stay within the registers of libmw_flex.so's."""
    from mc_water_ls_mw_amd import build
    build.build_nuc()
    out = subprocess.run([READELF, "--dyn-syms", "-W", build.NUC_LIB], capture_output=True, text=True, check=True).stdout
    rows = [ln.split() for ln in out.splitlines()]
    defined = {f[7].split("@")[0] for f in rows if len(f) == 8 and f[0].endswith(":") and f[6] != "UND" and f[7].startswith("mw_")}
    assert defined == set(_declared())
    data = open(build.NUC_LIB, "rb").read()
    for word in (b"mw_flex", b"k_flex_", b"mwflex", b"k_boo_", b"mw_boo_", b"k_pin_", b"k_md_", b"k_npt_", b"mw_sk_"):
        assert word not in data, word
    notes = subprocess.run([READELF, "--notes", _gfx950_code_object(build.NUC_LIB, tmp_path)], capture_output=True, text=True, check=True).stdout
    seen = set()
    for blk in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.match(r"_ZN5mwnuc\d+(k_nuc_[a-z0-9]+)(E|ILb[01]EEE)", name) or re.match(r"_ZN7mwcells\d+(k_cells_[a-z]+)(E)", name)
        assert m, name
        get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))     # noqa: E731
        print(m.group(1), m.group(2), "vgprs", get("vgpr_count"), "sgprs", get("sgpr_count"), "sgpr spills", get("sgpr_spill_count"), "lds", get("group_segment_fixed_size"))
        assert get("private_segment_fixed_size") == 0 and get("vgpr_spill_count") == 0, name
        if m.group(1) != "k_nuc_clusters":                                       # (its two dozen arguments park scalar registers in vector lanes)
            assert get("sgpr_spill_count") == 0, name
        if m.group(1) == "k_nuc_moments":
            assert get("vgpr_count") <= 128
        if m.group(1) == "k_nuc_forces":
            assert get("vgpr_count") <= 168 and get("group_segment_fixed_size") == 4 * 17 * 8
        if m.group(1) == "k_nuc_clusters":
            assert get("group_segment_fixed_size") <= 512                        # kClusterStaticLds: what the LDS rule of the labels leaves room for
        seen.add(m.group(1))
    assert seen == set(KERNELS)


def _args(nboxes=2, nwater=N):
    cells = np.tile(np.eye(3).ravel() * 30.0, (nboxes, 1))
    pos = np.arange(nboxes * nwater * 3, dtype=np.float64).reshape(nboxes, nwater, 3) * 0.07
    return cells, pos


LO = np.array([-1, 3], dtype=np.int32)
HI = np.array([N + 1, 40], dtype=np.int32)
_DEFAULT = object()


def _run(L, nboxes=2, nwater=N, cells=None, pos=None, vel=None, pos_ref=None, lo=_DEFAULT, hi=_DEFAULT, nsteps=10, sample_every=1, dt=100.0, mass=MASS, kT=1e-3,
         gamma=1e-3, pressure=1e-8, tau_p=4e4, beta_T=1e4, baro_every=2, coupling=3, axis=2, rc=6.6, threshold=0.5, min_conn=3, check_every=5,
         entry="mw_nuc_run"):
    """One run entry with outputs prefilled so that a write would show."""
    lo = LO if lo is _DEFAULT else lo
    hi = HI if hi is _DEFAULT else hi
    outs = [np.full(3 * 2 * N, -7.0), np.full(3 * 2 * N, -7.0), np.full(3 * 2 * N, -7.0), np.full(9 * 2, -7.0), np.full(3 * 2 * N, -7.0), np.full(18 * 200 * 2, -7.0),
            np.full(2 * 2, -7, dtype=np.int32), np.full(2 * 2 * N, -7, dtype=np.int32), np.full(2 * N, -7, dtype=np.int32), np.full(4 * 2, -7, dtype=np.int32)]
    ptr = lambda a: None if a is None else a.ctypes.data                   # noqa: E731
    rc_ = getattr(L, entry)(nboxes, nwater, ptr(cells), ptr(pos), ptr(vel), ptr(pos_ref), None, 1, 0, nsteps, sample_every, dt, mass, kT, gamma, pressure, tau_p,
                            beta_T, baro_every, coupling, axis, rc, threshold, min_conn, check_every, ptr(lo), ptr(hi), *[o.ctypes.data for o in outs])
    return rc_, L.mw_nuc_last_error().decode(), all(bool(np.all(o == -7)) for o in outs)


def test_calls_before_init_fail_with_not_initialised():
    L = _lib()
    assert not L.mw_nuc_is_initialised()                                     # (the CPU tests never initialise it)
    cells, pos = _args()
    rc_, msg, clean = _run(L, cells=cells, pos=pos)
    assert rc_ != 0 and "not initialised" in msg and "mw_nuc_run" in msg and clean, msg
    rc_, msg, clean = _run(L, cells=cells, pos=pos, entry="mw_nuc_run_device")
    assert rc_ != 0 and "not initialised" in msg and "mw_nuc_run_device" in msg and clean, msg
    out = (ctypes.c_int * 12)()
    t = [ctypes.c_float(-1.0) for _ in range(7)]
    for name, call in (("mw_nuc_last", lambda: L.mw_nuc_last(out, 12)), ("mw_nuc_elapsed_ms", lambda: L.mw_nuc_elapsed_ms(*[ctypes.byref(v) for v in t]))):
        assert call() != 0, name
        msg = L.mw_nuc_last_error().decode()
        assert "not initialised" in msg and name in msg, msg
    assert not any(out) and all(v.value == -1.0 for v in t)
    assert L.mw_nuc_finalize() == 0                                          # nothing to undo is not an error
    from mc_water_ls_mw_amd import nucleation
    with pytest.raises(nucleation.MwError, match="not initialised"):
        nucleation.nuc_last()


def test_argument_validation_needs_no_device():
    L = _lib()
    cells, pos = _args()
    narrow = cells.copy()
    narrow[1, 8] = 8.0
    nan, inf = float("nan"), float("inf")
    spoiled = pos.copy()
    spoiled[1, 2, 1] = nan

    def at(a, box, value):
        b = a.copy()
        b[box] = value
        return b

    cases = [
        # what the issue lists for the new arguments
        (dict(nwater=64, pos=pos[:, :64].copy()), r"nwater = 64\b.*one-wavefront-per-box.*box 0\b"),
        (dict(rc=A_SIGMA * (1.0 + 1e-12)), r"\brc\b.*a sigma.*box 0\b"), (dict(rc=A_SIGMA), r"\brc\b.*a sigma"),
        (dict(nsteps=12, check_every=5), r"check_every = 5\b.*nsteps = 12\b.*box 0\b"),
        (dict(lo=at(LO, 1, 40)), r"lam_lo = 40\b.*lam_hi = 40\b.*box 1\b"), (dict(lo=at(LO, 0, N + 1)), r"lam_lo.*lam_hi.*box 0\b"),
        (dict(min_conn=0), r"min_conn = 0\b.*box 0\b"),
        (dict(threshold=nan), r"threshold.*box 0\b"),
        # their other edges
        (dict(rc=0.0), r"\brc\b"), (dict(rc=nan), r"\brc\b"), (dict(rc=-1.0), r"\brc\b"), (dict(threshold=1.5), "threshold"), (dict(threshold=-1.5), "threshold"),
        (dict(min_conn=65), "min_conn"), (dict(check_every=0), "check_every"), (dict(check_every=-5), "check_every"), (dict(lo=at(LO, 1, -2)), r"lam_lo.*box 1\b"),
        (dict(lo=None), "lam_lo"), (dict(hi=None), "lam_hi"), (dict(nwater=1, pos=pos[:, :1].copy()), "nwater"),
        # every argument of mw_flex_run keeps its check
        (dict(nboxes=0), "nboxes"), (dict(nwater=0), "nwater"), (dict(cells=None), "cells"), (dict(pos=None), r"\bpos\b"),
        (dict(nsteps=-5), "nsteps"), (dict(nsteps=100000005), "nsteps"), (dict(sample_every=0), "sample_every"),
        (dict(dt=0.0), r"\bdt\b"), (dict(dt=nan), r"\bdt\b"), (dict(mass=0.0), "mass"), (dict(kT=-1e-9), "kT"), (dict(gamma=nan), "gamma"),
        (dict(pressure=nan), "pressure"), (dict(tau_p=0.0), "tau_p"), (dict(beta_T=inf), "beta_T"), (dict(baro_every=-1), "baro_every"),
        (dict(coupling=-1), "coupling"), (dict(coupling=4), "coupling"), (dict(axis=-1), "axis"), (dict(axis=3), "axis"),
        (dict(cells=narrow), r"a_sigma.*box 1\b"), (dict(pos=spoiled), r"\bpos\b.*box 1\b"), (dict(vel=spoiled), r"\bvel\b.*box 1\b"),
        (dict(pos_ref=spoiled), r"\bpos_ref\b.*box 1\b"),
    ]
    for change, pattern in cases:
        kw = dict(cells=cells, pos=pos)
        kw.update(change)
        rc_, msg, clean = _run(L, **kw)
        assert rc_ != 0 and re.search(pattern, msg) and "mw_nuc_run" in msg and "not initialised" not in msg and clean, (change, msg)
    # with good arguments -- the bounds themselves included -- the next thing a call without a device meets is the state
    import torch
    if not torch.cuda.is_available() and not L.mw_nuc_is_initialised():
        for kw in (dict(), dict(nsteps=0), dict(rc=A_SIGMA * (1.0 - 2e-9)), dict(threshold=-1.0), dict(threshold=1.0), dict(min_conn=64), dict(min_conn=1),
                   dict(check_every=10), dict(check_every=1), dict(lo=at(LO, 1, 39)), dict(lo=at(LO, 0, N)), dict(hi=at(HI, 0, 0)), dict(baro_every=0)):
            full = dict(cells=cells, pos=pos)
            full.update(kw)
            rc_, msg, clean = _run(L, **full)
            assert rc_ != 0 and "not initialised" in msg and clean, (kw, msg)
    # the device-pointer entry checks what it can see from the host before anything else
    for kw, pattern in ((dict(nboxes=0), "nboxes"), (dict(cells=None), "cells"), (dict(lo=None), "lam_lo"), (dict(hi=None), "lam_hi"), (dict(dt=nan), r"\bdt\b"),
                        (dict(nwater=64), "nwater = 64"), (dict(rc=9.0), r"\brc\b"), (dict(min_conn=0), "min_conn"), (dict(threshold=nan), "threshold"),
                        (dict(nsteps=12), "check_every"), (dict(coupling=7), "coupling")):
        full = dict(cells=cells, pos=pos)
        full.update(kw)
        rc_, msg, clean = _run(L, entry="mw_nuc_run_device", **full)
        assert rc_ != 0 and re.search(pattern, msg) and "mw_nuc_run_device" in msg and clean, msg
    from mc_water_ls_mw_amd import nucleation
    h, x = np.eye(3) * 30.0, np.zeros((N, 3))
    with pytest.raises(nucleation.MwError, match="coupling"):
        nucleation.nucleus_md(h, x, 5, 1.0, coupling="sheared")
    with pytest.raises(nucleation.MwError, match="lam_hi"):
        nucleation.nucleus_md(h, x, 5, 1.0, lam_hi=[1, 2])


def test_init_without_a_device_fails_with_its_message():
    import torch
    if torch.cuda.is_available():
        return                                                               # (the no-device behaviour belongs to a machine without one)
    L = _lib()
    assert L.mw_nuc_init(0) != 0
    msg = L.mw_nuc_last_error().decode()
    assert "no HIP device" in msg and "mw_nuc_init" in msg and not L.mw_nuc_is_initialised()


def test_plan_works_without_a_device_and_follows_mw_flex_plan():
    """The grid is that of a sigma, as mw_flex_plan's; the scratch of a box is flex's plus what the order parameter keeps; the
    labels live in LDS while 8 bytes per molecule fit 160 KiB less 512 bytes."""
    _lib()
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.flexcell import flex_plan, load_flex_library
    from mc_water_ls_mw_amd.nucleation import MwError, nuc_plan
    build.build_flex()
    assert load_flex_library() is not None
    a16 = lambda v: (v + 15) // 16 * 16                                      # noqa: E731
    budget = 256 << 20
    for h in (load_golden("ih4096_t015")["h"], np.array([[41.0, 0.0, 0.0], [9.0, 37.0, 0.0], [-6.0, 11.0, 45.0]])):
        for n in (65, 96, 1536, 20416, 20417, 32768):
            extra = a16(8 * 14 * n) + a16(4 * n) * 5 + a16(4 * 12 * n) + a16(8 * n) + 16 + a16(8 * 19) - a16(8 * 16)   # rec; cnt, sol, label and the two working arrays; list; nn; op; three more row doubles
            for nboxes in (1, 200, 3000000):
                p, q = nuc_plan(n, h, nboxes), flex_plan(n, h, nboxes)
                for f in ("small", "g1", "g2", "g3", "boxes_per_workgroup", "steps_per_launch"):
                    assert p[f] == q[f], (n, nboxes, f)
                assert p["scratch_bytes_per_box"] == q["scratch_bytes_per_box"] + extra, (n, p, q)
                most = min(budget // p["scratch_bytes_per_box"], 65535, nboxes)
                assert p["boxes_per_chunk"] == most and p["chunks"] == -(-nboxes // most), (n, nboxes, p)
                lds = a16(8 * n) <= 160 * 1024 - 512
                assert p["labels_in_lds"] == int(lds) == int(n <= 20416) and p["lds_bytes"] == (a16(8 * n) if lds else 0) + 512 and p["cluster_rounds"] == 0
    with pytest.raises(MwError, match="nwater"):
        nuc_plan(64, np.eye(3) * 40.0, 1)
    with pytest.raises(MwError, match=r"a_sigma.*box 0\b"):
        nuc_plan(96, np.diag([40.0, 40.0, 8.0]), 1)
