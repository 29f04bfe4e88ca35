"""CPU: libmw_pin.so builds for gfx950, loads without a GPU, exports what include/mw_pin.h declares and nothing else, keeps its
kernels free of private segments and vector-register spills, rejects bad arguments and uninitialised calls with messages that name
the entry, the argument and the first offending box and leaves the outputs alone, and reports the launch rules of mw_flex_plan
through mw_pin_plan."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from test_flex_abi import A_SIGMA, MASS, READELF, _gfx950_code_object

KERNELS = ("k_cells_bin", "k_cells_scan", "k_cells_place", "k_cells_rank", "k_pin_check", "k_pin_begin", "k_pin_finish", "k_pin_drift1", "k_pin_drift2",
           "k_pin_moments", "k_pin_rho", "k_pin_forces", "k_pin_row", "k_pin_small", "k_pin_baro", "k_pin_scale")


def _lib():
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.pinning import load_pin_library
    build.build_pin()
    return load_pin_library()


def _declared():
    text = open(os.path.join(ROOT, "include", "mw_pin.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mw_pin_\w+)\s*\(", text)))


def test_build_pin_compiles_for_gfx950_and_moves_with_no_other_library():
    from mc_water_ls_mw_amd import build
    lib = build.build_pin(force=True)
    assert lib == build.PIN_LIB and os.path.exists(lib)
    data = open(lib, "rb").read()
    assert b"__CLANG_OFFLOAD_BUNDLE__" in data and b"gfx950" in data
    for kernel in KERNELS:
        assert kernel.encode() in data, kernel
    header = os.path.join(ROOT, "include", "mw_pin.h")
    shared = [os.path.join(build.CSRC, f) for f in ("mw_lib_host.h", "mw_lib_cells.h", "mw_lib_forces.h", "mw_common.hip.h")]
    assert sorted(build.PIN_DEPS) == sorted([build.PIN_SRC, header, *shared]) and all(os.path.exists(p) for p in build.PIN_DEPS)
    for deps in (build.DEPS, build.SK_DEPS, build.BOO_DEPS, build.TET_DEPS, build.ADF_DEPS, build.RINGS_DEPS, build.QUENCH_BUILD_DEPS, build.MD_DEPS,
                 build.NPT_DEPS, build.TCF_DEPS, build.HESS_DEPS, build.TI_DEPS, build.FLEX_DEPS, build.COMMS_DEPS):
        assert not any(p in deps for p in (build.PIN_SRC, header))
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "mwbuild.build_pin(" in text
    assert re.search(r"for builder in \(.*build_pin\b", open(os.path.join(ROOT, "mc_water_ls_mw_amd", "build.py")).read())
    src = open(build.PIN_SRC).read()
    assert "sincospi(" in src and "atomicAdd" not in src and src.index("#pragma clang fp contract(off)") < src.index('#include "mw_lib_host.h"')


def test_every_declared_name_is_exported_and_listed():
    L = _lib()
    from mc_water_ls_mw_amd import flexcell, pinning
    names = _declared()
    assert len(names) == 9 and sorted(pinning.PIN_ABI_SYMBOLS) == names
    for name in names:
        assert hasattr(L, name), name
    text = open(os.path.join(ROOT, "include", "mw_pin.h")).read()
    for word, value in (("PLAN_FIELDS", 10), ("TRACE_FIELDS", 17), ("BLOCK_FIELDS", 4), ("MAX_STEPS", 100000000), ("MAX_N", 255)):
        assert re.search(r"#define\s+MW_PIN_%s\s+%d\b" % (word, value), text), word
    assert len(pinning.TRACE_FIELDS) == 17 and pinning.TRACE_FIELDS[:15] == flexcell.TRACE_FIELDS and len(pinning.BLOCK_FIELDS) == 4 and pinning.MAX_N == 255
    for name, value in flexcell.COUPLINGS.items():
        assert re.search(r"#define\s+MW_PIN_%s\s+%d\b" % (name.upper(), value), text), name
    import pin_ref
    assert pin_ref.TRACE_FIELDS == 17 and pin_ref.BLOCK_FIELDS == 4


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not in this image")
def test_the_library_exports_its_own_names_alone_and_no_kernel_has_a_private_segment(tmp_path):
    """The counts are printed.  The force pass stays within the 168 vector registers of three wavefronts per SIMD, as
    libmw_flex.so's; the moment pass within the 128 of four; the small kernel parks scalar registers in vector lanes, as
    libmw_flex.so's does."""
    from mc_water_ls_mw_amd import build
    build.build_pin()
    out = subprocess.run([READELF, "--dyn-syms", "-W", build.PIN_LIB], capture_output=True, text=True, check=True).stdout
    rows = [ln.split() for ln in out.splitlines()]
    defined = {f[7].split("@")[0] for f in rows if len(f) == 8 and f[0].endswith(":") and f[6] != "UND" and f[7].startswith("mw_")}
    assert defined == set(_declared())
    data = open(build.PIN_LIB, "rb").read()
    for word in (b"mw_flex", b"k_flex_", b"mwflex", b"k_ti_", b"mw_ti_", b"k_md_", b"k_npt_", b"mw_sk_"):
        assert word not in data, word
    notes = subprocess.run([READELF, "--notes", _gfx950_code_object(build.PIN_LIB, tmp_path)], capture_output=True, text=True, check=True).stdout
    seen = set()
    for blk in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.match(r"_ZN5mwpin\d+(k_pin_[a-z0-9]+)(E|ILb[01]EEE)", name) or re.match(r"_ZN7mwcells\d+(k_cells_[a-z]+)(E)", name)
        assert m, name
        get = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))     # noqa: E731
        print(m.group(1), m.group(2), "vgprs", get("vgpr_count"), "sgprs", get("sgpr_count"), "sgpr spills", get("sgpr_spill_count"), "lds", get("group_segment_fixed_size"))
        assert get("private_segment_fixed_size") == 0 and get("vgpr_spill_count") == 0, name
        if m.group(1) != "k_pin_small":
            assert get("sgpr_spill_count") == 0, name
        if m.group(1) == "k_pin_moments":
            assert get("vgpr_count") <= 128
        if m.group(1) == "k_pin_forces":
            assert get("vgpr_count") <= 168 and get("group_segment_fixed_size") == 4 * 17 * 8
        seen.add(m.group(1))
    assert seen == set(KERNELS)


def _args(nboxes=2, nwater=4):
    cells = np.tile(np.eye(3).ravel() * 20.0, (nboxes, 1))
    pos = np.arange(nboxes * nwater * 3, dtype=np.float64).reshape(nboxes, nwater, 3) * 0.7
    return cells, pos


NVEC = np.array([[1, 0, 0], [2, -3, 255]], dtype=np.int32)
KAPPAS = np.array([0.0, 0.5])
ANCHORS = np.array([0.0, 1.5])
_DEFAULT = object()


def _run(L, nboxes=2, nwater=4, cells=None, pos=None, vel=None, pos_ref=None, nvec=_DEFAULT, kappas=_DEFAULT, anchors=_DEFAULT, nsteps=10, sample_every=1,
         equil_steps=2, block_steps=4, dt=100.0, mass=MASS, kT=1e-3, gamma=1e-3, pressure=1e-8, tau_p=4e4, beta_T=1e4, baro_every=2, coupling=3, axis=2,
         entry="mw_pin_run"):
    """One run entry with outputs prefilled so that a write would show."""
    nvec = NVEC if nvec is _DEFAULT else nvec
    kappas = KAPPAS if kappas is _DEFAULT else kappas
    anchors = ANCHORS if anchors is _DEFAULT else anchors
    outs = [np.full(3 * 16, -7.0), np.full(3 * 16, -7.0), np.full(3 * 16, -7.0), np.full(9 * 2, -7.0), np.full(3 * 16, -7.0), np.full(17 * 200 * 2, -7.0),
            np.full(4 * 50 * 2, -7.0), np.full(2 * 2, -7, dtype=np.int32)]
    ptr = lambda a: None if a is None else a.ctypes.data                   # noqa: E731
    rc_ = getattr(L, entry)(nboxes, nwater, ptr(cells), ptr(pos), ptr(vel), ptr(pos_ref), ptr(nvec), ptr(kappas), ptr(anchors), None, 1, 0, nsteps, sample_every,
                            equil_steps, block_steps, dt, mass, kT, gamma, pressure, tau_p, beta_T, baro_every, coupling, axis, *[o.ctypes.data for o in outs])
    return rc_, L.mw_pin_last_error().decode(), all(bool(np.all(o == -7)) for o in outs)


def test_calls_before_init_fail_with_not_initialised():
    L = _lib()
    assert not L.mw_pin_is_initialised()                                     # (the CPU tests never initialise it)
    cells, pos = _args()
    for entry in ("mw_pin_run", "mw_pin_run_device"):
        rc_, msg, clean = _run(L, cells=cells, pos=pos, entry=entry)
        assert rc_ != 0 and "not initialised" in msg and entry in msg and clean, msg
    out = (ctypes.c_int * 10)()
    t = [ctypes.c_float(-1.0) for _ in range(6)]
    for name, call in (("mw_pin_last", lambda: L.mw_pin_last(out, 10)), ("mw_pin_elapsed_ms", lambda: L.mw_pin_elapsed_ms(*[ctypes.byref(v) for v in t]))):
        assert call() != 0, name
        msg = L.mw_pin_last_error().decode()
        assert "not initialised" in msg and name in msg, msg
    assert not any(out) and all(v.value == -1.0 for v in t)
    assert L.mw_pin_finalize() == 0                                          # nothing to undo is not an error
    from mc_water_ls_mw_amd import pinning
    with pytest.raises(pinning.MwError, match="not initialised"):
        pinning.pin_last()


def test_argument_validation_needs_no_device():
    L = _lib()
    cells, pos = _args(2, 4)
    narrow = cells.copy()
    narrow[1, 8] = 8.0
    nan, inf = float("nan"), float("inf")

    def at(a, box, value, col=None):
        b = a.copy()
        if col is None:
            b[box] = value
        else:
            b[box, col] = value
        return b

    spoiled = pos.copy()
    spoiled[1, 2, 1] = nan
    cases = [
        (dict(nboxes=0), "nboxes"), (dict(nwater=0), "nwater"), (dict(cells=None), "cells"), (dict(pos=None), r"\bpos\b"),
        (dict(nvec=None), "nvec"), (dict(kappas=None), "kappas"), (dict(anchors=None), "anchors"),
        (dict(nsteps=-1), "nsteps"), (dict(nsteps=100000001), "nsteps"), (dict(sample_every=0), "sample_every"),
        (dict(equil_steps=-1), "equil_steps"), (dict(block_steps=-1), "block_steps"),
        (dict(dt=0.0), r"\bdt\b"), (dict(dt=nan), r"\bdt\b"), (dict(mass=0.0), "mass"), (dict(kT=-1e-9), "kT"), (dict(gamma=nan), "gamma"),
        (dict(pressure=nan), "pressure"), (dict(tau_p=0.0), "tau_p"), (dict(beta_T=inf), "beta_T"), (dict(baro_every=-1), "baro_every"),
        (dict(coupling=-1), "coupling"), (dict(coupling=4), "coupling"), (dict(axis=-1), "axis"), (dict(axis=3), "axis"), (dict(coupling=0, axis=3), "axis"),
        (dict(nvec=at(NVEC, 1, 0)), r"nvec.*box 1\b.*\(0, 0, 0\)"), (dict(nvec=at(NVEC, 0, 0)), r"nvec.*box 0\b"),
        (dict(nvec=at(NVEC, 1, 256, 2)), r"nvec.*box 1\b.*256"), (dict(nvec=at(NVEC, 1, -256, 0)), r"nvec.*box 1\b.*-256"),
        (dict(kappas=at(KAPPAS, 1, nan)), r"kappas.*box 1\b"), (dict(kappas=at(KAPPAS, 0, -1e-9)), r"kappas.*box 0\b"), (dict(kappas=at(KAPPAS, 1, inf)), r"kappas.*box 1\b"),
        (dict(anchors=at(ANCHORS, 1, nan)), r"anchors.*box 1\b"), (dict(anchors=at(ANCHORS, 1, -0.5)), r"anchors.*box 1\b"), (dict(anchors=at(ANCHORS, 0, inf)), r"anchors.*box 0\b"),
        (dict(cells=narrow), r"a_sigma.*box 1\b"), (dict(pos=spoiled), r"\bpos\b.*box 1\b"), (dict(vel=spoiled), r"\bvel\b.*box 1\b"),
        (dict(pos_ref=spoiled), r"\bpos_ref\b.*box 1\b"),
    ]
    for change, pattern in cases:
        kw = dict(cells=cells, pos=pos)
        kw.update(change)
        rc_, msg, clean = _run(L, **kw)
        assert rc_ != 0 and re.search(pattern, msg) and "mw_pin_run" in msg and "not initialised" not in msg and clean, (change, msg)
    # with good arguments -- the bounds themselves included -- the next thing a call without a device meets is the state
    import torch
    if not torch.cuda.is_available() and not L.mw_pin_is_initialised():
        wide = cells.copy()
        wide[1, 0] = A_SIGMA * (1.0 + 1e-9) * (1.0 + 1e-15)
        for kw in (dict(), dict(nsteps=0), dict(cells=wide), dict(nvec=at(NVEC, 0, -255)), dict(kappas=at(KAPPAS, 1, 0.0)), dict(anchors=at(ANCHORS, 1, 0.0)),
                   dict(baro_every=0), dict(coupling=0, axis=0), dict(coupling=1), dict(block_steps=0), dict(equil_steps=50)):
            full = dict(cells=cells, pos=pos)
            full.update(kw)
            rc_, msg, clean = _run(L, **full)
            assert rc_ != 0 and "not initialised" in msg and clean, msg
    # the device-pointer entry checks what it can see from the host before anything else
    for kw, pattern in ((dict(nboxes=0), "nboxes"), (dict(cells=None), "cells"), (dict(nvec=None), "nvec"), (dict(kappas=None), "kappas"), (dict(anchors=None), "anchors"),
                        (dict(dt=nan), r"\bdt\b"), (dict(block_steps=-2), "block_steps"), (dict(coupling=7), "coupling"), (dict(axis=5), "axis")):
        full = dict(cells=cells, pos=pos)
        full.update(kw)
        rc_, msg, clean = _run(L, entry="mw_pin_run_device", **full)
        assert rc_ != 0 and re.search(pattern, msg) and "mw_pin_run_device" in msg and clean, msg
    from mc_water_ls_mw_amd import pinning
    h, x = np.eye(3) * 20.0, np.zeros((4, 3))
    with pytest.raises(pinning.MwError, match="coupling"):
        pinning.interface_pinning(h, x, (1, 0, 0), 1.0, 1.0, 1, 1.0, coupling="sheared")
    with pytest.raises(pinning.MwError, match="nvec"):
        pinning.interface_pinning(h, x, (1, 0), 1.0, 1.0, 1, 1.0)
    with pytest.raises(pinning.MwError, match="nvec"):
        pinning.interface_pinning(h, x, (1.0, 0.0, 0.0), 1.0, 1.0, 1, 1.0)
    with pytest.raises(pinning.MwError, match="kappa"):
        pinning.interface_pinning(h, x, (1, 0, 0), [1.0, 2.0], 1.0, 1, 1.0)


def test_init_without_a_device_fails_with_its_message():
    import torch
    if torch.cuda.is_available():
        return                                                               # (the no-device behaviour belongs to a machine without one)
    L = _lib()
    assert L.mw_pin_init(0) != 0
    msg = L.mw_pin_last_error().decode()
    assert "no HIP device" in msg and "mw_pin_init" in msg and not L.mw_pin_is_initialised()


def test_plan_is_that_of_mw_flex_plan_with_the_scratch_of_the_bias():
    """Geometry, grid, boxes per workgroup and steps per launch are mw_flex_plan's; the scratch of a box is its own plus two more
    row doubles, the four accumulators and, in the general geometry, the pair of every molecule, two partial sums per workgroup and
    the eight doubles of the mode; the LDS of the small geometry holds the accumulators, w and g k besides."""
    _lib()
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.flexcell import flex_plan, load_flex_library
    from mc_water_ls_mw_amd.pinning import MwError, pin_plan
    build.build_flex()
    assert load_flex_library() is not None
    a16 = lambda v: (v + 15) // 16 * 16                                      # noqa: E731
    budget = 256 << 20
    for h in (load_golden("ih4096_t015")["h"], np.array([[41.0, 0.0, 0.0], [9.0, 37.0, 0.0], [-6.0, 11.0, 45.0]])):
        for n in (2, 48, 64, 65, 96, 1536):
            small = n <= 64
            extra = 16 + a16(8 * 4) + (0 if small else a16(16 * n) + a16(16 * (-(-n // 256))) + a16(64))
            for nboxes in (1, 200, 3000000):
                p, q = pin_plan(n, h, nboxes), flex_plan(n, h, nboxes)
                for f in ("small", "g1", "g2", "g3", "boxes_per_workgroup", "steps_per_launch"):
                    assert p[f] == q[f], (n, nboxes, f)
                assert p["scratch_bytes_per_box"] == q["scratch_bytes_per_box"] + extra, (n, p, q)
                most = min(budget // p["scratch_bytes_per_box"], (1 << 20) if small else 65535, nboxes)
                assert p["boxes_per_chunk"] == most and p["chunks"] == -(-nboxes // most), (n, nboxes, p)
                assert p["lds_bytes"] == (4 * (13 * 64 + 4 + 64 + 4) * 8 if small else 4 * 17 * 8)
    with pytest.raises(MwError, match="nwater"):
        pin_plan(0, np.eye(3) * 40.0, 1)
    with pytest.raises(MwError, match=r"a_sigma.*box 0\b"):
        pin_plan(8, np.diag([40.0, 40.0, 8.0]), 1)


def test_the_host_helpers():
    from mc_water_ls_mw_amd import pinning
    blocks = np.zeros((4, 4))
    blocks[:, 0] = (5.0, 5.2, 4.8, 5.0)
    mu, err = pinning.delta_mu(blocks, 0.02, 4.0, 8.0, 1.0, 96)
    assert np.isclose(mu, -0.02 * (5.0 - 4.0) * 7.0 / 96.0, rtol=1e-14) and np.isclose(err, 0.02 * 7.0 / 96.0 * np.std(blocks[:, 0], ddof=1) / 2.0, rtol=1e-14)
    with pytest.raises(pinning.MwError, match="blocks"):
        pinning.delta_mu(blocks[:1], 0.02, 4.0, 8.0, 1.0, 96)
    assert pinning.anchor_for_fraction(8.0, 1.0, 0.5) == 4.5 and pinning.anchor_for_fraction(8.0, 1.0, 0.0) == 1.0
    with pytest.raises(pinning.MwError, match="fraction"):
        pinning.anchor_for_fraction(8.0, 1.0, 1.5)
    n = pinning._half_space(2, None)
    assert len(n) == (5 ** 3 - 1) // 2 and not any((-v).tolist() in n.tolist() for v in n)
    assert np.all(pinning._half_space(3, 2)[:, 2] == 0) and len(pinning._half_space(3, 2)) == (7 ** 2 - 1) // 2
    src = open(os.path.join(ROOT, "mc_water_ls_mw_amd", "pinning.py")).read()
    assert "oracle" not in src
