"""Build libmw_hip.so (the C-ABI engine), libmw_comms.so (the RCCL exchange layer for a Fortran host, include/mw_comms.h),
libmw_sk.so (the structure factor S(k), include/mw_sk.h), libmw_boo.so (the Steinhardt bond-order parameters,
include/mw_boo.h), libmw_tet.so (tetrahedral order, d5 and LSI from the sorted nearest neighbours, include/mw_tet.h),
libmw_adf.so (the O-O-O angle distribution, include/mw_adf.h), libmw_rings.so (the primitive rings of the bond network,
include/mw_rings.h), libmw_quench.so (inherent-structure quenches, include/mw_quench.h), libmw_md.so (molecular dynamics,
include/mw_md.h), libmw_npt.so (molecular dynamics at constant pressure, include/mw_npt.h), libmw_tcf.so (time correlation
functions of trajectories, include/mw_tcf.h), libmw_hess.so (the Hessian of the energy and its products with vectors,
include/mw_hess.h), libmw_ti.so (Einstein-crystal thermodynamic integration, include/mw_ti.h), libmw_flex.so (molecular
dynamics at constant pressure with a per-axis cell and the pressure tensor, include/mw_flex.h), libmw_pin.so (interface
pinning: that step with a bias on a collective density mode, include/mw_pin.h) and libmw_nuc.so (that step with the size of the
largest solid-like cluster watched and stopping rules on the device, include/mw_nuc.h) and libmw_coll.so (collective time
correlations of trajectories: F(k, t), the distinct van Hove function and the overlap sums, include/mw_coll.h) in-tree with
hipcc for gfx950.

    python -m mc_water_ls_mw_amd.build [--force]

Each library is one hipcc call (`_compile`), skipped when the library is newer than every file it depends on.  hipcc
cross-compiles gfx950 without a GPU.  The libraries stay inside the package directory, git-ignored.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
LIB = os.path.join(PKG, "libmw_hip.so")
SOURCES = [os.path.join(CSRC, "mw_api.hip")]
DEPS = SOURCES + sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip.h")) + \
    [os.path.join(os.path.dirname(PKG), "include", "mw_energy.h")]
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
               "-fno-fast-math", "-Wall", "-Wno-unused-function", "-Wno-unused-value", "-Wno-unused-result"]

COMMS_LIB = os.path.join(PKG, "libmw_comms.so")
COMMS_SRC = os.path.join(CSRC, "mw_comms.hip")
COMMS_DEPS = [COMMS_SRC, os.path.join(os.path.dirname(PKG), "include", "mw_comms.h")]

LIB_HOST = os.path.join(CSRC, "mw_lib_host.h")       # the host layer libmw_sk.so, libmw_boo.so, libmw_tet.so, libmw_adf.so and libmw_rings.so share; not a dependency of libmw_hip.so
LIB_CELLS = os.path.join(CSRC, "mw_lib_cells.h")     # the cell grid, counting sort and walks of libmw_boo.so, libmw_tet.so, libmw_adf.so and libmw_rings.so; not a
#                                                     `.hip.h`: DEPS takes every one of those for libmw_hip.so, and libmw_sk.so has no cell grid
SK_LIB = os.path.join(PKG, "libmw_sk.so")
SK_SRC = os.path.join(CSRC, "mw_sk.hip")
SK_DEPS = [SK_SRC, LIB_HOST, os.path.join(CSRC, "mw_common.hip.h"), os.path.join(os.path.dirname(PKG), "include", "mw_sk.h")]

BOO_LIB = os.path.join(PKG, "libmw_boo.so")
BOO_SRC = os.path.join(CSRC, "mw_boo.hip")
LIB_HARMONICS = os.path.join(CSRC, "mw_lib_harmonics.h")   # the real harmonics of l = 4 and 6 libmw_boo.so and libmw_nuc.so share
BOO_DEPS = [BOO_SRC, LIB_HOST, LIB_CELLS, LIB_HARMONICS, os.path.join(CSRC, "mw_common.hip.h"), os.path.join(os.path.dirname(PKG), "include", "mw_boo.h")]

TET_LIB = os.path.join(PKG, "libmw_tet.so")
TET_SRC = os.path.join(CSRC, "mw_tet.hip")
TET_DEPS = [TET_SRC, LIB_HOST, LIB_CELLS, os.path.join(CSRC, "mw_common.hip.h"), os.path.join(os.path.dirname(PKG), "include", "mw_tet.h")]

ADF_LIB = os.path.join(PKG, "libmw_adf.so")
ADF_SRC = os.path.join(CSRC, "mw_adf.hip")
ADF_DEPS = [ADF_SRC, LIB_HOST, LIB_CELLS, os.path.join(CSRC, "mw_common.hip.h"), os.path.join(os.path.dirname(PKG), "include", "mw_adf.h")]

RINGS_LIB = os.path.join(PKG, "libmw_rings.so")
RINGS_SRC = os.path.join(CSRC, "mw_rings.hip")
RINGS_DEPS = [RINGS_SRC, LIB_HOST, LIB_CELLS, os.path.join(CSRC, "mw_common.hip.h"), os.path.join(os.path.dirname(PKG), "include", "mw_rings.h")]

QUENCH_LIB = os.path.join(PKG, "libmw_quench.so")
QUENCH_SRC = os.path.join(CSRC, "mw_quench.hip")
QUENCH_DEPS = [QUENCH_SRC, LIB_HOST, LIB_CELLS, os.path.join(CSRC, "mw_common.hip.h"), os.path.join(os.path.dirname(PKG), "include", "mw_quench.h")]
LIB_FORCES = os.path.join(CSRC, "mw_lib_forces.h")   # the moments, the entry force and virial and the fixed-order reductions libmw_quench.so, libmw_md.so and libmw_npt.so share
QUENCH_BUILD_DEPS = [*QUENCH_DEPS, LIB_FORCES]       # what build_quench watches: the library's own files and the shared force layer

MD_LIB = os.path.join(PKG, "libmw_md.so")
MD_SRC = os.path.join(CSRC, "mw_md.hip")
MD_DEPS = [MD_SRC, LIB_HOST, LIB_CELLS, LIB_FORCES, os.path.join(CSRC, "mw_common.hip.h"), os.path.join(os.path.dirname(PKG), "include", "mw_md.h")]

NPT_LIB = os.path.join(PKG, "libmw_npt.so")
NPT_SRC = os.path.join(CSRC, "mw_npt.hip")
NPT_DEPS = [NPT_SRC, LIB_HOST, LIB_CELLS, LIB_FORCES, os.path.join(CSRC, "mw_common.hip.h"), os.path.join(os.path.dirname(PKG), "include", "mw_npt.h")]

TCF_LIB = os.path.join(PKG, "libmw_tcf.so")
TCF_SRC = os.path.join(CSRC, "mw_tcf.hip")
TCF_DEPS = [TCF_SRC, LIB_HOST, os.path.join(os.path.dirname(PKG), "include", "mw_tcf.h")]   # no cell grid and no shared device header

HESS_LIB = os.path.join(PKG, "libmw_hess.so")
HESS_SRC = os.path.join(CSRC, "mw_hess.hip")
HESS_DEPS = [HESS_SRC, LIB_HOST, LIB_CELLS, LIB_FORCES, os.path.join(CSRC, "mw_common.hip.h"), os.path.join(os.path.dirname(PKG), "include", "mw_hess.h")]

TI_LIB = os.path.join(PKG, "libmw_ti.so")
TI_SRC = os.path.join(CSRC, "mw_ti.hip")
TI_DEPS = [TI_SRC, LIB_HOST, LIB_CELLS, LIB_FORCES, os.path.join(CSRC, "mw_common.hip.h"), os.path.join(os.path.dirname(PKG), "include", "mw_ti.h")]

FLEX_LIB = os.path.join(PKG, "libmw_flex.so")
FLEX_SRC = os.path.join(CSRC, "mw_flex.hip")
FLEX_DEPS = [FLEX_SRC, LIB_HOST, LIB_CELLS, LIB_FORCES, os.path.join(CSRC, "mw_common.hip.h"), os.path.join(os.path.dirname(PKG), "include", "mw_flex.h")]

PIN_LIB = os.path.join(PKG, "libmw_pin.so")
PIN_SRC = os.path.join(CSRC, "mw_pin.hip")
PIN_DEPS = [PIN_SRC, LIB_HOST, LIB_CELLS, LIB_FORCES, os.path.join(CSRC, "mw_common.hip.h"), os.path.join(os.path.dirname(PKG), "include", "mw_pin.h")]

NUC_LIB = os.path.join(PKG, "libmw_nuc.so")
NUC_SRC = os.path.join(CSRC, "mw_nuc.hip")
NUC_DEPS = [NUC_SRC, LIB_HOST, LIB_CELLS, LIB_FORCES, LIB_HARMONICS, os.path.join(CSRC, "mw_common.hip.h"),
            os.path.join(os.path.dirname(PKG), "include", "mw_nuc.h"), os.path.join(os.path.dirname(PKG), "include", "mw_flex.h")]

COLL_LIB = os.path.join(PKG, "libmw_coll.so")
COLL_SRC = os.path.join(CSRC, "mw_coll.hip")
COLL_DEPS = [COLL_SRC, LIB_HOST, os.path.join(os.path.dirname(PKG), "include", "mw_coll.h")]   # no cell grid and no shared device header


def hipcc_path():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (ROCm is required to build libmw_hip.so)")


def needs_build():
    return _stale(LIB, DEPS)


def _stale(lib, deps):
    return not os.path.exists(lib) or any(os.path.getmtime(p) > os.path.getmtime(lib) for p in deps)


def _compile(lib, sources, deps, flags, link=(), force=False, verbose=False):
    """hipcc `flags` -o `lib` `sources` `link`, unless `lib` is newer than every file of `deps`."""
    if not force and not _stale(lib, deps):
        return lib
    cmd = [hipcc_path(), *flags, "-o", lib, *sources, *link]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return lib


def build(force=False, verbose=False, extra_flags=(), out=None):
    """`out`: another file name for a variant of the library (diagnostic builds, A/B measurements with MW_HIP_LIB)."""
    return _compile(out or LIB, SOURCES, DEPS, [*HIPCC_FLAGS, *extra_flags], force=force, verbose=verbose)


def build_comms(force=False, verbose=False):
    """libmw_comms.so: host code only (no kernels), linked against RCCL."""
    return _compile(COMMS_LIB, [COMMS_SRC], COMMS_DEPS, ["--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall"],
                    ["-L/opt/rocm/lib", "-lrccl", "-Wl,-rpath,/opt/rocm/lib"], force, verbose)


def build_sk(force=False, verbose=False):
    """libmw_sk.so: the structure-factor kernels and their C ABI, a translation unit of its own (libmw_hip.so's code object
    and symbols do not move with it)."""
    return _compile(SK_LIB, [SK_SRC], SK_DEPS, HIPCC_FLAGS, force=force, verbose=verbose)


def build_boo(force=False, verbose=False):
    """libmw_boo.so: the bond-order kernels and their C ABI, a translation unit of its own like libmw_sk.so."""
    return _compile(BOO_LIB, [BOO_SRC], BOO_DEPS, HIPCC_FLAGS, force=force, verbose=verbose)


def build_tet(force=False, verbose=False):
    """libmw_tet.so: the nearest-neighbour selection kernels and their C ABI, a translation unit of its own like libmw_boo.so."""
    return _compile(TET_LIB, [TET_SRC], TET_DEPS, HIPCC_FLAGS, force=force, verbose=verbose)


def build_adf(force=False, verbose=False):
    """libmw_adf.so: the O-O-O angle histogram kernels and their C ABI, a translation unit of its own like libmw_tet.so."""
    return _compile(ADF_LIB, [ADF_SRC], ADF_DEPS, HIPCC_FLAGS, force=force, verbose=verbose)


def build_rings(force=False, verbose=False):
    """libmw_rings.so: the adjacency and ring-walk kernels and their C ABI, a translation unit of its own like libmw_adf.so."""
    return _compile(RINGS_LIB, [RINGS_SRC], RINGS_DEPS, HIPCC_FLAGS, force=force, verbose=verbose)


def build_quench(force=False, verbose=False):
    """libmw_quench.so: the FIRE quench kernels and their C ABI, a translation unit of its own like libmw_rings.so."""
    return _compile(QUENCH_LIB, [QUENCH_SRC], QUENCH_BUILD_DEPS, HIPCC_FLAGS, force=force, verbose=verbose)


def build_md(force=False, verbose=False):
    """libmw_md.so: the molecular-dynamics kernels and their C ABI, a translation unit of its own like libmw_quench.so, whose
    force layer (mw_lib_forces.h) it shares."""
    return _compile(MD_LIB, [MD_SRC], MD_DEPS, HIPCC_FLAGS, force=force, verbose=verbose)


def build_npt(force=False, verbose=False):
    """libmw_npt.so: the constant-pressure molecular-dynamics kernels and their C ABI, a translation unit of its own like
    libmw_md.so, whose force layer (mw_lib_forces.h, with the virial) it shares."""
    return _compile(NPT_LIB, [NPT_SRC], NPT_DEPS, HIPCC_FLAGS, force=force, verbose=verbose)


def build_tcf(force=False, verbose=False):
    """libmw_tcf.so: the time-correlation kernels and their C ABI, a translation unit of its own over the libraries' host layer
    alone (it sorts nothing into cells)."""
    return _compile(TCF_LIB, [TCF_SRC], TCF_DEPS, HIPCC_FLAGS, force=force, verbose=verbose)


def build_hess(force=False, verbose=False):
    """libmw_hess.so: the Hessian kernels and their C ABI, a translation unit of its own like libmw_md.so, whose cell and force
    layers (mw_lib_cells.h, mw_lib_forces.h) it shares; the second derivatives are its own."""
    return _compile(HESS_LIB, [HESS_SRC], HESS_DEPS, HIPCC_FLAGS, force=force, verbose=verbose)


def build_ti(force=False, verbose=False):
    """libmw_ti.so: the Einstein-crystal thermodynamic-integration kernels and their C ABI, a translation unit of its own like
    libmw_md.so, whose step it restates and whose cell and force layers (mw_lib_cells.h, mw_lib_forces.h) it shares."""
    return _compile(TI_LIB, [TI_SRC], TI_DEPS, HIPCC_FLAGS, force=force, verbose=verbose)


def build_flex(force=False, verbose=False):
    """libmw_flex.so: the per-axis constant-pressure molecular-dynamics kernels and their C ABI, a translation unit of its own
    like libmw_npt.so, whose step it restates and whose cell and force layers (mw_lib_cells.h, mw_lib_forces.h, with the stress)
    it shares."""
    return _compile(FLEX_LIB, [FLEX_SRC], FLEX_DEPS, HIPCC_FLAGS, force=force, verbose=verbose)


def build_pin(force=False, verbose=False):
    """libmw_pin.so: the interface-pinning kernels and their C ABI, a translation unit of its own like libmw_flex.so, whose step
    it restates with the force of a harmonic bias on one collective density mode added."""
    return _compile(PIN_LIB, [PIN_SRC], PIN_DEPS, HIPCC_FLAGS, force=force, verbose=verbose)


def build_nuc(force=False, verbose=False):
    """libmw_nuc.so: nucleus-size molecular dynamics with on-device stopping rules and its C ABI, a translation unit of its own
    like libmw_pin.so: the step of libmw_flex.so restated, with the l = 6 bond order and the cluster pass beside it."""
    return _compile(NUC_LIB, [NUC_SRC], NUC_DEPS, HIPCC_FLAGS, force=force, verbose=verbose)


def build_coll(force=False, verbose=False):
    """libmw_coll.so: the collective time-correlation kernels and their C ABI, a translation unit of its own over the libraries'
    host layer alone, like libmw_tcf.so; the density modes restate libmw_sk.so's arithmetic, the pair pass mw_rdf's."""
    return _compile(COLL_LIB, [COLL_SRC], COLL_DEPS, HIPCC_FLAGS, force=force, verbose=verbose)


if __name__ == "__main__":
    force = "--force" in sys.argv
    for builder in (build, build_comms, build_sk, build_boo, build_tet, build_adf, build_rings, build_md, build_npt, build_tcf, build_hess, build_ti, build_flex, build_pin, build_nuc, build_coll, build_quench):
        print(builder(force=force, verbose=True))
