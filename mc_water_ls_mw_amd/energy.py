"""Host-side mirror of the reference's Fortran ``module energy`` (molint.F90:10-37)
over the C ABI of ``libmw_hip.so`` (include/mw_energy.h).

:class:`EnergyModule` keeps the reference's public names and argument meaning --
``energy_init``, ``energy_deinit``, ``compute_ivects(ils)``,
``compute_neighbours(ils)``, ``compute_model_energy(ils)`` (result in
``model_energy[ils-1]``), ``compute_local_real_energy(imol, ils)`` -- with 1-based
``ils`` / ``imol`` exactly as the Fortran callers pass them, and it holds the
implicit inputs the Fortran module reads from ``module model``
(``ljr``, ``hmatrix``, ``volume``; data_structures.f90:39-46) as host arrays the
caller mutates freely, like mc_moves.F90 does.  It is the same thin layer as
the ISO_C_BINDING module in ``fortran/energy_hip.F90`` and follows the same
host<->device coherence protocol (DESIGN.md "Coherence").

There is no CPU path: if ``libmw_hip.so`` is missing or no gfx950 device is
usable, construction / ``energy_init`` raises.
"""
from __future__ import annotations

import ctypes
import os
import sys

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "libmw_hip.so")
MAXNEIGH = 50  # molint.F90:79

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)
_llp = ctypes.POINTER(ctypes.c_longlong)
_fp = ctypes.POINTER(ctypes.c_float)

#: every symbol include/mw_energy.h declares (tests check the .so exports them all)
ABI_SYMBOLS = (
    "mw_init", "mw_finalize", "mw_is_initialised", "mw_last_error", "mw_constants",
    "mw_set_cell", "mw_get_ivects", "mw_upload_positions", "mw_download_positions", "mw_patch_position",
    "mw_upload_positions_range", "mw_download_positions_range", "mw_set_cells_range",
    "mw_build_neighbours", "mw_build_neighbours_batch", "mw_get_neighbours",
    "mw_model_energy", "mw_model_energy_of", "mw_model_energy_batch", "mw_model_energy_counts",
    "mw_model_energy_counts_total", "mw_neighbour_total",
    "mw_model_forces", "mw_model_forces_batch", "mw_model_forces_launch",
    "mw_ice_classes", "mw_ice_classes_batch", "mw_ice_classes_launch", "mw_ice_bonds",
    "mw_ice_clusters", "mw_ice_clusters_batch", "mw_ice_clusters_launch", "mw_ice_clusters_plan", "mw_ice_clusters_last",
    "mw_rdf", "mw_rdf_batch", "mw_rdf_launch",
    "mw_local_energy", "mw_local_energy_patched", "mw_local_energy_post", "mw_local_energy_collect",
    "mw_server_counts", "mw_local_energy_batch", "mw_delta_energy_batch",
    "mw_moves_upload", "mw_moves_launch", "mw_moves_fetch", "mw_moves_counts",
    "mw_model_energy_launch", "mw_step_launch", "mw_model_energy_fetch", "mw_build_neighbours_launch", "mw_sync",
    "mw_timer_start", "mw_timer_stop", "mw_timer_elapsed_ms", "mw_device_info",
    "mw_sweep_configure", "mw_set_model_energy", "mw_sweep_set_state", "mw_sweep_set_states_range", "mw_sweep_get_state",
    "mw_sweep_translation", "mw_sweep_translation_launch", "mw_sweep_lds_bytes", "mw_sweep_last_launch",
    "mw_sweep_options", "mw_sweep_get_tables", "mw_sweep_set_tables", "mw_sweep_get_switches", "mw_sweep_get_shifts_range",
    "mw_sweep_reduce_tables", "mw_sweep_broadcast_tables",
    "mw_sweep_get_tables_range", "mw_sweep_set_tables_range",
    "mw_sweep_moves", "mw_sweep_get_volume_moves", "mw_sweep_sync_cells", "mw_sweep_check_flags",
    "mw_sweep_leshift", "mw_sweep_minu", "mw_sweep_swetnam", "mw_sweep_dd", "mw_sweep_windows", "mw_sweep_set_factors", "mw_sweep_get_factors", "mw_sweep_steps", "mw_sweep_get_counters",
    "mw_last_dispatch", "mw_lds_plan",
)

#: the kernel families of mw_last_dispatch (MW_DISPATCH_*, by index) and the names of the fields it reports for each
#: ("moves": the last three fields follow the counts of that launch, not the launch alone -- ``moves_counts()`` updates them:
#: "counts" 0 there / 1 to be made on demand / 2 dropped, "count_passes" the on-demand passes since ``energy_init``, "declined"
#: the requests the launch left to the fallback kernel, -1 until ``moves_counts()`` has read the number back)
DISPATCH_FIELDS = {
    "build": ("ivcap", "boxes", "grid_boxes", "brute_boxes", "fused_sort", "legacy_search", "order_seg", "nseg", "lds_bytes"),
    "energy": ("ivcap", "boxes", "lds", "nsplit", "chunk", "grid_y", "moments", "lds_bytes", "block"),
    "moves": ("ivcap", "requests", "mlds", "noself", "use_mom", "fresh", "mchunk", "items", "lds_bytes", "build", "counts", "count_passes", "declined", "first_box"),
    "forces": ("ivcap", "boxes", "lds", "nsplit", "lds_bytes"),
    "ice": ("ivcap", "boxes", "lds", "nsplit", "lds_bytes"),
    "rdf": ("ivcap", "boxes", "small", "workgroups_per_box", "lds_bytes", "images"),
}
#: the LDS-staged builds of mw_lds_plan (MW_LDS_*, by index)
LDS_BUILDS = ("energy", "forces", "ice", "move", "sort", "order")


def lds_plan(nwater, image_capacity=32):
    """{build: (admitted, dynamic LDS bytes)} for every LDS-staged build at ``nwater`` molecules and ``image_capacity`` image
    vectors per box: the engine's own rules (mw_lds_plan), no device needed."""
    L = load_library()
    out = (ctypes.c_int * (2 * len(LDS_BUILDS)))()
    if L.mw_lds_plan(int(nwater), int(image_capacity), out, len(out)) != len(LDS_BUILDS):
        raise MwError(f"mw_lds_plan: no plan for {nwater} molecules, {image_capacity} image vectors")
    return {b: (bool(out[2 * k]), int(out[2 * k + 1])) for k, b in enumerate(LDS_BUILDS)}


class MwError(RuntimeError):
    """A C-ABI call returned nonzero; the text is mw_last_error()."""


_lib = None


def load_library(path=LIB_PATH):
    """dlopen libmw_hip.so.  Raises if it has not been built -- there is no fallback.
    (MW_HIP_LIB: another build of the same library, for A/B measurements inside one GPU session.)"""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("MW_HIP_LIB", path)
    if not os.path.exists(path):
        raise MwError(f"{path} not found: build it with `python -m mc_water_ls_mw_amd.build` "
                      "(the mW engine has no CPU fallback)")
    _share_hip_runtime_with_torch()
    L = ctypes.CDLL(path)
    L.mw_last_error.restype = ctypes.c_char_p
    _lib = L
    return L


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch-ROCm wheels carry their own
    libamdhip64.so (same SONAME as /opt/rocm's); if libmw_hip.so were loaded first it
    would bind the system copy, a later ``import torch`` would bring in a second
    runtime, and whichever initialises second sees no device.  So when torch is
    installed, its copy is loaded (globally) before ours, whatever the import order.
    A process without torch -- the Fortran host -- simply uses /opt/rocm's."""
    if "torch" in sys.modules:
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


def _d(a):
    return a.ctypes.data_as(_dp)


def _i(a):
    return a.ctypes.data_as(_ip)


def _u8(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


#: the classes of mw_ice_classes (CHILL+), by index
ICE_CLASS_NAMES = ("other", "cubic ice", "hexagonal ice", "interfacial ice", "clathrate", "interfacial clathrate")
#: the usual CHILL+ bond cutoff for mW, Angstrom
ICE_RC_ANG = 3.5


def _rc(rc_ang):
    return ctypes.c_double(float(rc_ang) / 0.5291772108)          # Angstrom -> bohr (constants.f90:42-43)


#: the classes whose clusters mw_ice_clusters follows by default: ice of either stacking and its interface ("cubic" and
#: "hexagonal" are short for the "cubic ice" and "hexagonal ice" of ICE_CLASS_NAMES)
ICE_CLUSTER_DEFAULT = ("cubic", "hexagonal", "interfacial ice")


def ice_cluster_mask(classes=ICE_CLUSTER_DEFAULT):
    """The class mask of mw_ice_clusters (bit k selects class k of ICE_CLASS_NAMES) from an int mask, one class name or a
    sequence of names; a name may drop a trailing " ice".  The engine refuses 0, bit 0 ("other") and bits above 5."""
    if isinstance(classes, (int, np.integer)):
        return int(classes)
    mask = 0
    for name in ((classes,) if isinstance(classes, str) else classes):
        hits = [k for k, full in enumerate(ICE_CLASS_NAMES) if name == full or name + " ice" == full]
        if not hits:
            raise MwError(f"ice class {name!r} is none of {ICE_CLASS_NAMES}")
        mask |= 1 << hits[0]
    return mask


def ice_clusters_plan(nwater):
    """{"lds", "threads", "lds_bytes", "lds_max_nwater"} of the cluster pass for a box of ``nwater`` molecules: the engine's
    own rule (mw_ice_clusters_plan), no device needed."""
    L = load_library()
    out = (ctypes.c_int * 4)()
    if L.mw_ice_clusters_plan(int(nwater), out) != 0:
        raise MwError(L.mw_last_error().decode())
    return {"lds": bool(out[0]), "threads": int(out[1]), "lds_bytes": int(out[2]), "lds_max_nwater": int(out[3])}


def cluster_sizes(label):
    """Cluster sizes, largest first, from the labels of one box (mw_ice_clusters: 0 = not selected).  Host arithmetic only."""
    label = np.asarray(label).ravel()
    return np.sort(np.unique(label[label > 0], return_counts=True)[1])[::-1].astype(np.int64)


def rdf_from_counts(hist, nwater, volume_bohr3, r_max_ang):
    """(r_ang [nbins], g [..., nbins], n [..., nbins]) from pair-distance histograms ``hist`` [..., nbins] (mw_rdf: ordered
    pairs, periodic images included) of boxes of ``nwater`` molecules and volume ``volume_bohr3`` (a scalar or one per
    leading index): g[b] = hist[b] / (N (N / V) 4 pi / 3 ((b+1)^3 - b^3) dr^3), the bin centres r[b] = (b + 1/2) dr, and
    n[b] = cumsum(hist)[b] / N, the neighbours within the bin's upper edge.  Host arithmetic only."""
    hist = np.asarray(hist)
    nbins = hist.shape[-1]
    dr_ang = float(r_max_ang) / nbins
    dr = dr_ang / 0.5291772108                                     # Angstrom -> bohr (constants.f90:42-43)
    b = np.arange(nbins, dtype=np.float64)
    shell = 4.0 * np.pi / 3.0 * ((b + 1.0) ** 3 - b ** 3) * dr ** 3
    n = float(nwater)
    vol = np.asarray(volume_bohr3, dtype=np.float64)[..., None]
    g = hist / (n * (n / vol) * shell)
    return (b + 0.5) * dr_ang, g, np.cumsum(hist, axis=-1) / n


class EnergyModule:
    """One process-wide engine context (like the Fortran module, it is a singleton)."""

    def __init__(self, nwater, num_lattices=1, maxneigh=MAXNEIGH, device=0):
        self.L = load_library()
        self.nwater = int(nwater)
        self.num_lattices = int(num_lattices)
        self.maxneigh = int(maxneigh)
        self.device = int(device)
        # module model (data_structures.f90): the host owns these and mutates them at will
        self.ljr = np.zeros((self.num_lattices, self.nwater, 3), dtype=np.float64)   # ljr(:,1,imol,ils)
        self.hmatrix = np.zeros((self.num_lattices, 3, 3), dtype=np.float64)          # [ils][k] = hmatrix(:,k,ils)
        self.volume = np.zeros(self.num_lattices, dtype=np.float64)
        # module energy public variables (molint.F90:33-37)
        self.model_energy = np.zeros(self.num_lattices, dtype=np.float64)
        self.nivect = np.zeros(self.num_lattices, dtype=np.int32)
        self._last_imol = [0] * self.num_lattices    # molecule queried last per lattice (coherence protocol)
        self._stale = [True] * self.num_lattices     # set by compute_ivects: bulk position change pending
        self._live = False
        self.warnings = []
        # the single call is latency-bound: everything that can be prepared once is
        self._local = self.L.mw_local_energy_patched
        self._e_out = [ctypes.c_double(0.0) for _ in range(self.num_lattices)]    # per lattice: distinct lattices may be
        self._e_ref = [ctypes.byref(v) for v in self._e_out]                      # queried from distinct host threads
        self._ljr_seen, self._ljr_addr = None, 0

    # -- plumbing ------------------------------------------------------------------
    def _chk(self, rc):
        if rc != 0:
            raise MwError(self.L.mw_last_error().decode())

    def _ils(self, ils):
        if not (1 <= ils <= self.num_lattices):
            raise MwError(f"lattice index {ils} outside 1..{self.num_lattices}")
        return ils - 1

    # -- energy_init / energy_deinit (molint.F90:91-171) ------------------------------
    def energy_init(self):
        """Allocate, set volume(ils) = |det h|, then ivects + neighbours + energy per lattice."""
        self.setup_boxes()                                                          # :125,134 + the mirrored positions
        # :147-148 for every lattice: all lists in one batch of launches, then all energies in one launch
        self.build_neighbours_batch(1, self.num_lattices)
        self.model_energy_batch(1, self.num_lattices)

    def setup_boxes(self):
        """mw_init + volume(ils) = |det h| + compute_ivects + the mirrored positions of EVERY box, in a handful of
        transfers whatever the number of boxes (farms hold thousands)."""
        self._chk(self.L.mw_init(self.device, self.nwater, self.num_lattices, self.maxneigh))
        self._live = True
        self.volume[:] = np.abs(np.linalg.det(self.hmatrix))                        # :125
        self.set_cells_range(1, self.num_lattices)                                  # :134
        self.upload_range(1, self.num_lattices)

    def set_cells_range(self, first_ils=1, count=None):
        """compute_ivects for ``count`` consecutive lattices in one call (one transfer per device array)."""
        count = self.num_lattices - first_ils + 1 if count is None else count
        self._ils(first_ils), self._ils(first_ils + count - 1)
        h = np.ascontiguousarray(self.hmatrix[first_ils - 1:first_ils - 1 + count], dtype=np.float64)
        n = np.zeros(count, dtype=np.int32)
        self._chk(self.L.mw_set_cells_range(first_ils, count, _d(h), _i(n)))
        self.nivect[first_ils - 1:first_ils - 1 + count] = n
        for b in range(first_ils - 1, first_ils - 1 + count):
            self._stale[b] = True

    def upload_range(self, first_ils=1, count=None):
        """Mirror ljr of ``count`` consecutive lattices in one transfer."""
        count = self.num_lattices - first_ils + 1 if count is None else count
        self._ils(first_ils), self._ils(first_ils + count - 1)
        x = np.ascontiguousarray(self.ljr[first_ils - 1:first_ils - 1 + count], dtype=np.float64)
        self._chk(self.L.mw_upload_positions_range(first_ils, count, _d(x)))
        for b in range(first_ils - 1, first_ils - 1 + count):
            self._last_imol[b] = 0
            self._stale[b] = False

    def energy_deinit(self):
        if self._live:
            self._chk(self.L.mw_finalize())
            self._live = False

    close = energy_deinit

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.energy_deinit()

    # -- compute_ivects (molint.F90:174-217) ------------------------------------------
    def compute_ivects(self, ils):
        b = self._ils(ils)
        h = np.ascontiguousarray(self.hmatrix[b], dtype=np.float64)
        n = ctypes.c_int(0)
        self._chk(self.L.mw_set_cell(ils, _d(h), ctypes.byref(n)))
        self.nivect[b] = n.value
        # a cell change comes with a bulk position change -- also when a volume move is REJECTED: the host
        # rescales every position back and calls nothing but compute_ivects (mc_moves.F90:1410-1514)
        self._stale[b] = True

    def ivect(self, ils):
        self._ils(ils)
        n = ctypes.c_int(0)
        self._chk(self.L.mw_get_ivects(ils, None, 0, ctypes.byref(n)))
        out = np.zeros((n.value, 3))
        self._chk(self.L.mw_get_ivects(ils, _d(out), n.value, ctypes.byref(n)))
        return out

    # -- compute_neighbours (molint.F90:501-559) --------------------------------------
    def _upload(self, ils):
        x = np.ascontiguousarray(self.ljr[ils - 1], dtype=np.float64)
        self._chk(self.L.mw_upload_positions(ils, _d(x)))
        self._last_imol[ils - 1] = 0
        self._stale[ils - 1] = False

    def compute_neighbours(self, ils):
        self._ils(ils)
        self.compute_ivects(ils)                                                    # :518
        self._upload(ils)
        mn, mx = ctypes.c_int(0), ctypes.c_int(0)
        self._chk(self.L.mw_build_neighbours(ils, ctypes.byref(mn), ctypes.byref(mx)))
        if mn.value < 16:                                                           # :552-554
            nn, _, _ = self.neighbours(ils)
            for imol in np.nonzero(nn < 16)[0]:
                msg = "WARNING: Molecule %5d has only %5d neighbours" % (imol + 1, nn[imol])
                self.warnings.append(msg)
                print(msg, file=sys.stderr)
        return mn.value, mx.value

    def neighbours(self, ils):
        """(nn, jn, vn) in the reference's layout and 1-based numbering."""
        self._ils(ils)
        nn = np.zeros(self.nwater, dtype=np.int32)
        jn = np.zeros((self.nwater, self.maxneigh), dtype=np.int32)
        vn = np.zeros((self.nwater, self.maxneigh), dtype=np.int32)
        self._chk(self.L.mw_get_neighbours(ils, _i(nn), _i(jn), _i(vn)))
        return nn, jn, vn

    # -- compute_model_energy (molint.F90:407-499) ------------------------------------
    def compute_model_energy(self, ils):
        """Full-box energy of lattice ils -> model_energy[ils-1].  All positions are
        re-mirrored first: callers reach this after bulk changes (volume move
        mc_moves.F90:1314-1357, chain sync :2331-2396, restart :842-852)."""
        b = self._ils(ils)
        self._upload(ils)
        e = ctypes.c_double(0.0)
        self._chk(self.L.mw_model_energy(ils, ctypes.byref(e)))
        self.model_energy[b] = e.value
        return e.value

    # -- gradient of compute_model_energy (no counterpart in the reference) -------------
    def compute_forces(self, ils):
        """(energy, forces [nwater, 3], virial [3, 3]) of lattice ils from the HOST's ljr, mirrored first as
        compute_model_energy does.  forces = -dE/dr (Hartree / bohr), virial W_ab = -dE/d(strain_ab) (Hartree): the
        instantaneous pressure is (N k_B T + tr W / 3) / volume.  model_energy is the caller's and is left alone."""
        self._ils(ils)
        self._upload(ils)
        e = ctypes.c_double(0.0)
        f = np.zeros((self.nwater, 3))
        w = np.zeros(9)
        self._chk(self.L.mw_model_forces(ils, ctypes.byref(e), _d(f), _d(w)))
        return e.value, f, w.reshape(3, 3).T.copy()          # w is column-major: w[a + 3 b] = W_ab

    def forces_batch(self, first_ils=1, count=None):
        """(energies [count], forces [count, nwater, 3], virials [count, 3, 3]) of ``count`` boxes from the positions and
        cells the DEVICE holds (after device sweeps those are the authoritative ones), in one launch of each pass."""
        count = self.num_lattices - first_ils + 1 if count is None else count
        self._ils(first_ils), self._ils(first_ils + count - 1)
        e = np.zeros(count)
        f = np.zeros((count, self.nwater, 3))
        w = np.zeros((count, 9))
        self._chk(self.L.mw_model_forces_batch(first_ils, count, _d(e), _d(f), _d(w)))
        return e, f, np.ascontiguousarray(w.reshape(count, 3, 3).transpose(0, 2, 1))

    def forces_launch(self, first_ils, count, timer_slot=-1):
        """The two passes of forces_batch, results left on the device; timer_slot >= 0: event timers timer_slot (moment
        pass) and timer_slot + 1 (force pass)."""
        self._chk(self.L.mw_model_forces_launch(first_ils, count, timer_slot))

    # -- ice structure classes, CHILL+ (no counterpart in the reference) ---------------
    def ice_classes(self, ils, rc_ang=ICE_RC_ANG):
        """(classes uint8 [nwater], counts [6]) of lattice ils from the HOST's ljr, mirrored first as compute_model_energy
        does, on the current list.  Class k is ICE_CLASS_NAMES[k]; ``rc_ang`` is the bond cutoff in Angstrom."""
        self._ils(ils)
        self._upload(ils)
        cls = np.zeros(self.nwater, dtype=np.uint8)
        counts = np.zeros(6, dtype=np.int32)
        self._chk(self.L.mw_ice_classes(ils, _rc(rc_ang), _u8(cls), _i(counts)))
        return cls, counts

    def ice_classes_batch(self, first_ils=1, count=None, rc_ang=ICE_RC_ANG):
        """(classes [count, nwater], counts [count, 6]) of ``count`` boxes from the positions and cells the DEVICE holds, in
        one launch of each pass."""
        count = self.num_lattices - first_ils + 1 if count is None else count
        self._ils(first_ils), self._ils(first_ils + count - 1)
        cls = np.zeros((count, self.nwater), dtype=np.uint8)
        counts = np.zeros((count, 6), dtype=np.int32)
        self._chk(self.L.mw_ice_classes_batch(first_ils, count, _rc(rc_ang), _u8(cls), _i(counts)))
        return cls, counts

    def ice_classes_launch(self, first_ils, count, rc_ang=ICE_RC_ANG, timer_slot=-1):
        """The two passes of ice_classes_batch, results left on the device; timer_slot >= 0: event timers timer_slot (pass 1,
        bond-order vectors) and timer_slot + 1 (pass 2, classes)."""
        self._chk(self.L.mw_ice_classes_launch(first_ils, count, _rc(rc_ang), timer_slot))

    def ice_bonds(self, ils, rc_ang=ICE_RC_ANG):
        """Bond value c of every list entry of lattice ils as [nwater, maxneigh], laid out like ``neighbours(ils)[1]``: 2.0
        where the entry is not a bond, NaN where it is degenerate.  The host's ljr is mirrored first, as in ice_classes."""
        self._ils(ils)
        self._upload(ils)
        c = np.zeros((self.nwater, self.maxneigh))
        self._chk(self.L.mw_ice_bonds(ils, _rc(rc_ang), _d(c)))
        return c

    # -- pair-distance histogram, g(r) and n(r) (no counterpart in the reference) --------
    # -- ice clusters: connected clusters of molecules of selected CHILL+ classes ---------
    def ice_clusters(self, ils, classes=ICE_CLUSTER_DEFAULT, rc_ang=ICE_RC_ANG):
        """(label int32 [nwater], summary int32 [4]) of lattice ils from the HOST's ljr, mirrored first as in ice_classes, on
        the current list.  label[i] is 0 for a molecule whose class is not in ``classes`` (names of ICE_CLASS_NAMES or an int
        mask), else the 1-based index of the smallest molecule of its cluster; summary = (selected molecules, clusters, size
        of the largest cluster, its label)."""
        self._ils(ils)
        self._upload(ils)
        label = np.zeros(self.nwater, dtype=np.int32)
        summary = np.zeros(4, dtype=np.int32)
        self._chk(self.L.mw_ice_clusters(ils, _rc(rc_ang), ice_cluster_mask(classes), _i(label), _i(summary)))
        return label, summary

    def ice_clusters_batch(self, first_ils=1, count=None, classes=ICE_CLUSTER_DEFAULT, rc_ang=ICE_RC_ANG):
        """(label [count, nwater], summary [count, 4]) of ``count`` boxes from the positions and cells the DEVICE holds, one
        launch per pass."""
        count = self.num_lattices - first_ils + 1 if count is None else count
        self._ils(first_ils), self._ils(first_ils + count - 1)
        label = np.zeros((count, self.nwater), dtype=np.int32)
        summary = np.zeros((count, 4), dtype=np.int32)
        self._chk(self.L.mw_ice_clusters_batch(first_ils, count, _rc(rc_ang), ice_cluster_mask(classes), _i(label), _i(summary)))
        return label, summary

    def ice_clusters_launch(self, first_ils, count, classes=ICE_CLUSTER_DEFAULT, rc_ang=ICE_RC_ANG, timer_slot=-1):
        """The passes of ice_clusters_batch, results left on the device; timer_slot >= 0: event timers timer_slot and
        timer_slot + 1 (the classification passes) and timer_slot + 2 (the cluster pass)."""
        self._chk(self.L.mw_ice_clusters_launch(first_ils, count, _rc(rc_ang), ice_cluster_mask(classes), timer_slot))

    def ice_clusters_last(self):
        """{"boxes", "lds", "threads", "rounds"} of the last cluster launch (rounds: the most hook / compress rounds any of its
        boxes took)."""
        out = (ctypes.c_int * 4)()
        self._chk(self.L.mw_ice_clusters_last(out))
        return {"boxes": int(out[0]), "lds": bool(out[1]), "threads": int(out[2]), "rounds": int(out[3])}

    def rdf_counts(self, ils, r_max_ang, nbins):
        """int64 [nbins]: the pair-distance histogram of lattice ils (mw_rdf: ordered pairs with all periodic images inside
        ``r_max_ang``, Angstrom) from the positions and the cell the DEVICE holds."""
        self._ils(ils)
        hist = np.zeros(max(int(nbins), 0), dtype=np.int64)
        self._chk(self.L.mw_rdf(ils, _rc(r_max_ang), int(nbins), hist.ctypes.data_as(_llp)))
        return hist

    def rdf_counts_batch(self, first_ils=1, count=None, r_max_ang=10.0, nbins=200):
        """int64 [count, nbins]: the pair-distance histograms of ``count`` boxes in one launch."""
        count = self.num_lattices - first_ils + 1 if count is None else count
        self._ils(first_ils), self._ils(first_ils + count - 1)
        hist = np.zeros((count, max(int(nbins), 0)), dtype=np.int64)
        self._chk(self.L.mw_rdf_batch(first_ils, count, _rc(r_max_ang), int(nbins), hist.ctypes.data_as(_llp)))
        return hist

    def rdf_launch(self, first_ils, count, r_max_ang, nbins, timer_slot=-1):
        """The launch of rdf_counts_batch, results left on the device; timer_slot >= 0: an event timer around it."""
        self._chk(self.L.mw_rdf_launch(first_ils, count, _rc(r_max_ang), int(nbins), timer_slot))

    def rdf(self, ils, r_max_ang=10.0, nbins=200):
        """(r_ang, g, n) of lattice ils: rdf_from_counts of rdf_counts with this module's volume[ils - 1]."""
        return rdf_from_counts(self.rdf_counts(ils, r_max_ang, nbins), self.nwater, self.volume[ils - 1], r_max_ang)

    # -- static structure factor S(k) (libmw_sk.so, include/mw_sk.h; no counterpart in the reference) ------------
    def structure_factor(self, first_ils=1, count=None, nvec=None, want_rho=False):
        """S [count, M] (with ``want_rho`` also rho, complex [count, M]) of ``count`` boxes for the integer triples ``nvec``
        [M, 3] (structure.kvectors), from the positions the DEVICE holds and this module's hmatrix (after device volume
        moves call ``WalkerFarm.sync_cells`` first).  The positions take one host hop (mw_download_positions_range, 24 bytes
        per molecule) on their way to libmw_sk.so, which shares nothing with the engine but the device."""
        from . import structure
        if nvec is None:
            raise MwError("structure_factor: nvec is required (structure.kvectors makes the triples of a cell)")
        count = self.num_lattices - first_ils + 1 if count is None else count
        self._ils(first_ils), self._ils(first_ils + count - 1)
        pos = np.zeros((count, self.nwater, 3))
        self._chk(self.L.mw_download_positions_range(first_ils, count, _d(pos)))
        return structure.structure_factor(self.hmatrix[first_ils - 1:first_ils - 1 + count], pos, nvec, want_rho=want_rho)

    # -- Steinhardt bond order (libmw_boo.so, include/mw_boo.h; no counterpart in the reference) -------------------
    def bond_order(self, first_ils=1, count=None, rc_ang=3.5, threshold=0.5):
        """(q [count, nwater, 4], nn [count, nwater, 2], summary [count, 4]) of ``count`` boxes -- bondorder.bond_order -- from
        the positions the DEVICE holds and this module's hmatrix (after device volume moves call ``WalkerFarm.sync_cells``
        first).  The positions take one host hop (mw_download_positions_range) on their way to libmw_boo.so, which shares
        nothing with the engine but the device."""
        from . import bondorder
        count = self.num_lattices - first_ils + 1 if count is None else count
        self._ils(first_ils), self._ils(first_ils + count - 1)
        pos = np.zeros((count, self.nwater, 3))
        self._chk(self.L.mw_download_positions_range(first_ils, count, _d(pos)))
        return bondorder.bond_order(self.hmatrix[first_ils - 1:first_ils - 1 + count], pos, rc_ang, threshold)

    # -- tetrahedral order, d5 and LSI (libmw_tet.so, include/mw_tet.h; no counterpart in the reference) ------------
    def tetrahedral_order(self, first_ils=1, count=None, r_search_ang=5.5, r_lsi_ang=3.7):
        """(order [count, nwater, 4], near [count, nwater, 4], counts [count, nwater, 2], summary [count, 8]) of ``count``
        boxes -- tetrahedral.tetrahedral_order -- from the positions the DEVICE holds and this module's hmatrix (after device
        volume moves call ``WalkerFarm.sync_cells`` first).  The positions take one host hop (mw_download_positions_range)
        on their way to libmw_tet.so, which shares nothing with the engine but the device."""
        from . import tetrahedral
        count = self.num_lattices - first_ils + 1 if count is None else count
        self._ils(first_ils), self._ils(first_ils + count - 1)
        pos = np.zeros((count, self.nwater, 3))
        self._chk(self.L.mw_download_positions_range(first_ils, count, _d(pos)))
        return tetrahedral.tetrahedral_order(self.hmatrix[first_ils - 1:first_ils - 1 + count], pos, r_search_ang, r_lsi_ang)

    # -- O-O-O angle distribution (libmw_adf.so, include/mw_adf.h; no counterpart in the reference) -----------------
    def angle_counts(self, first_ils=1, count=None, r_cut_ang=3.5, edges=None, group=None, ngroups=1):
        """(hist [count, ngroups, nbins], counts [count, nwater], summary [count, ngroups, 4]) of ``count`` boxes --
        angles.angle_counts, ``group`` [count, nwater] or None -- from the positions the DEVICE holds and this module's hmatrix
        (after device volume moves call ``WalkerFarm.sync_cells`` first).  The positions take one host hop
        (mw_download_positions_range) on their way to libmw_adf.so, which shares nothing with the engine but the device."""
        from . import angles
        count = self.num_lattices - first_ils + 1 if count is None else count
        self._ils(first_ils), self._ils(first_ils + count - 1)
        pos = np.zeros((count, self.nwater, 3))
        self._chk(self.L.mw_download_positions_range(first_ils, count, _d(pos)))
        return angles.angle_counts(self.hmatrix[first_ils - 1:first_ils - 1 + count], pos, r_cut_ang, edges, group, ngroups)

    # -- primitive ring statistics (libmw_rings.so, include/mw_rings.h; no counterpart in the reference) ------------
    def ring_statistics(self, first_ils=1, count=None, r_cut_ang=3.5, list_cap=0):
        """(hist [count, 5], closed [count, 5], member [count, nwater, 5], counts [count, nwater], summary [count, 4], list
        [count, list_cap, 8]) of ``count`` boxes -- rings.ring_statistics -- from the positions the DEVICE holds and this
        module's hmatrix (after device volume moves call ``WalkerFarm.sync_cells`` first).  The positions take one host hop
        (mw_download_positions_range) on their way to libmw_rings.so, which shares nothing with the engine but the device."""
        from . import rings
        count = self.num_lattices - first_ils + 1 if count is None else count
        self._ils(first_ils), self._ils(first_ils + count - 1)
        pos = np.zeros((count, self.nwater, 3))
        self._chk(self.L.mw_download_positions_range(first_ils, count, _d(pos)))
        return rings.ring_statistics(self.hmatrix[first_ils - 1:first_ils - 1 + count], pos, r_cut_ang, list_cap)

    # -- inherent structures (libmw_quench.so, include/mw_quench.h; no counterpart in the reference) -----------------
    def inherent_structures(self, first_ils=1, count=None, ftol=1e-8, max_iter=10000, fire=None):
        """(pos_out [count, nwater, 3], forces [count, nwater, 3], stats [count, 6], iters [count, 2]) of ``count`` boxes --
        quench.inherent_structures -- from the positions the DEVICE holds and this module's hmatrix (after device volume
        moves call ``WalkerFarm.sync_cells`` first).  The positions take one host hop (mw_download_positions_range) on their
        way to libmw_quench.so, which shares nothing with the engine but the device; the engine's own positions stay as
        they are."""
        from . import quench
        count = self.num_lattices - first_ils + 1 if count is None else count
        self._ils(first_ils), self._ils(first_ils + count - 1)
        pos = np.zeros((count, self.nwater, 3))
        self._chk(self.L.mw_download_positions_range(first_ils, count, _d(pos)))
        return quench.inherent_structures(self.hmatrix[first_ils - 1:first_ils - 1 + count], pos, ftol, max_iter, fire)

    # -- the Hessian and normal modes (libmw_hess.so, include/mw_hess.h; no counterpart in the reference) --------------
    def hessian(self, ils):
        """(H [3 nwater, 3 nwater], ef [2]) of box ``ils`` (from 1) -- phonons.hessian: the Gamma-point Hessian in Hartree /
        bohr^2 and beside it the energy and the largest |F| component -- from the positions the DEVICE holds and this
        module's hmatrix (after device volume moves call ``WalkerFarm.sync_cells`` first).  The positions take one host hop
        (mw_download_positions_range) on their way to libmw_hess.so, which shares nothing with the engine but the device."""
        from . import phonons
        self._ils(ils)
        pos = np.zeros((1, self.nwater, 3))
        self._chk(self.L.mw_download_positions_range(ils, 1, _d(pos)))
        return phonons.hessian(self.hmatrix[ils - 1], pos[0])

    def normal_modes(self, ils, mass=None, vectors=False):
        """phonons.normal_modes of :meth:`hessian` of box ``ils``: the signed frequencies in ascending order (negative: an
        unstable direction -- the instantaneous normal modes of a configuration that is not a minimum), with ``vectors`` the
        eigenvectors too.  ``mass`` defaults to phonons.MASS_WATER."""
        from . import phonons
        H, _ = self.hessian(ils)
        return phonons.normal_modes(H, phonons.MASS_WATER if mass is None else mass, vectors)

    # -- molecular dynamics (libmw_md.so, include/mw_md.h; no counterpart in the reference) --------------------------
    def molecular_dynamics(self, first_ils=1, count=None, nsteps=0, dt=1.0, **kwargs):
        """(pos_out, vel_out, forces [count, nwater, 3], trace [count, nsteps // sample_every + 1, 4], status [count, 2]) of
        ``count`` boxes -- dynamics.molecular_dynamics, which takes the keywords (kT, gamma, vel, mass, seed, streams, step0,
        sample_every, pos_ref) -- from the positions the DEVICE holds and this module's hmatrix (after device volume moves
        call ``WalkerFarm.sync_cells`` first).  The positions take one host hop (mw_download_positions_range) on their way to
        libmw_md.so, which shares nothing with the engine but the device; the engine's own positions stay as they are."""
        from . import dynamics
        count = self.num_lattices - first_ils + 1 if count is None else count
        self._ils(first_ils), self._ils(first_ils + count - 1)
        pos = np.zeros((count, self.nwater, 3))
        self._chk(self.L.mw_download_positions_range(first_ils, count, _d(pos)))
        return dynamics.molecular_dynamics(self.hmatrix[first_ils - 1:first_ils - 1 + count], pos, nsteps, dt, **kwargs)

    # -- molecular dynamics at constant pressure (libmw_npt.so, include/mw_npt.h) ---------------------------------------
    def molecular_dynamics_npt(self, first_ils=1, count=None, nsteps=0, dt=1.0, **kwargs):
        """(pos_out, vel_out, forces, cells_out [count, 3, 3], ref_out, trace [count, nsteps // sample_every + 1, 6], status
        [count, 2]) of ``count`` boxes -- npt.molecular_dynamics_npt, which takes the keywords (pressure, kT, gamma, tau_p,
        beta_T, baro_every, vel, mass, seed, streams, step0, sample_every, pos_ref) -- from the positions the DEVICE holds and
        this module's hmatrix, as :meth:`molecular_dynamics` takes them; the engine's own positions and cells stay as they
        are."""
        from . import npt
        count = self.num_lattices - first_ils + 1 if count is None else count
        self._ils(first_ils), self._ils(first_ils + count - 1)
        pos = np.zeros((count, self.nwater, 3))
        self._chk(self.L.mw_download_positions_range(first_ils, count, _d(pos)))
        return npt.molecular_dynamics_npt(self.hmatrix[first_ils - 1:first_ils - 1 + count], pos, nsteps, dt, **kwargs)

    def molecular_dynamics_flex(self, first_ils=1, count=None, nsteps=0, dt=1.0, **kwargs):
        """The seven results of :meth:`molecular_dynamics_npt` with a per-axis cell and a trace of 15 columns --
        flexcell.molecular_dynamics_flex, which takes the keywords of the NPT call and ``coupling`` and ``axis`` -- from the
        positions the DEVICE holds and this module's hmatrix; the engine's own positions and cells stay as they are."""
        from . import flexcell
        count = self.num_lattices - first_ils + 1 if count is None else count
        self._ils(first_ils), self._ils(first_ils + count - 1)
        pos = np.zeros((count, self.nwater, 3))
        self._chk(self.L.mw_download_positions_range(first_ils, count, _d(pos)))
        return flexcell.molecular_dynamics_flex(self.hmatrix[first_ils - 1:first_ils - 1 + count], pos, nsteps, dt, **kwargs)

    # -- interface pinning (libmw_pin.so, include/mw_pin.h; no counterpart in the reference) ------------------------------
    def interface_pinning(self, nvec, kappa, anchor, first_ils=1, count=None, nsteps=0, dt=1.0, **kwargs):
        """The eight results of pinning.interface_pinning -- the seven of :meth:`molecular_dynamics_flex` with a trace of 17
        columns, and the block averages before the status -- under the bias 1/2 ``kappa`` (Q - ``anchor``)^2 on the mode ``nvec``
        of every box, from the positions the DEVICE holds and this module's hmatrix; the other keywords are those of
        pinning.interface_pinning.  The engine's own positions and cells stay as they are."""
        from . import pinning
        count = self.num_lattices - first_ils + 1 if count is None else count
        self._ils(first_ils), self._ils(first_ils + count - 1)
        pos = np.zeros((count, self.nwater, 3))
        self._chk(self.L.mw_download_positions_range(first_ils, count, _d(pos)))
        return pinning.interface_pinning(self.hmatrix[first_ils - 1:first_ils - 1 + count], pos, nvec, kappa, anchor, nsteps, dt, **kwargs)

    # -- nucleus-size MD with on-device stopping rules (libmw_nuc.so, include/mw_nuc.h; no counterpart in the reference) --
    def nucleus_md(self, first_ils=1, count=None, nsteps=0, dt=1.0, **kwargs):
        """The eleven results of nucleation.nucleus_md -- the seven of :meth:`molecular_dynamics_flex` with a trace of 18
        columns and the status codes 3 and 4 of the stopping rule, then nn, label and op -- from the positions the DEVICE holds
        and this module's hmatrix; the keywords are those of nucleation.nucleus_md.  The engine's own positions and cells stay
        as they are."""
        from . import nucleation
        count = self.num_lattices - first_ils + 1 if count is None else count
        self._ils(first_ils), self._ils(first_ils + count - 1)
        pos = np.zeros((count, self.nwater, 3))
        self._chk(self.L.mw_download_positions_range(first_ils, count, _d(pos)))
        return nucleation.nucleus_md(self.hmatrix[first_ils - 1:first_ils - 1 + count], pos, nsteps, dt, **kwargs)

    # -- Einstein-crystal thermodynamic integration (libmw_ti.so, include/mw_ti.h; no counterpart in the reference) ------
    def einstein_md(self, ils, lambdas, springs, nsteps, dt, sites=None, **kwargs):
        """(pos_out, vel_out, forces [nl, nwater, 3], trace [nl, nsteps // sample_every + 1, 5], blocks [nl, nblocks, 5], status
        [nl, 2]) -- einstein.einstein_md, which takes the keywords (kT, gamma, pos, vel, mass, seed, streams, step0,
        sample_every, equil_steps, block_steps) -- of nl = len(``lambdas``) copies of box ``ils`` (from 1), one per lambda of
        a thermodynamic integration, with the Einstein sites ``sites`` [nwater, 3] (None: the positions the DEVICE holds, which
        take one host hop; for a free energy pass the box's inherent structure) and this module's hmatrix.  The engine's own
        positions stay as they are."""
        from . import einstein
        self._ils(ils)
        lambdas = np.atleast_1d(np.asarray(lambdas, dtype=np.float64))
        if sites is None:
            sites = np.zeros((1, self.nwater, 3))
            self._chk(self.L.mw_download_positions_range(ils, 1, _d(sites)))
        sites = np.asarray(sites, dtype=np.float64).reshape(1, self.nwater, 3)
        nl = lambdas.size
        cells = np.repeat(np.asarray(self.hmatrix[ils - 1:ils], dtype=np.float64), nl, axis=0)
        return einstein.einstein_md(cells, np.repeat(sites, nl, axis=0), lambdas, springs, nsteps, dt, **kwargs)

    # -- time correlation functions (libmw_md.so records, libmw_tcf.so correlates; include/mw_tcf.h) ---------------------
    def time_correlations(self, first_ils=1, count=None, nframes=2, steps_per_frame=1, dt=1.0, nlags=None, origin_every=1, q=None, edges=None,
                          hist_lags=(), remove_com=False, with_vacf=True, **md_keywords):
        """((msd, mqd, vacf, fs, hist), status [count, 2]) of ``count`` boxes: a recorded molecular-dynamics run of ``nframes``
        frames, ``steps_per_frame`` steps of ``dt`` apart (dynamics.trajectory with the keywords kT, gamma, vel, mass, seed,
        streams, step0), from the positions the DEVICE holds and this module's hmatrix, and its time correlation functions
        (timecorr.time_correlations_torch: per box and lag, host arrays; ``with_vacf=False`` leaves the velocities out).  The
        positions take one host hop (mw_download_positions_range), as :meth:`molecular_dynamics` takes them; the engine's own
        positions stay as they are."""
        import torch
        from . import dynamics, timecorr
        count = self.num_lattices - first_ils + 1 if count is None else count
        self._ils(first_ils), self._ils(first_ils + count - 1)
        pos = np.zeros((count, self.nwater, 3))
        self._chk(self.L.mw_download_positions_range(first_ils, count, _d(pos)))
        dev = torch.device("cuda", dynamics._dev.device or 0)
        up = lambda a, dtype=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev).contiguous()   # noqa: E731
        kw = dict(md_keywords)
        if kw.get("vel") is not None:
            kw["vel_t"] = up(np.asarray(kw["vel"], dtype=np.float64).reshape(count, self.nwater, 3))
        kw.pop("vel", None)
        if kw.get("streams") is not None:
            kw["streams_t"] = up(np.ascontiguousarray(kw["streams"], dtype=np.uint64).view(np.int64), torch.int64)
        kw.pop("streams", None)
        cells_t = up(self.hmatrix[first_ils - 1:first_ils - 1 + count])
        frames, vel_frames, _, status = dynamics.trajectory(cells_t, up(pos), nframes, steps_per_frame, dt, **kw)
        out = timecorr.time_correlations_torch(frames, vel_frames if with_vacf else None, nlags, origin_every, q, edges, hist_lags, remove_com)
        return tuple(None if t is None else t.cpu().numpy() for t in out), status.cpu().numpy()

    # -- collective time correlations (libmw_md.so records, libmw_coll.so correlates; include/mw_coll.h) -----------------
    def collective_correlations(self, first_ils=1, count=None, nframes=2, steps_per_frame=1, dt=1.0, nlags=None, origin_every=1, nvec=None,
                                r_max=0.0, nbins=0, hist_lags=(), overlap_a=0.0, outputs=("fkt", "gd", "qsum", "q2sum"), **md_keywords):
        """((rho, fkt, gd, qsum, q2sum), status [count, 2]) of ``count`` boxes: a recorded molecular-dynamics run of ``nframes``
        frames, ``steps_per_frame`` steps of ``dt`` apart (dynamics.trajectory with the keywords kT, gamma, vel, mass, seed,
        streams, step0), from the positions the DEVICE holds and this module's hmatrix, and its collective time correlations
        (collective.collective_correlations_torch: host arrays; rho, the modes of every frame, only if ``outputs`` names it).
        The positions take one host hop, as :meth:`time_correlations` takes them; the engine's own positions stay as they are."""
        import torch
        from . import collective, dynamics
        count = self.num_lattices - first_ils + 1 if count is None else count
        self._ils(first_ils), self._ils(first_ils + count - 1)
        pos = np.zeros((count, self.nwater, 3))
        self._chk(self.L.mw_download_positions_range(first_ils, count, _d(pos)))
        dev = torch.device("cuda", dynamics._dev.device or 0)
        up = lambda a, dtype=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev).contiguous()   # noqa: E731
        kw = dict(md_keywords)
        if kw.get("vel") is not None:
            kw["vel_t"] = up(np.asarray(kw["vel"], dtype=np.float64).reshape(count, self.nwater, 3))
        kw.pop("vel", None)
        if kw.get("streams") is not None:
            kw["streams_t"] = up(np.ascontiguousarray(kw["streams"], dtype=np.uint64).view(np.int64), torch.int64)
        kw.pop("streams", None)
        cells = np.ascontiguousarray(self.hmatrix[first_ils - 1:first_ils - 1 + count], dtype=np.float64)
        frames, _, _, status = dynamics.trajectory(up(cells), up(pos), nframes, steps_per_frame, dt, **kw)
        out = collective.collective_correlations_torch(cells, frames, nlags, origin_every, nvec, r_max, nbins, hist_lags, overlap_a, outputs)
        return tuple(None if t is None else t.cpu().numpy() for t in out), status.cpu().numpy()

    def model_energy_counts(self, ils):
        p, t = ctypes.c_longlong(0), ctypes.c_longlong(0)
        self._chk(self.L.mw_model_energy_counts(ils, ctypes.byref(p), ctypes.byref(t)))
        return p.value, t.value

    def model_energy_counts_total(self, first_ils=1, count=None):
        count = self.num_lattices - first_ils + 1 if count is None else count
        p, t = ctypes.c_longlong(0), ctypes.c_longlong(0)
        self._chk(self.L.mw_model_energy_counts_total(first_ils, count, ctypes.byref(p), ctypes.byref(t)))
        return p.value, t.value

    def neighbour_total(self, first_ils=1, count=None):
        count = self.num_lattices - first_ils + 1 if count is None else count
        t = ctypes.c_longlong(0)
        self._chk(self.L.mw_neighbour_total(first_ils, count, ctypes.byref(t)))
        return t.value

    # -- compute_local_real_energy (molint.F90:220-404) -------------------------------
    def compute_local_real_energy(self, imol, ils):
        """Local energy of molecule imol in lattice ils from the HOST's current ljr.

        The caller moves molecules without telling us (trial move
        mc_moves.F90:1079, silent revert :1186), so the host position of imol and
        of the molecule queried just before it travel with the call."""
        b = self._ils(ils)
        if not (1 <= imol <= self.nwater):
            raise MwError(f"molecule index {imol} outside 1..{self.nwater}")
        if self._stale[b]:
            self._upload(ils)
        prev = self._last_imol[b]
        e, eref = self._e_out[b], self._e_ref[b]
        lj = self.ljr
        if lj is not self._ljr_seen:           # (re)bound by the caller: its address, once, if it is laid out as we pass it
            ok = lj.dtype == np.float64 and lj.flags.c_contiguous and lj.shape == (self.num_lattices, self.nwater, 3)
            self._ljr_seen, self._ljr_addr = lj, (lj.ctypes.data if ok else 0)
        base = self._ljr_addr
        if base:                                # the two positions straight out of the caller's array (24 bytes per molecule)
            row = base + 24 * (b * self.nwater - 1)
            if prev >= 1 and prev != imol:
                rc = self._local(ils, imol, ctypes.c_void_p(row + 24 * imol), prev, ctypes.c_void_p(row + 24 * prev), eref)
            else:
                rc = self._local(ils, imol, ctypes.c_void_p(row + 24 * imol), 0, None, eref)
            if rc:
                self._chk(rc)
        else:
            r = np.ascontiguousarray(lj[b, imol - 1], dtype=np.float64)
            if prev >= 1 and prev != imol:
                rp = np.ascontiguousarray(lj[b, prev - 1], dtype=np.float64)
                self._chk(self._local(ils, imol, _d(r), prev, _d(rp), eref))
            else:
                self._chk(self._local(ils, imol, _d(r), 0, None, eref))
        self._last_imol[b] = imol
        return e.value

    def server_counts(self, ils):
        """Which routine of the resident server answered the single calls of lattice ils since ``energy_init``:
        {"moments", "scan", "plain", "updates", "starts"} (mw_server_counts; it stops the server, like every exclusive entry)."""
        self._ils(ils)
        out = (ctypes.c_longlong * 5)()
        self._chk(self.L.mw_server_counts(ils, out))
        return dict(zip(("moments", "scan", "plain", "updates", "starts"), (int(v) for v in out)))

    # -- batched single-move path -----------------------------------------------------
    def local_energy_batch(self, ils, imol, trial_xyz=None):
        """Local energies of many (ils[m], imol[m]) from the MIRRORED positions
        (call ``sync_positions`` first if the host changed ljr); with ``trial_xyz``
        molecule m is evaluated at that position instead."""
        ils = np.ascontiguousarray(np.broadcast_to(ils, np.shape(imol)), dtype=np.int32)
        imol = np.ascontiguousarray(imol, dtype=np.int32)
        out = np.zeros(len(imol))
        t = None if trial_xyz is None else np.ascontiguousarray(trial_xyz, dtype=np.float64)
        self._chk(self.L.mw_local_energy_batch(len(imol), _i(ils), _i(imol), None if t is None else _d(t), _d(out)))
        return out

    def delta_energy_batch(self, ils, imol, trial_xyz):
        """(e_old, e_new) per trial move: the two compute_local_real_energy calls of
        mc_water_translation (mc_moves.F90:1010,1083) for many moves in one launch."""
        ils = np.ascontiguousarray(np.broadcast_to(ils, np.shape(imol)), dtype=np.int32)
        imol = np.ascontiguousarray(imol, dtype=np.int32)
        t = np.ascontiguousarray(trial_xyz, dtype=np.float64)
        eo, en = np.zeros(len(imol)), np.zeros(len(imol))
        self._chk(self.L.mw_delta_energy_batch(len(imol), _i(ils), _i(imol), _d(t), _d(eo), _d(en)))
        return eo, en

    def sync_positions(self, ils=None):
        for b in ([ils] if ils else range(1, self.num_lattices + 1)):
            self._upload(b)

    def model_energy_batch(self, first_ils=1, count=None):
        """Full-box energies of ``count`` boxes in one launch (mirrored positions)."""
        count = self.num_lattices - first_ils + 1 if count is None else count
        out = np.zeros(count)
        self._chk(self.L.mw_model_energy_batch(first_ils, count, _d(out)))
        self.model_energy[first_ils - 1:first_ils - 1 + count] = out
        return out

    def build_neighbours_batch(self, first_ils=1, count=None):
        count = self.num_lattices - first_ils + 1 if count is None else count
        mn, mx = ctypes.c_int(0), ctypes.c_int(0)
        self._chk(self.L.mw_build_neighbours_batch(first_ils, count, ctypes.byref(mn), ctypes.byref(mx)))
        return mn.value, mx.value

    # -- device-resident pipeline used by bench.py ------------------------------------
    def moves_upload(self, ils, imol, trial_xyz):
        ils = np.ascontiguousarray(np.broadcast_to(ils, np.shape(imol)), dtype=np.int32)
        imol = np.ascontiguousarray(imol, dtype=np.int32)
        t = np.ascontiguousarray(trial_xyz, dtype=np.float64)
        self._chk(self.L.mw_moves_upload(len(imol), _i(ils), _i(imol), _d(t)))
        self._nmoves = len(imol)

    def moves_launch(self):
        self._chk(self.L.mw_moves_launch())

    def moves_fetch(self):
        eo, en = np.zeros(self._nmoves), np.zeros(self._nmoves)
        self._chk(self.L.mw_moves_fetch(_d(eo), _d(en)))
        return eo, en

    def moves_counts(self):
        """(interactions_old, slots_old, interactions_new, slots_new) summed over the staged moves of the last launch.

        They come from the move kernels themselves, counted ON DEMAND: a launch on the moment path computes energies only, and
        the first call here runs the same kernel once more over the same requests to count (a second call launches nothing).
        Ask between the launch and the next call that replaces the requests (``moves_upload``, ``local_energy_batch``,
        ``delta_energy_batch``) or that may move a molecule, change a cell or rebuild a list; after one of those, counts that
        were never made raise ``MwError``.  ``MW_MOVE_COUNTS=eager`` (at ``energy_init``) makes the launch count, as it used to."""
        out = (ctypes.c_longlong * 4)()
        self._chk(self.L.mw_moves_counts(out))
        return tuple(int(v) for v in out)

    def model_energy_launch(self, first_ils, count):
        self._chk(self.L.mw_model_energy_launch(first_ils, count))

    def step_launch(self, first_ils, count, timer_slot=-1):
        """model_energy_launch + moves_launch in one host call; timer_slot >= 0: event timers timer_slot (full-box
        kernel) and timer_slot + 1 (move kernels)."""
        self._chk(self.L.mw_step_launch(first_ils, count, timer_slot))

    def model_energy_fetch(self, first_ils, count):
        out = np.zeros(count)
        self._chk(self.L.mw_model_energy_fetch(first_ils, count, _d(out)))
        return out

    def build_neighbours_launch(self, first_ils, count):
        self._chk(self.L.mw_build_neighbours_launch(first_ils, count))

    def sync(self):
        self._chk(self.L.mw_sync())

    def timer_start(self, slot=0):
        self._chk(self.L.mw_timer_start(slot))

    def timer_stop(self, slot=0):
        self._chk(self.L.mw_timer_stop(slot))

    def timer_ms(self, slot=0):
        ms = ctypes.c_float(0.0)
        self._chk(self.L.mw_timer_elapsed_ms(slot, ctypes.byref(ms)))
        return ms.value

    def device_info(self):
        name = ctypes.create_string_buffer(256)
        cu, mem = ctypes.c_int(0), ctypes.c_longlong(0)
        self._chk(self.L.mw_device_info(name, 256, ctypes.byref(cu), ctypes.byref(mem)))
        return name.value.decode(), cu.value, mem.value

    def constants(self):
        out = np.zeros(8)
        self._chk(self.L.mw_constants(_d(out)))
        return out

    def last_dispatch(self, family):
        """What the last launch of ``family`` (a key of DISPATCH_FIELDS) did: {field: int} -- which build, its geometry and
        LDS (include/mw_energy.h, mw_last_dispatch)."""
        names = DISPATCH_FIELDS[family]
        out = (ctypes.c_int * len(names))()
        self._chk(self.L.mw_last_dispatch(list(DISPATCH_FIELDS).index(family), out, len(names)))
        return dict(zip(names, (int(v) for v in out)))


def load_boxes(h_list, xyz_list, maxneigh=MAXNEIGH, device=0):
    """Convenience: an initialised EnergyModule holding the given boxes (bohr)."""
    em = EnergyModule(len(xyz_list[0]), len(xyz_list), maxneigh=maxneigh, device=device)
    for b, (h, x) in enumerate(zip(h_list, xyz_list)):
        em.hmatrix[b] = h
        em.ljr[b] = x
    em.energy_init()
    return em
