"""GPU: the interface-pinning molecular dynamics of libmw_pin.so (pinning.interface_pinning / _torch, EnergyModule.interface_pinning,
WalkerFarm.interface_pinning) against libmw_flex.so (bytes, kappa = 0), against the numpy mirror of tests/pin_ref.py, against
libmw_sk.so's structure factor, and the bit rules of include/mw_pin.h.

Bars.  Every one is pin_ref's: ten times the spread the mirror shows against itself with its forces perturbed by +-F_ATOL, measured
on the CPU (tests/test_pin_ref.py measures them again, and shows that the mirror without the bias lies a hundred bars away); the
ensemble's is 5 standard errors plus the recorded time-step bias.  None comes from a device result."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from boo_ref import scaled_set
from quench_ref import load_case
import flex_ref
import md_ref
import npt_ref
import pin_ref
from md_ref import BAR_DT, BAR_GAMMA, BAR_KT, BAR_STEPS
from test_pin_ref import DEVICE_CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _library_lifetime():
    """The libraries are initialised by their first calls here and finalised when this file is done."""
    yield
    from mc_water_ls_mw_amd import flexcell, pinning, structure
    pinning.pin_finalize()
    flexcell.flex_finalize()
    structure._dev.finalize()


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _all_same(a, b):
    return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))


def _pin(*a, **kw):
    from mc_water_ls_mw_amd.pinning import interface_pinning
    return interface_pinning(*a, **kw)


def _flex(*a, **kw):
    from mc_water_ls_mw_amd.flexcell import molecular_dynamics_flex
    return molecular_dynamics_flex(*a, **kw)


def _batches():
    """One batch per geometry, as tests/test_gpu_flex.py's: (cells, positions, velocities)."""
    out = []
    for name in ("ih48_t020", "ic96"):
        hs, xs = scaled_set(name, 5, 0.1, 40)
        out.append((hs, xs, md_ref.maxwell_boltzmann(len(xs), xs.shape[1], BAR_KT, seed=21)))
    return out


LANGEVIN = dict(kT=BAR_KT, gamma=BAR_GAMMA, seed=77)
BARO = dict(pressure=npt_ref.BAR_PRESSURE, tau_p=npt_ref.BAR_TAU_P, beta_T=npt_ref.BAR_BETA_T)
STREAMS = np.array([11, 3, 2 ** 40, 5, 0], dtype=np.uint64)
#: a bias of its own for each of the five boxes of a batch: one without, one along an axis, three oblique
NVECS = np.array([[0, 0, 6], [3, -2, 1], [1, 1, 0], [0, 4, -4], [2, 0, -5]], dtype=np.int32)
KAPPAS = np.array([0.02, 0.0, 0.05, 0.01, 0.03])
ANCHORS = np.array([5.0, 0.0, 3.0, 6.0, 1.0])


# -- 1. kappa = 0: libmw_flex.so, byte for byte ---------------------------------------------------------
@pytest.mark.parametrize("every", (0, 5))
@pytest.mark.parametrize("langevin", (False, True), ids=("nve", "langevin"))
@pytest.mark.parametrize("k", (0, 1), ids=("small", "general"))
def test_without_a_bias_the_bytes_are_those_of_mw_flex_run(k, langevin, every):
    hs, xs, vs = _batches()[k]
    kw = dict(vel=vs, streams=STREAMS, sample_every=3, step0=17, pos_ref=xs + 0.25, baro_every=every, **(LANGEVIN if langevin else {}), **BARO)
    for coupling in (0, 1, 3):
        want = _flex(hs, xs, 30, BAR_DT, coupling=coupling, axis=1, **kw)
        got = _pin(hs, xs, NVECS, 0.0, ANCHORS, 30, BAR_DT, coupling=coupling, axis=1, equil_steps=6, block_steps=8, **kw)
        for j, i in ((0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (7, 6)):
            assert _same(got[j], want[i]), (coupling, j)
        assert got[5].shape == (5, 11, 17) and _same(np.ascontiguousarray(got[5][..., :15]), want[5]) and np.all(got[5][..., 15:] == 0.0)
        assert got[6].shape == (5, 3, 4) and np.all(got[6][..., :2] == 0.0) and np.all(got[6][..., 2] > 0.0)
        assert np.all(want[6] == (30, 0)) and (every == 0 or not np.any(want[3][:, 1, 1] == hs[:, 1, 1]))


# -- 2. trajectories against the mirror ------------------------------------------------------------
def _hold_to(got, ref, label):
    pos, vel, forces, cell, refp, trace, blocks, status = got
    d = dict(pos=float(np.abs(pos - ref["pos"]).max()), vel=float(np.abs(vel - ref["vel"]).max()), cell=float(np.abs(cell - ref["cell"]).max()),
             ref=float(np.abs(refp - ref["ref"]).max()))
    dt, db = np.abs(trace - ref["trace"]).max(axis=0), np.abs(blocks - ref["blocks"]).max(axis=0)
    print(label, "status", tuple(status), "pos %.2e (bar %.2e) vel %.2e (bar %.2e) cell %.2e (bar %.2e)" % (d["pos"], pin_ref.POS_TOL, d["vel"], pin_ref.VEL_TOL,
                                                                                                          d["cell"], pin_ref.CELL_TOL),
          "trace", " ".join("%.2e" % v for v in dt), "bars", " ".join("%.2e" % v for v in pin_ref.TRACE_TOL),
          "blocks", " ".join("%.2e" % v for v in db), "bars", " ".join("%.2e" % v for v in pin_ref.BLOCK_TOL))
    assert tuple(status) == tuple(ref["status"])
    assert d["pos"] <= pin_ref.POS_TOL and d["ref"] <= pin_ref.POS_TOL and d["vel"] <= pin_ref.VEL_TOL and d["cell"] <= pin_ref.CELL_TOL
    assert np.all(dt <= np.array(pin_ref.TRACE_TOL)) and blocks.shape == ref["blocks"].shape and np.all(db <= np.array(pin_ref.BLOCK_TOL))


@pytest.mark.parametrize("coupling,axis,every", pin_ref.BAR_RUNS, ids=("uniaxial_1", "aniso_5", "uniaxial_5", "aniso_1"))
@pytest.mark.parametrize("langevin", (False, True), ids=("deterministic", "langevin"))
@pytest.mark.parametrize("name,skew", DEVICE_CASES, ids=[n + ("_skew" if s else "") for n, s in DEVICE_CASES])
def test_forty_biased_steps_land_where_the_mirror_lands(name, skew, langevin, coupling, axis, every):
    """Both geometries, 64 and 65 molecules, orthorhombic and triclinic cells (ic64_sheared, ic65_interstitial), an oblique triple
    with a negative component: state, cell, all 17 columns and the four block averages."""
    h, xyz = load_case(name)
    nvec, kappa, anchor, _ = pin_ref.bias_case(name, skew)
    ref = pin_ref.reference(name, langevin, every, coupling, axis, True, False, skew)      # (computed once per process, read-only)
    got = _pin(h, xyz, np.array(nvec), kappa, anchor, BAR_STEPS, BAR_DT, vel=md_ref.bar_velocities(name), streams=[3], coupling=coupling, axis=axis,
               equil_steps=pin_ref.BLOCK_EQUIL, block_steps=pin_ref.BLOCK_STEPS, **npt_ref.bar_kwargs(langevin, every))
    _hold_to(got, ref, "%s%s coupling %d every %d %s" % (name, " skew" if skew else "", coupling, every, "langevin" if langevin else "deterministic"))
    from mc_water_ls_mw_amd.pinning import pin_last
    assert tuple(got[7]) == (BAR_STEPS, 0) and pin_last()["small"] == (len(xyz) <= 64)


# -- 3. the single point ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,skew", DEVICE_CASES + (("ih1536_t012", False),), ids=[n + ("_skew" if s else "") for n, s in DEVICE_CASES] + ["ih1536_t012"])
def test_a_single_point_has_the_structure_factors_q_and_the_mirrors_bias_force(name, skew):
    """nsteps = 0: column 15 is pinning.order_parameter (libmw_sk.so) within the bar of the column, forces minus the forces of
    libmw_flex.so is the mirror's F_b within the bar of column 3 (the largest force component's), and the state is the input's.
    ih1536_t012 has several workgroups per box; its triple is (0, 0, 6)."""
    from mc_water_ls_mw_amd.pinning import order_parameter
    h, xyz = load_case(name)
    nvec, kappa, anchor, _ = pin_ref.bias_case(name, skew) if name != "ih1536_t012" else ((0, 0, 6), 0.02, 10.0, None)
    pos, vel, forces, cell, ref, trace, blocks, status = _pin(h, xyz, np.array(nvec), kappa, anchor, 0, BAR_DT, baro_every=1)
    plain = _flex(h, xyz, 0, BAR_DT, baro_every=1, coupling="uniaxial")
    q, u, fb = pin_ref.bias(h, xyz, nvec, kappa, anchor)
    q_sk = order_parameter(h, xyz, nvec)
    df = np.abs((forces - plain[2]) - fb).max()
    print(name, nvec, "Q %.10f: against the mirror %.2e, against S(k) %.2e (bar %.2e); U_b %.3e off by %.2e (bar %.2e); F_b off by %.2e (bar %.2e) of %.2e"
          % (trace[0, 15], abs(trace[0, 15] - q), abs(trace[0, 15] - q_sk), pin_ref.TRACE_TOL[15], u, abs(trace[0, 16] - u), pin_ref.TRACE_TOL[16], df,
             pin_ref.TRACE_TOL[3], np.abs(fb).max()))
    assert trace.shape == (1, 17) and blocks.shape == (0, 4) and tuple(status) == (0, 0)
    assert _same(pos, np.ascontiguousarray(xyz)) and _same(cell, np.ascontiguousarray(h)) and _same(np.ascontiguousarray(trace[:, :3]), np.ascontiguousarray(plain[5][:, :3]))
    assert abs(trace[0, 15] - q) <= pin_ref.TRACE_TOL[15] and abs(trace[0, 15] - q_sk) <= pin_ref.TRACE_TOL[15]
    assert abs(trace[0, 16] - u) <= pin_ref.TRACE_TOL[16]
    assert df <= pin_ref.TRACE_TOL[3] and np.abs(fb).max() > 1000.0 * pin_ref.TRACE_TOL[3]
    assert abs(trace[0, 3] - np.abs(plain[2] + fb).max()) <= pin_ref.TRACE_TOL[3]
    assert _same(np.ascontiguousarray(trace[:, 4:15]), np.ascontiguousarray(plain[5][:, 4:]))          # the bias has no virial


def test_choose_wavevector_finds_the_mirrors_triple():
    from mc_water_ls_mw_amd.pinning import choose_wavevector
    for name in ("ih48_t020", "ic96"):
        h, xyz = load_case(name)
        assert tuple(choose_wavevector(h, xyz)) == pin_ref.bias_case(name)[0]
        n2 = choose_wavevector(h, xyz, axis=2)
        assert n2[2] == 0 and tuple(n2) == tuple(pin_ref.choose_wavevector(h, xyz, axis=2))


# -- 4. bit rules -------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (0, 1), ids=("small", "general"))
def test_a_batch_equals_the_single_calls_and_a_run_equals_its_halves_bit_for_bit(k):
    """Five boxes with five biases in one call against five calls, a part of the batch, the same call twice; 24 steps against
    10 + 14 (the first run ends with a barostat application) and 12 + 12; blocks that do not depend on sample_every."""
    hs, xs, vs = _batches()[k]
    kw = dict(sample_every=2, baro_every=5, coupling="uniaxial", axis=2, equil_steps=3, block_steps=7, **LANGEVIN, **BARO)
    got = _pin(hs, xs, NVECS, KAPPAS, ANCHORS, 24, BAR_DT, vel=vs, step0=100, streams=STREAMS, **kw)
    assert got[5].shape == (5, 13, 17) and got[6].shape == (5, 3, 4) and np.all(got[7] == (24, 0)) and not np.any(got[3][:, 2, 2] == hs[:, 2, 2])
    assert np.all(got[5][1, :, 15:] == 0.0) and np.all(got[5][[0, 2, 3, 4], :, 15] > 0.0) and np.all(got[6][[0, 2, 3, 4], :, 0] > 0.0)
    assert _all_same(_pin(hs, xs, NVECS, KAPPAS, ANCHORS, 24, BAR_DT, vel=vs, step0=100, streams=STREAMS, **kw), got)
    for b in range(5):
        alone = _pin(hs[b], xs[b], NVECS[b], KAPPAS[b], ANCHORS[b], 24, BAR_DT, vel=vs[b], step0=100, streams=STREAMS[b:b + 1], **kw)
        assert _all_same(alone, [o[b] for o in got]), b
    assert _all_same(_pin(hs[2:], xs[2:], NVECS[2:], KAPPAS[2:], ANCHORS[2:], 24, BAR_DT, vel=vs[2:], step0=100, streams=STREAMS[2:], **kw), [o[2:] for o in got])
    # box 1 has no bias: the bytes of libmw_flex.so in the middle of a biased batch
    plain = _flex(hs[1], xs[1], 24, BAR_DT, vel=vs[1], step0=100, streams=STREAMS[1:2], sample_every=2, baro_every=5, coupling="uniaxial", axis=2, **LANGEVIN, **BARO)
    assert _same(got[0][1], plain[0]) and _same(got[1][1], plain[1]) and _same(np.ascontiguousarray(got[5][1][:, :15]), plain[5])
    for first_steps in (10, 12):
        a = _pin(hs, xs, NVECS, KAPPAS, ANCHORS, first_steps, BAR_DT, vel=vs, step0=100, streams=STREAMS, **kw)
        b = _pin(a[3], a[0], NVECS, KAPPAS, ANCHORS, 24 - first_steps, BAR_DT, vel=a[1], step0=100 + first_steps, pos_ref=a[4], streams=STREAMS, **kw)
        assert np.all(a[7] == (first_steps, 0)) and _all_same(b[:5], got[:5]), first_steps
        r = first_steps // 2
        assert _same(a[5], np.ascontiguousarray(got[5][:, :r + 1])) and _same(b[5], np.ascontiguousarray(got[5][:, r:])), first_steps
    for every in (1, 24, 5):
        other = _pin(hs, xs, NVECS, KAPPAS, ANCHORS, 24, BAR_DT, vel=vs, step0=100, streams=STREAMS, **dict(kw, sample_every=every))
        assert _same(other[6], got[6]) and _all_same(other[:5], got[:5]), every
    # the blocks are the averages of the rows: sample_every = 1 shows them
    rows = _pin(hs, xs, NVECS, KAPPAS, ANCHORS, 24, BAR_DT, vel=vs, step0=100, streams=STREAMS, **dict(kw, sample_every=1))[5]
    for j in range(3):
        seg = rows[:, 4 + 7 * j:11 + 7 * j]
        want = np.stack([seg[..., 15].mean(axis=1), (seg[..., 15] ** 2).mean(axis=1), seg[..., 4].mean(axis=1), seg[..., 0].mean(axis=1)], axis=-1)
        assert np.allclose(got[6][:, j], want, rtol=1e-13, atol=0), j
    assert not _same(_pin(hs, xs, NVECS, KAPPAS + 1e-3, ANCHORS, 24, BAR_DT, vel=vs, step0=100, streams=STREAMS, **kw)[0][0], got[0][0])


def test_device_tensors_and_null_outputs_give_the_bits_of_the_host_entry():
    import torch
    from mc_water_ls_mw_amd.pinning import interface_pinning_torch, load_pin_library
    dev = torch.device("cuda:0")
    for hs, xs, vs in _batches():
        kw = dict(baro_every=3, coupling="aniso", axis=1, equil_steps=2, block_steps=6, **LANGEVIN, **BARO)
        got = _pin(hs, xs, NVECS, KAPPAS, ANCHORS, 20, BAR_DT, vel=vs, streams=STREAMS, pos_ref=xs + 0.25, **kw)
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)       # noqa: E731
        t = interface_pinning_torch(to(hs), to(xs), to(NVECS), to(KAPPAS), to(ANCHORS), 20, BAR_DT, vel_t=to(vs), streams_t=to(STREAMS.view(np.int64)),
                                    pos_ref_t=to(xs + 0.25), **kw)
        assert all(v.is_cuda for v in t) and t[6].dtype == torch.float64 and t[7].dtype == torch.int32
        assert _all_same([v.cpu().numpy() for v in t], got)
        L = load_pin_library()
        cells, pos, vel, ref = (np.ascontiguousarray(a) for a in (hs, xs, vs, xs + 0.25))
        for keep in range(8):
            outs = [np.zeros_like(o) for o in got]
            ptrs = [o.ctypes.data if j == keep else None for j, o in enumerate(outs)]
            assert L.mw_pin_run(len(xs), xs.shape[1], cells.ctypes.data, pos.ctypes.data, vel.ctypes.data, ref.ctypes.data, NVECS.ctypes.data, KAPPAS.ctypes.data,
                                ANCHORS.ctypes.data, STREAMS.ctypes.data, 77, 0, 20, 1, 2, 6, BAR_DT, md_ref.MASS_WATER, BAR_KT, BAR_GAMMA, BARO["pressure"],
                                BARO["tau_p"], BARO["beta_T"], 3, 1, 1, *ptrs) == 0, L.mw_pin_last_error()
            assert _same(outs[keep], got[keep]), keep


def test_rejected_calls_on_a_live_library_write_nothing():
    from mc_water_ls_mw_amd.pinning import load_pin_library, pin_init
    pin_init()
    L = load_pin_library()
    hs, xs, vs = _batches()[0]
    cells, pos = np.ascontiguousarray(hs), np.ascontiguousarray(xs)
    for nvec, kappas, anchors, word in ((NVECS * 0, KAPPAS, ANCHORS, "nvec"), (NVECS * 100, KAPPAS, ANCHORS, "nvec"), (NVECS, -KAPPAS, ANCHORS, "kappas"),
                                        (NVECS, KAPPAS * np.nan, ANCHORS, "kappas"), (NVECS, KAPPAS, -ANCHORS, "anchors")):
        nvec, kappas, anchors = np.ascontiguousarray(nvec, dtype=np.int32), np.ascontiguousarray(kappas), np.ascontiguousarray(anchors)
        outs = [np.full(5 * 48 * 3, -7.0) for _ in range(3)] + [np.full(45, -7.0), np.full(5 * 48 * 3, -7.0), np.full(5 * 11 * 17, -7.0), np.full(5 * 2 * 4, -7.0),
                                                                np.full(10, -7, dtype=np.int32)]
        rc = L.mw_pin_run(5, 48, cells.ctypes.data, pos.ctypes.data, None, None, nvec.ctypes.data, kappas.ctypes.data, anchors.ctypes.data, None, 1, 0, 10, 1, 2, 4,
                          BAR_DT, md_ref.MASS_WATER, 0.0, 0.0, BARO["pressure"], BARO["tau_p"], BARO["beta_T"], 2, 3, 2, *[o.ctypes.data for o in outs])
        msg = L.mw_pin_last_error().decode()
        assert rc != 0 and word in msg and "mw_pin_run" in msg and "box" in msg and all(bool(np.all(o == -7)) for o in outs), msg


def _switch_cases():
    """More boxes of each geometry than 1 MiB of scratch holds: (cells, positions, velocities, nvec, kappas, anchors)."""
    out = []
    for name, count in (("ic48_t015", 260), ("ic96", 50)):
        hs, xs = scaled_set(name, count, 0.05, 300)
        k = np.arange(count)
        out.append((hs, xs, md_ref.maxwell_boltzmann(count, xs.shape[1], BAR_KT, seed=31), NVECS[k % 5], KAPPAS[k % 5], ANCHORS[k % 5]))
    return out


SWITCH_STEPS = 70                                                          # more than one launch of 64 steps


def _switch_run(hs, xs, vs, nvec, kappas, anchors):
    return _pin(hs, xs, nvec, kappas, anchors, SWITCH_STEPS, BAR_DT, vel=vs, sample_every=7, baro_every=9, step0=5, coupling="uniaxial", equil_steps=5, block_steps=13,
                **LANGEVIN, **BARO)


def test_chunks_and_slices_do_not_change_a_byte(tmp_path):
    """A fresh process with 3 steps per launch of the small geometry and 1 MiB of scratch (several chunks, the last one ragged)
    returns the bytes of this process (64 steps per launch, 256 MiB), blocks included."""
    from mc_water_ls_mw_amd.pinning import pin_last
    got, fits = [], []
    for case in _switch_cases():
        got.append(_switch_run(*case))
        last = pin_last()
        assert last["chunks"] == 1 and last["steps_per_launch"] == (64 if last["small"] else 1)
        fits.append((1 << 20) // last["scratch_bytes_per_box"])
        assert 1 < fits[-1] < len(case[1]) and len(case[1]) % fits[-1] != 0 and np.all(got[-1][7] == (SWITCH_STEPS, 0)) and got[-1][6].shape[1] == 5
    out = tmp_path / "switch.npz"
    env = dict(os.environ, MW_PIN_SCRATCH_MB="1", MW_PIN_SLICE="3")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, (res.stdout[-1000:], res.stderr[-3000:])
    z = np.load(out)
    for k in range(2):
        assert int(z[f"boxes_per_chunk{k}"]) == fits[k] and int(z[f"chunks{k}"]) == -(-len(got[k][0]) // fits[k]) >= 2
        assert int(z[f"steps_per_launch{k}"]) == (3 if k == 0 else 1)
        assert _all_same([z[f"out{k}_{j}"] for j in range(8)], got[k]), k


# -- 5. the guards --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (0, 1), ids=("small", "general"))
def test_a_huge_kappa_trips_the_drift_guard_and_leaves_the_neighbours_alone(k):
    """Box 2 gets kappa = 1e6 Hartree: its first kick is beyond a sigma / 4 per half step.  Status (steps completed < 12, 1), a
    finite state, the last row repeated in the trace and in the blocks; the other boxes have the bytes of the call without it."""
    hs, xs, vs = _batches()[k]
    kappas = KAPPAS.copy()
    kappas[2] = 1e6
    kw = dict(vel=vs, streams=STREAMS, baro_every=4, coupling="uniaxial", equil_steps=2, block_steps=5, **BARO)
    got = _pin(hs, xs, NVECS, kappas, ANCHORS, 12, BAR_DT, **kw)
    want = _pin(hs, xs, NVECS, KAPPAS, ANCHORS, 12, BAR_DT, **kw)
    done = int(got[7][2, 0])
    print("frozen after", done, "steps; rows", got[5][2, :, 15])
    assert got[7][2, 1] == 1 and done < 12 and all(np.all(np.isfinite(o[2])) for o in got[:7])
    assert np.all(got[5][2, done:] == got[5][2, done]) and np.all(got[6][2, 1] == [got[5][2, done, 15], got[5][2, done, 15] ** 2, got[5][2, done, 4], got[5][2, done, 0]])
    for b in (0, 1, 3, 4):
        assert _all_same([o[b] for o in got], [o[b] for o in want]), b
    assert np.all(want[7] == (12, 0))


# -- 6. the ensemble --------------------------------------------------------------------------------
def test_the_bias_holds_a_dilute_gas_at_the_mean_and_the_variance_of_its_law():
    """FREE_BOXES boxes of 20 molecules spread uniformly over a fixed cube of 244 bohr at kT = 0.05 Hartree (30 cutoffs wide: the mW
    forces are those of a dilute gas, as in tests/test_gpu_flex.py), thermostatted, under 1/2 kappa (Q - a)^2 with kappa = 4 kT,
    a = 2 on the mode (24, -12, 8), for FREE_STEPS steps: pin_ref's free ensemble.  <Q> and var Q within 5 standard errors (the
    device ensemble's and the reference draw's) plus the recorded time-step bias of the exact law, which lies 0.56 above the
    unbiased mean."""
    nb, n = pin_ref.FREE_BOXES, pin_ref.FREE_N
    mean, var, se_mean, se_var = pin_ref.free_law()
    x, v = pin_ref.free_start(nb, 17)
    h = np.tile(np.eye(3) * pin_ref.FREE_SIDE, (nb, 1, 1))
    out = _pin(h, x, np.array(pin_ref.FREE_NVEC), pin_ref.FREE_KAPPA, pin_ref.FREE_ANCHOR, pin_ref.FREE_STEPS, pin_ref.FREE_DT, vel=v, kT=pin_ref.FREE_KT,
               gamma=pin_ref.FREE_GAMMA_DT / pin_ref.FREE_DT, baro_every=0, seed=11, streams=np.arange(1000, 1000 + nb), sample_every=pin_ref.FREE_STEPS)
    trace, status = out[5], out[7]
    q0, q = trace[:, 0, 15], trace[:, 1, 15]
    m4 = float(((q - q.mean()) ** 4).mean())
    dev_se_mean, dev_se_var = math.sqrt(q.var() / nb), math.sqrt((m4 - q.var() ** 2) / nb)
    dm, dv = q.mean() - mean, q.var() - var
    print("frozen", int((status[:, 1] != 0).sum()), "start <Q> %.4f; <Q> - law = %.3e (5 se %.3e + bias %.3e), var Q - law = %.3e (5 se %.3e + bias %.3e); K / (3 N kT / 2) - 1 = %.3e"
          % (q0.mean(), dm, 5 * math.hypot(dev_se_mean, se_mean), pin_ref.FREE_BIAS, dv, 5 * math.hypot(dev_se_var, se_var), pin_ref.FREE_VAR_BIAS,
             trace[:, 1, 1].mean() / (1.5 * n * pin_ref.FREE_KT) - 1.0))
    assert np.all(status == (pin_ref.FREE_STEPS, 0))
    assert abs(q0.mean() - math.sqrt(math.pi) / 2.0) < 0.05 and mean - q0.mean() > 0.4          # the start is the unbiased law, far away
    assert abs(dm) <= 5.0 * math.hypot(dev_se_mean, se_mean) + pin_ref.FREE_BIAS
    assert abs(dv) <= 5.0 * math.hypot(dev_se_var, se_var) + pin_ref.FREE_VAR_BIAS


# -- 7. with the engine in the same process -----------------------------------------------------------
def test_the_engine_and_the_farm_give_what_the_arrays_give():
    from test_gpu_md import _farm
    from mc_water_ls_mw_amd.pinning import delta_mu, pin_elapsed_ms
    em, farm = _farm()
    try:
        farm.sweep(96, seed=41)
        nb = em.num_lattices
        e0 = em.model_energy_batch(1, nb).copy()
        vel = md_ref.maxwell_boltzmann(nb, 48, BAR_KT, seed=9)
        kw = dict(kT=BAR_KT, gamma=BAR_GAMMA, vel=vel, seed=13, sample_every=5, baro_every=5, tau_p=npt_ref.BAR_TAU_P, beta_T=npt_ref.BAR_BETA_T, coupling="uniaxial",
                  axis=2, equil_steps=5, block_steps=10)
        pos_f, vel_f, cells_f, trace_f, blocks_f, status_f = farm.interface_pinning((0, 0, 6), 0.02, 4.0, 25, BAR_DT, first_global_walker=6, **kw)
        hs = farm.sync_cells()
        pos = np.array([farm.positions(b + 1) for b in range(nb)])
        streams = 6 * 2 + np.arange(nb)
        want = _pin(hs, pos, (0, 0, 6), 0.02, 4.0, 25, BAR_DT, streams=streams, pressure=farm.pressure, **kw)
        assert pos_f.shape == (2, 2, 48, 3) and trace_f.shape == (2, 2, 6, 17) and blocks_f.shape == (2, 2, 2, 4) and status_f.shape == (2, 2, 2)
        assert _same(pos_f.reshape(nb, 48, 3), want[0]) and _same(vel_f.reshape(nb, 48, 3), want[1]) and _same(cells_f.reshape(nb, 3, 3), want[3])
        assert _same(trace_f.reshape(nb, 6, 17), want[5]) and _same(blocks_f.reshape(nb, 2, 4), want[6]) and _same(status_f.reshape(nb, 2), want[7])
        assert np.all(status_f[:, :, 0] == 25) and np.all(trace_f[..., 15] > 0.0)
        assert _all_same(em.interface_pinning((0, 0, 6), 0.02, 4.0, 1, nb, 25, BAR_DT, streams=streams, pressure=farm.pressure, **kw), want)
        t = pin_elapsed_ms()
        assert len(t) == 6 and t[2] > 0.0 and t[4] > 0.0
        mu, err = delta_mu(want[6][0], 0.02, 4.0, 6.0, 1.0, 48)
        assert np.isfinite(mu) and err >= 0.0
        assert np.array_equal(em.model_energy_batch(1, nb), e0) and np.array_equal(farm.sync_cells(), hs)
    finally:
        em.energy_deinit()


if __name__ == "__main__":
    # the child of test_chunks_and_slices_do_not_change_a_byte: the switches are set, mw_pin_init reads them
    from mc_water_ls_mw_amd.pinning import pin_finalize, pin_last
    out = {}
    for k, case in enumerate(_switch_cases()):
        r = _switch_run(*case)
        last = pin_last()
        out.update({f"out{k}_{j}": r[j] for j in range(8)})
        out.update({f"chunks{k}": last["chunks"], f"boxes_per_chunk{k}": last["boxes_per_chunk"], f"steps_per_launch{k}": last["steps_per_launch"]})
    pin_finalize()
    np.savez(sys.argv[1], **out)
