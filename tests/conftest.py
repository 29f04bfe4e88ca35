import glob
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")

# mw_sweep_sync_cells no longer re-uploads the image vectors the device's volume moves built: under test, every call reads the
# device's tables back and fails unless they equal the host's own compute_ivects bit for bit (read once, at the first call).
os.environ.setdefault("MW_SYNC_CELLS_VERIFY", "1")

#: parity bar of BASELINE.json's north_star: energies within 1e-10 relative of the Fortran reference
RTOL = 1e-10
#: the reference author's own absolute tolerance on a move's energy change (mc_moves.F90:1099), Hartree
DE_ATOL = 1e-10


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def golden_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz"))
                  if os.path.basename(p) not in ("constants.npz", "ls_pair48.npz") and not os.path.basename(p).startswith("chain_"))   # (chain_*: the driver's golden chains, tests/test_chain_fixtures.py)


def load_golden(name):
    from mc_water_ls_mw_amd import lattice as lat
    z = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
    if "xyz" not in z:   # big synthetic boxes are regenerated from their recipe and checked by digest
        kind = name[:2]
        reps = {"4096": (8, 8, 8), "32768": (16, 16, 16)}[name[2:].split("_")[0]]
        sigma = 0.15 if name.endswith("t015") else 0.0
        h, xyz = lat.ice_box(kind, reps, sigma, seed=20250228)
        import hashlib
        assert hashlib.sha256(np.ascontiguousarray(xyz).tobytes()).hexdigest() == str(z["xyz_sha256"]), \
            f"{name}: regenerated positions differ from the ones the golden vector was made from"
        assert np.array_equal(h, z["h"])
        z["xyz"] = xyz
    return z


def list_digest(nn, jn, vn):
    import hashlib
    mask = np.arange(jn.shape[1])[None, :] < nn[:, None]
    m = hashlib.sha256()
    for a in (nn.astype(np.int32), jn[mask].astype(np.int32), vn[mask].astype(np.int32)):
        m.update(np.ascontiguousarray(a).tobytes())
    return m.hexdigest()


@pytest.fixture(scope="session")
def c_oracle():
    from oracle import COracle
    return COracle()


#: what the reference program's runs in the pin tests wrote (oracle/_ref/mc_water_ref_rng*): recorded where the reference's
#: sources are at hand and oracle/_ref/ is built (MW_RECORD_REF_RUNS=1), replayed everywhere else
REF_RUNS = os.path.join(GOLDEN, "ref_runs")


def _file_digests(d):
    import hashlib
    return {n: hashlib.sha256(open(os.path.join(d, n), "rb").read()).hexdigest()
            for n in sorted(os.listdir(d)) if os.path.isfile(os.path.join(d, n))}


def _ref_run_path(binary, args, before, env):
    """A run is keyed by the program, its arguments, the files of its working directory and the interposition switches."""
    import hashlib
    m = hashlib.sha256()
    for part in [os.path.basename(binary), *args, *(f"{n}:{h}" for n, h in before.items()),
                 *(f"{k}={env[k]}" for k in sorted(env) if k.startswith("MW_WRAP_"))]:
        m.update(part.encode() + b"\0")
    return os.path.join(REF_RUNS, f"{os.path.basename(binary)}_{m.hexdigest()[:20]}.npz")


def run_reference_program(binary, args, cwd, env=None, timeout=600):
    """subprocess.run([binary, *args], cwd=cwd, ...) for a reference program under oracle/_ref/.  Where it is not built (its
    recipe needs the reference's sources), the recorded run with the same inputs writes its files into `cwd` instead; a run
    that was never recorded skips the test."""
    import subprocess
    env = dict(os.environ if env is None else env)
    before = _file_digests(cwd)
    path = _ref_run_path(binary, args, before, env)
    if not os.path.exists(binary):
        if not os.path.exists(path):
            pytest.skip(f"oracle/_ref/{os.path.basename(binary)} not built and this run of it not recorded under tests/golden/ref_runs")
        z = np.load(path)
        for k in z.files:
            if k.startswith("file:"):
                with open(os.path.join(cwd, k[5:]), "wb") as fh:
                    fh.write(z[k].tobytes())
        return subprocess.CompletedProcess([binary, *args], int(z["returncode"]), z["stdout"].tobytes().decode(),
                                           z["stderr"].tobytes().decode())
    out = subprocess.run([binary, *args], cwd=cwd, capture_output=True, text=True, timeout=timeout, env=env)
    if os.environ.get("MW_RECORD_REF_RUNS") == "1" and out.returncode == 0:
        after = _file_digests(cwd)
        files = {"file:" + n: np.frombuffer(open(os.path.join(cwd, n), "rb").read(), dtype=np.uint8)
                 for n, h in after.items() if before.get(n) != h}
        os.makedirs(REF_RUNS, exist_ok=True)
        np.savez_compressed(path, returncode=np.int32(out.returncode), stdout=np.frombuffer(out.stdout.encode(), dtype=np.uint8),
                            stderr=np.frombuffer(out.stderr.encode(), dtype=np.uint8), **files)
    return out
