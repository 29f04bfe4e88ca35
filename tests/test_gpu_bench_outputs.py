"""GPU: a plain bench.py run prints the headline line only, and --dump-outputs writes what its last timed step computed --
walker 0 is the golden fixture ih4096_t015, so its full-box energy and the old / new energies of its first trial moves are
the reference's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    out_dir = str(tmp_path / "outputs")
    env = dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--walkers", "4", "--moves", "256", "--dump-outputs", out_dir],
                         env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, (res.stdout[-1500:], res.stderr[-3000:])
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, res.stdout[-1500:]
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "interactions/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["full"] is False and "kernels" not in line and "cpu_baseline" not in line and "secondary" not in line

    a = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in os.listdir(out_dir)}
    assert sorted(a) == ["interaction_counts", "model_energy", "trial_energy_new", "trial_energy_old"]
    assert all(v.dtype == np.float64 for v in a.values())
    assert a["model_energy"].shape == (4,) and a["trial_energy_old"].shape == a["trial_energy_new"].shape == (4 * 256,)
    gold = np.load(os.path.join(GOLDEN, "ih4096_t015.npz"))
    ref = float(gold["model_energy"])
    assert abs(a["model_energy"][0] - ref) <= 1e-10 * abs(ref)
    n = min(256, len(gold["trial_old"]))
    assert np.all(np.abs(a["trial_energy_old"][:n] - gold["trial_old"][:n]) <= 1e-10 * np.abs(gold["trial_old"][:n]))
    assert np.all(np.abs(a["trial_energy_new"][:n] - gold["trial_new"][:n]) <= 1e-10 * np.abs(gold["trial_new"][:n]))
    c = a["interaction_counts"]
    assert c.shape == (4,) and np.all(c > 0)
    assert line["value"] == pytest.approx(c.sum() / (line["ms_per_step"] * 1e-3), rel=1e-9)     # interactions of one step / its time
