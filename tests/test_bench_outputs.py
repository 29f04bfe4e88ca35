"""CPU: bench.py --dump-outputs writes the last step's results as float64 .npy files, whole while they fit the size limit and
as a fixed, seeded sample of the trial moves beyond it."""
import importlib.util
import os
import sys

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_outputs_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        spec.loader.exec_module(mod)
    finally:
        sys.argv = argv
    return mod


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_outputs_are_written_whole(bench, tmp_path):
    me, eo, en = np.linspace(-1.0, -2.0, 8), np.arange(64.0), -np.arange(64.0)
    bench.dump_outputs(str(tmp_path), me, eo, en, (10, 20, 30, 40))
    a = _load(tmp_path)
    assert sorted(a) == ["interaction_counts", "model_energy", "trial_energy_new", "trial_energy_old"]
    assert all(v.dtype == np.float64 for v in a.values())
    assert np.array_equal(a["model_energy"], me) and np.array_equal(a["trial_energy_old"], eo)
    assert np.array_equal(a["trial_energy_new"], en) and a["interaction_counts"].tolist() == [10.0, 20.0, 30.0, 40.0]


def test_large_outputs_are_a_fixed_sample_within_the_limit(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 200_000)
    n = 100_000
    eo, en = np.arange(n, dtype=np.float64), -np.arange(n, dtype=np.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), np.zeros(4), eo, en, (1, 2, 3, 4))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(os.path.getsize(os.path.join(tmp_path, "a", f)) for f in os.listdir(tmp_path / "a")) <= 200_000
    idx = a["trial_sample_index"]
    assert 0 < len(idx) < n and np.all(np.diff(idx) > 0)
    assert np.array_equal(a["trial_energy_old"], eo[idx.astype(np.int64)]) and np.array_equal(a["trial_energy_new"], -idx)
    assert all(np.array_equal(a[k], b[k]) for k in a)                 # the same sample every time
