"""CPU: the force entries of the C ABI are exported, listed in ABI_SYMBOLS, and fail with a message before mw_init."""
import ctypes

import numpy as np
import pytest

NAMES = ("mw_model_forces", "mw_model_forces_batch", "mw_model_forces_launch")


def _lib():
    from mc_water_ls_mw_amd import build
    from mc_water_ls_mw_amd.energy import load_library
    build.build()
    return load_library()


def test_force_entries_are_exported_and_listed():
    L = _lib()
    from mc_water_ls_mw_amd.energy import ABI_SYMBOLS
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in ABI_SYMBOLS, name


def test_force_entries_fail_with_a_message_before_init():
    L = _lib()
    if L.mw_is_initialised():
        pytest.skip("engine is live in this process")
    dp = ctypes.POINTER(ctypes.c_double)
    e, f, w = np.zeros(1), np.zeros(48 * 3), np.zeros(9)
    calls = [lambda: L.mw_model_forces(1, e.ctypes.data_as(dp), f.ctypes.data_as(dp), w.ctypes.data_as(dp)),
             lambda: L.mw_model_forces_batch(1, 1, e.ctypes.data_as(dp), f.ctypes.data_as(dp), w.ctypes.data_as(dp)),
             lambda: L.mw_model_forces_launch(1, 1, -1)]
    for call in calls:
        assert call() != 0
        assert b"not initialised" in L.mw_last_error()


def test_python_methods_raise_before_init():
    from mc_water_ls_mw_amd.energy import EnergyModule, MwError
    em = EnergyModule(48, 2)
    if em.L.mw_is_initialised():
        pytest.skip("engine is live in this process")
    with pytest.raises(MwError, match="not initialised"):
        em.forces_batch()
    with pytest.raises(MwError, match="outside"):
        em.forces_batch(2, 2)
