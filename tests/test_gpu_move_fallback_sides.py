"""GPU: k_move_fallback with two wavefronts per declined request -- one for the mirrored, one for the trial position, each writing
its own energy and its own two count words, only the sides the launch asks for -- evaluating with local_energy_wave_batched.  The
dense diamond boxes of tests/test_gpu_move_fallback_tail.py (216 molecules, rows of up to 34 entries, 159 of 160 requests declined):
old-only, trial-only and old + trial launches, two in a row (the list's two count words), and launches with an odd and with an even
number of declined requests.  Energies 1e-10 relative, counts exact (tests/move_counts_ref.py)."""
import numpy as np
import pytest

from test_gpu_move_fallback_tail import NREQ, _ask, _Dense, _want

pytestmark = pytest.mark.gpu

TOL = 1e-10


@pytest.fixture(scope="module")
def dense(c_oracle):
    return _Dense(c_oracle)


def _check(got, mode, ro, rn, ref):
    eo, en, c, ndecl = got
    if mode & 1:
        print("mode", mode, "declined", ndecl, "max rel err e_old", np.max(np.abs(eo - ro) / np.abs(ro)))
        assert np.all(np.abs(eo - ro) <= TOL * np.abs(ro))
    if mode & 2:
        print("mode", mode, "declined", ndecl, "max rel err e_new", np.max(np.abs(en - rn) / np.abs(rn)))
        assert np.all(np.abs(en - rn) <= TOL * np.abs(rn))
    assert c == _want(ref, mode)


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_the_sides_a_launch_asks_for_twice_in_a_row(dense, mode):
    em = dense.engine()
    try:
        runs = [_ask(em, mode, 1, dense.imol[0], dense.trial[0]) for _ in range(2)]
        for got in runs:
            assert 64 <= got[3] <= NREQ
            _check(got, mode, dense.eo[0], dense.en[0], dense.ref[0])
        assert runs[1][3] == runs[0][3]
        for k in (0, 1):
            assert (runs[0][k] is None) == (runs[1][k] is None) == (not (mode >> k) & 1)
            if runs[0][k] is not None:
                assert np.array_equal(runs[0][k], runs[1][k])
    finally:
        em.energy_deinit()


def test_odd_and_even_numbers_of_declined_requests(dense):
    """Twice as many wavefronts have work as requests were declined; the last pair must not depend on a partner."""
    em = dense.engine()
    try:
        imol, trial, ro, rn, ref = dense.imol[0], dense.trial[0], dense.eo[0], dense.en[0], dense.ref[0]
        every = _ask(em, 3, 1, imol, trial)
        _check(every, 3, ro, rn, ref)
        # without one declined request: request 0, unless it is the one the fused routine serves
        drop = 0 if _ask(em, 3, 1, imol[:1], trial[:1])[3] == 1 else 1
        keep = np.arange(NREQ) != drop
        fewer = _ask(em, 3, 1, imol[keep], trial[keep])
        _check(fewer, 3, ro[keep], rn[keep], ref[keep])
        print("declined", every[3], fewer[3])
        assert fewer[3] == every[3] - 1 and {every[3] % 2, fewer[3] % 2} == {0, 1}
    finally:
        em.energy_deinit()
