"""GPU: k_move_fallback, which serves the requests the fused move routines decline, one wavefront each with the plain routine.
A compressed diamond lattice (the construction of tests/test_gpu_parity.py's test_dense_boxes_take_the_plain_routines, d_OO = 2.2 A:
216 molecules, rows of up to 34 entries, more than 24 in-range neighbours) declines 159 of 160 requests; a second box of the same
size at d_OO = 2.35 A declines none.  Energies 1e-10 relative, counts exact (tests/move_counts_ref.py), for old-only, trial-only and
old + trial launches, and the list's two count words in turn."""
import numpy as np
import pytest

from conftest import DE_ATOL, RTOL
from move_counts_ref import request_counts

pytestmark = pytest.mark.gpu

NREQ = 160


class _Dense:
    def __init__(self, oracle):
        from mc_water_ls_mw_amd import lattice as lat
        self.h, self.x, self.lists, self.iv = [], [], [], []
        for d_oo in (2.2, 2.35):
            h, x = lat.ice_ic_cell(d_oo)
            h, x = lat.replicate(h, x, (3, 3, 3))
            x = lat.thermalise(x, 0.05, 1)
            iv = oracle.ivects(h)
            self.h.append(h); self.x.append(x); self.iv.append(iv); self.lists.append(oracle.neighbours(x, iv, 64))
        self.imol, self.trial, self.eo, self.en, self.ref = [], [], [], [], []
        for b in range(2):
            i, t = lat.trial_moves(self.x[b], NREQ, max_trans_ang=0.6, seed=8)
            o, n = oracle.trial_moves(i, t, self.x[b], self.iv[b], *self.lists[b])
            self.imol.append(i.astype(np.int32)); self.trial.append(t); self.eo.append(o); self.en.append(n)
            self.ref.append(request_counts(oracle, self.x[b], self.iv[b], *self.lists[b], i, t)[0])

    def engine(self):
        from mc_water_ls_mw_amd.energy import load_boxes
        return load_boxes(self.h, self.x, maxneigh=64)


@pytest.fixture(scope="module")
def dense(c_oracle):
    return _Dense(c_oracle)


def _ask(em, mode, ils, imol, trial):
    """(e_old or None, e_new or None, counts, declined) of one launch in `mode` (1 old, 2 trial, 3 both)."""
    eo = en = None
    if mode == 1:
        eo = em.local_energy_batch(ils, imol)
    elif mode == 2:
        en = em.local_energy_batch(ils, imol, trial)
    else:
        eo, en = em.delta_energy_batch(ils, imol, trial)
    c = em.moves_counts()
    return eo, en, c, em.last_dispatch("moves")["declined"]


def _want(ref, mode):
    t = ref.sum(axis=0) if ref.ndim == 2 else ref
    return (int(t[0]) if mode & 1 else 0, int(t[1]) if mode & 1 else 0, int(t[2]) if mode & 2 else 0, int(t[3]) if mode & 2 else 0)


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_declined_requests_against_the_oracle(dense, mode):
    em = dense.engine()
    try:
        imol, trial, ro, rn, ref = dense.imol[0], dense.trial[0], dense.eo[0], dense.en[0], dense.ref[0]
        eo, en, c, ndecl = _ask(em, mode, 1, imol, trial)
        print("mode", mode, "declined", ndecl, "of", NREQ, "counts", c)
        assert 64 <= ndecl <= 400
        if eo is not None:
            assert np.all(np.abs(eo - ro) <= RTOL * np.abs(ro))
        if en is not None:
            assert np.all(np.abs(en - rn) <= RTOL * np.abs(rn))
        if mode == 3:
            assert np.all(np.abs((en - eo) - (rn - ro)) <= DE_ATOL)
        assert c == _want(ref, mode)
        # request by request: a batch of one, which the fallback serves whenever the batch above left it that request.  (No entry
        # point exposes per-request counts: in the batch above, which runs the kernel's stride loop, the counts can only be held as
        # totals; its energies, which share the output index with the counts, are held per request.)
        served_by_fallback = 0
        for m in range(NREQ):
            eo1, en1, c1, d1 = _ask(em, mode, 1, imol[m:m + 1], trial[m:m + 1])
            served_by_fallback += d1
            assert c1 == _want(ref[m], mode), (m, c1, ref[m])
            if eo1 is not None:
                assert abs(eo1[0] - ro[m]) <= RTOL * abs(ro[m])
            if en1 is not None:
                assert abs(en1[0] - rn[m]) <= RTOL * abs(rn[m])
        assert served_by_fallback == ndecl
    finally:
        em.energy_deinit()


def test_a_launch_with_none_declined_behind_one_with_many(dense):
    """The list's two count words alternate between launches and the fallback zeroes the other one: after a launch that declined
    159 requests, launches that decline none must find their word at zero and serve nothing twice -- and the next dense launch
    must come out as the first."""
    em = dense.engine()
    try:
        first = _ask(em, 3, 1, dense.imol[0], dense.trial[0])
        assert first[3] >= 64
        for _ in range(2):                                                  # both count words in turn
            eo, en, c, ndecl = _ask(em, 3, 2, dense.imol[1], dense.trial[1])
            assert ndecl == 0 and c == _want(dense.ref[1], 3)
            assert np.all(np.abs(eo - dense.eo[1]) <= RTOL * np.abs(dense.eo[1])) and np.all(np.abs(en - dense.en[1]) <= RTOL * np.abs(dense.en[1]))
        again = _ask(em, 3, 1, dense.imol[0], dense.trial[0])
        assert again[3] == first[3] and again[2] == first[2] == _want(dense.ref[0], 3)
        assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])
    finally:
        em.energy_deinit()
