"""What mw_moves_counts must total for a batch of requests, from the C oracle and the oracle's own lists.

interactions: COracle.local_energy(..., counts=True) -- in-range pairs plus triplet slots with cos(theta) < 0.99 -- of the
requested molecule at its mirrored position (old) and, the lists unchanged, at its trial position (new).
slots: the definition of include/mw_energy.h -- nn(i) plus nn(j) of every in-range row entry j of i -- evaluated here on the oracle's
lists with the oracle's cutoff (sigma a)^2; the oracle does not count them itself."""
import numpy as np


def request_counts(oracle, x, iv, nn, jn, vn, imol, trial=None):
    """[len(imol), 4] int64 = (interactions old, slots old, interactions new, slots new) per request, and [len(imol), 2] = the
    in-range row entries at the old and the trial position.  ``trial`` None: the new half is zero."""
    sigma, small_a = oracle.constants()[0], oracle.constants()[6]
    rcsq = sigma * small_a * sigma * small_a
    out = np.zeros((len(imol), 4), dtype=np.int64)
    inrange = np.zeros((len(imol), 2), dtype=np.int64)
    for m, i1 in enumerate(imol):
        i = int(i1) - 1
        n = int(nn[i])
        j, v = jn[i, :n] - 1, vn[i, :n] - 1
        q = x[j] + iv[v]
        for geo in range(2 if trial is not None else 1):
            p = x[i] if geo == 0 else trial[m]
            d = q - p
            inr = np.einsum("sc,sc->s", d, d) < rcsq
            y = x
            if geo == 1:
                y = x.copy()
                y[i] = trial[m]
            c = oracle.local_energy(i + 1, y, iv, nn, jn, vn, counts=True)[1]
            out[m, 2 * geo] = int(c.sum())
            out[m, 2 * geo + 1] = n + int(nn[j[inr]].sum())
            inrange[m, geo] = int(inr.sum())
    return out, inrange
