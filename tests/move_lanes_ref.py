"""Which requests the lane-pair moment path of the move kernel (mw_move_lanes.hip.h) must decline, predicted on the host from the
oracle's lists.  A request (molecule i, old position, trial position) is declined when
  * more than 16 entries of i's row are in range of the old OR the trial position ("cap"),
  * i lists itself ("self"),
  * at either position P, a pair (a, b) of entries both in range of P has
      cos(theta_aPb) >= 0.99 - 1e-9                                              ("jik": the j--i--k term the reference drops), or
      |ab| < cutoff and cos(theta_Pab) or cos(theta_Pba) >= 0.99 - 1e-9          ("ijk": a third body in a neighbour's moments).
`margin` is the smallest distance of any quantity from the threshold it is compared with -- |r - rc| of every row entry at both
positions and of every pair of in-range entries (bohr), and |cos - 0.99| of every angle tested: a prediction is exact when it is
far above the rounding of the device's squares."""
import numpy as np

CAP = 16
COS_MAX = 0.99 - 1e-9


def predict(oracle, x, iv, nn, jn, vn, imol, trial):
    """Per request: dict of arrays `union` (entries in range of either position), `n_old`, `n_new`, `row` (row length), `cap`, `self`,
    `jik`, `ijk`, `declined` (bools) and `margin`."""
    sigma, small_a = oracle.constants()[0], oracle.constants()[6]
    rc = sigma * small_a
    m = len(imol)
    out = {k: np.zeros(m, dtype=bool) for k in ("cap", "self", "jik", "ijk", "declined")}
    out.update({k: np.zeros(m, dtype=np.int64) for k in ("union", "n_old", "n_new", "row")})
    out["margin"] = np.full(m, np.inf)
    for r, i1 in enumerate(imol):
        i = int(i1) - 1
        n = int(nn[i])
        j, v = jn[i, :n] - 1, vn[i, :n] - 1
        q = x[j] + iv[v]
        margin = np.inf
        inr = []
        for p in (x[i], np.asarray(trial[r], dtype=np.float64)):
            d = np.linalg.norm(q - p, axis=1)
            margin = min(margin, np.min(np.abs(d - rc)))
            inr.append(d < rc)
        out["row"][r] = n
        out["n_old"][r], out["n_new"][r] = inr[0].sum(), inr[1].sum()
        out["union"][r] = (inr[0] | inr[1]).sum()
        out["cap"][r] = out["union"][r] > CAP
        out["self"][r] = bool(np.any(j == i))
        for p, sel in zip((x[i], np.asarray(trial[r], dtype=np.float64)), inr):
            qs = q[sel]
            for a in range(len(qs)):
                for b in range(a + 1, len(qs)):
                    A, B, D = qs[a] - p, qs[b] - p, qs[b] - qs[a]
                    ra, rb, rab = np.linalg.norm(A), np.linalg.norm(B), np.linalg.norm(D)
                    c_p = A @ B / (ra * rb)
                    margin = min(margin, abs(c_p - COS_MAX), abs(rab - rc))
                    out["jik"][r] |= c_p >= COS_MAX
                    if rab < rc:
                        c_a, c_b = -(A @ D) / (ra * rab), (B @ D) / (rb * rab)
                        margin = min(margin, abs(c_a - COS_MAX), abs(c_b - COS_MAX))
                        out["ijk"][r] |= (c_a >= COS_MAX) or (c_b >= COS_MAX)
        out["margin"][r] = margin
    out["declined"] = out["cap"] | out["self"] | out["jik"] | out["ijk"]
    return out
