"""THE GATE of the move kernel's 0.99 rule (mw_move_lanes.hip.h, mode bit 7 of k_move_energy) restated on the host, beside the rule
it gates.  For a pair (a, b) of queue entries and a position P, with Q = |Pa|^2, R = |Pb|^2, S = |ab|^2 and t = Q + R - S,

    thin(Q, R, S):   QR - (t/2)^2  <=  (1 - 0.98^2) max(QR, QS, RS)

(the left side is 4 Area^2 of the triangle P a b, and sin^2 of the angle at a vertex is 4 Area^2 over the product of the two squared
sides that meet there), and the pair FIRES when S < rc^2 and it is thin at the old or at the trial position.  `thin` is written in
float64 in the device's order of operations; the device contracts `a * b + c` into one rounding where numpy makes two, which moves
a side of the inequality by parts in 1e-16 of QR -- the margin the gate keeps over the rule is 0.0197 max(QR, QS, RS).
`rule_drops` is the rule itself as move_lanes_ref.predict words it, in long double: both entries in range of P, and the cosine at P
at least 0.99 - 1e-9, or |ab| < rc and the cosine at a or at b at least 0.99 - 1e-9."""
import numpy as np

from move_lanes_ref import COS_MAX

KAPPA_GATE = 0.98
THIN = 1.0 - 0.98 * 0.98


def dist2(d):
    """dx^2 + dy^2 + dz^2 of the rows of `d`, in the device's order."""
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def sides(P, a, b):
    """(Q, R, S) of the triangles P a b (arrays of shape (..., 3)), float64."""
    return dist2(a - P), dist2(b - P), dist2(b - a)


def thin_sides(Q, R, S):
    """(left, right) of the inequality."""
    th = 0.5 * (R - S) + 0.5 * Q
    QR = Q * R
    return QR - th * th, THIN * np.maximum(np.maximum(QR, Q * S), R * S)


def thin(Q, R, S):
    left, right = thin_sides(Q, R, S)
    return left <= right


def fires(P_old, P_new, a, b, rc):
    """The gate of the pair (a, b) of a request with the positions P_old and P_new."""
    Q, R, S = sides(P_old, a, b)
    Qt, Rt, _ = sides(P_new, a, b)
    return (S < rc * rc) & (thin(Q, R, S) | thin(Qt, Rt, S))


def rule_drops(P, a, b, rc):
    """The 0.99 rule at ONE position, long double: does the reference drop a triplet of P, a, b that the moment path sums?"""
    L = np.longdouble
    P, a, b = (np.asarray(v, dtype=L) for v in (P, a, b))
    A, B, D = a - P, b - P, b - a
    ra, rb, rab = (np.sqrt((v * v).sum(axis=-1)) for v in (A, B, D))
    with np.errstate(invalid="ignore", divide="ignore"):
        c_p = (A * B).sum(axis=-1) / (ra * rb)
        c_a = -(A * D).sum(axis=-1) / (ra * rab)
        c_b = (B * D).sum(axis=-1) / (rb * rab)
    cmax, rcl = L(COS_MAX), L(rc)
    return (ra < rcl) & (rb < rcl) & ((c_p >= cmax) | ((rab < rcl) & ((c_a >= cmax) | (c_b >= cmax))))


def queue_pairs(x, iv, nn, jn, vn, imol, trial, rc):
    """Every pair (a < b) of every request's queue -- the row entries in range of the old or the trial position, in row order --
    as arrays (request, P_old, P_new, a, b)."""
    req, Po, Pn, qa, qb = [], [], [], [], []
    for r, i1 in enumerate(imol):
        i = int(i1) - 1
        n = int(nn[i])
        q = x[jn[i, :n] - 1] + iv[vn[i, :n] - 1]
        inr = (np.sqrt(dist2(q - x[i])) < rc) | (np.sqrt(dist2(q - trial[r])) < rc)
        q = q[inr]
        ia, ib = np.triu_indices(len(q), 1)
        req.append(np.full(len(ia), r)); qa.append(q[ia]); qb.append(q[ib])
        Po.append(np.broadcast_to(x[i], (len(ia), 3))); Pn.append(np.broadcast_to(trial[r], (len(ia), 3)))
    return tuple(np.concatenate(v) for v in (req, Po, Pn, qa, qb))
