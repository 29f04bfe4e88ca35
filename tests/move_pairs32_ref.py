"""THE F32 PAIR GATE of the move kernel's 0.99 rule (lanes_pairs32 of mw_move_lanes.hip.h, mode bit 8 of k_move_energy) restated
on the host, beside the float64 gate of tests/move_gate_ref.py.  A walking group keeps, per queue entry a,

    v = fl32(a - P),   Qo = fl32(|a - P|^2),   Qn = fl32(|a - P'|^2)        (formed in float64, rounded once; P the OLD position)

and a pair (a, b) fires when S = |v_b - v_a|^2 < rc^2 (1 + EPS) and thin(Qo_a, Qo_b, S) or thin(Qn_a, Qn_b, S), all in float32.
A request moved by more than WIDE, or with an entry nearer than TINY to either position, fires for every pair (the device hands
such a group to the float64 loop whole): inside those two bounds the float32 error of either side of `thin` is below 1e-4 QR
(the header of lanes_pairs32), against the 0.0197 max(QR, QS, RS) the gate keeps over the rule.
`fma=True` evaluates every a * b + c with ONE rounding, as the device's contracted code does: the product of two float32 is exact
in float64, the sum is rounded there and again to float32 (a double rounding that differs from a true fused multiply-add in about
one case in 2^29); `fma=False` rounds the product to float32 first.  The gate must hold in both orders."""
import numpy as np

from move_gate_ref import THIN, dist2

F = np.float32
EPS = 1e-5
WIDE2 = 256.0                                # bohr^2: |P' - P| <= 16 bohr, so every |v| component is below 32
TINY = 0.03                                  # of rc


def _fma(a, b, c, fma):
    if fma:
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)
    return (a * b).astype(F) + c


def dist2_32(d, fma):
    """dx^2 + dy^2 + dz^2 of float32 rows, in the device's order."""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return _fma(z, z, _fma(y, y, (x * x).astype(F), fma), fma)


def state(P_old, P_new, a):
    """The five float32 words of the entries `a` of requests at (P_old, P_new)."""
    return (a - P_old).astype(F), dist2(a - P_old).astype(F), dist2(a - P_new).astype(F)


def thin_sides32(Q, R, S, fma):
    """(left, right) of the inequality, float32."""
    half = F(0.5)
    th = _fma(half * np.ones_like(Q), (R - S).astype(F), (half * Q).astype(F), fma)
    QR = (Q * R).astype(F)
    left = _fma(-th, th, QR, fma)
    return left, (F(THIN) * np.maximum(np.maximum(QR, (Q * S).astype(F)), (R * S).astype(F))).astype(F)


def thin32(Q, R, S, fma):
    left, right = thin_sides32(Q, R, S, fma)
    return left <= right


def guard(P_old, P_new, a, b, rc):
    """The requests the device does not trust to float32: moved too far, or an entry too near a position."""
    tiny = (TINY * rc) ** 2
    near0 = np.minimum(np.minimum(dist2(a - P_old), dist2(a - P_new)), np.minimum(dist2(b - P_old), dist2(b - P_new))) < tiny
    return (dist2(P_new - P_old) > WIDE2) | near0


def gate32(P_old, P_new, a, b, rc, fma=True):
    """The float32 test alone, of the pair (a, b) of a request with the positions P_old and P_new."""
    va, Qo, Qn = state(P_old, P_new, a)
    vb, Ro, Rn = state(P_old, P_new, b)
    S = dist2_32((vb - va).astype(F), fma)
    near = S < F(rc * rc * (1.0 + EPS))
    return near & (thin32(Qo, Ro, S, fma) | thin32(Qn, Rn, S, fma))


def fires32(P_old, P_new, a, b, rc, fma=True):
    """What the device serves in float64: the pairs the float32 test passes, and every pair of a guarded request."""
    return gate32(P_old, P_new, a, b, rc, fma) | guard(P_old, P_new, a, b, rc)
