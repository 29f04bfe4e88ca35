"""CPU: THE F32 PAIR GATE of the move kernel (lanes_pairs32 of mw_move_lanes.hip.h; tests/move_pairs32_ref.py restates it in numpy
float32, with and without fused multiply-adds) never misses a triplet the 0.99 rule drops, and stays rare on thermal ice.

The bound: the float64 gate keeps left <= 0.5025 right for a dropped triangle (tests/test_move_gate_ref.py).  In float32, inside
the guards of the device (moved by at most 16 bohr, no entry nearer than 0.03 rc to a position), the left side moves by less than
1e-4 QR <= 1e-4 / 0.0396 = 0.0026 of the right side (the header of lanes_pairs32), so a dropped triangle has left <= 0.5051 right,
asked for here as 0.52.  Measured worst case over the sets below: 0.5025 fused and not fused, 0.017 below the bound."""
import numpy as np
import pytest

from move_gate_ref import fires, queue_pairs, rule_drops, sides
from move_lanes_ref import COS_MAX
from move_pairs32_ref import EPS, F, dist2_32, fires32, gate32, guard, state, thin_sides32
from test_move_gate_ref import ANG, VERTICES, _cosines, _rc, _triangles, _unit

ORDERS = (True, False)                       # with fused multiply-adds, and without


def _arms(rng, vertex, cos, l1, l2):
    """As test_move_gate_ref._triangles, with the two arms that meet at `vertex` given: (P, a, b)."""
    n = len(cos)
    V = rng.uniform(0.0, 60.0, (n, 3))
    u = _unit(rng, n)
    w = np.cross(u, _unit(rng, n))
    w /= np.linalg.norm(w, axis=1)[:, None]
    X = V + l1[:, None] * u
    Y = V + l2[:, None] * (cos[:, None] * u + np.sqrt(np.maximum(0.0, 1.0 - cos * cos))[:, None] * w)
    return {"P": (V, X, Y), "a": (X, V, Y), "b": (X, Y, V)}[vertex]


def _sets(rng, vertex, rc):
    """name -> (P, a, b): the constructed triangles of test_move_gate_ref.py, then |ab|^2 within +- 4 float32 ulp of rc^2 (|ab| is
    an arm where the thin vertex is a or b), then arms of 0.05 rc beside arms of up to 1.05 rc."""
    out = {name: _triangles(rng, vertex, cos, rc) for name, cos in _cosines(rng).items()}
    if vertex != "P":
        n = 9 * 1500
        ulp = float(np.spacing(F(rc * rc)))
        lab = np.sqrt(rc * rc + ulp * np.repeat(np.arange(-4, 5), 1500))
        lp = rng.uniform(0.05 * rc, 0.999 * rc, n)
        cos = rng.uniform(0.98, 1.0, n)
        # at vertex a the arms are |aP| and |ab|; at vertex b they are |bP| and |ba|
        out["|ab|^2 = rc^2 +- 4 ulp32"] = _arms(rng, vertex, cos, lp, lab)
    n = 20000
    short, long_ = np.full(n, 0.05 * rc), rng.uniform(0.9 * rc, 1.05 * rc, n)
    flip = rng.random(n) < 0.5
    out["arms 0.05 rc beside 1.05 rc"] = _arms(rng, vertex, rng.uniform(0.98, 1.0, n), np.where(flip, short, long_), np.where(flip, long_, short))
    return out


@pytest.mark.parametrize("vertex", VERTICES)
def test_the_f32_gate_misses_no_dropped_triangle(c_oracle, vertex):
    rc = _rc(c_oracle)
    rng = np.random.default_rng(1200 + VERTICES.index(vertex))
    total = dropped_total = 0
    for name, (P, a, b) in _sets(rng, vertex, rc).items():
        # the partner lane's position: the same molecule moved by up to 1.1 A; the pair must fire for a drop at EITHER of the two
        P2 = P + _unit(rng, len(P)) * rng.uniform(0.0, 1.1 * ANG, len(P))[:, None]
        drop1, drop2 = rule_drops(P, a, b, rc), rule_drops(P2, a, b, rc)
        own = ~guard(P, P2, a, b, rc)                          # (the float32 test itself is held here: a guarded request does not reach it)
        for fma in ORDERS:
            fire = gate32(P, P2, a, b, rc, fma)
            misses = int(np.sum((drop1 | drop2) & own & ~fire))
            va, Qo, _ = state(P, P2, a)
            vb, Ro, _ = state(P, P2, b)
            left, right = thin_sides32(Qo, Ro, dist2_32((vb - va).astype(F), fma), fma)
            worst = float(np.max(left[drop1 & own].astype(np.float64) / right[drop1 & own])) if (drop1 & own).any() else 0.0
            print(f"thin at {vertex}, {name}, fused {fma}: {len(P)} triangles ({int((~own).sum())} guarded), dropped {int(drop1.sum())} (+{int((drop2 & ~drop1).sum())} at "
                  f"the partner's position only), fired {int(fire.sum())}, misses {misses}, largest left/right of a dropped one {worst:.4f}")
            assert misses == 0
            assert worst <= 0.52
        if name.startswith("|ab|^2"):
            S64 = sides(P, a, b)[2]
            assert (S64 < rc * rc).sum() >= 3000 and (S64 >= rc * rc).sum() >= 3000    # both sides of the cutoff
            assert (drop1 & own).sum() >= 500                  # (dropped while inside)
        if name.startswith("arms"):
            assert (drop1 & own).sum() >= 1000
        total += len(P)
        dropped_total += int((drop1 & own).sum())
    assert total >= 120000 and dropped_total >= 30000


def test_the_f32_gate_is_rare_on_thermal_ice(c_oracle):
    """Walker 0 of the benchmark (test_move_gate_ref.py: the float64 gate fires for 9 of its 79 459 pairs).  The condition on the
    design: at most 1 pair in 1000 fires in float32, in either order of evaluation, and every pair the float64 gate or the rule
    names is among them -- the float64 loop behind the gate sees every row it needs."""
    from mc_water_ls_mw_amd import lattice as lat
    rc = _rc(c_oracle)
    h, x0 = lat.ice_box("ih", (8, 8, 8))
    x = lat.thermalise(x0, 0.15, 20250228)
    imol, trial = lat.trial_moves(x, 2048, seed=1)
    iv = c_oracle.ivects(h)
    nn, jn, vn = c_oracle.neighbours(x, iv)
    req, Po, Pn, a, b = queue_pairs(x, iv, nn, jn, vn, imol, trial, rc)
    fire64 = fires(Po, Pn, a, b, rc)
    drop = rule_drops(Po, a, b, rc) | rule_drops(Pn, a, b, rc)
    assert not guard(Po, Pn, a, b, rc).any()
    for fma in ORDERS:
        fire = fires32(Po, Pn, a, b, rc, fma)
        print(f"fused {fma}: {len(req)} pairs of {len(imol)} queues, fired in float32 {int(fire.sum())}, in float64 {int(fire64.sum())}, "
              f"dropped by the rule {int(drop.sum())}, float64 fires missed {int((fire64 & ~fire).sum())}")
        assert fire.sum() * 1000 <= len(req)
        assert not np.any(drop & ~fire)
    assert EPS < 1e-4 and COS_MAX < 0.99
