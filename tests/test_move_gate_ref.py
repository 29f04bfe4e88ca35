"""CPU: THE GATE in front of the move kernel's 0.99 rule (mw_move_lanes.hip.h; tests/move_gate_ref.py restates both) never misses
a triplet the rule drops, and on thermal ice it is rare where |ab| < rc is not.

The bound: a dropped triplet has cos >= 0.99 - 1e-9 at a vertex, so sin^2 <= 0.0199000020 there and the gate's left side, 4 Area^2,
is at most 0.0199000020 max(QR, QS, RS) where its right side is 0.0396 max(QR, QS, RS): a factor 0.5025, asked for here as
left <= 0.51 right -- the other 0.0075 is far above the float64 rounding of either side (parts in 1e-16 of QR)."""
import numpy as np
import pytest

from move_gate_ref import fires, queue_pairs, rule_drops, sides, thin_sides
from move_lanes_ref import COS_MAX

ANG = 1.0 / 0.5291772108
VERTICES = ("P", "a", "b")


def _rc(oracle):
    c = oracle.constants()
    return c[0] * c[6]


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def _triangles(rng, vertex, cos, rc):
    """One triangle per entry of `cos`, thin at `vertex` with that cosine there: arms of 0.05 rc to 1.05 rc, any orientation,
    somewhere in a 60-bohr box.  Returns (P, a, b)."""
    n = len(cos)
    V = rng.uniform(0.0, 60.0, (n, 3))
    u = _unit(rng, n)
    w = np.cross(u, _unit(rng, n))
    w /= np.linalg.norm(w, axis=1)[:, None]
    l1, l2 = rng.uniform(0.05 * rc, 1.05 * rc, (2, n))
    X = V + l1[:, None] * u
    Y = V + l2[:, None] * (cos[:, None] * u + np.sqrt(np.maximum(0.0, 1.0 - cos * cos))[:, None] * w)
    return {"P": (V, X, Y), "a": (X, V, Y), "b": (X, Y, V)}[vertex]


def _cosines(rng):
    ulp = np.spacing(COS_MAX)
    edge = COS_MAX + ulp * np.repeat(np.arange(-4, 5), 1500)
    return {"0.98 to 1": rng.uniform(0.98, 1.0, 120000), "COS_MAX +- 4 ulp": edge, "collinear": np.ones(6000)}


@pytest.mark.parametrize("vertex", VERTICES)
def test_the_gate_misses_no_dropped_triangle(c_oracle, vertex):
    rc = _rc(c_oracle)
    rng = np.random.default_rng(1100 + VERTICES.index(vertex))
    total = dropped_total = 0
    for name, cos in _cosines(rng).items():
        P, a, b = _triangles(rng, vertex, cos, rc)
        # the partner lane's position: the same molecule moved by up to 1.1 A, and the pair must fire for a drop at EITHER of the two
        P2 = P + _unit(rng, len(P)) * rng.uniform(0.0, 1.1 * ANG, len(P))[:, None]
        drop1, drop2 = rule_drops(P, a, b, rc), rule_drops(P2, a, b, rc)
        fire = fires(P, P2, a, b, rc)
        swapped = fires(P2, P, a, b, rc)
        misses = int(np.sum((drop1 | drop2) & ~fire))
        left, right = thin_sides(*sides(P, a, b))
        worst = float(np.max(left[drop1] / right[drop1])) if drop1.any() else 0.0
        print(f"thin at {vertex}, cos {name}: {len(cos)} triangles, dropped {int(drop1.sum())} (+{int((drop2 & ~drop1).sum())} at the "
              f"partner's position only), fired {int(fire.sum())}, misses {misses}, largest left/right of a dropped one {worst:.4f}")
        assert misses == 0
        assert np.array_equal(fire, swapped)                  # (the two lanes of a pair agree)
        assert worst <= 0.51
        if name == "0.98 to 1":
            assert drop1.sum() >= 20000 and (~drop1).sum() >= 20000
            assert (drop2 & ~drop1).sum() >= 1                # (hard at the other position only: it happens in this set)
        if name == "COS_MAX +- 4 ulp":
            assert 0 < drop1.sum()                            # (both sides of the threshold where the arms are in range; rounding decides)
        if name == "collinear":
            inr = (np.linalg.norm(a - P, axis=1) < rc) & (np.linalg.norm(b - P, axis=1) < rc)
            if vertex == "P":                                 # (cos = 1 at P: dropped exactly where both arms are in range)
                assert np.array_equal(drop1, inr) and fire[inr].all()
            assert drop1.sum() >= len(cos) // 2
        total += len(cos)
        dropped_total += int(drop1.sum())
    assert total >= 100000 and dropped_total >= 30000


def test_the_gate_is_rare_on_thermal_ice(c_oracle):
    """Walker 0 of the benchmark: 2048 trial moves of a thermal 4096-molecule ice Ih box.  About 18 700 of its queues' pairs have
    |ab| < rc -- nearly a quarter; the gate fires for 9 of them (measured), asked here: fewer than 1 %.  Every pair the rule drops at
    either position is among them."""
    from mc_water_ls_mw_amd import lattice as lat
    rc = _rc(c_oracle)
    h, x0 = lat.ice_box("ih", (8, 8, 8))
    x = lat.thermalise(x0, 0.15, 20250228)
    imol, trial = lat.trial_moves(x, 2048, seed=1)
    iv = c_oracle.ivects(h)
    nn, jn, vn = c_oracle.neighbours(x, iv)
    req, Po, Pn, a, b = queue_pairs(x, iv, nn, jn, vn, imol, trial, rc)
    near = sides(Po, a, b)[2] < rc * rc
    fire = fires(Po, Pn, a, b, rc)
    drop = rule_drops(Po, a, b, rc) | rule_drops(Pn, a, b, rc)
    print(f"{len(req)} pairs of {len(imol)} queues ({len(req) / len(imol):.1f} per request), |ab| < rc: {int(near.sum())} "
          f"({near.mean():.3f}), fired {int(fire.sum())}, dropped by the rule {int(drop.sum())}, requests with a firing pair "
          f"{len(set(req[fire]))}")
    assert 15000 <= near.sum() <= 22000
    assert fire.sum() < 0.01 * near.sum()
    assert not np.any(fire & ~near) and not np.any(drop & ~fire)
