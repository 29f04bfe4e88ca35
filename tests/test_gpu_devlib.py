"""GPU: what libmw_sk.so and libmw_boo.so have in common through csrc/mw_lib_host.h and _devlib.py -- a call leaves the
caller's device current, tensors of another device than the library's are refused in Python -- and what every library on that
header's Runtime has, libmw_sk.so and the ten on the cell layer: one that was finalised and initialised again gives the same
bits and has forgotten its last call."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

NVEC = np.array([[1, 0, 0], [0, 1, 1], [-1, 2, 0]], dtype=np.int32)


@pytest.fixture(scope="module", autouse=True)
def _library_lifetime():
    """Later files find the libraries as this one found them: not initialised."""
    yield
    import importlib
    for which, module in LIBRARIES.items():
        getattr(importlib.import_module("mc_water_ls_mw_amd." + module), f"{which}_finalize")()


def _sk_call():
    """The smallest S(k) call, host pointers: 1 box x 4 molecules x 3 vectors -> (S, rho)."""
    from mc_water_ls_mw_amd.structure import structure_factor
    h = np.diag([20.0, 21.0, 22.0])
    xyz = np.array([[1.0, 2.0, 3.0], [7.5, -3.25, 11.0], [19.0, 20.5, 0.125], [4.0, 9.0, 15.5]])
    return structure_factor(h, xyz, NVEC, want_rho=True)


def _boo_call():
    """The smallest bond-order call, host pointers: the golden eight-molecule box -> (q, nn, summary)."""
    from mc_water_ls_mw_amd.bondorder import bond_order
    z = load_golden("ih8_small")
    return bond_order(z["h"], z["xyz"])


def _ice_call(which):
    """The smallest call of an analysis library, host pointers: the golden eight-molecule box at 3.5 Angstrom."""
    from mc_water_ls_mw_amd.angles import angle_counts
    from mc_water_ls_mw_amd.rings import ring_statistics
    from mc_water_ls_mw_amd.tetrahedral import tetrahedral_order
    z = load_golden("ih8_small")
    return {"tet": lambda: tetrahedral_order(z["h"], z["xyz"], 3.5, 3.5), "adf": lambda: angle_counts(z["h"], z["xyz"], 3.5),
            "rings": lambda: ring_statistics(z["h"], z["xyz"], 3.5)}[which]()


def _gas_call(which):
    """A single point of a force library, host pointers: the golden dense gas of 20 molecules."""
    from mc_water_ls_mw_amd.dynamics import molecular_dynamics
    from mc_water_ls_mw_amd.einstein import einstein_md
    from mc_water_ls_mw_amd.flexcell import molecular_dynamics_flex
    from mc_water_ls_mw_amd.npt import molecular_dynamics_npt
    from mc_water_ls_mw_amd.phonons import hessian
    from mc_water_ls_mw_amd.quench import inherent_structures
    z = load_golden("gas20")
    h, xyz = z["h"], z["xyz"]
    return {"quench": lambda: inherent_structures(h, xyz, 1e-10, 0), "md": lambda: molecular_dynamics(h, xyz, 0, 200.0),
            "npt": lambda: molecular_dynamics_npt(h, xyz, 0, 200.0, baro_every=0), "flex": lambda: molecular_dynamics_flex(h, xyz, 0, 200.0, baro_every=0),
            "hess": lambda: hessian(h, xyz), "ti": lambda: einstein_md(h, xyz + 0.05, 0.3, 0.02, 0, 200.0, pos=xyz)}[which]()


#: the library's name in its symbols -> its module
LIBRARIES = {"sk": "structure", "boo": "bondorder", "tet": "tetrahedral", "adf": "angles", "rings": "rings", "quench": "quench", "md": "dynamics",
             "npt": "npt", "flex": "flexcell", "hess": "phonons", "ti": "einstein"}


def _same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _two_devices():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip(f"needs two devices, this machine shows {torch.cuda.device_count()}")
    return torch


def test_calls_leave_the_callers_device_current():
    torch = _two_devices()
    from mc_water_ls_mw_amd.bondorder import boo_init, boo_last
    from mc_water_ls_mw_amd.structure import sk_elapsed_ms, sk_init, sk_last, sk_plan
    sk_init(0)
    boo_init(0)
    before = torch.cuda.current_device()
    try:
        torch.cuda.set_device(0)
        sk0, boo0, last0 = _sk_call(), _boo_call(), (sk_last(), boo_last())
        torch.cuda.set_device(1)
        sk1, boo1 = _sk_call(), _boo_call()
        assert torch.cuda.current_device() == 1
        assert sk_plan(4, (1, 2, 1), 3, 1) == sk_last() and (sk_last(), boo_last()) == last0 and len(sk_elapsed_ms()) == 2
        assert torch.cuda.current_device() == 1
    finally:
        torch.cuda.set_device(before)
    assert _same(sk0, sk1) and _same(boo0, boo1)


def test_tensors_of_another_device_are_refused():
    torch = _two_devices()
    from mc_water_ls_mw_amd.bondorder import MwError, bond_order_torch, boo_init, boo_last
    from mc_water_ls_mw_amd.structure import sk_init, sk_last, structure_factor_torch
    sk_init(0)
    boo_init(0)
    _sk_call(), _boo_call()
    last = sk_last(), boo_last()
    z = load_golden("ic48")                                          # another shape than the last call's: a launch would show
    other = torch.device("cuda:1")
    cells = torch.from_numpy(np.ascontiguousarray(z["h"][None])).to(other)
    pos = torch.from_numpy(np.ascontiguousarray(z["xyz"][None])).to(other)
    with pytest.raises(MwError, match=r"libmw_sk\.so is initialised on device 0, not on device 1"):
        structure_factor_torch(cells, pos, torch.from_numpy(NVEC).to(other))
    with pytest.raises(MwError, match=r"libmw_boo\.so is initialised on device 0, not on device 1"):
        bond_order_torch(cells, pos)
    assert (sk_last(), boo_last()) == last


@pytest.mark.parametrize("which", list(LIBRARIES))
def test_finalize_then_init_again(which):
    import importlib
    mod = importlib.import_module("mc_water_ls_mw_amd." + LIBRARIES[which])
    call = {"sk": _sk_call, "boo": _boo_call}.get(which) or (lambda: (_ice_call if which in ("tet", "adf", "rings") else _gas_call)(which))
    init, finalize, last = (getattr(mod, f"{which}_{name}") for name in ("init", "finalize", "last"))
    L = getattr(mod, f"load_{which}_library")()
    is_live = getattr(L, f"mw_{which}_is_initialised")
    finalize()
    init(0)
    first, plan = call(), last()
    finalize()
    assert not is_live()
    init(0)
    assert is_live()
    with pytest.raises(mod.MwError, match=f"mw_{which}_last: no call has launched yet"):
        last()
    assert _same(first, call()) and last() == plan
