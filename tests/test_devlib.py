"""CPU: the loader structure.py and bondorder.py share (mc_water_ls_mw_amd/_devlib.py), driven through a stand-in library
object: one init on device 0 by default, the remembered-device rule and its message, finalize forgetting the device, the
library's own error text on a nonzero return, the not-built message, and the plan fields with `small` as a bool."""
import importlib
import types

import pytest

MODULES = [("structure", "sk", "libmw_sk.so"), ("bondorder", "boo", "libmw_boo.so")]


class StandIn:
    """What the loader needs of a library, in plain Python: mw_X_is_initialised / init / finalize / last_error."""

    def __init__(self, prefix):
        self.live, self.inits, self.fail_with = False, [], None
        for name in ("is_initialised", "init", "finalize", "last_error"):
            setattr(self, f"mw_{prefix}_{name}", getattr(self, "_" + name))

    def _is_initialised(self):
        return int(self.live)

    def _init(self, device):
        if self.fail_with:
            return 1
        self.live = True
        self.inits.append(device)
        return 0

    def _finalize(self):
        self.live = False
        return 0

    def _last_error(self):
        return (self.fail_with or "").encode()


@pytest.fixture(params=MODULES, ids=[m[0] for m in MODULES])
def devlib(request):
    """(module, its loader with a stand-in library in place, the stand-in, prefix, file name); the loader's state is put
    back afterwards."""
    modname, prefix, soname = request.param
    mod = importlib.import_module("mc_water_ls_mw_amd." + modname)
    dev = mod._dev
    saved = (dev.lib, dev.device)
    dev.lib, dev.device = StandIn(prefix), None
    yield types.SimpleNamespace(mod=mod, dev=dev, lib=dev.lib, prefix=prefix, soname=soname)
    dev.lib, dev.device = saved


def test_live_initialises_once_on_device_0_by_default(devlib):
    assert devlib.dev.live() is devlib.lib and devlib.dev.live() is devlib.lib and devlib.dev.live(0) is devlib.lib
    assert devlib.lib.inits == [0] and devlib.dev.device == 0


def test_another_device_is_refused_until_finalize(devlib):
    mod, prefix = devlib.mod, devlib.prefix
    init, finalize = getattr(mod, prefix + "_init"), getattr(mod, prefix + "_finalize")
    init(0)
    with pytest.raises(mod.MwError) as err:
        devlib.dev.live(1)
    msg = str(err.value)
    assert devlib.soname in msg and "on device 0" in msg and "on device 1" in msg and prefix + "_finalize()" in msg, msg
    with pytest.raises(mod.MwError, match="not on device 1"):
        init(1)
    assert devlib.lib.inits == [0]
    finalize()
    assert devlib.dev.device is None and not devlib.lib.live
    assert init(1) is devlib.lib and devlib.lib.inits == [0, 1] and devlib.dev.device == 1


def test_a_nonzero_return_raises_the_librarys_own_text(devlib):
    devlib.lib.fail_with = f"mw_{devlib.prefix}_init: no HIP device available (stand-in)"
    with pytest.raises(devlib.mod.MwError) as err:
        devlib.dev.live()
    assert str(err.value) == devlib.lib.fail_with
    assert devlib.dev.device is None and devlib.lib.inits == []
    devlib.dev.chk(0)                                                 # 0 is success


def test_a_library_that_is_not_built_says_how_to_build_it(devlib, tmp_path):
    devlib.dev.lib = None                                             # nothing loaded: the path is looked at
    missing = str(tmp_path / devlib.soname)
    with pytest.raises(devlib.mod.MwError) as err:
        getattr(devlib.mod, f"load_{devlib.prefix}_library")(missing)
    assert "not found: build it with" in str(err.value) and missing in str(err.value) and "no CPU fallback" in str(err.value)
    assert devlib.dev.lib is None


def test_fields_name_the_plan_fields_and_make_small_a_bool(devlib):
    names = devlib.mod.PLAN_FIELDS
    assert devlib.dev.plan_fields is names and len(devlib.dev.plan_out()) == len(names) == 9
    for small in (0, 1):
        raw = [10 + k for k in range(len(names))]
        raw[names.index("small")] = small
        d = devlib.dev.fields(raw)
        assert list(d) == list(names) and d["small"] is bool(small)
        assert all(d[n] == v and type(d[n]) is int for n, v in zip(names, raw) if n != "small")
