"""``icem_plan_step_cem_batch`` / ``icem_cem_batch_launches`` -- the CEM baseline's MPC step for B planners in one call -- are
declared in ``include/icem_hip.h``, exported by the built library and bound in ``icem_amd/_lib.py``; the wrappers
``IcemPlanner.plan_step_cem_batch`` and ``MpcCemStdHip.get_action_batch`` exist.  No device compute here: the bits are held
by tests/test_gpu_cem_batch.py."""
import inspect
import os
import re

import pytest

from icem_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("icem_plan_step_cem_batch", "icem_cem_batch_launches")


@pytest.fixture(scope="module")
def lib():
    from icem_amd import build as B
    if B.build_info()["stale"]:
        import __graft_entry__ as g
        g.build()
    return L.load_library()


def test_the_batch_entry_is_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "icem_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(icem_[a-z_0-9]+)\s*\(", hdr))
    bound = {name: (res, args) for name, res, args in L.SYMBOLS}
    for name in NEW:
        assert name in declared and name in bound and hasattr(lib, name), name
    # handles, n, buffers, params, mpc_steps_host, results, stream
    res, args = bound["icem_plan_step_cem_batch"]
    assert len(args) == 7 and len(bound["icem_cem_batch_launches"][1]) == 1
    m = re.search(r"int\s+icem_plan_step_cem_batch\s*\(([^)]*)\)", hdr)
    assert m and len(m.group(1).split(",")) == 7
    # no handle: the launch count is 0, the entry an argument error (nothing is touched without a device either)
    assert lib.icem_cem_batch_launches(None) == 0
    assert lib.icem_plan_step_cem_batch(None, 0, None, None, None, None, None) == L.ICEM_E_INVALID
    assert b"icem_plan_step_cem_batch" in lib.icem_last_error()


def test_nothing_an_existing_test_pins_has_moved(lib):
    assert lib.icem_abi_version() == L.ABI_VERSION == 6
    assert "cem_step" in L.option_names()


def test_the_wrappers_exist():
    from icem_amd import IcemPlanner, MpcCemStdHip
    sig = inspect.signature(IcemPlanner.plan_step_cem_batch)
    assert list(sig.parameters)[:3] == ["planners", "observations", "dists"]
    for kw in ("like_levine", "shift_means", "execute_best_elite"):
        assert sig.parameters[kw].kind is inspect.Parameter.KEYWORD_ONLY
    assert isinstance(inspect.getattr_static(IcemPlanner, "plan_step_cem_batch"), staticmethod)
    sig = inspect.signature(MpcCemStdHip.get_action_batch)
    assert list(sig.parameters) == ["controllers", "observations", "states", "mode"]
    assert isinstance(inspect.getattr_static(MpcCemStdHip, "get_action_batch"), staticmethod)
    assert isinstance(inspect.getattr_static(IcemPlanner, "cem_batch_launches"), property)
