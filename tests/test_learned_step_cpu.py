"""The learned-dynamics step's entries (icem_plan_step_learned*, learned_step.hip) without a device: the four symbols are
exported, declared and bound; the development option that switches them exists and is on; argument errors are reported
before any device is looked for."""
import ctypes as C
import os
import re

import pytest

from icem_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["icem_plan_step_learned_ok", "icem_plan_step_learned", "icem_plan_step_learned_batch", "icem_learned_step_launches"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.lib_path()):
        import __graft_entry__ as g
        g.build()
    return L.load_library()


def test_symbols_are_exported_declared_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "icem_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(icem_[a-z_0-9]+)\s*\(", hdr))
    bound = {name for name, _, _ in L.SYMBOLS}
    for name in NEW:
        assert name in declared and name in bound and hasattr(lib, name), name
    assert re.search(r"#define\s+ICEM_RSSM_OBS_DIM\s+230\b", hdr) and L.RSSM_OBS_DIM == 230
    assert lib.icem_abi_version() == 6   # an added symbol breaks no caller


def test_the_switch_is_an_option_and_on_by_default(lib):
    assert "learned_step" in L.option_names()
    L.reset_options()
    assert L.get_option("learned_step") == 1.0
    L.set_option("learned_step", 0)
    assert L.get_option("learned_step") == 0.0
    L.reset_options()


def test_argument_errors_need_no_device(lib):
    h = C.c_void_p(1)   # (never dereferenced: every call below fails on another argument first)
    cb = L.IcemPlanBuffersC()
    hs = (C.c_void_p * 1)(h)
    steps = (C.c_int32 * 1)(0)
    params = C.c_void_p(16)
    assert lib.icem_plan_step_learned_ok(None) == 0
    assert lib.icem_learned_step_launches(None) == 0
    assert lib.icem_plan_step_learned(None, C.byref(cb), params, 0, None) == L.ICEM_E_INVALID
    assert lib.icem_plan_step_learned(h, None, params, 0, None) == L.ICEM_E_INVALID
    assert lib.icem_plan_step_learned(h, C.byref(cb), None, 0, None) == L.ICEM_E_INVALID
    assert lib.icem_plan_step_learned_batch(None, 1, C.byref(cb), params, steps, None, None) == L.ICEM_E_INVALID
    assert lib.icem_plan_step_learned_batch(hs, 1, None, params, steps, None, None) == L.ICEM_E_INVALID
    assert lib.icem_plan_step_learned_batch(hs, 1, C.byref(cb), None, steps, None, None) == L.ICEM_E_INVALID
    for n in (0, -1, 33):
        assert lib.icem_plan_step_learned_batch(hs, n, C.byref(cb), params, steps, None, None) == L.ICEM_E_INVALID, n
    null = (C.c_void_p * 2)(None, None)
    assert lib.icem_plan_step_learned_batch(null, 2, (L.IcemPlanBuffersC * 2)(), params, (C.c_int32 * 2)(0, 0), None, None) == L.ICEM_E_INVALID
    assert b"learned" in lib.icem_last_error()
