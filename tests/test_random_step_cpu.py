"""The random-shooting baseline's step entries (icem_plan_step_random / icem_plan_step_random_batch, random_step.hip + k_random.hip)
without a device: the five symbols are exported, declared and bound; the ABI version stays 6; the buffers struct has the header's size;
the development option that switches the entries exists and is on; argument errors are reported before any device is looked for; the
planner and the controller carry the new interface."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import pytest

from icem_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["icem_plan_step_random_ok", "icem_plan_step_random", "icem_random_step_launches", "icem_plan_step_random_batch",
       "icem_random_batch_launches"]


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
    bound = {name: (res, args) for name, res, args in L.SYMBOLS}
    for name in NEW:
        assert name in declared and name in bound and hasattr(lib, name), name
    assert re.search(r"typedef struct icem_random_buffers\s*\{", hdr)
    assert len(bound["icem_plan_step_random"][1]) == 7 and len(bound["icem_plan_step_random_batch"][1]) == 7
    m = re.search(r"int\s+icem_plan_step_random_batch\s*\(([^)]*)\)", hdr)
    assert m and len(m.group(1).split(",")) == 7
    assert lib.icem_abi_version() == L.ABI_VERSION == 6   # an added symbol breaks no caller
    exported = subprocess.check_output(["nm", "-D", "--defined-only", L.lib_path()], text=True) if shutil.which("nm") else None
    if exported is not None:
        for name in NEW:
            assert re.search(rf"\bT {name}$", exported, flags=re.M), name


def test_struct_size_and_fields():
    assert C.sizeof(L.IcemRandomBuffersC) == 7 * 8
    assert [n for n, _ in L.IcemRandomBuffersC._fields_] == ["low", "high", "obs0", "actions", "costs", "best_actions", "result"]


def test_struct_size_matches_c_compiler(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    hdr = os.path.join(ROOT, "include", "icem_hip.h")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu", '
                   'sizeof(icem_random_buffers), offsetof(icem_random_buffers, best_actions), '
                   'offsetof(icem_random_buffers, result));return 0;}' % hdr)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(L.IcemRandomBuffersC), L.IcemRandomBuffersC.best_actions.offset, L.IcemRandomBuffersC.result.offset]


def test_the_switch_is_an_option_and_on_by_default(lib):
    assert "random_step" in L.option_names()
    L.reset_options()
    assert L.get_option("random_step") == 1.0
    L.set_option("random_step", 0)
    assert L.get_option("random_step") == 0.0
    L.reset_options()
    assert L.get_option("random_step") == 1.0 and L.get_option("cem_step") == 1.0


def _buffers(**null):
    b = L.IcemRandomBuffersC(*([8] * 7))   # (never dereferenced)
    for k in null:
        setattr(b, k, None)
    return b


def test_argument_errors_need_no_device(lib):
    h = C.c_void_p(1)   # (never dereferenced: every call below fails on another argument first)
    ok = _buffers()
    assert lib.icem_plan_step_random_ok(None) == 0
    assert lib.icem_random_step_launches(None) == 0 and lib.icem_random_batch_launches(None) == 0
    assert lib.icem_plan_step_random(None, C.byref(ok), 0, 0, 0, None, None) == L.ICEM_E_INVALID
    assert lib.icem_plan_step_random(h, None, 0, 0, 0, None, None) == L.ICEM_E_INVALID
    assert b"icem_plan_step_random" in lib.icem_last_error()
    assert lib.icem_plan_step_random(h, C.byref(ok), -1, 0, 0, None, None) == L.ICEM_E_INVALID   # a negative change_freq
    assert b"change_freq" in lib.icem_last_error()
    assert lib.icem_plan_step_random(h, C.byref(ok), 0, -1, 0, None, None) == L.ICEM_E_INVALID   # a negative offset
    assert b"call_offset" in lib.icem_last_error()
    for name, _ in L.IcemRandomBuffersC._fields_:
        bad = _buffers(**{name: None})
        assert lib.icem_plan_step_random(h, C.byref(bad), 0, 0, 0, None, None) == L.ICEM_E_INVALID, name
        assert b"null buffer" in lib.icem_last_error()


def test_batch_argument_errors_need_no_device(lib):
    hs = (C.c_void_p * 33)(*([1] * 33))
    bs = (L.IcemRandomBuffersC * 33)(*[_buffers() for _ in range(33)])
    offs = (C.c_int64 * 33)(*([0] * 33))
    call = lib.icem_plan_step_random_batch
    assert call(None, 1, bs, 0, offs, None, None) == L.ICEM_E_INVALID
    assert call(hs, 1, None, 0, offs, None, None) == L.ICEM_E_INVALID
    assert call(hs, 1, bs, 0, None, None, None) == L.ICEM_E_INVALID
    assert call(hs, 0, bs, 0, offs, None, None) == L.ICEM_E_INVALID
    assert call(hs, 33, bs, 0, offs, None, None) == L.ICEM_E_INVALID
    assert b"icem_plan_step_random_batch" in lib.icem_last_error()
    assert call((C.c_void_p * 2)(1, None), 2, bs, 0, offs, None, None) == L.ICEM_E_INVALID            # a null handle
    assert call((C.c_void_p * 2)(1, 1), 2, bs, 0, offs, None, None) == L.ICEM_E_INVALID               # a handle twice
    assert b"twice" in lib.icem_last_error()
    # n == 1 reads its handle only behind the argument refusals
    assert call(hs, 1, bs, -1, offs, None, None) == L.ICEM_E_INVALID
    assert call(hs, 1, bs, 0, (C.c_int64 * 1)(-5), None, None) == L.ICEM_E_INVALID
    assert call(hs, 1, (L.IcemRandomBuffersC * 1)(_buffers(costs=None)), 0, offs, None, None) == L.ICEM_E_INVALID
    assert b"null buffer" in lib.icem_last_error()


def test_the_planner_and_the_controller_carry_the_interface():
    from icem_amd import IcemPlanner, MpcRandomHip
    for attr in ("random_step_ok", "plan_step_random", "plan_step_random_batch"):
        assert callable(getattr(IcemPlanner, attr)), attr
    assert isinstance(inspect.getattr_static(IcemPlanner, "plan_step_random_batch"), staticmethod)
    for attr in ("random_step_launches", "random_batch_launches", "random_batch_results"):
        assert isinstance(inspect.getattr_static(IcemPlanner, attr), property), attr
    assert list(inspect.signature(IcemPlanner.plan_step_random).parameters) == ["self", "obs", "call_offset", "change_freq", "u", "first_block"]
    assert list(inspect.signature(IcemPlanner.plan_step_random_batch).parameters) == ["planners", "observations", "call_offsets", "change_freq"]
    assert inspect.signature(MpcRandomHip.__init__).parameters["fused_step"].default is None
    assert isinstance(inspect.getattr_static(MpcRandomHip, "get_action_batch"), staticmethod)
    assert list(inspect.signature(MpcRandomHip.get_action_batch).parameters) == ["controllers", "observations", "states", "mode"]
    assert callable(MpcRandomHip._fused_step_refusal)
