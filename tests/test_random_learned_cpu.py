"""The random-shooting step's learned-dynamics entries (icem_plan_step_random_learned / icem_plan_step_random_learned_batch,
random_step.hip + k_random_learned.hip) without a device: the three symbols are declared with the issue's signatures, exported and
bound; the ABI version stays 6; argument errors are reported before any device is looked for; the planner and the controller carry the
new interface."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import pytest

from icem_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {
    "icem_plan_step_random_learned_ok": "int (const icem_handle* h)",
    "icem_plan_step_random_learned": "int (icem_handle* h, const icem_random_buffers* b, const void* params, int32_t change_freq, "
                                     "int64_t call_offset, void* stream)",
    "icem_plan_step_random_learned_batch": "int (icem_handle* const* handles, int32_t n, const icem_random_buffers* buffers, "
                                           "const void* params, int32_t change_freq, const int64_t* call_offsets_host, void* results, "
                                           "void* stream)",
}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.lib_path()):
        import __graft_entry__ as g
        g.build()
    return L.load_library()


def _squash(s):
    return re.sub(r"\s+", " ", s).strip()


def test_the_header_declares_the_entries_with_these_signatures():
    hdr = open(os.path.join(ROOT, "include", "icem_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, sig in SIGNATURES.items():
        m = re.search(rf"^(\w+)\s+{name}\s*\(([^)]*)\)\s*;", hdr, flags=re.M)
        assert m, name
        assert _squash(f"{m.group(1)} ({_squash(m.group(2))})") == sig, name


def test_the_library_exports_them_and_lib_binds_them(lib):
    bound = {name: (res, args) for name, res, args in L.SYMBOLS}
    for name in SIGNATURES:
        assert name in bound and hasattr(lib, name), name
        assert bound[name][0] is C.c_int
    VP, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
    assert bound["icem_plan_step_random_learned_ok"][1] == [VP]
    assert bound["icem_plan_step_random_learned"][1] == [VP, C.POINTER(L.IcemRandomBuffersC), VP, I32, I64, VP]
    assert bound["icem_plan_step_random_learned_batch"][1] == [C.POINTER(VP), I32, C.POINTER(L.IcemRandomBuffersC), VP, I32, C.POINTER(I64), VP, VP]
    assert lib.icem_abi_version() == L.ABI_VERSION == 6   # an added symbol breaks no caller
    if shutil.which("nm") is not None:
        exported = subprocess.check_output(["nm", "-D", "--defined-only", L.lib_path()], text=True)
        for name in SIGNATURES:
            assert re.search(rf"\bT {name}$", exported, flags=re.M), name


def _buffers(**null):
    b = L.IcemRandomBuffersC(*([8] * 7))   # (never dereferenced)
    for k in null:
        setattr(b, k, None)
    return b


def test_argument_errors_need_no_device(lib):
    h, prm = C.c_void_p(1), C.c_void_p(8)   # (never dereferenced: every call below fails on another argument first)
    ok = _buffers()
    call = lib.icem_plan_step_random_learned
    assert lib.icem_plan_step_random_learned_ok(None) == 0
    assert call(None, C.byref(ok), prm, 0, 0, None) == L.ICEM_E_INVALID
    assert call(h, None, prm, 0, 0, None) == L.ICEM_E_INVALID
    assert call(h, C.byref(ok), None, 0, 0, None) == L.ICEM_E_INVALID
    assert b"icem_plan_step_random_learned" in lib.icem_last_error()
    assert call(h, C.byref(ok), prm, -1, 0, None) == L.ICEM_E_INVALID   # a negative change_freq
    assert b"change_freq" in lib.icem_last_error()
    assert call(h, C.byref(ok), prm, 0, -1, None) == L.ICEM_E_INVALID   # a negative offset
    assert b"call_offset" in lib.icem_last_error()
    for name, _ in L.IcemRandomBuffersC._fields_:
        bad = _buffers(**{name: None})
        assert call(h, C.byref(bad), prm, 0, 0, None) == L.ICEM_E_INVALID, name
        assert b"null buffer" in lib.icem_last_error()


def test_batch_argument_errors_need_no_device(lib):
    hs = (C.c_void_p * 33)(*([1] * 33))
    bs = (L.IcemRandomBuffersC * 33)(*[_buffers() for _ in range(33)])
    offs = (C.c_int64 * 33)(*([0] * 33))
    prm = C.c_void_p(8)
    call = lib.icem_plan_step_random_learned_batch
    assert call(None, 1, bs, prm, 0, offs, None, None) == L.ICEM_E_INVALID
    assert call(hs, 1, None, prm, 0, offs, None, None) == L.ICEM_E_INVALID
    assert call(hs, 1, bs, None, 0, offs, None, None) == L.ICEM_E_INVALID
    assert call(hs, 1, bs, prm, 0, None, None, None) == L.ICEM_E_INVALID
    assert call(hs, 0, bs, prm, 0, offs, None, None) == L.ICEM_E_INVALID
    assert call(hs, 33, bs, prm, 0, offs, None, None) == L.ICEM_E_INVALID
    assert b"icem_plan_step_random_learned_batch" in lib.icem_last_error()
    assert call((C.c_void_p * 2)(1, None), 2, bs, prm, 0, offs, None, None) == L.ICEM_E_INVALID   # a null handle
    assert call((C.c_void_p * 2)(1, 1), 2, bs, prm, 0, offs, None, None) == L.ICEM_E_INVALID      # a handle twice
    assert b"twice" in lib.icem_last_error()
    # n == 1 reads its handle only behind the argument refusals
    assert call(hs, 1, bs, prm, -1, offs, None, None) == L.ICEM_E_INVALID
    assert call(hs, 1, bs, prm, 0, (C.c_int64 * 1)(-5), None, None) == L.ICEM_E_INVALID
    assert call(hs, 1, (L.IcemRandomBuffersC * 1)(_buffers(costs=None)), prm, 0, offs, None, None) == L.ICEM_E_INVALID
    assert b"null buffer" in lib.icem_last_error()


def test_the_planner_and_the_controller_carry_the_interface():
    from icem_amd import IcemPlanner, MpcRandomHip
    for attr in ("random_learned_step_ok", "plan_step_random_learned", "plan_step_random_learned_batch"):
        assert callable(getattr(IcemPlanner, attr)), attr
    assert isinstance(inspect.getattr_static(IcemPlanner, "plan_step_random_learned_batch"), staticmethod)
    assert list(inspect.signature(IcemPlanner.plan_step_random_learned).parameters) == ["self", "model", "obs", "call_offset", "change_freq"]
    assert list(inspect.signature(IcemPlanner.plan_step_random_learned_batch).parameters) == ["planners", "model", "observations", "call_offsets",
                                                                                              "change_freq"]
    assert callable(MpcRandomHip._steps_through_the_rssm) and callable(MpcRandomHip._model_is_the_library_rssm)
    assert "icem_plan_step_random_learned" in MpcRandomHip._fused_step_refusal.__doc__


def test_the_new_kernels_have_a_unit_of_their_own():
    from icem_amd import build as B
    assert "k_random_learned.hip" in B.UNITS and os.path.exists(os.path.join(B.CSRC, "k_random_learned.hip"))
    assert os.path.exists(os.path.join(B.CSRC, "random_dev.h"))
