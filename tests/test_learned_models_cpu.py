"""icem_plan_step_learned_models / icem_plan_step_learned_models_ok (learned_step.hip) without a device: the two symbols are
exported, declared with the documented prototypes and bound with matching ctypes; what the entry refuses on its arguments
alone comes back with the documented code and a message, before any handle is dereferenced (the handles below are host
addresses no accepted call could use); the Python layer's own refusals, which come before the library; and the predicate that
tells the library's own ensemble from an instrumented one."""
import ctypes as C
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

from icem_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {
    "icem_plan_step_learned_models_ok": "int (const icem_handle* h, int32_t n, int32_t members)",
    "icem_plan_step_learned_models": "int (icem_handle* const* handles, int32_t n, const icem_plan_buffers* buffers, int32_t members, "
                                     "const void* const* params_host, int32_t reduce, const int32_t* mpc_steps_host, void* member_costs, "
                                     "void* results, void* stream)",
}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.lib_path()):
        import __graft_entry__ as g
        g.build()
    return L.load_library()


def _squash(s):
    return re.sub(r"\s+", " ", s).strip()


def test_the_header_declares_the_entries():
    hdr = open(os.path.join(ROOT, "include", "icem_hip.h")).read()
    doc = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int icem_plan_step_learned_models_ok", hdr, flags=re.S)
    assert doc, "the entries carry a comment"
    for cited in ("abstract_models.py:17-53", "rollout_utils.py:46-58, 129-152", "member-major", "e * stride + row0 + i",
                  "ICEM_E_INVALID", "ICEM_E_UNSUPPORTED", "ICEM_E_STATE"):
        assert cited in doc.group(1), cited
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, sig in SIGNATURES.items():
        m = re.search(rf"^(\w+)\s+{name}\s*\(([^)]*)\)\s*;", hdr, flags=re.M)
        assert m, name
        assert _squash(f"{m.group(1)} ({_squash(m.group(2))})") == sig, name


def test_the_library_exports_them_and_lib_binds_them(lib):
    bound = {name: (res, args) for name, res, args in L.SYMBOLS}
    VP, I32, H = C.c_void_p, C.c_int32, C.c_void_p
    assert bound["icem_plan_step_learned_models_ok"] == (C.c_int, [H, I32, I32])
    assert bound["icem_plan_step_learned_models"] == (C.c_int, [C.POINTER(H), I32, C.POINTER(L.IcemPlanBuffersC), I32, C.POINTER(VP), I32,
                                                               C.POINTER(I32), VP, VP, VP])
    # the ctypes of _lib.py against the header's prototype, argument by argument
    kinds = {"const icem_handle*": H, "int32_t": I32, "icem_handle* const*": C.POINTER(H), "const icem_plan_buffers*": C.POINTER(L.IcemPlanBuffersC),
             "const void* const*": C.POINTER(VP), "const int32_t*": C.POINTER(I32), "void*": VP}
    for name, sig in SIGNATURES.items():
        args = [a.strip().rsplit(" ", 1)[0] for a in sig[sig.index("(") + 1:-1].split(",")]
        assert [kinds[a] for a in args] == bound[name][1], name
    assert lib.icem_abi_version() == L.ABI_VERSION == 6   # added symbols break no caller
    for name in SIGNATURES:
        assert hasattr(lib, name), name
    if shutil.which("nm") is not None:
        exported = subprocess.check_output(["nm", "-D", "--defined-only", L.lib_path()], text=True)
        for name in SIGNATURES:
            assert re.search(rf"\bT {name}$", exported, flags=re.M), name


# ---- what the entry refuses on its arguments alone ---------------------------------------------------------------------------
_dummy = (C.c_float * 4)()
P = C.addressof(_dummy)


def call(lib, n=1, members=2, reduce=0, handles="ok", buffers=True, table="ok", steps=True, null_entry=None, n_handles=None):
    k = max(n if n_handles is None else n_handles, 1)
    hs = None if handles is None else (C.c_void_p * k)(*([P + 64 * i for i in range(k)] if handles == "ok" else handles))
    bs = (L.IcemPlanBuffersC * k)() if buffers else None
    entries = max(k * max(members, 1), 1)
    tab = None if table is None else (C.c_void_p * entries)(*[None if i == null_entry else P for i in range(entries)])
    st = (C.c_int32 * k)() if steps else None
    return lib.icem_plan_step_learned_models(hs, n, bs, members, tab, reduce, st, None, None, None)


@pytest.mark.parametrize("kw,word", [
    (dict(handles=None), b"null argument"), (dict(buffers=False), b"null argument"), (dict(table=None), b"null argument"),
    (dict(steps=False), b"null argument"),
    (dict(n=0), b"n outside"), (dict(n=-1), b"n outside"), (dict(n=33, n_handles=1), b"n outside"),
    (dict(members=0), b"members"), (dict(members=-3), b"members"), (dict(members=33), b"members"),
    (dict(reduce=2), b"reduce"), (dict(reduce=-1), b"reduce"),
    (dict(null_entry=0), b"null params entry"), (dict(null_entry=1), b"null params entry"),
    (dict(n=2, members=3, null_entry=5), b"null params entry"),
    (dict(n=2, handles=[P, None]), b"null handle"),
    (dict(n=2, handles=[P, P]), b"the same handle twice"),
])
def test_bad_arguments_are_invalid_and_say_why(lib, kw, word):
    assert call(lib, **kw) == L.ICEM_E_INVALID
    err = lib.icem_last_error()
    assert b"icem_plan_step_learned_models" in err and word in err, err


@pytest.mark.parametrize("n,members", [(2, 17), (3, 11), (11, 3), (32, 2), (5, 7)])
def test_more_than_32_problems_are_unsupported(lib, n, members):
    """n * members > 32: the rollout's table is a kernel argument.  Refused on the counts alone, before a handle is looked at."""
    assert n * members > 32
    assert call(lib, n=n, members=members) == L.ICEM_E_UNSUPPORTED
    assert b"32" in lib.icem_last_error() and b"nothing was launched" in lib.icem_last_error()


def test_ok_answers_zero_without_a_handle_or_outside_the_counts(lib):
    assert lib.icem_plan_step_learned_models_ok(None, 1, 1) == 0
    assert lib.icem_plan_step_learned_models_ok(None, 4, 5) == 0


# ---- the Python layer ----------------------------------------------------------------------------------------------------------
def _bare_model(act_dim=6):
    from icem_amd import DeviceRSSMModel
    m = object.__new__(DeviceRSSMModel)
    m.act_dim = act_dim
    m.params = torch.zeros(4, dtype=torch.int16)
    return m


def test_the_planner_checks_its_models_before_the_library():
    from icem_amd import IcemPlanner
    f = IcemPlanner.plan_step_learned_models
    pl = [object(), object()]   # (never looked at: the models are wrong first)
    m = _bare_model()
    with pytest.raises(ValueError, match="2 planners but models for 1"):
        f(pl, [m], np.zeros((2, 230)))
    with pytest.raises(ValueError, match="same number"):
        f(pl, [[m, m], [m]], np.zeros((2, 230)))
    with pytest.raises(ValueError, match="same number"):
        f(pl, [[], []], np.zeros((2, 230)))
    with pytest.raises(ValueError, match="are DeviceRSSMModels"):
        f(pl, [[m], [object()]], np.zeros((2, 230)))
    with pytest.raises(ValueError, match="one action width"):
        f(pl, [m, _bare_model(2)], np.zeros((2, 230)))
    with pytest.raises(ValueError, match="reduce must be"):
        f(pl, [m, m], np.zeros((2, 230)), reduce="median")
    assert callable(IcemPlanner.learned_models_step_ok)


def test_no_planners_is_the_entrys_own_refusal(lib):
    from icem_amd import IcemPlanner
    with pytest.raises(L.IcemError) as e:
        IcemPlanner.plan_step_learned_models([], [], [])
    assert e.value.code == L.ICEM_E_INVALID


def _holder(model, device="cpu"):
    from icem_amd import MpcICemHip
    c = object.__new__(MpcICemHip)
    c.forward_model = model
    c.planner = types.SimpleNamespace(device=torch.device(device))
    return c


def test_the_predicate_knows_the_librarys_own_ensemble(lib):
    """True for a plain DeviceRSSMEnsemble; false once rollout_cost or rollout_cost_batch is replaced on the instance or in a
    subclass, for a plain model, and for an ensemble on another device than the planner's.  _model_is_the_library_rssm stays
    false for every ensemble."""
    from icem_amd import DeviceRSSMEnsemble, DeviceRSSMModel
    ms = [DeviceRSSMModel(seed=s, device="cpu", act_dim=2) for s in (3, 4)]
    e = DeviceRSSMEnsemble(models=ms)
    c = _holder(e)
    assert c._model_is_the_library_ensemble() is True and c._model_is_the_library_rssm() is False
    assert _holder(e, device="meta")._model_is_the_library_ensemble() is False
    assert _holder(ms[0])._model_is_the_library_ensemble() is False and _holder(ms[0])._model_is_the_library_rssm() is True
    for name in ("rollout_cost", "rollout_cost_batch"):
        inst = DeviceRSSMEnsemble(models=ms)
        inner = getattr(inst, name)
        setattr(inst, name, lambda *a, _f=inner, **k: _f(*a, **k))
        assert _holder(inst)._model_is_the_library_ensemble() is False, name

        class Sub(DeviceRSSMEnsemble):
            pass
        setattr(Sub, name, lambda self, *a, **k: None)
        assert _holder(Sub(models=ms))._model_is_the_library_ensemble() is False, name

    class Plain(DeviceRSSMEnsemble):
        pass
    assert _holder(Plain(models=ms))._model_is_the_library_ensemble() is True   # (a subclass that replaces neither)


def test_controllers_that_are_not_served_say_so_without_a_device(lib):
    """_learned_models_ok: false on the device path, with external noise, verbose, or with a model that is neither the library's
    ensemble nor its RSSM -- decided before the library is asked."""
    from icem_amd import DeviceRSSMEnsemble, DeviceRSSMModel
    e = DeviceRSSMEnsemble(models=[DeviceRSSMModel(seed=3, device="cpu", act_dim=2)])
    c = _holder(e)
    c.planner.cfg = types.SimpleNamespace(world=1)
    c.rssm_path, c.device_path, c.verbose = True, False, False
    assert c._learned_models_ok(lambda n: None, 1) is False      # external noise
    c.verbose = True
    assert c._learned_models_ok(None, 1) is False
    c.verbose, c.device_path = False, True
    assert c._learned_models_ok(None, 1) is False
    c.device_path = False
    e.rollout_cost = lambda *a, **k: None                         # instrumented
    assert c._learned_models_ok(None, 1) is False
