"""icem_plan_step_cem_learned_models / icem_plan_step_random_learned_models and their *_ok queries (cem_step.hip, random_step.hip)
without a device: the four symbols are exported, declared with the documented prototypes and bound with matching ctypes; what the
entries refuse on their arguments alone comes back with the documented code and a message before any handle is dereferenced (the
handles below are host addresses no accepted call could use), as tests/test_learned_models_cpu.py holds their sibling; the planner's
methods exist and make their own refusals before the library; the controllers' entry for models of their own exists."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from icem_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {
    "icem_plan_step_cem_learned_models_ok": "int (const icem_handle* h, int32_t n, int32_t members)",
    "icem_plan_step_cem_learned_models": "int (icem_handle* const* handles, int32_t n, const icem_cem_buffers* buffers, "
                                         "const icem_cem_params* p, int32_t members, const void* const* params_host, int32_t reduce, "
                                         "const int32_t* mpc_steps_host, void* member_costs, void* results, void* stream)",
    "icem_plan_step_random_learned_models_ok": "int (const icem_handle* h, int32_t n, int32_t members)",
    "icem_plan_step_random_learned_models": "int (icem_handle* const* handles, int32_t n, const icem_random_buffers* buffers, "
                                            "int32_t members, const void* const* params_host, int32_t reduce, int32_t change_freq, "
                                            "const int64_t* call_offsets_host, void* member_costs, void* results, void* stream)",
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
    doc = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int icem_plan_step_cem_learned_models_ok", hdr, flags=re.S)
    assert doc, "the entries carry a comment"
    for cited in ("member-major", "3 launches", "icem_cem_batch_launches", "icem_random_batch_launches", "ICEM_E_INVALID",
                  "ICEM_E_UNSUPPORTED", "ICEM_E_STATE", "cem_update_members_batch_kernel", "random_select_members_batch_kernel"):
        assert cited in doc.group(1), cited
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, sig in SIGNATURES.items():
        m = re.search(rf"^(\w+)\s+{name}\s*\(([^)]*)\)\s*;", hdr, flags=re.M)
        assert m, name
        assert _squash(f"{m.group(1)} ({_squash(m.group(2))})") == sig, name


def test_the_library_exports_them_and_lib_binds_them(lib):
    bound = {name: (res, args) for name, res, args in L.SYMBOLS}
    VP, I32, I64, H = C.c_void_p, C.c_int32, C.c_int64, C.c_void_p
    kinds = {"const icem_handle*": H, "int32_t": I32, "icem_handle* const*": C.POINTER(H), "const icem_cem_buffers*": C.POINTER(L.IcemCemBuffersC),
             "const icem_cem_params*": C.POINTER(L.IcemCemParamsC), "const icem_random_buffers*": C.POINTER(L.IcemRandomBuffersC),
             "const void* const*": C.POINTER(VP), "const int32_t*": C.POINTER(I32), "const int64_t*": C.POINTER(I64), "void*": VP}
    for name, sig in SIGNATURES.items():
        args = [a.strip().rsplit(" ", 1)[0] for a in sig[sig.index("(") + 1:-1].split(",")]
        assert bound[name] == (C.c_int, [kinds[a] for a in args]), name
        assert hasattr(lib, name), name
    assert lib.icem_abi_version() == L.ABI_VERSION == 6   # added symbols break no caller
    if shutil.which("nm") is not None:
        exported = subprocess.check_output(["nm", "-D", "--defined-only", L.lib_path()], text=True)
        for name in SIGNATURES:
            assert re.search(rf"\bT {name}$", exported, flags=re.M), name


# ---- what the entries refuse on their arguments alone --------------------------------------------------------------------------
_dummy = (C.c_float * 4)()
P = C.addressof(_dummy)


def call(lib, which, n=1, members=2, reduce=0, handles="ok", buffers=True, table="ok", steps=True, flags=True, null_entry=None, n_handles=None):
    k = max(n if n_handles is None else n_handles, 1)
    hs = None if handles is None else (C.c_void_p * k)(*([P + 64 * i for i in range(k)] if handles == "ok" else handles))
    entries = max(k * max(members, 1), 1)
    tab = None if table is None else (C.c_void_p * entries)(*[None if i == null_entry else P for i in range(entries)])
    if which == "cem":
        bs = (L.IcemCemBuffersC * k)() if buffers else None
        prm = L.IcemCemParamsC(0, 1, 1, 0)
        st = (C.c_int32 * k)() if steps else None
        return lib.icem_plan_step_cem_learned_models(hs, n, bs, C.byref(prm) if flags else None, members, tab, reduce, st, None, None, None)
    bs = (L.IcemRandomBuffersC * k)() if buffers else None
    st = (C.c_int64 * k)() if steps else None
    return lib.icem_plan_step_random_learned_models(hs, n, bs, members, tab, reduce, 1, st, None, None, None)


BAD = [
    (dict(handles=None), b"null argument"), (dict(buffers=False), b"null argument"), (dict(table=None), b"null argument"),
    (dict(steps=False), b"null argument"), (dict(flags=False), b"null argument"),
    (dict(n=0), b"n outside"), (dict(n=-1), b"n outside"), (dict(n=33, n_handles=1), b"n outside"),
    (dict(members=0), b"members"), (dict(members=-3), b"members"), (dict(members=33), b"members"),
    (dict(reduce=2), b"reduce"), (dict(reduce=-1), b"reduce"),
    (dict(null_entry=0), b"null params entry"), (dict(null_entry=1), b"null params entry"),
    (dict(n=2, members=3, null_entry=5), b"null params entry"),
    (dict(n=2, handles=[P, None]), b"null handle"),
    (dict(n=2, handles=[P, P]), b"the same handle twice"),
]


# (the random-shooting step has no flags block)
@pytest.mark.parametrize("which,kw,word", [(w, kw, word) for w in ("cem", "random") for kw, word in BAD if not (w == "random" and "flags" in kw)])
def test_bad_arguments_are_invalid_and_say_why(lib, which, kw, word):
    assert call(lib, which, **kw) == L.ICEM_E_INVALID
    err = lib.icem_last_error()
    assert (b"icem_plan_step_cem_learned_models" if which == "cem" else b"icem_plan_step_random_learned_models") in err and word in err, err


@pytest.mark.parametrize("which", ["cem", "random"])
@pytest.mark.parametrize("n,members", [(2, 17), (11, 3), (32, 2)])
def test_more_than_32_problems_are_unsupported(lib, which, n, members):
    """n * members > 32: the rollout's table is a kernel argument.  Refused on the counts alone, before a handle is looked at."""
    assert call(lib, which, n=n, members=members) == L.ICEM_E_UNSUPPORTED
    assert b"32" in lib.icem_last_error() and b"nothing was launched" in lib.icem_last_error()


def test_ok_answers_zero_without_a_handle(lib):
    for f in (lib.icem_plan_step_cem_learned_models_ok, lib.icem_plan_step_random_learned_models_ok):
        assert f(None, 1, 1) == 0 and f(None, 4, 5) == 0


# ---- the Python layer ----------------------------------------------------------------------------------------------------------
def _bare_model(act_dim=6):
    from icem_amd import DeviceRSSMModel
    m = object.__new__(DeviceRSSMModel)
    m.act_dim = act_dim
    m.params = torch.zeros(4, dtype=torch.int16)
    return m


def test_the_planner_methods_exist_with_the_documented_arguments():
    from icem_amd import IcemPlanner
    assert list(inspect.signature(IcemPlanner.cem_learned_models_step_ok).parameters) == ["self", "n", "members"]
    assert list(inspect.signature(IcemPlanner.random_learned_models_step_ok).parameters) == ["self", "n", "members"]
    cem = inspect.signature(IcemPlanner.plan_step_cem_learned_models).parameters
    assert list(cem) == ["planners", "models", "observations", "dists", "like_levine", "shift_means", "execute_best_elite", "reduce", "member_costs"]
    assert all(cem[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(cem)[4:]) and cem["reduce"].default is None
    rnd = inspect.signature(IcemPlanner.plan_step_random_learned_models).parameters
    assert list(rnd) == ["planners", "models", "observations", "call_offsets", "change_freq", "reduce", "member_costs"]
    assert rnd["reduce"].default is None and rnd["member_costs"].default is None


def test_the_planner_checks_its_models_before_the_library():
    from icem_amd import IcemPlanner
    pl = [object(), object()]   # (never looked at: the models are wrong first)
    m = _bare_model()
    flags = dict(like_levine=False, shift_means=True, execute_best_elite=True)
    for f in (lambda models, **kw: IcemPlanner.plan_step_cem_learned_models(pl, models, np.zeros((2, 230)), [None, None], **flags, **kw),
              lambda models, **kw: IcemPlanner.plan_step_random_learned_models(pl, models, np.zeros((2, 230)), [0, 0], 1, **kw)):
        with pytest.raises(ValueError, match="2 planners but models for 1"):
            f([m])
        with pytest.raises(ValueError, match="same number"):
            f([[m, m], [m]])
        with pytest.raises(ValueError, match="are DeviceRSSMModels"):
            f([[m], [object()]])
        with pytest.raises(ValueError, match="one action width"):
            f([m, _bare_model(2)])
        with pytest.raises(ValueError, match="reduce must be"):
            f([m, m], reduce="median")


def test_an_ensemble_each_names_its_own_stacked_parameters():
    from icem_amd import DeviceRSSMEnsemble, DeviceRSSMModel, IcemPlanner
    ms = [DeviceRSSMModel(seed=s, device="cpu", act_dim=2) for s in (3, 4, 5)]
    a, b = DeviceRSSMEnsemble(models=ms[:2], reduce="max"), DeviceRSSMEnsemble(models=ms[1:], reduce="max")
    ens, table, width_of, reduce = IcemPlanner._models_table([a, b], 2, None, "x")
    assert ens is None and table == [a._param_ptrs(), b._param_ptrs()] and width_of.act_dim == 2 and reduce == "max"
    with pytest.raises(ValueError, match="reduce differently"):
        IcemPlanner._models_table([a, DeviceRSSMEnsemble(models=ms[1:], reduce="mean")], 2, None, "x")
    with pytest.raises(ValueError, match="same number"):
        IcemPlanner._models_table([a, DeviceRSSMEnsemble(models=ms, reduce="max")], 2, None, "x")
    ens, table, _, reduce = IcemPlanner._models_table(a, 3, None, "x")   # one ensemble for all: its pointers per problem
    assert ens is a and table == [a._param_ptrs()] * 3 and reduce == "max"


def test_no_planners_is_the_entrys_own_refusal(lib):
    from icem_amd import IcemPlanner
    with pytest.raises(L.IcemError) as e:
        IcemPlanner.plan_step_cem_learned_models([], [], [], [], like_levine=False, shift_means=True, execute_best_elite=True)
    assert e.value.code == L.ICEM_E_INVALID
    with pytest.raises(L.IcemError) as e:
        IcemPlanner.plan_step_random_learned_models([], [], [], [], 1)
    assert e.value.code == L.ICEM_E_INVALID


def test_the_baselines_step_controllers_with_models_of_their_own():
    """``own_models`` is a keyword on ``MpcICemHip.get_action_batch``; the baselines, whose ``get_action_batch`` keeps its four
    parameters, offer it as ``get_action_batch_own_models`` with the same four."""
    from icem_amd import MpcCemStdHip, MpcICemHip, MpcRandomHip
    assert inspect.signature(MpcICemHip.get_action_batch).parameters["own_models"].default is False
    for cls in (MpcCemStdHip, MpcRandomHip):
        assert isinstance(inspect.getattr_static(cls, "get_action_batch_own_models"), staticmethod)
        assert list(inspect.signature(cls.get_action_batch_own_models).parameters) == list(inspect.signature(cls.get_action_batch).parameters)
        assert inspect.signature(cls._batch_refusal).parameters["own_models"].default is False
