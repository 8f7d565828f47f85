"""icem_plan_step_mlp / icem_plan_step_mlp_ok / icem_mlp_step_launches (learned_step.hip) without a device: the three symbols are
exported, declared with the documented prototypes and bound with matching ctypes; development option ``mlp_step``; what the entry
refuses on the counts, the table and the model's own fields comes back with the documented code and a message that names the
entry, before any handle is dereferenced (the handles below are host addresses no accepted call could use); and the Python
layer's own refusals, which come before the library."""
import ctypes as C
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
    "icem_plan_step_mlp_ok": "int (const icem_handle* h, int32_t n, int32_t members)",
    "icem_plan_step_mlp": "int (icem_handle* const* handles, int32_t n, const icem_plan_buffers* buffers, const icem_mlp_step_model* model, "
                          "int32_t members, const void* const* params_host, int32_t reduce, const int32_t* mpc_steps_host, "
                          "void* member_costs, void* results, void* stream)",
    "icem_mlp_step_launches": "int64_t (const icem_handle* h)",
}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.lib_path()):
        import __graft_entry__ as g
        g.build()
    return L.load_library()


def _squash(s):
    return re.sub(r"\s+", " ", s).strip()


def test_the_header_declares_the_entries_and_the_struct():
    hdr = open(os.path.join(ROOT, "include", "icem_hip.h")).read()
    doc = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*typedef struct icem_mlp_step_model", hdr, flags=re.S)
    assert doc, "the entries carry a comment"
    for cited in ("icem_plan_step_learned_models", "member-major", "mlp_step", "ICEM_E_INVALID", "ICEM_E_UNSUPPORTED", "3 launches per iteration"):
        assert cited in doc.group(1), cited
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, sig in SIGNATURES.items():
        m = re.search(rf"^(\w+)\s+{name}\s*\(([^)]*)\)\s*;", hdr, flags=re.M)
        assert m, name
        assert _squash(f"{m.group(1)} ({_squash(m.group(2))})") == sig, name
    st = re.search(r"typedef struct icem_mlp_step_model \{(.*?)\} icem_mlp_step_model;", hdr, flags=re.S)
    assert st and _squash(st.group(1)) == "int32_t obs_dim, layers, activation; const icem_cost_spec* cost; const icem_cost_terms* terms;"
    assert re.search(r"#define ICEM_ABI_VERSION 6\b", hdr)


def test_the_library_exports_them_and_lib_binds_them(lib):
    bound = {name: (res, args) for name, res, args in L.SYMBOLS}
    VP, I32, H = C.c_void_p, C.c_int32, C.c_void_p
    kinds = {"const icem_handle*": H, "int32_t": I32, "icem_handle* const*": C.POINTER(H), "const icem_plan_buffers*": C.POINTER(L.IcemPlanBuffersC),
             "const icem_mlp_step_model*": C.POINTER(L.IcemMlpStepModelC), "const void* const*": C.POINTER(VP), "const int32_t*": C.POINTER(I32),
             "void*": VP}
    results = {"int": C.c_int, "int64_t": C.c_int64}
    for name, sig in SIGNATURES.items():
        args = [a.strip().rsplit(" ", 1)[0] for a in sig[sig.index("(") + 1:-1].split(",")]
        assert bound[name] == (results[sig.split(" ", 1)[0]], [kinds[a] for a in args]), name
        assert hasattr(lib, name), name
    assert [f[0] for f in L.IcemMlpStepModelC._fields_] == ["obs_dim", "layers", "activation", "cost", "terms"]
    assert C.sizeof(L.IcemMlpStepModelC) == 32   # three int32, padding, two pointers
    assert lib.icem_abi_version() == L.ABI_VERSION == 6   # added symbols break no caller
    if shutil.which("nm") is not None:
        exported = subprocess.check_output(["nm", "-D", "--defined-only", L.lib_path()], text=True)
        for name in SIGNATURES:
            assert re.search(rf"\bT {name}$", exported, flags=re.M), name


def test_the_option_exists_defaults_to_one_and_resets(lib):
    assert "mlp_step" in L.option_names()
    L.reset_options()
    assert L.get_option("mlp_step") == 1.0
    L.set_option("mlp_step", 0)
    assert L.get_option("mlp_step") == 0.0 and L.get_option("learned_step") == 1.0   # (a switch of its own)
    L.reset_options()
    assert L.get_option("mlp_step") == 1.0


def test_ok_and_launches_answer_zero_without_a_handle(lib):
    assert lib.icem_plan_step_mlp_ok(None, 1, 1) == 0 and lib.icem_plan_step_mlp_ok(None, 4, 5) == 0
    assert lib.icem_mlp_step_launches(None) == 0


# ---- what the entry refuses on its arguments alone ---------------------------------------------------------------------------
_dummy = (C.c_float * 4)()
P = C.addressof(_dummy)
_cost = L.IcemCostSpecC(0.1, -1.0, 10.0, 1.5, 8, 1)


def call(lib, n=1, members=2, reduce=0, handles="ok", buffers=True, table="ok", steps=True, null_entry=None, n_handles=None, model="ok",
         obs_dim=17, layers=2, activation=0, cost=True):
    k = max(n if n_handles is None else n_handles, 1)
    hs = None if handles is None else (C.c_void_p * k)(*([P + 64 * i for i in range(k)] if handles == "ok" else handles))
    bs = (L.IcemPlanBuffersC * k)() if buffers else None
    entries = max(k * max(members, 1), 1)
    tab = None if table is None else (C.c_void_p * entries)(*[None if i == null_entry else P for i in range(entries)])
    st = (C.c_int32 * k)() if steps else None
    mo = None if model is None else C.byref(L.IcemMlpStepModelC(obs_dim, layers, activation, C.pointer(_cost) if cost else None, None))
    return lib.icem_plan_step_mlp(hs, n, bs, mo, members, tab, reduce, st, None, None, None)


@pytest.mark.parametrize("kw,word", [
    (dict(handles=None), b"null argument"), (dict(buffers=False), b"null argument"), (dict(table=None), b"null argument"),
    (dict(steps=False), b"null argument"), (dict(model=None), b"null argument"), (dict(cost=False), b"null cost"),
    (dict(n=0), b"n outside"), (dict(n=-1), b"n outside"), (dict(n=33, n_handles=1), b"n outside"),
    (dict(members=0), b"members"), (dict(members=-3), b"members"), (dict(members=33), b"members"),
    (dict(reduce=2), b"reduce"), (dict(reduce=-1), b"reduce"),
    (dict(activation=2), b"activation"), (dict(activation=-1), b"activation"),
    (dict(null_entry=0), b"null params entry"), (dict(null_entry=1), b"null params entry"),
    (dict(n=2, members=3, null_entry=5), b"null params entry"),
    (dict(n=2, handles=[P, None]), b"null handle"),
    (dict(n=2, handles=[P, P]), b"the same handle twice"),
])
def test_bad_arguments_are_invalid_and_say_why(lib, kw, word):
    assert call(lib, **kw) == L.ICEM_E_INVALID
    err = lib.icem_last_error()
    assert b"icem_plan_step_mlp" in err and word in err, err


@pytest.mark.parametrize("n,members", [(3, 11), (11, 3), (2, 17), (32, 2)])
def test_more_than_32_problems_are_unsupported(lib, n, members):
    """n * members > 32 (3 x 11 = 33 among them): the rollout's table is a kernel argument.  Refused on the counts alone."""
    assert n * members > 32
    assert call(lib, n=n, members=members) == L.ICEM_E_UNSUPPORTED
    err = lib.icem_last_error()
    assert b"icem_plan_step_mlp" in err and b"32" in err and b"nothing was launched" in err, err


@pytest.mark.parametrize("kw", [dict(obs_dim=65), dict(obs_dim=0), dict(layers=5), dict(layers=0)])
def test_a_shape_outside_the_mlps_ranges_is_unsupported(lib, kw):
    assert call(lib, **kw) == L.ICEM_E_UNSUPPORTED
    err = lib.icem_last_error()
    assert b"icem_plan_step_mlp" in err and b"obs_dim" in err and b"layers" in err, err


# ---- the Python layer ----------------------------------------------------------------------------------------------------------
def _bare(kind="model", act_dim=6, obs_dim=17, activation="swish", members=2, reduce="mean"):
    from icem_amd import DeviceMLPEnsemble, DeviceMLPModel
    m = object.__new__(DeviceMLPEnsemble if kind == "ensemble" else DeviceMLPModel)
    m.obs_dim, m.act_dim, m.layers, m.activation = obs_dim, act_dim, 2, activation
    m.params = torch.zeros(4, dtype=torch.int16)
    m._cost_c, m._terms_c = _cost, None
    if kind == "ensemble":
        m.members, m.reduce = members, reduce
    return m


def test_the_planner_checks_its_models_before_the_library():
    from icem_amd import IcemPlanner
    f = IcemPlanner.plan_step_mlp
    pl = [object(), object()]   # (never looked at: the models are wrong first)
    m, ob = _bare(), np.zeros((2, 17))
    with pytest.raises(ValueError, match="2 planners but models for 1"):
        f(pl, [m], ob)
    with pytest.raises(ValueError, match="one kind for all planners"):
        f(pl, [m, _bare("ensemble")], ob)
    with pytest.raises(ValueError, match="one kind for all planners"):
        f(pl, [m, object()], ob)
    with pytest.raises(ValueError, match="one shape"):
        f(pl, [m, _bare(obs_dim=18)], ob)
    with pytest.raises(ValueError, match="one activation"):
        f(pl, [m, _bare(activation="relu")], ob)
    with pytest.raises(ValueError, match="same number"):
        f(pl, [_bare("ensemble"), _bare("ensemble", members=3)], ob)
    with pytest.raises(ValueError, match="reduce differently"):
        f(pl, [_bare("ensemble"), _bare("ensemble", reduce="max")], ob)
    with pytest.raises(ValueError, match="reduce must be"):
        f(pl, [m, m], ob, reduce="median")
    for attr in ("mlp_step_ok", "mlp_step_launches", "plan_step_mlp"):
        assert hasattr(IcemPlanner, attr), attr


def test_no_planners_is_the_entrys_own_refusal(lib):
    from icem_amd import IcemPlanner
    with pytest.raises(L.IcemError) as e:
        IcemPlanner.plan_step_mlp([], [], np.zeros((0, 17)))
    assert e.value.code == L.ICEM_E_INVALID and "icem_plan_step_mlp" in str(e.value)


def test_the_controllers_predicates_tell_the_librarys_own_models_from_instrumented_ones():
    from icem_amd import DeviceMLPEnsemble, DeviceMLPModel, MpcICemHip
    import types

    def ctrl(m):
        c = object.__new__(MpcICemHip)
        c.forward_model = m
        c.planner = types.SimpleNamespace(device=m.params.device)
        return c
    m, e = _bare(), _bare("ensemble")
    assert ctrl(m)._model_is_the_library_mlp() and not ctrl(m)._model_is_the_library_mlp_ensemble()
    assert ctrl(e)._model_is_the_library_mlp_ensemble() and not ctrl(e)._model_is_the_library_mlp()
    for c in (ctrl(m), ctrl(e)):   # (the RSSM's predicates stay false for MLP models)
        assert not c._model_is_the_library_rssm() and not c._model_is_the_library_ensemble()
    m.rollout_cost = lambda *a, **k: None             # replaced on the instance
    e.rollout_cost_batch = lambda *a, **k: None
    assert not ctrl(m)._model_is_the_library_mlp() and not ctrl(e)._model_is_the_library_mlp_ensemble()
    sub = type("Timed", (DeviceMLPModel,), dict(rollout_cost=lambda self, *a, **k: None))   # ... or on the type
    s = _bare()
    s.__class__ = sub
    assert not ctrl(s)._model_is_the_library_mlp()
    batched = type("Batched", (DeviceMLPModel,), dict(rollout_cost_batch=lambda self, *a, **k: None))
    s = _bare()
    s.__class__ = batched
    assert not ctrl(s)._model_is_the_library_mlp()
    assert not hasattr(DeviceMLPModel, "rollout_cost_batch") and hasattr(DeviceMLPEnsemble, "rollout_cost_batch")
