"""icem_mlp_rollout_cost_models / icem_mlp_rollout_cost_ensemble (abi.hip, k_mlp_rollout.hip) and their Python side without a
device: the entries and the struct in the header, the exports and icem_amd._lib; what the entries refuse before any HIP call
(ICEM_E_INVALID / ICEM_E_UNSUPPORTED with a message; the pointers handed over are host addresses no accepted call could use);
the Python wrappers' own checks, which come before the library."""
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
    "icem_mlp_rollout_cost_models": "int (int32_t n_problems, const icem_mlp_problem* problems_host, int32_t horizon, int32_t obs_dim, "
                                    "int32_t act_dim, int32_t layers, int32_t activation, int32_t cost_mode, const icem_cost_spec* cost, "
                                    "const icem_cost_terms* terms, const void* obs0, int32_t n_obs, const void* actions, "
                                    "int64_t n_action_rows, void* costs, void* observations, void* stream)",
    "icem_mlp_rollout_cost_ensemble": "int (int32_t members, const void* const* params_host, int32_t n, int32_t horizon, int32_t obs_dim, "
                                      "int32_t act_dim, int32_t layers, int32_t activation, int32_t cost_mode, int32_t reduce, "
                                      "const icem_cost_spec* cost, const icem_cost_terms* terms, const void* obs0, const void* actions, "
                                      "void* member_costs, void* costs, void* stream)",
}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.lib_path()):
        import __graft_entry__ as g
        g.build()
    return L.load_library()


def _squash(s):
    return re.sub(r"\s+,", ",", re.sub(r"\s+", " ", s)).strip()   # (a parameter's own comment, once stripped, leaves a blank)


def test_the_header_declares_the_entries_and_the_struct():
    hdr = open(os.path.join(ROOT, "include", "icem_hip.h")).read()
    for name in SIGNATURES:
        doc = re.search(rf"/\*((?:(?!\*/).)*?)\*/\s*(?:#define ICEM_MLP_MAX_PROBLEMS 32\s*typedef struct icem_mlp_problem \{{.*?\}} icem_mlp_problem;\s*)?"
                        rf"int {name}\b", hdr, flags=re.S)
        assert doc, f"{name} carries a comment"
        for cited in ("bit for bit", "ICEM_E_INVALID", "before anything is launched"):
            assert cited in doc.group(1), (name, cited)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, sig in SIGNATURES.items():
        m = re.search(rf"^(\w+)\s+{name}\s*\(([^)]*)\)\s*;", hdr, flags=re.M)
        assert m, name
        assert _squash(f"{m.group(1)} ({_squash(m.group(2))})") == sig, name
    m = re.search(r"typedef struct icem_mlp_problem \{(.*?)\} icem_mlp_problem;", hdr, flags=re.S)
    assert m and _squash(m.group(1)) == "const void* params; int64_t action_row0; int32_t rows; int32_t obs_row;"
    assert re.search(r"#define ICEM_MLP_MAX_PROBLEMS 32\b", hdr)


def test_the_library_exports_them_and_lib_binds_them(lib):
    bound = {name: (res, args) for name, res, args in L.SYMBOLS}
    VP, I32, I64 = C.c_void_p, C.c_int32, C.c_int64
    cost, terms = C.POINTER(L.IcemCostSpecC), C.POINTER(L.IcemCostTermsC)
    assert bound["icem_mlp_rollout_cost_models"] == (C.c_int, [I32, C.POINTER(L.IcemMlpProblemC), I32, I32, I32, I32, I32, I32, cost, terms,
                                                               VP, I32, VP, I64, VP, VP, VP])
    assert bound["icem_mlp_rollout_cost_ensemble"] == (C.c_int, [I32, C.POINTER(VP), I32, I32, I32, I32, I32, I32, I32, I32, cost, terms,
                                                                 VP, VP, VP, VP, VP])
    for name in SIGNATURES:
        assert hasattr(lib, name), name
    assert L.MLP_MAX_PROBLEMS == 32
    assert lib.icem_abi_version() == L.ABI_VERSION == 6   # added symbols break no caller
    if shutil.which("nm") is not None:
        exported = subprocess.check_output(["nm", "-D", "--defined-only", L.lib_path()], text=True)
        for name in SIGNATURES:
            assert re.search(rf"\bT {name}$", exported, flags=re.M), name


def test_the_struct_is_the_c_compilers(tmp_path):
    assert C.sizeof(L.IcemMlpProblemC) == 24
    assert [(n, getattr(L.IcemMlpProblemC, n).offset) for n, _ in L.IcemMlpProblemC._fields_] == [
        ("params", 0), ("action_row0", 8), ("rows", 16), ("obs_row", 20)]
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler in this image")
    hdr = os.path.join(ROOT, "include", "icem_hip.h")
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu %%zu %%d", '
                   'sizeof(icem_mlp_problem), offsetof(icem_mlp_problem, params), offsetof(icem_mlp_problem, action_row0), '
                   'offsetof(icem_mlp_problem, rows), offsetof(icem_mlp_problem, obs_row), ICEM_MLP_MAX_PROBLEMS);return 0;}' % hdr)
    exe = tmp_path / "s"
    subprocess.check_call([cc, str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)], text=True).split() == [str(C.sizeof(L.IcemMlpProblemC)), "0", "8", "16", "20", "32"]


# ---- what the entries refuse, on host addresses ------------------------------------------------------------------------------
_dummy = (C.c_float * 4)()
P = C.c_void_p(C.addressof(_dummy))
GOOD = (P.value, 0, 5, 0)


def _terms(**kw):
    t = L.IcemCostTermsC(diff_idx=-1, health_idx=-1, box_from=-1)
    terms = kw.pop("terms", ())
    for k, v in kw.items():
        setattr(t, k, v)
    t.n_terms = kw.get("n_terms", len(terms))
    for j, tm in enumerate(terms):
        t.terms[j] = L.IcemCostTermC(**dict(dict(weight=1.0, kind=0, a=0, b=-1, len=1, gate_idx=-1), **tm))
    return t


def _spec(cost_kw=None):
    return L.IcemCostSpecC(**dict(dict(ctrl_weight=0.1, lin_weight=-1.0, flip_penalty=10.0, flip_thresh=1.5, lin_idx=8, flip_idx=1),
                                  **(cost_kw or {})))


def models(lib, problems=(GOOD, GOOD), h=12, o=17, d=6, layers=2, act=0, mode=0, terms=None, cost_kw=None, n_obs=4, n_action_rows=100,
           n_problems=None, null=None):
    """rc of icem_mlp_rollout_cost_models; problems: [(params, action_row0, rows, obs_row)]; ``null``: the NULL argument."""
    arr = (L.IcemMlpProblemC * max(len(problems), 1))(*[L.IcemMlpProblemC(*p) for p in problems])
    ptr = {k: (None if null == k else P) for k in ("obs0", "actions", "costs")}
    spec = _spec(cost_kw)
    n = len(problems) if n_problems is None else n_problems
    return lib.icem_mlp_rollout_cost_models(n, None if null == "problems" else arr, h, o, d, layers, act, mode,
                                            None if null == "cost" else C.byref(spec), None if terms is None else C.byref(terms),
                                            ptr["obs0"], n_obs, ptr["actions"], n_action_rows, ptr["costs"], None, None)


def ensemble(lib, members=2, n=16, h=12, o=17, d=6, layers=2, act=0, mode=0, reduce=0, terms=None, cost_kw=None, null=None,
             null_member=None):
    ptrs = (C.c_void_p * max(members, 1))(*[None if e == null_member else P.value for e in range(max(members, 1))])
    ptr = {k: (None if null == k else P) for k in ("obs0", "actions", "member_costs", "costs")}
    spec = _spec(cost_kw)
    return lib.icem_mlp_rollout_cost_ensemble(members, None if null == "params" else ptrs, n, h, o, d, layers, act, mode, reduce,
                                              None if null == "cost" else C.byref(spec), None if terms is None else C.byref(terms),
                                              ptr["obs0"], ptr["actions"], ptr["member_costs"], ptr["costs"], None)


@pytest.mark.parametrize("null", ["problems", "cost", "obs0", "actions", "costs"])
def test_models_null_pointer(lib, null):
    assert models(lib, null=null) == L.ICEM_E_INVALID
    assert b"icem_mlp_rollout_cost_models" in lib.icem_last_error() and b"null" in lib.icem_last_error()


# what icem_mlp_rollout_cost calls invalid about the modes and the cost pair (test_mlp_cpu.py's list), for both entries
COST_PAIR = [
    (dict(mode=3), b"cost_mode"), (dict(mode=-1), b"cost_mode"),
    (dict(act=2), b"activation"), (dict(act=-1), b"activation"),
    (dict(cost_kw=dict(lin_idx=17)), b"cost index outside the observation"), (dict(cost_kw=dict(lin_idx=-1)), b"cost index outside the observation"),
    (dict(cost_kw=dict(flip_idx=17)), b"cost index outside the observation"),
    (dict(o=8), b"cost index outside the observation"),
    (dict(terms=_terms(n_terms=9)), b"n_terms must be in [0, 8]"), (dict(terms=_terms(n_terms=-1)), b"n_terms must be in [0, 8]"),
    (dict(terms=_terms(terms=[dict(kind=6)])), b"unknown cost term kind"),
    (dict(terms=_terms(terms=[dict(len=0)])), b"cost term len"), (dict(terms=_terms(terms=[dict(len=65)])), b"cost term len"),
    (dict(terms=_terms(box_from=2)), b"box_from"),
    (dict(terms=_terms(diff_idx=17)), b"cost term index outside the observation"),
    (dict(terms=_terms(health_idx=17)), b"cost term index outside the observation"),
    (dict(terms=_terms(health_idx=1, box_from=17)), b"cost term index outside the observation"),
    (dict(terms=_terms(terms=[dict(a=15, len=3)])), b"cost term slice outside the observation"),
    (dict(terms=_terms(terms=[dict(a=-1)])), b"cost term slice outside the observation"),
    (dict(terms=_terms(terms=[dict(gate_idx=17)])), b"cost term slice outside the observation"),
]
UNSUPPORTED = [
    (dict(o=0, cost_kw=dict(lin_idx=0, flip_idx=-1)), b"obs_dim"), (dict(o=65), b"obs_dim"),
    (dict(d=0), b"act_dim"), (dict(d=33), b"act_dim"),
    (dict(layers=0), b"layers"), (dict(layers=5), b"layers"),
    (dict(h=0), b"horizon"), (dict(h=65), b"horizon"), (dict(h=-1), b"horizon"),
]


@pytest.mark.parametrize("kw,word", [
    (dict(problems=[], n_problems=0), b"n_problems"),
    (dict(problems=[GOOD], n_problems=-1), b"n_problems"),
    (dict(problems=[GOOD] * 33), b"n_problems"),
    (dict(problems=[GOOD, (None, 0, 5, 0)]), b"params"),
    (dict(problems=[GOOD, (P.value, 0, 0, 0)]), b"row"),
    (dict(problems=[GOOD, (P.value, 0, -3, 0)]), b"row"),
    (dict(problems=[GOOD, (P.value, -1, 5, 0)]), b"action_row0"),
    (dict(problems=[GOOD, (P.value, 96, 5, 0)]), b"action_row0"),
    (dict(problems=[GOOD, (P.value, 2 ** 40, 5, 0)]), b"action_row0"),
    (dict(problems=[GOOD, (P.value, 2 ** 63 - 1, 5, 0)]), b"action_row0"),
    (dict(problems=[GOOD], n_action_rows=4), b"action_row0"),
    (dict(problems=[GOOD, (P.value, 0, 5, 4)]), b"obs_row"),
    (dict(problems=[GOOD, (P.value, 0, 5, -1)]), b"obs_row"),
    (dict(problems=[GOOD], n_obs=0), b"obs_row"),
] + COST_PAIR)
def test_models_bad_arguments_are_invalid_and_say_why(lib, kw, word):
    assert models(lib, **kw) == L.ICEM_E_INVALID
    err = lib.icem_last_error()
    assert b"icem_mlp_rollout_cost_models: " in err and word in err, err


@pytest.mark.parametrize("kw,word", UNSUPPORTED)
def test_models_shapes_outside_the_compiled_ranges_are_unsupported(lib, kw, word):
    assert models(lib, **kw) == L.ICEM_E_UNSUPPORTED
    err = lib.icem_last_error()
    assert b"icem_mlp_rollout_cost_models: " in err and word in err, err


def test_the_last_rows_there_are_may_be_named(lib):
    """Rows 95 .. 99 of 100 and the last observation pass the row checks: what is refused is what comes after them."""
    assert models(lib, [(P.value, 95, 5, 3)], h=0) == L.ICEM_E_UNSUPPORTED and b"horizon" in lib.icem_last_error()
    assert models(lib, [(P.value, 0, 100, 3)] * 32, h=0) == L.ICEM_E_UNSUPPORTED and b"horizon" in lib.icem_last_error()


@pytest.mark.parametrize("kw,word", [
    (dict(null="params"), b"null"), (dict(null="cost"), b"null"), (dict(null="obs0"), b"null"), (dict(null="actions"), b"null"),
    (dict(null="member_costs"), b"null"), (dict(null="costs"), b"null"),
    (dict(null_member=1), b"params"),
    (dict(members=0), b"members"), (dict(members=33), b"members"), (dict(members=-2), b"members"),
    (dict(n=0), b"row"), (dict(n=-5), b"row"),
    (dict(reduce=2), b"reduce"), (dict(reduce=-1), b"reduce"),
] + COST_PAIR)
def test_ensemble_bad_arguments_are_invalid_and_say_why(lib, kw, word):
    assert ensemble(lib, **kw) == L.ICEM_E_INVALID
    err = lib.icem_last_error()
    assert b"icem_mlp_rollout_cost_ensemble: " in err and word in err, err


@pytest.mark.parametrize("kw,word", UNSUPPORTED)
def test_ensemble_shapes_outside_the_compiled_ranges_are_unsupported(lib, kw, word):
    assert ensemble(lib, **kw) == L.ICEM_E_UNSUPPORTED
    err = lib.icem_last_error()
    assert b"icem_mlp_rollout_cost_ensemble: " in err and word in err, err


def test_the_solo_entrys_messages_are_its_own(lib):
    """The shared argument check names the entry that was called."""
    spec = _spec()
    assert lib.icem_mlp_rollout_cost(16, 12, 17, 6, 2, 0, 3, C.byref(spec), None, P, P, P, P, None, None) == L.ICEM_E_INVALID
    assert lib.icem_last_error() == b"icem_mlp_rollout_cost: bad cost_mode"
    assert lib.icem_mlp_rollout_cost(16, 65, 17, 6, 2, 0, 0, C.byref(spec), None, P, P, P, P, None, None) == L.ICEM_E_UNSUPPORTED
    assert lib.icem_last_error() == b"icem_mlp_rollout_cost: horizon must be in [1, 64]"


# ---- the Python layer ----------------------------------------------------------------------------------------------------------
def test_the_names_are_exported_and_the_ensemble_is_a_sibling():
    import icem_amd
    from icem_amd import DeviceMLPEnsemble, DeviceMLPModel, DeviceRSSMEnsemble, mlp_rollout_cost_models
    from icem_amd.models import ForwardModel
    assert icem_amd.DeviceMLPEnsemble is DeviceMLPEnsemble and callable(mlp_rollout_cost_models)
    assert issubclass(DeviceMLPEnsemble, ForwardModel)
    assert not issubclass(DeviceMLPEnsemble, DeviceRSSMEnsemble) and not issubclass(DeviceMLPEnsemble, DeviceMLPModel)
    assert not hasattr(DeviceMLPModel, "rollout_cost_batch")   # controllers that step together share a DeviceMLPEnsemble
    assert hasattr(DeviceMLPEnsemble, "rollout_cost_batch") and hasattr(DeviceMLPEnsemble, "rollout_cost")
    assert "no batched launch" not in DeviceMLPModel.__doc__ and "DeviceMLPEnsemble" in DeviceMLPModel.__doc__


def _spec_py(**kw):
    from icem_amd import CostSpec
    return CostSpec(0.1, 8, -1.0, 1, 10.0, kw.get("flip_thresh", 0.7))


_cache = {}


def _model(o=17, d=6, layers=1, activation="relu", seed=0, **kw):
    """A DeviceMLPModel on the host (packing needs no device)."""
    from icem_amd import DeviceMLPModel
    key = (o, d, layers, activation, seed, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = DeviceMLPModel(o, d, layers=layers, activation=activation, seed=seed, cost_spec=_spec_py(**kw), device="cpu")
    return _cache[key]


def test_the_wrapper_checks_models_and_shapes_before_the_library(lib):
    from icem_amd import mlp_rollout_cost_models as f
    m, acts = _model(), torch.zeros((5, 3, 6))
    ob2 = np.zeros((2, 17))
    with pytest.raises(ValueError, match="1 to 32 problems"):
        f([], np.zeros((0, 17)), acts, [])
    with pytest.raises(ValueError, match="1 to 32 problems"):
        f([m] * 33, np.zeros((33, 17)), acts, [1] * 33)
    with pytest.raises(ValueError, match="one shape"):
        f([m, _model(o=18)], ob2, acts, [2, 3])
    with pytest.raises(ValueError, match="one shape"):
        f([m, _model(d=5)], ob2, acts, [2, 3])
    with pytest.raises(ValueError, match="one shape"):
        f([m, _model(layers=2)], ob2, acts, [2, 3])
    with pytest.raises(ValueError, match="one activation"):
        f([m, _model(activation="swish")], ob2, acts, [2, 3])
    with pytest.raises(ValueError, match="one cost program"):
        f([m, _model(flip_thresh=0.8)], ob2, acts, [2, 3])
    with pytest.raises(ValueError, match="2 problems but 3 row counts"):
        f([m, m], ob2, acts, [2, 2, 1])
    with pytest.raises(ValueError, match="rows sum to 6"):
        f([m, m], ob2, acts, [2, 4])
    with pytest.raises(ValueError, match="at least one row"):
        f([m, m], ob2, acts, [5, 0])
    with pytest.raises(ValueError, match="actions must be"):
        f([m, m], ob2, torch.zeros((5, 3, 5)), [2, 3])
    with pytest.raises(ValueError, match=r"observations must be \[2, 17\]"):
        f([m, m], np.zeros((2, 230)), acts, [2, 3])
    with pytest.raises(ValueError, match="observations must be"):
        f([m, m], np.zeros((3, 17)), acts, [2, 3])
    with pytest.raises(ValueError, match="first action rows"):
        f([m, m], ob2, acts, [2, 3], action_row0=[0])
    with pytest.raises(ValueError, match="outside actions' 5 rows"):
        f([m, m], ob2, acts, [5, 5], action_row0=[0, 1])
    with pytest.raises(ValueError, match="outside actions' 5 rows"):
        f([m, m], ob2, acts, [2, 3], action_row0=[-1, 0])


def test_the_rssm_callers_shape_check_is_unchanged():
    from icem_amd.models import _check_problem_shapes as chk
    rows, row0, ob = chk(6, 2, np.zeros((2, 230)), torch.zeros((5, 3, 6)), [2, 3], None)
    assert (rows, row0, ob.shape, ob.dtype) == ([2, 3], [0, 2], (2, 230), np.float32)
    with pytest.raises(ValueError, match=r"observations must be \[2, 230\]"):
        chk(6, 2, np.zeros((2, 17)), torch.zeros((5, 3, 6)), [2, 3], None)
    assert chk(6, 2, np.zeros((2, 17)), torch.zeros((5, 3, 6)), [2, 3], [1, 2], 17)[1] == [1, 2]


def test_the_ensemble_checks_its_members_and_shapes(lib):
    from icem_amd import DeviceMLPEnsemble as E
    kw = dict(obs_dim=17, act_dim=6, layers=1, cost_spec=_spec_py(), device="cpu")
    with pytest.raises(ValueError, match="reduce must be"):
        E(seeds=[1], reduce="median", **kw)
    with pytest.raises(ValueError, match="either models"):
        E()
    with pytest.raises(ValueError, match="either models"):
        E(models=[_model()], seeds=[1])
    with pytest.raises(ValueError, match="1 to 32 members"):
        E(models=[])
    with pytest.raises(ValueError, match="1 to 32 members"):
        E(seeds=list(range(33)), **kw)
    with pytest.raises(ValueError, match="are DeviceMLPModels"):
        E(models=[_model(), object()])
    with pytest.raises(ValueError, match="one shape"):
        E(models=[_model(), _model(o=18)])
    with pytest.raises(ValueError, match="one activation"):
        E(models=[_model(), _model(activation="swish")])
    with pytest.raises(ValueError, match="one cost program"):
        E(models=[_model(), _model(flip_thresh=0.8)])
    with pytest.raises(ValueError, match="their own shape"):
        E(models=[_model()], obs_dim=17)
    with pytest.raises(ValueError, match="neither seed"):
        E(seeds=[1, 2], seed=3, **kw)
    e = object.__new__(E)   # (no device: what rollout_cost and rollout_cost_batch check first)
    e.obs_dim, e.act_dim, e.members = 17, 6, 5
    with pytest.raises(ValueError, match="actions must be"):
        e.rollout_cost(np.zeros(17), torch.zeros((4, 3, 5)))
    with pytest.raises(ValueError, match="at least one row"):
        e.rollout_cost(np.zeros(17), torch.zeros((0, 3, 6)))
    with pytest.raises(ValueError, match=r"obs must be \[17\]"):
        e.rollout_cost(np.zeros(230), torch.zeros((4, 3, 6)))
    with pytest.raises(ValueError, match="7 planners x 5 members = 35 problems"):
        e.rollout_cost_batch(np.zeros((7, 17)), torch.zeros((7, 3, 6)), [1] * 7)
    with pytest.raises(ValueError, match="rows sum to 5"):
        e.rollout_cost_batch(np.zeros((2, 17)), torch.zeros((4, 3, 6)), [2, 3])
    with pytest.raises(ValueError, match="observations must be"):
        e.rollout_cost_batch(np.zeros((3, 17)), torch.zeros((5, 3, 6)), [2, 3])


def test_an_ensemble_on_the_host_stacks_its_members_and_takes_no_fused_entry(lib):
    """Built on the CPU: params [E, elems] in member order, predict is member 0's, and a controller's duck-typed learned-dynamics
    path would see rollout_cost + params + rollout_cost_batch while both _model_is_the_library_* stay false."""
    from icem_amd import DeviceMLPEnsemble, MpcICemHip
    ms = [_model(seed=3), _model(seed=4)]
    e = DeviceMLPEnsemble(models=ms, reduce="max")
    assert (e.members, e.obs_dim, e.act_dim, e.layers, e.activation, e.reduce) == (2, 17, 6, 1, "relu", "max") and e.member_costs is None
    assert tuple(e.params.shape) == (2, lib.icem_mlp_param_elems(17, 6, 1))
    assert torch.equal(e.params[0], ms[0].params) and torch.equal(e.params[1], ms[1].params) and not torch.equal(e.params[0], e.params[1])
    assert hasattr(e, "rollout_cost") and hasattr(e, "params") and hasattr(e, "rollout_cost_batch")
    holder = object.__new__(MpcICemHip)
    holder.forward_model = e
    assert holder._model_is_the_library_rssm() is False and holder._model_is_the_library_ensemble() is False
    ob, a = np.zeros((1, 17)), np.full((1, 6), 0.25)
    want = ms[0].predict(observations=ob, states=None, actions=a)[0]
    assert np.array_equal(e.predict(observations=ob, states=None, actions=a)[0], want)
    seeded = DeviceMLPEnsemble(seeds=[3, 4], obs_dim=17, act_dim=6, layers=1, cost_spec=_spec_py(), device="cpu")
    assert seeded.params.equal(e.params) and seeded.reduce == "mean"
