"""icem_mlp_param_elems / icem_mlp_rollout_cost (abi.hip, k_mlp_rollout.hip) and the Python side of the feed-forward learned
dynamics without a device: the two symbols are exported, declared with a documented prototype and bound with matching ctypes; the
ABI version stays 6; the library's buffer size is the packer's over the edge shapes; every refusal comes back with its code and a
message before anything could be launched (the pointers below are host addresses no accepted call could use); pack_mlp puts
every padded weight where icem_mlp.h says and folds an input normalisation exactly; DeviceMLPModel wants a cost."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import mlp_cases as MC
from icem_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {
    "icem_mlp_param_elems": "size_t (int32_t obs_dim, int32_t act_dim, int32_t layers)",
    "icem_mlp_rollout_cost": "int (int32_t n, int32_t horizon, int32_t obs_dim, int32_t act_dim, int32_t layers, int32_t activation, "
                             "int32_t cost_mode, const icem_cost_spec* cost, const icem_cost_terms* terms, const void* params, "
                             "const void* obs0, const void* actions, void* costs, void* observations, void* stream)",
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
    doc = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int icem_mlp_rollout_cost", hdr, flags=re.S)
    assert doc, "the entry carries a comment"
    for cited in ("s_{t+1} = s_t + f(s_t, a_t)", "horizon + 1", "ICEM_E_INVALID", "ICEM_E_UNSUPPORTED", "bf16", "captured"):
        assert cited in doc.group(1), cited
    assert re.search(r"/\*((?:(?!\*/).)*?icem_mlp\.h(?:(?!\*/).)*?)\*/\s*#define ICEM_MLP_MAX_OBS_DIM 64", hdr, flags=re.S), "the layout is cited"
    assert re.search(r"enum \{ ICEM_MLP_RELU = 0, ICEM_MLP_SWISH = 1 \};", hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, sig in SIGNATURES.items():
        m = re.search(rf"^(\w+)\s+{name}\s*\(([^)]*)\)\s*;", hdr, flags=re.M)
        assert m, name
        assert _squash(f"{m.group(1)} ({_squash(m.group(2))})") == sig, name


def test_the_library_exports_them_and_lib_binds_them(lib):
    bound = {name: (res, args) for name, res, args in L.SYMBOLS}
    VP, I32 = C.c_void_p, C.c_int32
    kinds = {"int32_t": I32, "const icem_cost_spec*": C.POINTER(L.IcemCostSpecC), "const icem_cost_terms*": C.POINTER(L.IcemCostTermsC),
             "const void*": VP, "void*": VP}
    res = {"size_t": C.c_size_t, "int": C.c_int}
    for name, sig in SIGNATURES.items():
        args = [a.strip().rsplit(" ", 1)[0] for a in sig[sig.index("(") + 1:-1].split(",")]
        assert bound[name] == (res[sig.split(" ", 1)[0]], [kinds[a] for a in args]), name
        assert hasattr(lib, name), name
    assert lib.icem_abi_version() == L.ABI_VERSION == 6   # added symbols break no caller
    if shutil.which("nm") is not None:
        exported = subprocess.check_output(["nm", "-D", "--defined-only", L.lib_path()], text=True)
        for name in SIGNATURES:
            assert re.search(rf"\bT {name}$", exported, flags=re.M), name
    assert L.MLP_ACTIVATIONS == {"relu": 0, "swish": 1}


def test_the_new_names_are_exported_from_the_package():
    import icem_amd
    for name in ("DeviceMLPModel", "declared_mlp", "pack_mlp"):
        assert hasattr(icem_amd, name), name


# ---- sizes ------------------------------------------------------------------------------------------------------------------
EDGE_O = [1, 16, 17, 32, 33, 39, 64]
EDGE_D = [1, 6, 32]


@pytest.mark.parametrize("L_", [1, 2, 4])
def test_param_elems_is_the_packers_size(lib, L_):
    from icem_amd.models import declared_mlp, pack_mlp
    for o in EDGE_O:
        for d in EDGE_D:
            want = lib.icem_mlp_param_elems(o, d, L_)
            assert want == MC.param_elems(o, d, L_) > 0
            if d == 6 or o in (1, 33):   # (the packer's own count: one action width per o, every width at two)
                assert pack_mlp(declared_mlp(o, d, layers=L_, device="cpu").module).numel() == want, (o, d, L_)


@pytest.mark.parametrize("o,d,L_", [(0, 6, 2), (65, 6, 2), (-1, 6, 2), (17, 0, 2), (17, 33, 2), (17, 6, 0), (17, 6, 5), (17, -6, 2)])
def test_param_elems_is_zero_outside_the_ranges(lib, o, d, L_):
    assert lib.icem_mlp_param_elems(o, d, L_) == 0


# ---- refusals ---------------------------------------------------------------------------------------------------------------
_dummy = (C.c_float * 4)()
P = C.c_void_p(C.addressof(_dummy))


def _terms(**kw):
    t = L.IcemCostTermsC(diff_idx=-1, health_idx=-1, box_from=-1)
    terms = kw.pop("terms", ())
    for k, v in kw.items():
        setattr(t, k, v)
    t.n_terms = kw.get("n_terms", len(terms))
    for j, tm in enumerate(terms):
        t.terms[j] = L.IcemCostTermC(**dict(dict(weight=1.0, kind=0, a=0, b=-1, len=1, gate_idx=-1), **tm))
    return t


def call(lib, n=16, h=12, o=17, d=6, layers=2, act=0, mode=0, cost="ok", terms=None, params=P, obs0=P, actions=P, costs=P, cost_kw=None):
    spec = None if cost is None else L.IcemCostSpecC(**dict(dict(ctrl_weight=0.1, lin_weight=-1.0, flip_penalty=10.0, flip_thresh=1.5, lin_idx=8,
                                                                 flip_idx=1), **(cost_kw or {})))
    return lib.icem_mlp_rollout_cost(n, h, o, d, layers, act, mode, None if spec is None else C.byref(spec),
                                     None if terms is None else C.byref(terms), params, obs0, actions, costs, None, None)


@pytest.mark.parametrize("kw,word", [
    (dict(cost=None), b"null pointer"), (dict(params=None), b"null pointer"), (dict(obs0=None), b"null pointer"),
    (dict(actions=None), b"null pointer"), (dict(costs=None), b"null pointer"),
    (dict(n=-1), b"n must be >= 0"),
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
    (dict(terms=_terms(terms=[dict(a=0, b=15, len=3)])), b"cost term slice outside the observation"),
    (dict(terms=_terms(terms=[dict(gate_idx=17)])), b"cost term slice outside the observation"),
])
def test_bad_arguments_are_invalid_and_say_why(lib, kw, word):
    assert call(lib, **kw) == L.ICEM_E_INVALID
    err = lib.icem_last_error()
    assert b"icem_mlp_rollout_cost" in err and word in err, err


@pytest.mark.parametrize("kw,word", [
    (dict(o=0, cost_kw=dict(lin_idx=0, flip_idx=-1)), b"obs_dim"), (dict(o=65), b"obs_dim"),
    (dict(d=0), b"act_dim"), (dict(d=33), b"act_dim"),
    (dict(layers=0), b"layers"), (dict(layers=5), b"layers"),
    (dict(h=0), b"horizon"), (dict(h=65), b"horizon"), (dict(h=-1), b"horizon"),
])
def test_shapes_outside_the_compiled_ranges_are_unsupported(lib, kw, word):
    assert call(lib, **kw) == L.ICEM_E_UNSUPPORTED
    err = lib.icem_last_error()
    assert b"icem_mlp_rollout_cost" in err and word in err, err


def test_no_rows_is_ok_and_launches_nothing(lib):
    """n == 0 with every other argument in range: ICEM_OK on a machine without a device -- nothing was launched."""
    assert call(lib, n=0) == 0
    assert call(lib, n=0, h=64, o=64, d=32, layers=4, act=1, mode=2) == 0
    assert call(lib, n=0, terms=_terms(diff_idx=0, terms=[dict(a=14, len=3), dict(kind=5, a=16, gate_idx=16)])) == 0


# ---- the packer -------------------------------------------------------------------------------------------------------------
def _padded(net, o, d):
    """The padded layers [(W, b)] of icem_mlp.h from the module's own tensors (f32 arrays)."""
    sk, ob = (o + 31) // 32, (o + 15) // 16
    w1 = net.hidden[0].weight.detach().numpy()
    W1 = np.zeros((208, 32 * (sk + 1)), np.float32)
    W1[:200, :o] = w1[:, :o]
    W1[:200, 32 * sk:32 * sk + d] = w1[:, o:]
    vec = lambda b, n: np.concatenate([b.detach().numpy(), np.zeros(n - len(b), np.float32)])  # noqa: E731
    out = [(W1, vec(net.hidden[0].bias, 208))]
    for lin in list(net.hidden)[1:]:
        W = np.zeros((208, 224), np.float32)
        W[:200, :200] = lin.weight.detach().numpy()
        out.append((W, vec(lin.bias, 208)))
    W = np.zeros((16 * ob, 224), np.float32)
    W[:o, :200] = net.out.weight.detach().numpy()
    out.append((W, vec(net.out.bias, 16 * ob)))
    return out


@pytest.mark.parametrize("o", EDGE_O)
@pytest.mark.parametrize("d", EDGE_D)
def test_unpacking_reproduces_the_padded_weights_entry_for_entry(o, d):
    from icem_amd.models import declared_mlp, pack_mlp
    L_ = 1 + (o + d) % 3   # 1, 2 or 3 hidden layers
    net = declared_mlp(o, d, layers=L_, activation="swish", seed=o + d, device="cpu").module
    got = MC.unpack(pack_mlp(net), o, d, L_)
    want = _padded(net, o, d)
    assert len(got) == len(want) == L_ + 1
    for k, ((gw, gb), (ww, wb)) in enumerate(zip(got, want)):
        assert gw.shape == ww.shape and gb.shape == wb.shape, k
        assert np.array_equal(gw, MC.bf16(ww)), (k, np.argwhere(gw != MC.bf16(ww))[:4])
        assert np.array_equal(gb, wb), k   # the biases stay f32
        assert np.abs(ww).sum() > 0


def test_folded_normalisation_is_the_normalised_module_in_float64():
    from icem_amd.models import declared_mlp, fold_input_norm, pack_mlp
    o, d = 17, 6
    net = declared_mlp(o, d, layers=2, seed=3, device="cpu").module
    rs = np.random.RandomState(0)
    mean, std = rs.randn(o + d), rs.uniform(0.3, 3.0, o + d)
    w, b = fold_input_norm(net.hidden[0].weight, net.hidden[0].bias, mean, std)
    assert w.dtype == b.dtype == torch.float64
    x = torch.as_tensor(rs.randn(50, o + d) * 2)
    explicit = ((x - torch.as_tensor(mean)) / torch.as_tensor(std)) @ net.hidden[0].weight.double().T + net.hidden[0].bias.double()
    torch.testing.assert_close(x @ w.T + b, explicit, rtol=1e-12, atol=1e-12)
    # ... and that is what gets packed: the input layer of the buffer is the folded weight rounded to bf16, the bias in f32
    (gw, gb), = MC.unpack(pack_mlp(net, mean, std), o, d, 2)[:1]
    assert np.array_equal(gw[:200, :o], MC.bf16(w.float().numpy()[:, :o])) and np.array_equal(gw[:200, 32:32 + d], MC.bf16(w.float().numpy()[:, o:]))
    assert np.array_equal(gb[:200], b.float().numpy())
    with pytest.raises(ValueError):
        fold_input_norm(net.hidden[0].weight, net.hidden[0].bias, mean[:-1], std)
    with pytest.raises(ValueError):
        fold_input_norm(net.hidden[0].weight, net.hidden[0].bias, mean, np.zeros(o + d))


def test_the_packer_refuses_what_the_kernel_is_not_compiled_for():
    from icem_amd.models import declared_mlp, pack_mlp
    for kw in (dict(hidden=128), dict(layers=5)):
        with pytest.raises(ValueError):
            pack_mlp(declared_mlp(17, 6, device="cpu", **kw).module)
    with pytest.raises(ValueError):
        pack_mlp(declared_mlp(65, 6, device="cpu").module)
    with pytest.raises(ValueError):
        declared_mlp(17, 6, activation="tanh", device="cpu")


def test_declared_mlp_is_reproducible_and_has_no_cost():
    from icem_amd.models import declared_mlp
    a, b = declared_mlp(17, 6, seed=5, device="cpu"), declared_mlp(17, 6, seed=5, device="cpu")
    c = declared_mlp(17, 6, seed=6, device="cpu")
    assert a.cost is None and (a.obs_dim, a.act_dim) == (17, 6)
    for pa, pb, pc in zip(a.module.parameters(), b.module.parameters(), c.module.parameters()):
        assert torch.equal(pa, pb) and not torch.equal(pa, pc)
    o, act = torch.randn(5, 17), torch.randn(5, 6)
    x = torch.relu(a.module.hidden[0](torch.cat([o, act], -1)))
    x = torch.relu(a.module.hidden[1](x))
    torch.testing.assert_close(a.module(o, act), o + a.module.out(x))


def test_the_emulation_without_rounding_is_the_torch_module():
    case = MC.BY_NAME["o16d6-L2-swish-16x12"]
    net = MC.module(case).double()
    (ob, acts), = MC.launches(case)[:1]
    s = torch.as_tensor(ob)[None].repeat(len(acts), 1)
    want = [s]
    for t in range(case.h):
        s = net(s, torch.as_tensor(acts[:, t]))
        want.append(s)
    MC._modules.clear()   # (the cached module was turned to float64 above)
    got = MC.emulated_states(MC.params(case), ob, acts)
    np.testing.assert_allclose(got, torch.stack(want, 1).detach().numpy(), rtol=1e-6, atol=1e-7)   # the f32 module's weights, float64 arithmetic


def test_the_device_model_wants_a_cost():
    from icem_amd import DeviceMLPModel
    with pytest.raises(ValueError, match="cost"):
        DeviceMLPModel(17, 6, device="cpu")
    with pytest.raises(ValueError, match="cost"):
        DeviceMLPModel(17, 6, device="cpu", env=object())
