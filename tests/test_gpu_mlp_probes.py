"""icem_mlp_rollout_cost (k_mlp_rollout.hip) on the MI355X: its states (``observations``) against the float64 emulation of its
rounding points on the case table of mlp_cases.py, under that module's per-row criterion (bounds measured between two CPU
evaluations of the reference, none taken from the kernel; test_mlp_sensitivity_cpu.py shows what the criterion rejects); its
costs against the float64 oracle cost evaluated on the kernel's OWN states and the f32 actions, under cost_term_cases.py's
criterion, for the environments' cost programs at their widths and all three reductions; and what has to hold bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import cost_term_cases as CT
import mlp_cases as MC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_models = {}


def device_model(key, module, spec):
    from icem_amd import DeviceMLPModel
    if key not in _models:
        _models[key] = DeviceMLPModel(module=module, cost_spec=spec, device=DEV)
    return _models[key]


def _plain_spec(o):
    """A HalfCheetah-shaped cost at any width (the state cases do not look at the costs)."""
    from icem_amd import CostSpec
    return CostSpec(0.1, min(8, o - 1), -1.0, min(1, o - 1), 10.0, 0.7)


def _dev(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32, device=DEV)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


# ---- the states -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MC.CASES, ids=lambda c: c.name)
def test_states_on_the_case_table(case):
    m = device_model(("case", case.name), MC.module(case), _plain_spec(case.o))
    got = MC.over_launches(case, lambda ob, acts: _np(m.rollout_cost(ob, _dev(acts), 0, return_observations=True)[1]))
    want = MC.want(case)
    print(case.name, MC.errors(got, want))
    assert got.shape == want.shape == (case.n * case.launches, case.h + 1, case.o)
    assert MC.agree(got, want), (MC.violations(got, want), MC.errors(got, want))
    # ... and bf16 accuracy against the network itself
    exact = MC.over_launches(case, lambda ob, acts: MC.emulated_states(MC.params(case), ob, acts))
    assert np.abs(got - exact).max() <= 5e-2 * (1 + np.abs(exact).max()), (np.abs(got - exact).max(), np.abs(exact).max())


# ---- the costs --------------------------------------------------------------------------------------------------------------
def env_model(env):
    return device_model(("env", env.name), MC.cost_module(env), env.spec)


@pytest.mark.parametrize("mode", list(MC.MODES))
@pytest.mark.parametrize("env", MC.COST_ENVS, ids=lambda e: e.name)
def test_costs_against_the_float64_cost_on_the_kernels_own_states(env, mode):
    m = env_model(env)
    costs, states, bare = [], [], []
    for ob, acts in MC.cost_launches(env):
        c, s = m.rollout_cost(ob, _dev(acts), MC.MODES[mode], return_observations=True)
        bare.append(m.rollout_cost(ob, _dev(acts), MC.MODES[mode]))
        assert torch.equal(c, bare[-1]), "the costs differ with and without observations"
        costs.append(_np(c))
        states.append(_np(s))
    got, states = np.concatenate(costs), np.concatenate(states)
    case = MC.cost_case(f"mlp-gpu-{env.name}-{mode}", env.spec, mode, states, MC.cost_actions(env))
    print(env.name, mode, CT.errors(got, case))
    assert CT.near(case).mean() <= 0.05   # the condition test_mlp_sensitivity_cpu.py puts on the emulation's states holds for the kernel's
    assert CT.agree(got, case), (CT.violations(got, case), CT.errors(got, case))
    # the states the costs were taken on are the emulation's to bf16 accuracy (a flipped operand rounding moves a state by
    # 2^-9 of an entry): the comparisons fire on them as test_mlp_sensitivity_cpu.py measured on the emulation's
    emu = MC.cost_states(env)
    assert np.abs(states - emu).max() <= 2.0 ** -6 * np.abs(emu).max(), (np.abs(states - emu).max(), np.abs(emu).max())
    rates = MC.comparison_rates(env.spec, states)
    assert env.name in MC.LOPSIDED or all(0.05 <= r <= 0.95 for r in rates.values()), rates


# ---- bit for bit ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def door():
    """Door's cost program (a term list with thresholds) on its 39 / 28 shape: 1007 rows, h = 12."""
    env = MC.COST_ENV_BY_NAME["door"]
    ob, _ = MC.cost_launches(env)[1]
    acts = np.random.RandomState(5).uniform(-1, 1, (1007, 12, env.d)).astype(np.float32)
    return env_model(env), ob, _dev(acts)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_a_rows_cost_does_not_depend_on_where_it_sits(door, mode):
    m, ob, acts = door
    base = m.rollout_cost(ob, acts, mode)
    perm = torch.as_tensor(np.random.RandomState(mode).permutation(len(acts)), device=DEV)
    assert torch.equal(m.rollout_cost(ob, acts[perm].contiguous(), mode), base[perm])
    assert torch.equal(m.rollout_cost(ob, acts[:17].contiguous(), mode), base[:17])
    c, s = m.rollout_cost(ob, acts, mode, return_observations=True)
    assert torch.equal(c, base) and torch.isfinite(s).all()


def test_a_nan_in_one_rows_actions_stays_in_that_row(door):
    m, ob, acts = door
    base, states = m.rollout_cost(ob, acts, 0, return_observations=True)
    bad = acts.clone()
    row = 16 * 7 + 5   # a row in the middle of the eighth tile
    bad[row, 3, 2] = float("nan")
    got, s2 = m.rollout_cost(ob, bad, 0, return_observations=True)
    others = torch.ones(len(acts), dtype=torch.bool, device=DEV)
    others[row] = False
    assert torch.isnan(got[row]) and torch.equal(got[others], base[others])   # (its own cost: 0 * NaN^2 in the control term)
    assert torch.equal(s2[others], states[others]) and torch.equal(s2[row, :4], states[row, :4])


def test_the_first_call_of_a_shape_can_be_captured():
    """Nothing is allocated or staged by the entry: a torch.cuda.graph capture of the first call ever made at a shape replays to
    the eager call's bits."""
    from icem_amd import CostSpec, CostTerm, DeviceMLPModel, _lib as L
    o, d, layers, n, h = 21, 5, 3, 77, 7   # a shape no other test launches
    spec = CostSpec(0.05, 3, -1.0, 2, 5.0, 0.4, diff_idx=0, diff_weight=-2.0, terms=(CostTerm(0, 17, 2, 3, 0.5),))
    m = DeviceMLPModel(o, d, layers=layers, activation="swish", seed=9, cost_spec=spec, device=DEV)
    ob = _dev(0.3 * np.random.RandomState(1).randn(o))
    acts = _dev(np.random.RandomState(2).uniform(-1, 1, (n, h, d)))
    costs = torch.full((n,), -1.0, device=DEV)
    states = torch.full((n, h + 1, o), -1.0, device=DEV)

    def launch():
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        L.check(m.lib.icem_mlp_rollout_cost(n, h, o, d, layers, L.MLP_ACTIVATIONS["swish"], 0, C.byref(m._cost_c), C.byref(m._terms_c),
                                            C.c_void_p(m.params.data_ptr()), C.c_void_p(ob.data_ptr()), C.c_void_p(acts.data_ptr()),
                                            C.c_void_p(costs.data_ptr()), C.c_void_p(states.data_ptr()), st))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    g.replay()
    torch.cuda.synchronize()
    replayed = (costs.clone(), states.clone())
    costs.fill_(-1.0)
    states.fill_(-1.0)
    eager_c, eager_s = m.rollout_cost(_np(ob), acts, 0, return_observations=True)
    assert torch.isfinite(replayed[0]).all() and torch.equal(replayed[0], eager_c) and torch.equal(replayed[1], eager_s)
    acts.mul_(0.5)   # the graph reads the buffers it was captured on
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(costs, m.rollout_cost(_np(ob), acts, 0))


def test_the_model_checks_its_arguments():
    m = env_model(MC.COST_ENV_BY_NAME["reacher"])
    with pytest.raises(ValueError):
        m.rollout_cost(np.zeros(11), torch.zeros((4, 12, 3), device=DEV))
    with pytest.raises(ValueError):
        m.rollout_cost(np.zeros(12), torch.zeros((4, 12, 2), device=DEV))
    assert m.rollout_cost(np.zeros(11), torch.zeros((0, 12, 2), device=DEV)).shape == (0,)
    assert not hasattr(m, "rollout_cost_batch")
    nxt, _, rew = m.predict(observations=np.zeros((3, 11)), states=None, actions=np.zeros((3, 2)))
    assert nxt.shape == (3, 11) and rew.shape == (3, 1) and np.isfinite(nxt).all()
