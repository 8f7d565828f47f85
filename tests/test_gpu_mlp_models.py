"""icem_mlp_rollout_cost_models / icem_mlp_rollout_cost_ensemble (k_mlp_rollout.hip's mlp_rollout_models_kernel) on the MI355X.
Everything is bit for bit: every cost and every state of every problem of a launch against that problem's OWN
``DeviceMLPModel.rollout_cost(..., return_observations=True)`` (mlp_models_cases.launch_mismatches -- np.array_equal, no
tolerance; test_mlp_models_sensitivity_cpu.py shows which single faults that comparison rejects on these layouts), the ensemble's
``member_costs`` against the members alone and its ``costs`` against a float32 NumPy restatement of the reduction.  Then the
capture of a first call, every refusal on real device buffers, and the three controllers planning through a
``DeviceMLPEnsemble`` -- ``MpcICemHip.get_action_batch`` included."""
import ctypes as C

import numpy as np
import pytest
import torch

import mlp_cases as MC
import mlp_models_cases as MM
from test_gpu_mlp_controllers import H, ITERS, KINDS, N, controller, observations, record

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_models, _solo = {}, {}


def _dev(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.float32, device=DEV)


def _np(t):
    return t.detach().cpu().numpy()


def shape_model(shape, k):
    from icem_amd import DeviceMLPModel
    key = (shape.name, k)
    if key not in _models:
        _models[key] = DeviceMLPModel(module=MM.shape_module(shape, k), cost_spec=MM.plain_spec(shape.case.o), device=DEV)
    return _models[key]


def hopper_model(k):
    from icem_amd import DeviceMLPModel
    key = ("hopper", k)
    if key not in _models:
        _models[key] = DeviceMLPModel(module=MM.hopper_module(k), cost_spec=MM.HOPPER.spec, device=DEV)
    return _models[key]


class Launch:
    """The inputs of one layout on the device, the launch through the library and the solo reference per problem."""

    def __init__(self, tag, models, layout, o, d, h, obs_scale=1.0, seed=0):
        self.tag, self.models, self.layout, self.h, self.o = tag, models, layout, h, o
        obs, acts = MM.inputs(o, d, h, layout, seed)
        self.obs, self.acts = (obs_scale * obs).astype(np.float32), acts
        self.obs_dev, self.acts_dev = _dev(self.obs), _dev(acts)

    def run(self, mode, states=True, problems=None, acts_dev=None):
        """(costs, states or None) of icem_mlp_rollout_cost_models over the layout's table (every field of the problem table:
        the wrapper beneath mlp_rollout_cost_models, which itself names observation p for problem p)."""
        from icem_amd.models import _mlp_models_launch
        problems = self.layout.problems if problems is None else problems
        acts_dev = self.acts_dev if acts_dev is None else acts_dev
        total = sum(q[3] for q in problems)
        s = torch.full((total, self.h + 1, self.o), -7.0, device=DEV) if states else None
        c = _mlp_models_launch(self.models[0], [self.models[q[0]].params.data_ptr() for q in problems], [q[1] for q in problems],
                               [q[2] for q in problems], [q[3] for q in problems], self.obs_dev, len(self.obs), acts_dev, mode,
                               out=torch.full((total,), -7.0, device=DEV), states=s)
        return _np(c), None if s is None else _np(s)

    def solo(self, mode, problems=None):
        problems = self.layout.problems if problems is None else problems

        def one(p):
            model, obs_row, a0, rows = problems[p]
            key = (self.tag, model, obs_row, a0, rows, mode)
            if key not in _solo:
                c, s = self.models[model].rollout_cost(self.obs[obs_row], self.acts_dev[a0:a0 + rows], mode, return_observations=True)
                _solo[key] = (_np(c), _np(s))
            return _solo[key]
        return one


_launches = {}


def launch_of(shape, layout):
    key = (shape.name, layout.name)
    if key not in _launches:
        models = [shape_model(shape, k) for k in range(layout.n_models)]
        _launches[key] = Launch(key, models, layout, shape.case.o, shape.case.d, shape.h)
    return _launches[key]


# ---- problems against solo: costs and states -----------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", MM.LAYOUTS, ids=lambda l: l.name)
@pytest.mark.parametrize("shape", MM.SHAPES, ids=lambda s: s.name)
def test_every_problem_is_its_solo_launch_bit_for_bit(shape, layout):
    la = launch_of(shape, layout)
    for mode in (0, 1, 2):
        costs, states = la.run(mode)
        assert np.isfinite(costs).all() and np.isfinite(states).all()
        assert MM.launch_mismatches(costs, states, layout.problems, la.solo(mode)) == [], (shape.name, layout.name, mode)
        bare, _ = la.run(mode, states=False)   # `observations` NULL: the last transition is skipped, the cost bits stay
        assert np.array_equal(bare, costs), (shape.name, layout.name, mode)


@pytest.mark.parametrize("layout", [MM.LAYOUT_BY_NAME[n] for n in ("mixed-1-15-16-17-33", "three-overlap", "thirty-two")], ids=lambda l: l.name)
@pytest.mark.parametrize("h", [2, 12])
def test_the_difference_and_health_terms(layout, h):
    """Hopper's program: the difference term reads s_h (the step count is the horizon with and without `observations`), the
    health term and its box sweep the state."""
    env = MM.HOPPER
    assert env.spec.diff_idx >= 0 and env.spec.health_idx >= 0 and env.spec.box_from >= 0
    la = Launch(("hopper", layout.name, h), [hopper_model(k) for k in range(layout.n_models)], layout, env.o, env.d, h, obs_scale=0.2, seed=3)
    for mode in (0, 1, 2):
        costs, states = la.run(mode)
        assert MM.launch_mismatches(costs, states, layout.problems, la.solo(mode)) == [], (layout.name, h, mode)
        assert np.array_equal(la.run(mode, states=False)[0], costs)
    assert len(np.unique(costs)) > 1


def test_the_public_wrapper_names_observation_p_for_problem_p():
    from icem_amd import mlp_rollout_cost_models
    shape, layout = MM.SHAPE_BY_NAME["o33d6-L2-relu-h12"], MM.LAYOUT_BY_NAME["three-overlap"]
    la = launch_of(shape, layout)
    ms = [la.models[q[0]] for q in layout.problems]
    obs = la.obs[[q[1] for q in layout.problems]]
    rows, row0 = [q[3] for q in layout.problems], [q[2] for q in layout.problems]
    want_c, want_s = la.run(0)
    for observations in (obs, _dev(obs)):   # host rows, or a device tensor used as is
        c, s = mlp_rollout_cost_models(ms, observations, la.acts_dev, rows, action_row0=row0, return_observations=True)
        assert np.array_equal(_np(c), want_c) and np.array_equal(_np(s), want_s)
        assert torch.equal(mlp_rollout_cost_models(ms, observations, la.acts_dev, rows, action_row0=row0), c)
    # back to back without action_row0
    rows = [16, 1, 20]
    b2b = mlp_rollout_cost_models(ms, obs, la.acts_dev[:sum(rows)], rows, cost_mode=2)
    problems = [(q[0], q[1], a, r) for q, a, r in zip(layout.problems, MM._back_to_back(rows), rows)]
    assert MM.launch_mismatches(_np(b2b), None, problems, la.solo(2, problems)) == []


# ---- each problem reads its own inputs -----------------------------------------------------------------------------------------------
SHAPE0 = MM.SHAPE_BY_NAME["o17d6-L2-relu-h12"]


def _custom(name, **kw):
    layout = MM._layout(name, **kw)
    models = [shape_model(SHAPE0, k) for k in range(max(layout.n_models, 3))]
    return Launch(("custom", name), models, layout, SHAPE0.case.o, SHAPE0.case.d, SHAPE0.h)


def test_permuting_the_models_permutes_the_costs():
    la = _custom("perm", rows=[17, 17, 17], models=[0, 1, 2], action_row0=[0, 0, 0], obs_rows=[0, 0, 0])
    base, sb = la.run(0)
    a, b, c = np.split(base, 3)
    assert (a != b).all() and (a != c).all() and (b != c).all()   # identical but for the model: every row differs
    perm = [2, 0, 1]
    got, sp = la.run(0, problems=[(perm[p], 0, 0, 17) for p in range(3)])
    assert np.array_equal(got, np.concatenate([(a, b, c)[k] for k in perm]))
    assert np.array_equal(sp, np.concatenate([np.split(sb, 3)[k] for k in perm]))


def test_two_problems_identical_but_for_the_observation_differ():
    la = _custom("obs", rows=[17, 17], models=[0, 0], action_row0=[0, 0], obs_rows=[0, 1])
    costs, states = la.run(0)
    assert (costs[:17] != costs[17:]).all() and (states[:17, 0] != states[17:, 0]).any(axis=1).all()
    assert MM.launch_mismatches(costs, states, la.layout.problems, la.solo(0)) == []


def test_a_problem_behind_a_17_row_neighbour_has_the_bits_it_has_in_front():
    """Its cost base is 17, not 32, and the neighbour's padding rows are the NEIGHBOUR's last row, never stored."""
    la = _custom("behind", rows=[17, 5], models=[0, 1], obs_rows=[1, 0])
    (m0, o0, a0, r0), (m1, o1, a1, r1) = la.layout.problems
    behind_c, behind_s = la.run(0)
    front_c, front_s = la.run(0, problems=[(m1, o1, a1, r1), (m0, o0, a0, r0)])
    assert np.array_equal(behind_c[17:], front_c[:5]) and np.array_equal(behind_s[17:], front_s[:5])
    assert np.array_equal(behind_c[:17], front_c[5:]) and np.array_equal(behind_s[:17], front_s[5:])


def test_nan_in_the_action_rows_around_a_problem_changes_nothing():
    la = _custom("poison", rows=[17, 5, 16], models=[0, 1, 2], action_row0=[3, 25, 33], obs_rows=[2, 0, 1], n_action_rows=52)
    clean_c, clean_s = la.run(1)
    assert MM.launch_mismatches(clean_c, clean_s, la.layout.problems, la.solo(1)) == []
    inside = np.zeros(52, bool)
    for _, _, a0, rows in la.layout.problems:
        inside[a0:a0 + rows] = True
    assert (~inside).sum() == 52 - 38 and not inside[[2, 20, 24, 30, 32, 49]].any()   # rows just outside every problem
    poisoned = la.acts_dev.clone()
    poisoned[torch.as_tensor(~inside, device=DEV)] = float("nan")
    got_c, got_s = la.run(1, acts_dev=poisoned)
    assert np.array_equal(got_c, clean_c) and np.array_equal(got_s, clean_s)
    assert np.array_equal(la.run(1, states=False, acts_dev=poisoned)[0], clean_c)


# ---- the ensemble ------------------------------------------------------------------------------------------------------------------------
ENS_SHAPE = MM.SHAPE_BY_NAME["o17d6-L1-swish-h2"]


def _ensemble(E, reduce="mean", shape=ENS_SHAPE):
    from icem_amd import DeviceMLPEnsemble
    return DeviceMLPEnsemble(models=[shape_model(shape, k) for k in range(E)], reduce=reduce)


def _ens_inputs(n, shape=ENS_SHAPE, seed=5):
    rs = np.random.RandomState(seed)
    return (0.5 * rs.randn(shape.case.o)).astype(np.float32), _dev(rs.uniform(-1, 1, (n, shape.h, shape.case.d)))


@pytest.mark.parametrize("n", [17, 40])
@pytest.mark.parametrize("E", [1, 2, 5, 32])
def test_the_ensemble_is_its_members_alone_and_their_restated_reduction(E, n):
    ob, acts = _ens_inputs(n)
    for reduce in ("mean", "max"):
        ens = _ensemble(E, reduce)
        for mode in (0, 1, 2):
            costs = ens.rollout_cost(ob, acts, mode)
            solo = np.stack([_np(m.rollout_cost(ob, acts, mode)) for m in ens.models])
            assert tuple(ens.member_costs.shape) == (E, n) and np.isfinite(solo).all()
            assert MM.ensemble_mismatches(_np(ens.member_costs), _np(costs), solo, reduce) == [], (E, n, reduce, mode)
            if E == 1:
                assert np.array_equal(_np(costs), solo[0])   # one member: the solo launch's bits in both outputs
    if E > 1:
        assert (solo[0] != solo[1]).all()


@pytest.mark.parametrize("shape", ["o33d6-L2-relu-h12", "o33d1-L4-swish-h12"])
def test_the_ensemble_at_two_state_blocks(shape):
    shape = MM.SHAPE_BY_NAME[shape]
    ob, acts = _ens_inputs(40, shape)
    ens = _ensemble(3, "mean", shape)
    costs = ens.rollout_cost(ob, acts, 0)
    solo = np.stack([_np(m.rollout_cost(ob, acts, 0)) for m in ens.models])
    assert MM.ensemble_mismatches(_np(ens.member_costs), _np(costs), solo, "mean") == []


@pytest.mark.parametrize("reduce", ["mean", "max"])
def test_a_member_with_a_nan_makes_every_row_nan_and_leaves_the_others_alone(reduce):
    from icem_amd import DeviceMLPEnsemble
    ob, acts = _ens_inputs(40)
    good = _ensemble(3, reduce)
    good.rollout_cost(ob, acts, 0)
    want = _np(good.member_costs)
    ens = DeviceMLPEnsemble(models=good.models, reduce=reduce)
    first = MC.param_elems(ENS_SHAPE.case.o, ENS_SHAPE.case.d, ENS_SHAPE.case.L) - 32 * ((ENS_SHAPE.case.o + 15) // 16)
    ens.params[1, first:] = 0x7FC0   # bout of member 1 := NaN in every entry (an f32 of two such 16-bit words is a NaN)
    costs = _np(ens.rollout_cost(ob, acts, 0))
    mc = _np(ens.member_costs)
    assert np.isnan(costs).all() and np.isnan(mc[1]).all()
    assert np.array_equal(mc[0], want[0]) and np.array_equal(mc[2], want[2]) and np.isfinite(mc[[0, 2]]).all()
    assert MM.ensemble_mismatches(mc, costs, mc, reduce) == []


def test_rollout_cost_batch_is_rollout_cost_per_planner():
    rows = [5, 17, 40]
    obs = (0.5 * np.random.RandomState(11).randn(3, ENS_SHAPE.case.o)).astype(np.float32)
    acts = _dev(np.random.RandomState(12).uniform(-1, 1, (sum(rows), ENS_SHAPE.h, ENS_SHAPE.case.d)))
    for reduce in ("mean", "max"):
        ens = _ensemble(3, reduce)
        for observations in (obs, _dev(obs)):
            got = ens.rollout_cost_batch(observations, acts, rows, 0)
            members, at = ens.member_costs.clone(), 0
            assert tuple(members.shape) == (3, sum(rows))
            for b, r in enumerate(rows):
                want = ens.rollout_cost(obs[b], acts[at:at + r], 0)
                assert torch.equal(got[at:at + r], want) and torch.equal(members[:, at:at + r], ens.member_costs), (reduce, b)
                at += r


def test_thirty_two_problems_are_served_and_thirty_three_refused():
    ens = _ensemble(8)
    obs = (0.5 * np.random.RandomState(13).randn(4, ENS_SHAPE.case.o)).astype(np.float32)
    rows = [3, 17, 1, 16]
    acts = _dev(np.random.RandomState(14).uniform(-1, 1, (sum(rows), ENS_SHAPE.h, ENS_SHAPE.case.d)))
    got = ens.rollout_cost_batch(obs, acts, rows, 0)   # 4 planners x 8 members
    at = 0
    for b, r in enumerate(rows):
        assert torch.equal(got[at:at + r], ens.rollout_cost(obs[b], acts[at:at + r], 0))
        at += r
    with pytest.raises(ValueError, match="3 planners x 11 members = 33 problems"):
        _ensemble(11).rollout_cost_batch(obs[:3], acts[:21], [3, 17, 1], 0)


# ---- capture -------------------------------------------------------------------------------------------------------------------------------
def test_the_first_call_of_a_shape_can_be_captured():
    """Nothing is allocated or staged by either entry (the problem table travels in the kernel arguments): a torch.cuda.graph
    capture of the first calls ever made at a shape replays to the eager calls' bits."""
    from icem_amd import CostSpec, CostTerm, DeviceMLPEnsemble, DeviceMLPModel, _lib as L
    from icem_amd.models import _mlp_models_launch
    o, d, layers, h = 23, 4, 3, 7   # a shape no other test launches
    spec = CostSpec(0.05, 3, -1.0, 2, 5.0, 0.4, diff_idx=0, diff_weight=-2.0, terms=(CostTerm(0, 17, 2, 3, 0.5),))
    ms = [DeviceMLPModel(o, d, layers=layers, activation="swish", seed=20 + k, cost_spec=spec, device=DEV) for k in range(3)]
    ens = DeviceMLPEnsemble(models=ms)
    rs = np.random.RandomState(1)
    obs = _dev(0.3 * rs.randn(3, o))
    rows, row0 = [33, 5, 17], [0, 30, 20]
    acts = _dev(rs.uniform(-1, 1, (40, h, d)))
    costs = torch.full((sum(rows),), -1.0, device=DEV)
    states = torch.full((sum(rows), h + 1, o), -1.0, device=DEV)
    mcosts, ecosts = torch.full((3, 40), -1.0, device=DEV), torch.full((40,), -1.0, device=DEV)
    ptrs = (C.c_void_p * 3)(*[m.params.data_ptr() for m in ms])

    def launch():
        _mlp_models_launch(ms[0], [m.params.data_ptr() for m in ms], [2, 0, 1], row0, rows, obs, 3, acts, 0, out=costs, states=states)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        L.check(ens.lib.icem_mlp_rollout_cost_ensemble(3, ptrs, 40, h, o, d, layers, L.MLP_ACTIVATIONS["swish"], 0, 0, C.byref(ms[0]._cost_c),
                                                       C.byref(ms[0]._terms_c), C.c_void_p(obs.data_ptr()), C.c_void_p(acts.data_ptr()),
                                                       C.c_void_p(mcosts.data_ptr()), C.c_void_p(ecosts.data_ptr()), st))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    g.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in (costs, states, mcosts, ecosts)]
    for t in (costs, states, mcosts, ecosts):
        t.fill_(-1.0)
    launch()
    torch.cuda.synchronize()
    assert torch.isfinite(replayed[0]).all() and torch.isfinite(replayed[3]).all()
    for a, b in zip(replayed, (costs, states, mcosts, ecosts)):
        assert torch.equal(a, b)
    at = 0
    for p, (k, r, a0) in enumerate(zip([2, 0, 1], rows, row0)):   # ... which are the solo launches'
        c, s = ms[p].rollout_cost(_np(obs[k]), acts[a0:a0 + r], 0, return_observations=True)
        assert torch.equal(replayed[0][at:at + r], c) and torch.equal(replayed[1][at:at + r], s)
        at += r
    assert torch.equal(replayed[3], ens.rollout_cost(_np(obs[0]), acts, 0)) and torch.equal(replayed[2], ens.member_costs)
    acts.mul_(0.5)   # the graph reads the buffers it was captured on
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(ecosts, ens.rollout_cost(_np(obs[0]), acts, 0))


# ---- refusals, on device buffers ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refusing():
    from icem_amd import _lib as L
    m = shape_model(SHAPE0, 0)
    o, d, h = SHAPE0.case.o, SHAPE0.case.d, SHAPE0.h
    buf = dict(obs=_dev(np.zeros((4, o))), acts=_dev(np.zeros((100, h, d))), costs=torch.full((200,), 3.5, device=DEV),
               member_costs=torch.full((2, 100), 3.5, device=DEV))
    lib = m.lib

    def models(problems=None, n_problems=None, h=h, o=o, d=d, layers=2, act=0, mode=0, n_obs=4, n_action_rows=100, null=None, cost=None):
        problems = [(m.params.data_ptr(), 0, 5, 0)] * 2 if problems is None else problems
        arr = (L.IcemMlpProblemC * max(len(problems), 1))(*[L.IcemMlpProblemC(*p) for p in problems])
        ptr = {k: (None if null == k else C.c_void_p(buf[k].data_ptr())) for k in ("obs", "acts", "costs")}
        return lib.icem_mlp_rollout_cost_models(len(problems) if n_problems is None else n_problems, None if null == "problems" else arr,
                                                h, o, d, layers, act, mode, None if null == "cost" else C.byref(cost or m._cost_c), None,
                                                ptr["obs"], n_obs, ptr["acts"], n_action_rows, ptr["costs"], None, None)

    def ensemble(members=2, n=100, h=h, o=o, d=d, layers=2, act=0, mode=0, reduce=0, null=None, null_member=None, cost=None):
        ptrs = (C.c_void_p * max(members, 1))(*[None if e == null_member else m.params.data_ptr() for e in range(max(members, 1))])
        ptr = {k: (None if null == k else C.c_void_p(buf[k].data_ptr())) for k in ("obs", "acts", "member_costs", "costs")}
        return lib.icem_mlp_rollout_cost_ensemble(members, None if null == "params" else ptrs, n, h, o, d, layers, act, mode, reduce,
                                                  None if null == "cost" else C.byref(cost or m._cost_c), None, ptr["obs"], ptr["acts"],
                                                  ptr["member_costs"], ptr["costs"], None)
    return m, buf, models, ensemble


def _bad_cost():
    from icem_amd import _lib as L
    return L.IcemCostSpecC(ctrl_weight=0.1, lin_weight=-1.0, flip_penalty=10.0, flip_thresh=1.5, lin_idx=17, flip_idx=1)


INVALID, UNSUPPORTED = -1, -2   # ICEM_E_INVALID / ICEM_E_UNSUPPORTED (asserted against icem_amd._lib below)
P0 = "params"                   # (stands for the model's parameter pointer in the tables below)
MODELS_REFUSALS = [
    (dict(null="problems"), INVALID), (dict(null="cost"), INVALID), (dict(null="obs"), INVALID), (dict(null="acts"), INVALID),
    (dict(null="costs"), INVALID),
    (dict(problems=[(P0, 0, 5, 0), (None, 0, 5, 0)]), INVALID),
    (dict(problems=[], n_problems=0), INVALID), (dict(problems=[(P0, 0, 5, 0)] * 33), INVALID),
    (dict(problems=[(P0, 0, 5, 0), (P0, 0, 0, 0)]), INVALID),
    (dict(problems=[(P0, 0, 5, 4)]), INVALID), (dict(problems=[(P0, 0, 5, -1)]), INVALID),
    (dict(problems=[(P0, 96, 5, 0)]), INVALID), (dict(problems=[(P0, -1, 5, 0)]), INVALID), (dict(problems=[(P0, 0, 101, 0)]), INVALID),
    (dict(mode=3), INVALID), (dict(act=2), INVALID), (dict(cost="bad"), INVALID),
    (dict(o=65), UNSUPPORTED), (dict(d=33), UNSUPPORTED), (dict(layers=5), UNSUPPORTED), (dict(h=65), UNSUPPORTED), (dict(h=0), UNSUPPORTED),
]
ENSEMBLE_REFUSALS = [
    (dict(null="params"), INVALID), (dict(null="cost"), INVALID), (dict(null="obs"), INVALID), (dict(null="acts"), INVALID),
    (dict(null="member_costs"), INVALID), (dict(null="costs"), INVALID), (dict(null_member=1), INVALID),
    (dict(members=0), INVALID), (dict(members=33), INVALID), (dict(n=0), INVALID),
    (dict(reduce=2), INVALID), (dict(reduce=-1), INVALID), (dict(mode=-1), INVALID), (dict(act=-1), INVALID), (dict(cost="bad"), INVALID),
    (dict(o=0), UNSUPPORTED), (dict(d=0), UNSUPPORTED), (dict(layers=0), UNSUPPORTED), (dict(h=65), UNSUPPORTED),
]


def test_every_refusal_comes_with_its_code_and_leaves_the_buffers_alone(refusing):
    from icem_amd import _lib as L
    assert (L.ICEM_E_INVALID, L.ICEM_E_UNSUPPORTED) == (INVALID, UNSUPPORTED)
    m, buf, models, ensemble = refusing
    for entry, table in ((models, MODELS_REFUSALS), (ensemble, ENSEMBLE_REFUSALS)):
        for kw, code in table:
            kw = dict(kw)
            if kw.get("cost") == "bad":
                kw["cost"] = _bad_cost()
            if "problems" in kw:
                kw["problems"] = [(m.params.data_ptr() if q[0] == P0 else q[0],) + q[1:] for q in kw["problems"]]
            assert entry(**kw) == code, (entry.__name__, kw, m.lib.icem_last_error())
    torch.cuda.synchronize()
    assert bool((buf["costs"] == 3.5).all()) and bool((buf["member_costs"] == 3.5).all())
    # ... and the same buffers are served once the arguments are right
    assert models() == 0 and ensemble() == 0
    torch.cuda.synchronize()
    assert bool((buf["costs"][:100] != 3.5).all()) and bool((buf["member_costs"] != 3.5).all())


# ---- the controllers --------------------------------------------------------------------------------------------------------------------
def _ctrl_ensemble(E=3, seed0=3):
    from icem_amd import DeviceMLPEnsemble, halfcheetah_env
    return DeviceMLPEnsemble(seeds=list(range(seed0, seed0 + E)), obs_dim=17, act_dim=6, layers=2, activation="swish",
                             env=halfcheetah_env(17), device=DEV)


@pytest.mark.parametrize("kind", KINDS)
def test_the_controllers_plan_stage_by_stage_through_the_ensemble(kind):
    m, twin_m = _ctrl_ensemble(), _ctrl_ensemble()
    calls, inner = record(m)
    a, b = controller(kind, m), controller(kind, twin_m)
    for c in (a, b):
        assert c.rssm_path and not c.device_path and not c.torch_path
        assert not c._model_is_the_library_rssm() and not c._model_is_the_library_ensemble()   # no fused *_learned_models entry
    obs = observations()
    for c in (a, b):
        c.beginning_of_rollout(observation=obs[0], state=None, mode="train")
    per_step = ITERS if kind != "random" else 1
    for k, ob in enumerate(obs):
        before = len(calls)
        act = a.get_action(ob, None)
        assert act.shape == (6,) and np.isfinite(act).all()
        assert np.array_equal(act, b.get_action(ob, None)), (kind, k)      # two equal controllers: the same bits
        assert a.last_min_cost == b.last_min_cost, (kind, k)
        mine = calls[before:]
        assert len(mine) == per_step, (kind, k, len(mine))                  # one rollout_cost per iteration: stage by stage
        direct = [inner(o, acts, mode) for o, acts, _, mode in mine]
        for d, (o, acts, out, mode) in zip(direct, mine):
            assert torch.equal(d, out) and np.array_equal(o, ob.astype(np.float32)) and acts.shape[1:] == (H, 6) and mode == 0
        pools = direct if kind == "icem" else direct[-1:]
        assert a.last_min_cost == float(min(_np(d).min() for d in pools)), (kind, k)
        assert mine[-1][1].shape[0] <= N and tuple(m.member_costs.shape) == (3, mine[-1][1].shape[0])


@pytest.mark.parametrize("kind", KINDS)
def test_an_ensemble_of_one_executes_the_plain_members_bits(kind):
    from icem_amd import DeviceMLPEnsemble
    from test_gpu_mlp_controllers import model
    plain = model(seed=6)
    a, b = controller(kind, plain), controller(kind, DeviceMLPEnsemble(models=[model(seed=6)]))
    obs = observations()
    for c in (a, b):
        c.beginning_of_rollout(observation=obs[0], state=None, mode="train")
    for k, ob in enumerate(obs):
        assert np.array_equal(a.get_action(ob, None), b.get_action(ob, None)), (kind, k)
        assert a.last_min_cost == b.last_min_cost, (kind, k)


def test_get_action_batch_over_one_ensemble_is_get_action_per_controller():
    from icem_amd import MpcICemHip
    ens = _ctrl_ensemble()
    calls = []
    inner = ens.rollout_cost_batch
    ens.rollout_cost_batch = lambda *a, **kw: (calls.append(1), inner(*a, **kw))[1]   # (on the instance: counted, still the class's launch)
    seeds = (1, 2, 3)
    ctrls = [controller("icem", ens, seed=s) for s in seeds]
    twins = [controller("icem", _ctrl_ensemble(), seed=s) for s in seeds]
    rs = np.random.RandomState(21)
    obs = [[0.3 * rs.randn(17) for _ in seeds] for _ in range(3)]
    for c, t, ob in zip(ctrls, twins, obs[0]):
        c.beginning_of_rollout(observation=ob, state=None, mode="train")
        t.beginning_of_rollout(observation=ob, state=None, mode="train")
    for k, obk in enumerate(obs):
        if k == 1:   # one controller starts a new episode a step later: it has no shifted elites, its first pool is shorter
            ctrls[2].beginning_of_rollout(observation=obk[2], state=None, mode="train")
            twins[2].beginning_of_rollout(observation=obk[2], state=None, mode="train")
        before = len(calls)
        got = MpcICemHip.get_action_batch(ctrls, obk)
        assert len(calls) - before == ITERS   # one launch of 3 x 3 problems per CEM iteration
        for i, (c, t, ob) in enumerate(zip(ctrls, twins, obk)):
            want = t.get_action(ob, None)
            assert np.array_equal(np.asarray(got[i]), want), (k, i)
            assert c.last_min_cost == t.last_min_cost, (k, i)
    assert [c.planner.mpc_step for c in ctrls] == [t.planner.mpc_step for t in twins]
