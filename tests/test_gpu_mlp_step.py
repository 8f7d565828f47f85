"""icem_plan_step_mlp (learned_step.hip): the iCEM MPC step through feed-forward models -- a DeviceMLPModel, a DeviceMLPEnsemble,
one of either per planner -- as one library call: sample, (shift), ONE launch_mlp_rollout_models of n x members problems in
member-major order, and the one-launch update that reduces the members' costs.  The step is DEFINED by the operator loop
(mlp_step_loop.py: the public stage-wise operators called one by one), and the entry only rearranges its launches, so every
comparison in this file is ``np.array_equal`` / ``torch.equal``: no tolerance appears.

Shapes (mlp_step_loop.SHAPES): o = 17, d = 6, h = 12, 2 layers, swish, N = 128 -- rows 128 (+ 3 shifted elites from a
problem's second step on), 102, 81 --, and o = 40, d = 3, h = 10, 1 layer, relu, N = 100 with factor_decrease 1.3 -- the SK = 2
instantiation, rows 100 (+ 3), 76, 58: no row count a multiple of 16, a ragged last tile in every launch.  3 iterations, kept
and shifted elites (0.3 reused), the mean as row 0 of the last iteration, colored noise (beta 0.25), K = 10; 3 MPC steps: a
first step without shifted elites, shifting ones, both elite halves."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import mlp_step_loop as ML

pytestmark = pytest.mark.gpu

np_ = ML.np_
ITERS, STEPS = ML.ITERS, 3
SENTINEL = -12345.0


@contextlib.contextmanager
def option(name, value):
    from icem_amd import _lib as L
    L.set_option(name, value)
    try:
        yield
    finally:
        L.reset_options()


def rows_of(p, it, shifted):
    return p.population_sizes[it] + (p.n_reuse if it == 0 and shifted else 0)


def check_planner(p, ref, row, what, solo):
    """Planner ``p`` behind a fused step against the operator loop's record ``ref`` of the same step (``row``: its results row)."""
    assert np.array_equal(np_(row), ref["result"]), (what, "results row")
    assert np.array_equal(np_(torch.cat([p.executed, p.best_cost])), ref["result"]), (what, "executed | best_cost")
    q = ref["planner"]
    assert p.mpc_step == q.mpc_step, what
    assert np.array_equal(np_(p.mean), np_(q.mean)) and np.array_equal(np_(p.std), np_(q.std)), (what, "mean / std")
    g = (p.mpc_step * p.cfg.opt_iters) & 1
    for half, el, name in ((g, ref["elites"], "current elites"), (g ^ 1, ref["before"], "the elites before them")):
        assert np.array_equal(np_(p.elites_actions[half]), np_(el[0])) and np.array_equal(np_(p.elites_costs[half]), np_(el[1])), (what, name)
    if solo:   # (one problem works in its own buffers: the last pool is there)
        r = ref["costs"].shape[0]
        assert np.array_equal(np_(p.actions[:r]), ref["actions"]) and np.array_equal(np_(p.costs[:r]), ref["costs"]), (what, "last pool")


class Arrangement:
    """n fused planners + n reference planners of one shape and what they plan through.  kind: "model" (one DeviceMLPModel for
    all), "ensemble" (one DeviceMLPEnsemble for all), "model each", "ensemble each"."""

    def __init__(self, shape, n, kind, E=1, reduce="mean", seed0=11):
        self.shape, self.n, self.kind, self.E, self.reduce = shape, n, kind, E, reduce
        self.p = [ML.planner(shape, seed0 + i) for i in range(n)]      # on the entry
        self.q = [ML.planner(shape, seed0 + i) for i in range(n)]      # on the operators
        self.fused_models, self.ref_models = self.models(), self.models()
        self.elites = [None] * n
        self.started = [0] * n                                          # the step at which each planner's episode began
        self.obs0 = ML.observations(shape, n)

    def models(self):
        s, n, E = self.shape, self.n, self.E
        if self.kind == "model":
            return ML.model(s, 3)
        if self.kind == "ensemble":
            return ML.ensemble(s, range(3, 3 + E), self.reduce)
        if self.kind == "model each":
            return [ML.model(s, 3 + i) for i in range(n)]
        return [ML.ensemble(s, range(3 + E * i, 3 + E * (i + 1)), self.reduce) for i in range(n)]

    def per_planner(self, models):
        return models if isinstance(models, list) else [models] * self.n

    def restart(self, i, k):
        for pl in (self.p[i], self.q[i]):
            ML.restart(pl)
        self.elites[i], self.started[i] = None, k

    def step(self, k, member_costs=None):
        """Step k of all planners on the entry and on the operators; compares everything the issue names."""
        from icem_amd import IcemPlanner
        what = (self.shape, self.n, self.kind, self.E, self.reduce, k)
        obs = [ob + 0.02 * k for ob in self.obs0]
        results = IcemPlanner.plan_step_mlp(self.p, self.fused_models, obs, member_costs=member_costs)
        shifting = any(k > s0 for s0 in self.started)
        assert self.p[0].mlp_step_launches == 3 * ITERS + (1 if shifting else 0), (what, "launches")
        assert self.p[0].learned_step_launches == 0, (what, "the RSSM steps' count is their own")
        refs = []
        for i, (q, m) in enumerate(zip(self.q, self.per_planner(self.ref_models))):
            r = ML.operator_step(q, m, obs[i], self.elites[i])
            r["planner"] = q
            self.elites[i] = r["elites"]
            refs.append(r)
        for i, (p, r) in enumerate(zip(self.p, refs)):
            check_planner(p, r, results[i], what + (i,), self.n == 1)
        table = ML.member_table(refs)
        if member_costs is not None:
            got = np_(member_costs[:table.size]).reshape(table.shape)
            assert np.array_equal(got, table), (what, "member_costs")
        if self.kind == "ensemble":   # (as its own rollout_cost / rollout_cost_batch would leave them)
            assert np.array_equal(np_(self.fused_models.member_costs), table), (what, "the ensemble's member_costs")
        if self.kind == "ensemble each":
            for m, r in zip(self.fused_models, refs):
                assert np.array_equal(np_(m.member_costs), r["member_costs"]), (what, "each ensemble's member_costs")
        return results


ARRANGEMENTS = [
    ("o17", 1, "model", 1, "mean"), ("o40", 1, "model", 1, "mean"),
    ("o17", 1, "ensemble", 3, "mean"), ("o40", 1, "ensemble", 3, "mean"),
    ("o17", 1, "ensemble", 3, "max"),
    ("o17", 3, "ensemble", 3, "mean"), ("o40", 3, "ensemble", 3, "mean"),
    ("o17", 3, "model each", 1, "mean"),
    ("o17", 2, "ensemble each", 2, "mean"),
]


# ---- 1. bits against the operator loop -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("caller_buffer", [False, True], ids=["scratch", "callers_member_costs"])
@pytest.mark.parametrize("shape,n,kind,E,reduce", ARRANGEMENTS)
def test_the_step_is_the_operator_loop_bit_for_bit(shape, n, kind, E, reduce, caller_buffer):
    """3 MPC steps; with n = 3 on one ensemble planner 2 starts a new episode at step 1 (no shifted elites, a shorter first pool
    than its peers: 128 against 131).  With and without the caller's member_costs buffer: the same reference, so the same
    outputs."""
    a = Arrangement(shape, n, kind, E, reduce)
    assert a.p[0].mlp_step_ok(n, E, a.per_planner(a.fused_models)[0])
    mc = None
    if caller_buffer:
        need = E * n * (a.p[0].population_sizes[0] + a.p[0].n_reuse)
        mc = torch.full((need + 5,), SENTINEL, dtype=torch.float32, device=ML.DEV)
    for k in range(STEPS):
        if k == 1 and n == 3 and kind == "ensemble":
            a.restart(2, k)
        a.step(k, mc)
    if mc is not None:
        assert bool((mc[-5:] == SENTINEL).all()), "nothing is written behind members * n * max rows"


# ---- 2. identities -----------------------------------------------------------------------------------------------------------
def test_one_shared_model_gives_each_planners_solo_bits():
    """members == 1 with the same pointer three times against three planners stepping alone."""
    from icem_amd import IcemPlanner
    m = ML.model("o17", 3)
    batch = [ML.planner("o17", 11 + i) for i in range(3)]
    solo = [ML.planner("o17", 11 + i) for i in range(3)]
    obs0 = ML.observations("o17", 3)
    for k in range(STEPS):
        obs = [ob + 0.02 * k for ob in obs0]
        res = IcemPlanner.plan_step_mlp(batch, m, obs)
        for i, (b, s) in enumerate(zip(batch, solo)):
            want = IcemPlanner.plan_step_mlp([s], m, [obs[i]])[0]
            assert torch.equal(res[i], want), (k, i)
            for x, y in ((b.mean, s.mean), (b.std, s.std), (b.elites_actions, s.elites_actions), (b.elites_costs, s.elites_costs),
                         (b.executed, s.executed), (b.best_cost, s.best_cost)):
                assert torch.equal(x, y), (k, i)


def test_an_ensemble_of_one_gives_the_plain_models_bits():
    from icem_amd import IcemPlanner
    m, e = ML.model("o40", 3), ML.ensemble("o40", [3])
    a, b = ML.planner("o40", 11), ML.planner("o40", 11)
    ob0 = ML.observations("o40", 1)[0]
    for k in range(STEPS):
        ra = IcemPlanner.plan_step_mlp([a], m, [ob0 + 0.02 * k])
        rb = IcemPlanner.plan_step_mlp([b], e, [ob0 + 0.02 * k])
        assert torch.equal(ra, rb), k
        for x, y in ((a.mean, b.mean), (a.std, b.std), (a.elites_actions, b.elites_actions), (a.elites_costs, b.elites_costs),
                     (a.actions, b.actions), (a.costs, b.costs)):
            assert torch.equal(x, y), k
        assert torch.equal(e.member_costs[0], b.costs[:e.member_costs.shape[1]]), k


# ---- 3. launches: 3 per iteration, + 1 in a step that shifts elites -- from the design, not measured ----------------------------
@pytest.mark.parametrize("n,kind,E", [(1, "model", 1), (3, "ensemble", 3)])
def test_the_launch_count_is_the_designs(n, kind, E):
    from icem_amd import IcemPlanner
    a = Arrangement("o17", n, kind, E)
    assert a.p[0].mlp_step_launches == 0
    for k in range(2):
        IcemPlanner.plan_step_mlp(a.p, a.fused_models, a.obs0)
        assert a.p[0].mlp_step_launches == 3 * ITERS + (1 if k > 0 else 0) == ML.launches(a.p[0], k), (n, k)
        assert all(pl.mlp_step_launches == 0 for pl in a.p[1:]), "counted with the planner that led the step"


# ---- 4. refusals leave everything as it was ------------------------------------------------------------------------------------
def model_struct(m, cost_spec=None):
    from icem_amd import _lib as L
    cost, terms = (m._cost_c, m._terms_c) if cost_spec is None else L.cost_spec_structs(cost_spec)
    st = L.IcemMlpStepModelC(m.obs_dim, m.layers, L.MLP_ACTIVATIONS[m.activation], C.pointer(cost), C.pointer(terms) if terms is not None else None)
    st._keep = (cost, terms)
    return st


def raw(pls, table, obs, mdl, reduce=0, mc=None, res=None, z_r=None):
    """The entry itself: ``table`` [n][members] of parameter addresses."""
    from icem_amd import _lib as L
    k, members = len(pls), len(table[0])
    cbs = [pl._learned_buffers(obs[i].data_ptr()) for i, pl in enumerate(pls)]
    if z_r is not None:
        cbs[0].z_r = z_r.data_ptr()
    hs = (C.c_void_p * k)(*[pl._h for pl in pls])
    bs = (L.IcemPlanBuffersC * k)(*cbs)
    steps = (C.c_int32 * k)(*[pl.mpc_step for pl in pls])
    ptrs = (C.c_void_p * (k * members))(*[a for row in table for a in row])
    return pls[0].lib.icem_plan_step_mlp(hs, k, bs, C.byref(mdl), members, ptrs, reduce, steps, None if mc is None else C.c_void_p(mc.data_ptr()),
                                         None if res is None else C.c_void_p(res.data_ptr()), pls[0]._stream())


def buffers_of(p):
    return (p.mean, p.std, p.elites_actions, p.elites_costs, p.executed, p.best_cost, p.actions, p.costs)


def test_refusals_happen_before_anything_runs():
    from icem_amd import IcemPlanner
    from icem_amd import _lib as L
    from icem_amd.envs import TERM_SUMSQ, CostSpec, CostTerm
    ms = [ML.model("o17", s) for s in (3, 4, 5)]
    ptr = [m.params.data_ptr() for m in ms]
    mdl = model_struct(ms[0])
    beyond = model_struct(ms[0], CostSpec(terms=(CostTerm(TERM_SUMSQ, a=15, len=7),)))   # reads obs[15 .. 21] of 17
    good, mate, third = ML.planner("o17", 21), ML.planner("o17", 22), ML.planner("o17", 24)
    f64 = ML.planner("o17", 25, dtype="f64")
    h11 = ML.planner("o17", 26, horizon=11)
    small = ML.planner("o17", 27, n=112)    # (another configuration)
    all_pls = (good, mate, third, f64, h11, small)
    obs = torch.zeros((3, 17), dtype=torch.float32, device=ML.DEV)
    z = torch.zeros((128, 6, 7), dtype=torch.float32, device=ML.DEV)
    mc = torch.full((3 * 11 * 131,), SENTINEL, dtype=torch.float32, device=ML.DEV)
    res = torch.full((3, 7), SENTINEL, dtype=torch.float32, device=ML.DEV)
    for p in all_pls:
        for t in buffers_of(p):
            t.fill_(SENTINEL)
    kw = dict(mc=mc, res=res)

    def switched_off():
        with option("mlp_step", 0):
            assert not good.mlp_step_ok()
            return raw([good, mate], [ptr] * 2, obs, mdl, **kw)
    cases = [
        ("an f64 handle", lambda: raw([f64], [ptr], obs, mdl, **kw), L.ICEM_E_UNSUPPORTED, b"f32"),
        ("a horizon outside the sampler's list", lambda: raw([h11], [ptr], obs, mdl, **kw), L.ICEM_E_UNSUPPORTED, b"horizon"),
        ("mlp_step = 0", switched_off, L.ICEM_E_UNSUPPORTED, b"mlp_step"),
        ("a non-NULL z_r", lambda: raw([good, mate], [ptr] * 2, obs, mdl, z_r=z, **kw), L.ICEM_E_UNSUPPORTED, b"z_*"),
        ("3 x 11 = 33 problems", lambda: raw([good, mate, third], [[ptr[e % 3] for e in range(11)]] * 3, obs, mdl, **kw),
         L.ICEM_E_UNSUPPORTED, b"32"),
        ("the same handle twice", lambda: raw([good, good], [ptr[:2]] * 2, obs, mdl, **kw), L.ICEM_E_INVALID, b"twice"),
        ("handles of two configurations", lambda: raw([good, small], [ptr[:2]] * 2, obs, mdl, **kw), L.ICEM_E_INVALID, b"one configuration"),
        ("a cost term index beyond obs_dim", lambda: raw([good, mate], [ptr] * 2, obs, beyond, **kw), L.ICEM_E_INVALID, b"cost term slice outside the observation"),
    ]
    for what, call, code, word in cases:
        assert call() == code, (what, good.lib.icem_last_error())
        err = good.lib.icem_last_error()
        assert b"icem_plan_step_mlp" in err and word in err, (what, err)
        torch.cuda.synchronize()
        for p in all_pls:
            assert p.mpc_step == 0 and p.mlp_step_launches == 0, what
            for t in buffers_of(p):
                assert bool((t == SENTINEL).all()), what
        assert bool((mc == SENTINEL).all()) and bool((res == SENTINEL).all()), what
    assert good.mlp_step_ok(2, 3) and good.mlp_step_ok(1, 32) and not good.mlp_step_ok(3, 11) and not good.mlp_step_ok(1, 33)
    assert not f64.mlp_step_ok() and not h11.mlp_step_ok()
    # the Python entry: refused before any planner has advanced
    with option("mlp_step", 0):
        with pytest.raises(L.IcemError) as e:
            IcemPlanner.plan_step_mlp([good, mate], ms[0], np_(obs[:2]))
    assert e.value.code == L.ICEM_E_UNSUPPORTED and good.mpc_step == mate.mpc_step == 0
    # ... and the same handles and buffers are served once the arguments are right: a fresh twin's bits
    twins = [ML.planner("o17", 21), ML.planner("o17", 22)]
    for p in (good, mate):
        p.reset_distribution(p.mean, p.std)
    ob = ML.observations("o17", 2)
    obs[:2].copy_(torch.as_tensor(np.asarray(ob, dtype=np.float32)))
    assert raw([good, mate], [ptr] * 2, obs, mdl, **kw) == 0
    ens = ML.ensemble("o17", (3, 4, 5))
    want = IcemPlanner.plan_step_mlp(twins, ens, ob)
    assert torch.equal(res[:2], want) and good.mlp_step_launches == 3 * ITERS
    assert torch.equal(mc[:3 * 2 * 81].view(3, 162), ens.member_costs)
    for p, t in zip((good, mate), twins):
        for x, y in zip(buffers_of(p)[:6], buffers_of(t)[:6]):
            assert torch.equal(x, y)


# ---- 5. controllers ------------------------------------------------------------------------------------------------------------
N, H = 128, 12


def cmodel(seed, activation="swish"):
    from icem_amd import DeviceMLPModel, halfcheetah_env
    return DeviceMLPModel(17, 6, layers=2, activation=activation, seed=seed, env=halfcheetah_env(17), device=ML.DEV)


def censemble(seeds, reduce="mean"):
    from icem_amd import DeviceMLPEnsemble, halfcheetah_env
    return DeviceMLPEnsemble(seeds=list(seeds), reduce=reduce, obs_dim=17, act_dim=6, layers=2, activation="swish", env=halfcheetah_env(17),
                             device=ML.DEV)


def controller(m, seed=5, cls=None):
    from icem_amd import MpcICemHip, halfcheetah_env
    asp = dict(alpha=0.1, elites_size=10, opt_iterations=ITERS, init_std=0.5, use_mean_actions=True, keep_previous_elites=True,
               shift_elites_over_time=True, fraction_elites_reused=0.3, noise_beta=0.25)
    return (cls or MpcICemHip)(env=halfcheetah_env(17), forward_model=m, horizon=H, num_simulated_trajectories=N, factor_decrease_num=1.25,
                               cost_along_trajectory="sum", dtype="f32", seed=seed, action_sampler_params=asp)


def instrument(m):
    """Replace the instance's rollout_cost by a counting one: such a model is called stage by stage."""
    calls, inner = [], m.rollout_cost

    def counting(obs, actions, cost_mode=0, **kw):
        calls.append(actions.shape[0])
        return inner(obs, actions, cost_mode, **kw)
    m.rollout_cost = counting
    return calls


def cobs(n=1, seed=7):
    rs = np.random.RandomState(seed)
    return [[0.3 * rs.randn(17) + 0.02 * k for k in range(STEPS)] for _ in range(n)]


def begin(c, ob):
    c.beginning_of_rollout(observation=ob, state=None, mode="train")


def same_controller_state(a, b, what):
    assert a.last_min_cost == b.last_min_cost and a.planner.mpc_step == b.planner.mpc_step, what
    for x, y in ((a.mean, b.mean), (a.std, b.std), (np_(a._elite_actions), np_(b._elite_actions)), (np_(a._elite_costs), np_(b._elite_costs))):
        assert np.array_equal(x, y), what


@pytest.mark.parametrize("kind", ["model", "ensemble"])
def test_a_controller_takes_the_fused_call_and_executes_the_stagewise_bits(kind):
    """An uninstrumented controller (the fused call: the launch count says so) against an instrumented twin (stage by stage) and
    against a third one under mlp_step = 0 (stage by stage through the untouched model)."""
    make = (lambda: cmodel(3)) if kind == "model" else (lambda: censemble((3, 4, 5)))
    c, t, s = controller(make()), controller(make()), controller(make())
    calls = instrument(t.forward_model)
    assert c._mlp_step_ok(None, 1) and not t._mlp_step_ok(None, 1)
    assert not c._model_is_the_library_rssm() and not c._model_is_the_library_ensemble()
    obs = cobs()[0]
    for x in (c, t, s):
        begin(x, obs[0])
    for k, ob in enumerate(obs):
        got = c.get_action(ob, None)
        assert c.planner.mlp_step_launches == ML.launches(c.planner, k), (kind, k, "the fused call")
        before = len(calls)
        want = t.get_action(ob, None)
        assert len(calls) - before == ITERS and t.planner.mlp_step_launches == 0, (kind, k, "one rollout_cost per iteration")
        assert np.array_equal(got, want), (kind, k)
        same_controller_state(c, t, (kind, k))
        with option("mlp_step", 0):
            assert not s._mlp_step_ok(None, 1)
            off = s.get_action(ob, None)
        assert s.planner.mlp_step_launches == 0 and np.array_equal(off, want), (kind, k, "mlp_step = 0")
        same_controller_state(s, t, (kind, k, "mlp_step = 0"))
        if kind == "ensemble":
            assert torch.equal(c.forward_model.member_costs, t.forward_model.member_costs), (kind, k, "member_costs")


def test_one_handle_alternates_between_the_fused_and_the_stagewise_step():
    c, t = controller(cmodel(3)), controller(cmodel(3))
    obs = cobs()[0] + [cobs(seed=8)[0][0]]
    begin(c, obs[0])
    begin(t, obs[0])
    for k, ob in enumerate(obs):
        with option("mlp_step", k % 2):   # (c: stage-wise at even steps, fused at odd ones)
            got = c.get_action(ob, None)
        with option("mlp_step", 0):
            want = t.get_action(ob, None)
        assert (c.planner.mlp_step_launches > 0) == (k > 0) and t.planner.mlp_step_launches == 0, k
        assert np.array_equal(got, want), k
        same_controller_state(c, t, k)


def drive_batch(ctrls, twins, own_models, what, restart=None):
    from icem_amd import MpcICemHip
    obs = cobs(len(ctrls))
    for c, t, ob in zip(ctrls, twins, obs):
        begin(c, ob[0])
        begin(t, ob[0])
    for k in range(STEPS):
        obk = [ob[k] for ob in obs]
        if restart is not None and k == 1:   # one controller starts a new episode a step later: no shifted elites, a shorter first pool
            begin(ctrls[restart], obk[restart])
            begin(twins[restart], obk[restart])
        got = MpcICemHip.get_action_batch(ctrls, obk, own_models=own_models)
        shifting = k > 0
        assert ctrls[0].planner.mlp_step_launches == 3 * ITERS + (1 if shifting else 0), (what, k, "one fused call for all")
        for i, (c, t, ob) in enumerate(zip(ctrls, twins, obk)):
            want = t.get_action(ob, None)
            assert np.array_equal(np.asarray(got[i]), want), (what, k, i)
            same_controller_state(c, t, (what, k, i))


def test_get_action_batch_over_one_shared_ensemble():
    ens, twin_ens = censemble((3, 4, 5)), censemble((3, 4, 5))
    drive_batch([controller(ens, seed=s) for s in (1, 2, 3)], [controller(twin_ens, seed=s) for s in (1, 2, 3)], False, "one ensemble", restart=2)


def test_get_action_batch_own_models_over_a_model_each():
    drive_batch([controller(cmodel(3 + i), seed=1 + i) for i in range(3)], [controller(cmodel(3 + i), seed=1 + i) for i in range(3)], True,
                "a model each")


def test_get_action_batch_own_models_over_an_ensemble_each():
    mk = lambda i: censemble((3 + 2 * i, 4 + 2 * i))   # noqa: E731
    ctrls, twins = [controller(mk(i), seed=1 + i) for i in range(2)], [controller(mk(i), seed=1 + i) for i in range(2)]
    drive_batch(ctrls, twins, True, "an ensemble each")
    for c, t in zip(ctrls, twins):
        assert torch.equal(c.forward_model.member_costs, t.forward_model.member_costs)


def test_get_action_batch_own_models_over_a_model_each_steps_stagewise_where_the_entry_refuses():
    """mlp_step = 0: the batch steps stage-wise around ONE mlp_rollout_cost_models launch per iteration (no fused call), the
    bits of each controller's own stage-wise get_action."""
    from icem_amd import MpcICemHip
    ctrls = [controller(cmodel(3 + i), seed=1 + i) for i in range(3)]
    twins = [controller(cmodel(3 + i), seed=1 + i) for i in range(3)]
    obs = cobs(3)
    for c, t, ob in zip(ctrls, twins, obs):
        begin(c, ob[0])
        begin(t, ob[0])
    for k in range(STEPS):
        obk = [ob[k] for ob in obs]
        with option("mlp_step", 0):
            got = MpcICemHip.get_action_batch(ctrls, obk, own_models=True)
            want = [t.get_action(ob, None) for t, ob in zip(twins, obk)]
        for i, (c, t) in enumerate(zip(ctrls, twins)):
            assert c.planner.mlp_step_launches == 0 and t.planner.mlp_step_launches == 0, (k, i, "no fused call")
            assert np.array_equal(np.asarray(got[i]), want[i]), (k, i)
            same_controller_state(c, t, (k, i))


def test_get_action_batch_over_an_ensemble_each_is_refused_where_the_entry_refuses():
    """The stage-wise step has no launch for an ensemble each: under mlp_step = 0 the batch is refused, nothing has advanced."""
    from icem_amd import MpcICemHip
    ctrls = [controller(censemble((3 + 2 * i, 4 + 2 * i)), seed=1 + i) for i in range(2)]
    obs = cobs(2)
    for c, ob in zip(ctrls, obs):
        begin(c, ob[0])
    with option("mlp_step", 0):
        with pytest.raises(NotImplementedError, match="ensemble each.*mlp_step_ok.*call get_action per controller"):
            MpcICemHip.get_action_batch(ctrls, [ob[0] for ob in obs], own_models=True)
    assert [c.planner.mpc_step for c in ctrls] == [0, 0] and all(c.planner.mlp_step_launches == 0 for c in ctrls)


def test_controllers_that_share_one_plain_model_are_still_refused():
    from icem_amd import MpcICemHip
    m = cmodel(3)
    ctrls = [controller(m, seed=s) for s in (1, 2)]
    obs = cobs(2)
    for c, ob in zip(ctrls, obs):
        begin(c, ob[0])
    for own in (False, True):
        with pytest.raises(NotImplementedError, match="the learned-dynamics model has no rollout_cost_batch"):
            MpcICemHip.get_action_batch(ctrls, [ob[0] for ob in obs], own_models=own)
    assert [c.planner.mpc_step for c in ctrls] == [0, 0]


def test_a_compute_new_mean_override_gets_an_observation_behind_a_fused_step():
    from icem_amd import MpcICemHip
    seen = []

    def override(self, obs):
        seen.append(np.asarray(obs, dtype=np.float64).copy())
        return self.mean[-1] * 0 + 0.25
    cls = type("OverridingMpcICemHip", (MpcICemHip,), dict(compute_new_mean=override))
    c = controller(cmodel(4, activation="relu"), cls=cls)
    obs = cobs()[0]
    begin(c, obs[0])
    for k, ob in enumerate(obs):
        c.get_action(ob, None)
        assert c.planner.mlp_step_launches == ML.launches(c.planner, k), k
        assert len(seen) == k + 1 and seen[-1].shape == (17,) and np.isfinite(seen[-1]).all(), (k, seen[-1:])
    assert np.allclose(np.asarray(c.mean)[-1], 0.25)
