"""The float64 rollout on the f64 matrix cores (``icem_set_f64_arith(ICEM_F64_MFMA)``, k_rollout_f64.hip) against the float64
oracle: lane maps on exact integers, shape edges, the whole case table of cost_term_cases.py (the first float64 evaluation
of its o > 32 cases), position independence, whole Philox MPC steps, NaN rows, refusals and the order of the setters.

Tolerances are the suite's own for float64: rtol 1e-10 / atol 1e-12 on costs and observations, rtol 1e-9 / atol 1e-11 on whole
MPC steps (test_gpu_parity.py).  The matrix instruction sums the contraction in blocks of four; re-summing the oracle's model
step that way on the CPU moved the worst row of the case table by 1 % of the bound (relocate-unit25-k0-sum).

``icem_create`` refuses a horizon below 2 for every dtype, so the horizon axis of the shape edges is {2, 30}; that refusal is
asserted here."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import cost_term_cases as CC
from golden_util import Golden
from oracle import icem_oracle as O
from test_gpu_cost_term_probes import device_spec, np_

pytestmark = pytest.mark.gpu

F64_RTOL, F64_ATOL = CC.F64_RTOL, CC.F64_ATOL
STEP_TOL = dict(rtol=1e-9, atol=1e-11)
BUILTIN = lambda o: O.CostSpec(0.1, o - 1, -1.0, min(1, o - 1), 10.0, 0.3)  # noqa: E731


def mk(o, d, h, model=None, spec=None, mode="sum", arith="mfma", N=64, cost_first=False, **cfg):
    """An f64 planner with ``arith`` set BEFORE the model; spec: an oracle CostSpec (None: none set)."""
    from icem_amd import IcemConfig, IcemPlanner
    pl = IcemPlanner(IcemConfig(horizon=h, act_dim=d, num_traj=N, dtype="f64", cost_mode=mode, **cfg), -np.ones(d), np.ones(d))
    if arith is not None:
        assert pl.set_f64_arith(arith) == arith
    if cost_first and spec is not None:
        pl.set_cost_spec(device_spec(spec))
    if model is not None:
        pl.set_model(model.kind, model.A, model.B)
    if not cost_first and spec is not None:
        pl.set_cost_spec(device_spec(spec))
    return pl


def roll(pl, obs0, acts, observations=True):
    out = pl.rollout_cost(obs0, torch.as_tensor(acts, dtype=pl.dt, device=pl.device), return_observations=observations)
    return (np_(out[0]), np_(out[1])) if observations else np_(out)


# ---- 1. exact integers: the lane maps ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["final", "sum"])
def test_integer_model_is_reproduced_bitwise(mode):
    """o = 35 (three column tiles, the last with 3 columns), d = 6 (contraction 41: a ragged block of four), n = 17 (a second
    row tile with one row): every product and sum is an integer below 2^53, so any row / column / k mix-up changes bits."""
    o, d, h, n = 35, 6, 4, 17
    rs = np.random.RandomState(5)
    A = rs.randint(-2, 4, (o, o)).astype(np.float64) * (rs.uniform(size=(o, o)) < 0.3)
    B = rs.randint(-3, 5, (d, o)).astype(np.float64)
    obs0 = rs.randint(-4, 6, o).astype(np.float64)
    acts = rs.randint(-3, 4, (n, h, d)).astype(np.float64)
    om = O.SyntheticModel(A, B, O.MODEL_LINEAR)
    spec = O.CostSpec(2.0, 33, -3.0, 34, 10.0, 0.5)
    want_obs = O.rollout_observations(om, obs0, acts)
    assert 100 < np.abs(want_obs[:, -1]).max() and np.abs(want_obs).max() < 2.0 ** 40   # grown, and exact in float64
    assert len({tuple(r) for r in want_obs[:, -1]}) == n
    want = O.rollout_costs(om, spec, obs0, acts, mode=mode)
    pl = mk(o, d, h, om, spec, mode)
    got, got_obs = roll(pl, obs0, acts)
    assert np.array_equal(got_obs, want_obs), np.argwhere(got_obs != want_obs)[:8]
    assert np.array_equal(got, want), (got, want)
    assert np.array_equal(roll(pl, obs0, acts, observations=False), want)   # the instantiation that writes no observations


# ---- 2. shape edges ----------------------------------------------------------------------------------------------------------
EDGES = [  # o, d, n, h, kind, mode            (o + d) mod 4
    (1, 3, 1, 2, 0, "sum"),                  # 0
    (15, 2, 15, 30, 1, "best"),              # 1
    (16, 6, 16, 2, 0, "final"),              # 2
    (17, 6, 17, 30, 1, "sum"),               # 3
    (32, 5, 33, 2, 1, "best"),               # 1
    (33, 7, 17, 30, 0, "final"),             # 0
    (48, 1, 33, 2, 1, "sum"),                # 1
    (113, 8, 15, 30, 0, "best"),             # 1
    (378, 17, 33, 30, 1, "final"),           # 3
    (384, 64, 17, 2, 0, "sum"),              # 0: the largest LDS tile
    (384, 64, 16, 30, 1, "best"),
]


@pytest.mark.parametrize("o,d,n,h,kind,mode", EDGES)
def test_shape_edges_against_the_oracle(o, d, n, h, kind, mode):
    rs = np.random.RandomState(o + d)
    om = O.SyntheticModel.make(o, d, kind)
    spec = BUILTIN(o)
    obs0, acts = rs.randn(o), rs.uniform(-1, 1, (n, h, d))
    pl = mk(o, d, h, om, spec, mode)
    got, got_obs = roll(pl, obs0, acts)
    want, want_obs = O.rollout_costs(om, spec, obs0, acts, mode=mode), O.rollout_observations(om, obs0, acts)
    print(o, d, n, h, kind, mode, "cost err", np.abs(got - want).max(), "obs err", np.abs(got_obs - want_obs).max())
    np.testing.assert_allclose(got_obs, want_obs, rtol=F64_RTOL, atol=F64_ATOL)
    np.testing.assert_allclose(got, want, rtol=F64_RTOL, atol=F64_ATOL)
    np.testing.assert_array_equal(roll(pl, obs0, acts, observations=False), got)


def test_horizon_one_is_refused_at_create():
    from icem_amd import IcemConfig, IcemPlanner
    with pytest.raises(Exception, match="UNSUPPORTED"):
        IcemPlanner(IcemConfig(horizon=1, act_dim=2, num_traj=8, dtype="f64"), -np.ones(2), np.ones(2))


# ---- 3. the case table -------------------------------------------------------------------------------------------------------
_planners = {}


def _case_costs(case):
    om, ob, acts = CC.inputs(case)
    key = (case.o, case.d, case.h, case.mode, case.high)
    if key not in _planners:   # (this module's own planners: the probes' float64 planners stay on the chain)
        from icem_amd import IcemConfig, IcemPlanner
        pl = IcemPlanner(IcemConfig(horizon=case.h, act_dim=case.d, num_traj=1100, opt_iters=1, dtype="f64", seed=7, cost_mode=case.mode),
                         -case.high * np.ones(case.d), case.high * np.ones(case.d))
        pl.set_f64_arith("mfma")
        _planners[key] = pl
    pl = _planners[key]
    pl.set_model(om.kind, om.A, om.B)
    pl.set_cost_spec(device_spec(case.spec))
    return roll(pl, ob, acts, observations=False)


@pytest.mark.parametrize("group", sorted({c.group for c in CC.CASES}))
def test_case_table_in_float64(group):
    """Every case of cost_term_cases.CASES through icem_rollout_cost, under the criterion of the probes' general-f64."""
    bad, worst = [], 0.0
    for case in (c for c in CC.CASES if c.group == group):
        got, w = _case_costs(case), CC.want(case)
        assert got.shape == w.shape
        excess = np.abs(got - w) / (F64_ATOL + F64_RTOL * np.abs(w))
        worst = max(worst, float(excess.max()))
        if not (excess <= 1.0).all():
            bad.append(f"{case.name} {case.what}: f64 costs off by {np.abs(got - w).max():.3g} ({excess.max():.3g} of the bound)")
    print(group, "worst error / bound", worst)
    assert not bad, f"{len(bad)} violations:\n" + "\n".join(bad[:40])


# ---- 4. position independence ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["door", "standup"])
def test_a_row_costs_the_same_wherever_it_sits(shape):
    rs = np.random.RandomState(11)
    if shape == "door":
        o, d, h, spec, kind = 39, 28, 30, O.CostSpec.door(), 1
    else:
        o, d, h, spec, kind = 378, 17, 12, O.CostSpec.humanoid_standup(), 0
    om = O.SyntheticModel.make(o, d, kind)
    pl = mk(o, d, h, om, spec)
    obs0, acts = 0.2 * rs.randn(o), rs.uniform(-1, 1, (50, h, d))
    base = roll(pl, obs0, acts, observations=False)
    perm = rs.permutation(50)
    assert not np.array_equal(perm, np.arange(50))
    np.testing.assert_array_equal(roll(pl, obs0, acts[perm], observations=False), base[perm])
    np.testing.assert_array_equal(roll(pl, obs0, acts[37:38], observations=False), base[37:38])


# ---- 5. whole steps ----------------------------------------------------------------------------------------------------------
def _oracle(om, spec, env_low, env_high, h, N, iters, seed, d):
    noise = O.PhiloxNoiseSchedule(seed, iters, d, h, dtype=np.float64)
    orc = O.IcemOracle(O.IcemParams(horizon=h, num_simulated_trajectories=N, opt_iterations=iters), env_low, env_high,
                       lambda ob, ac: O.rollout_costs(om, spec, ob, ac), lambda num: tuple(z.astype(np.float64) for z in noise(num)))
    orc.beginning_of_rollout()
    return orc, noise


@pytest.mark.parametrize("shape", ["standup", "door", "halfcheetah"])
def test_philox_mpc_steps_match_the_oracle(shape):
    """plan_step x 3 against IcemOracle + PhiloxNoiseSchedule: executed actions, mean, and per iteration the elite set (its
    costs, and its rows: the oracle's pool rows at the oracle's elite indices).  The per-iteration form and the one-call
    icem_plan_step are both run and must agree bit for bit."""
    from icem_amd import envs as E
    if shape == "standup":
        env, spec, kind, h, N = E.humanoid_standup_env(378), O.CostSpec.humanoid_standup(), 1, 12, 80
    elif shape == "door":
        env, spec, kind, h, N = E.door_env(), O.CostSpec.door(), 1, 30, 80
    else:
        env, spec, kind, h, N = E.halfcheetah_env(17), O.CostSpec.halfcheetah(17), 1, 30, 200
    o, d, iters, seed = env.obs_dim, env.action_space.shape[0], 3, 99
    lo, hi = env.action_space.low.astype(np.float64), env.action_space.high.astype(np.float64)
    om = O.SyntheticModel.make(o, d, kind)

    def planner():
        from icem_amd import IcemConfig, IcemPlanner
        pl = IcemPlanner(IcemConfig(horizon=h, act_dim=d, num_traj=N, opt_iters=iters, dtype="f64", seed=seed), lo, hi)
        pl.set_f64_arith("mfma")
        pl.set_model(om.kind, om.A, om.B)
        pl.set_cost_spec(env.cost_spec)
        pl.reset()
        return pl

    a, b = planner(), planner()
    orc, noise = _oracle(om, spec, lo, hi, h, N, iters, seed, d)
    for s in range(3):
        ob = 0.1 * np.random.RandomState(s).randn(o)
        if s:
            noise.begin_step()
        want = orc.get_action(ob)
        trace = orc.trace[-1]

        def check(it):
            tr = trace[it]
            gi = (a.mpc_step * iters + it + 1) & 1
            np.testing.assert_allclose(np_(a.elites_costs[gi]), tr.costs[tr.elite_idx], **STEP_TOL)
            pool = tr.actions if tr.costs.shape[0] == tr.actions.shape[0] else None
            ea = np_(a.elites_actions[gi])
            for r, e in enumerate(tr.elite_idx):   # the same rows: the elite index set (kept elites sit behind the pool)
                if pool is not None or e < tr.actions.shape[0]:
                    np.testing.assert_allclose(ea[r], tr.actions[e], **STEP_TOL)

        got = np_(a.plan_step(ob, on_iteration=check))
        np.testing.assert_allclose(got, want, **STEP_TOL)
        np.testing.assert_array_equal(np_(b.plan_step(ob)), got)   # icem_plan_step: the same launches
    np.testing.assert_allclose(np_(a.mean), orc.mean, **STEP_TOL)
    np.testing.assert_array_equal(np_(b.mean), np_(a.mean))


def test_golden_replay_with_external_noise():
    """The reference's own white draws (z_r / z_i) through the sampler, the matrix-core rollout and the selection."""
    g = Golden("c1_halfcheetah_n128")
    from icem_amd import IcemConfig, IcemPlanner
    pl = IcemPlanner(IcemConfig(horizon=g.h, act_dim=g.d, num_traj=g.N, elites_size=g.K, opt_iters=g.iters, cost_mode=g.cost_mode,
                                use_mean_actions=g.use_mean, keep_previous_elites=g.keep, shift_elites=g.shift, factor_decrease=g.gamma,
                                alpha=g.alpha, init_std=g.init_std, fraction_reused=g.xi, noise_beta=g.beta, dtype="f64", seed=1234),
                     g.low, g.high)
    pl.set_f64_arith("mfma")
    pl.set_model(g.kind, g.A, g.B)
    spec = O.CostSpec.halfcheetah(g.o) if g.env_kind == "halfcheetah" else O.CostSpec.humanoid_standup()
    pl.set_cost(spec.ctrl_weight, spec.lin_idx, spec.lin_weight, spec.flip_idx, spec.flip_penalty, spec.flip_thresh)
    pl.reset()
    calls = iter(range(g.n_noise_calls))
    it_global = [0]
    t = dict(rtol=F64_RTOL, atol=F64_ATOL)

    def noise(num):
        zr, zi = g.noise(next(calls))
        assert zr.shape[0] == num
        return zr, zi

    for s in range(g.n_steps):
        def check(it):
            ref = g.it(it_global[0])
            gi = (pl.mpc_step * g.iters + it + 1) & 1
            np.testing.assert_allclose(np_(pl.elites_costs[gi]), ref["costs"][ref["elite"]], **t)
            it_global[0] += 1

        np.testing.assert_allclose(np_(pl.plan_step(g.obs[s], noise=noise, on_iteration=check)), g.executed[s], **t)
    assert next(calls, None) is None


def test_emulated_world_of_two_equals_world_one():
    """o = 40: two planners whose records are concatenated in place of the all-gather reproduce world 1 bit for bit."""
    from icem_amd import IcemConfig, IcemPlanner, _lib as L
    o, d, h, N, iters, seed = 40, 6, 12, 200, 3, 99
    om = O.SyntheticModel.make(o, d, 1)
    spec = O.CostSpec(0.1, 8, -1.0, 1, 10.0, float(np.pi / 2))

    def planner(rank, world):
        pl = IcemPlanner(IcemConfig(horizon=h, act_dim=d, num_traj=N, opt_iters=iters, dtype="f64", seed=seed, rank=rank, world=world),
                         -np.ones(d), np.ones(d))
        pl.set_f64_arith("mfma")
        pl.set_model(om.kind, om.A, om.B)
        pl.set_cost_spec(device_spec(spec))
        pl.reset()
        return pl

    obs_seq = [0.1 * np.random.RandomState(s).randn(o) for s in range(2)]
    single = planner(0, 1)
    acts1 = [np_(single.plan_step(ob)).copy() for ob in obs_seq]
    orc, noise = _oracle(om, spec, -np.ones(d), np.ones(d), h, N, iters, seed, d)
    for s, ob in enumerate(obs_seq):
        if s:
            noise.begin_step()
        np.testing.assert_allclose(acts1[s], orc.get_action(ob), **STEP_TOL)
    pls = [planner(r, 2) for r in range(2)]
    st = pls[0]._stream()
    for s, ob in enumerate(obs_seq):
        for pl in pls:
            pl.obs0.copy_(torch.as_tensor(ob, dtype=pl.dt))
        for it in range(iters):
            for pl in pls:
                L.check(pl.lib.icem_plan_iter_local(pl._h, C.byref(pl._cb), s, it, st))
            K = pls[0].K
            full = torch.cat([pl.records[r * K:(r + 1) * K] for r, pl in enumerate(pls)], dim=0)
            for pl in pls:
                pl.records.copy_(full)
                L.check(pl.lib.icem_plan_iter_merge(pl._h, C.byref(pl._cb), s, it, st))
        for pl in pls:
            assert np.array_equal(np_(pl.executed), acts1[s])
    for pl in pls:
        assert np.array_equal(np_(pl.mean), np_(single.mean))


def test_controller_on_door_equals_a_planner_driven_directly():
    from icem_amd import DeviceSyntheticModel, IcemConfig, IcemPlanner, MpcICemHip
    from icem_amd import envs as E
    env = E.door_env()
    model = DeviceSyntheticModel.make(39, 28, kind=1)
    params = dict(alpha=0.1, elites_size=10, opt_iterations=3, init_std=0.5, use_mean_actions=True, keep_previous_elites=True,
                  shift_elites_over_time=True, fraction_elites_reused=0.3, noise_beta=2.0)
    ctrl = MpcICemHip(env=env, forward_model=model, horizon=30, num_simulated_trajectories=80, factor_decrease_num=1.25,
                      cost_along_trajectory="sum", dtype="f64", f64_arith="mfma", seed=4, action_sampler_params=params)
    assert ctrl.device_path and ctrl.planner.f64_arith == "mfma" and ctrl.planner.obs_dim == 39
    pl = IcemPlanner(IcemConfig(horizon=30, act_dim=28, num_traj=80, elites_size=10, opt_iters=3, factor_decrease=1.25, alpha=0.1,
                                init_std=0.5, fraction_reused=0.3, noise_beta=2.0, dtype="f64", seed=4),
                     env.action_space.low, env.action_space.high)
    pl.set_f64_arith("mfma")
    pl.set_model(model.kind, model.A, model.B)
    pl.set_cost_spec(env.cost_spec)
    pl.new_episode()
    pl.reset()
    obs = [0.1 * np.random.RandomState(40 + s).randn(39) for s in range(2)]
    ctrl.beginning_of_rollout(observation=obs[0], state=None, mode="train")
    for ob in obs:
        np.testing.assert_array_equal(ctrl.get_action(ob, None), np_(pl.plan_step(ob)))
    bt = ctrl._last_predicted_observation(obs[-1], np.zeros((30, 28)))   # observations at o = 39 in float64
    om = O.SyntheticModel(model.A, model.B, model.kind)
    np.testing.assert_allclose(bt, O.rollout_observations(om, obs[-1], np.zeros((1, 30, 28)))[0, -1], rtol=F64_RTOL, atol=F64_ATOL)


# ---- 6. NaN ------------------------------------------------------------------------------------------------------------------
def test_nan_stays_in_its_row():
    o, d, h, n = 40, 6, 12, 17
    rs = np.random.RandomState(2)
    om, spec = O.SyntheticModel.make(o, d, 1), O.CostSpec(0.1, 8, -1.0, 1, 10.0, 0.3)
    pl = mk(o, d, h, om, spec)
    obs0, acts = 0.2 * rs.randn(o), rs.uniform(-1, 1, (n, h, d))
    want = O.rollout_costs(om, spec, obs0, acts)
    bad_obs = obs0.copy()
    bad_obs[23] = np.nan
    assert np.isnan(roll(pl, bad_obs, acts, observations=False)).all()   # every row starts from that observation
    bad_acts = acts.copy()
    bad_acts[5, 3, 2] = np.nan
    got = roll(pl, obs0, bad_acts, observations=False)
    assert np.isnan(got[5])
    keep = np.arange(n) != 5
    np.testing.assert_allclose(got[keep], want[keep], rtol=F64_RTOL, atol=F64_ATOL)   # its 15 tile-mates and the second tile
    # an infinite entry: what the reference's matmul makes of it -- +-1 behind a tanh, inf - inf = NaN in a linear model
    bad_obs[23] = np.inf
    np.testing.assert_allclose(roll(pl, bad_obs, acts, observations=False), O.rollout_costs(om, spec, bad_obs, acts),
                               rtol=F64_RTOL, atol=F64_ATOL, equal_nan=True)
    lin = O.SyntheticModel.make(o, d, 0)
    with np.errstate(invalid="ignore"):
        want_lin = O.rollout_costs(lin, spec, bad_obs, acts)
    assert not np.isfinite(want_lin).any()
    np.testing.assert_allclose(roll(mk(o, d, h, lin, spec), bad_obs, acts, observations=False), want_lin, rtol=F64_RTOL, atol=F64_ATOL,
                               equal_nan=True)


# ---- 7. refusals and state ---------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was():
    from icem_amd import IcemConfig, IcemPlanner
    d, h = 5, 12
    rs = np.random.RandomState(9)
    acts = rs.uniform(-1, 1, (33, h, d))
    # the default mode still refuses o = 40 on f64, and reports the chain
    dflt = mk(40, d, h, arith=None)
    assert dflt.f64_arith == "chain"
    with pytest.raises(Exception, match="UNSUPPORTED"):
        dflt.set_model(0, np.eye(40), np.zeros((d, 40)))
    # an f32 handle
    om17, spec17 = O.SyntheticModel.make(17, d, 1), BUILTIN(17)
    f32 = IcemPlanner(IcemConfig(horizon=h, act_dim=d, num_traj=64, dtype="f32"), -np.ones(d), np.ones(d))
    f32.set_model(om17.kind, om17.A, om17.B)
    f32.set_cost_spec(device_spec(spec17))
    obs17 = rs.randn(17)
    before = np_(f32.rollout_cost(obs17, torch.as_tensor(acts, dtype=f32.dt, device=f32.device)))
    with pytest.raises(Exception, match="UNSUPPORTED"):
        f32.set_f64_arith("mfma")
    assert f32.f64_arith == "chain"
    np.testing.assert_array_equal(np_(f32.rollout_cost(obs17, torch.as_tensor(acts, dtype=f32.dt, device=f32.device))), before)
    # a bad mode value; back to the chain on a wide model
    om40, spec40 = O.SyntheticModel.make(40, d, 1), BUILTIN(40)
    wide = mk(40, d, h, om40, spec40)
    obs40 = rs.randn(40)
    before = roll(wide, obs40, acts, observations=False)
    for mode, code in ((2, "INVALID"), (-1, "INVALID"), ("chain", "UNSUPPORTED")):
        with pytest.raises(Exception, match=code):
            wide.set_f64_arith(mode)
        assert wide.f64_arith == "mfma"
        np.testing.assert_array_equal(roll(wide, obs40, acts, observations=False), before)
    np.testing.assert_allclose(before, O.rollout_costs(om40, spec40, obs40, acts), rtol=F64_RTOL, atol=F64_ATOL)
    # more than 32 elites at a wide observation: the selection runs on the cost array
    many = mk(40, d, h, om40, spec40, N=200, elites_size=40, opt_iters=2)
    assert many.K == 40
    many.reset()
    assert np.isfinite(np_(many.plan_step(obs40))).all()


def test_batched_f64_step_refuses_mfma_handles():
    from icem_amd import IcemPlanner
    o, d, h = 17, 6, 12
    om, spec = O.SyntheticModel.make(o, d, 1), BUILTIN(o)
    pls = [mk(o, d, h, om, spec, N=128, opt_iters=2, seed=s) for s in range(2)]
    obs = [0.1 * np.random.RandomState(s).randn(o) for s in range(2)]
    for pl, ob in zip(pls, obs):
        pl.reset()
        pl.plan_step(ob)
    state = [(np_(pl.mean).copy(), np_(pl.executed).copy(), np_(pl.costs).copy(), pl.mpc_step) for pl in pls]
    with pytest.raises(Exception, match="UNSUPPORTED"):
        IcemPlanner.plan_step_batch_f64(pls, obs)
    for pl, (mean, ex, costs, step) in zip(pls, state):
        assert pl.mpc_step == step and pl.f64_arith == "mfma"
        np.testing.assert_array_equal(np_(pl.mean), mean)
        np.testing.assert_array_equal(np_(pl.executed), ex)
        np.testing.assert_array_equal(np_(pl.costs), costs)
    # ... and a chain handle beside an MFMA handle is refused as well
    pls[0].set_f64_arith("chain")
    with pytest.raises(Exception, match="UNSUPPORTED"):
        IcemPlanner.plan_step_batch_f64(pls, obs)


@pytest.mark.parametrize("o,spec", [(17, BUILTIN(17)), (39, O.CostSpec.door())], ids=["o17", "door"])
def test_the_device_copies_follow_whichever_setter_came_last(o, spec):
    d, h = (6, 12) if o == 17 else (28, 12)
    rs = np.random.RandomState(o)
    om, other = O.SyntheticModel.make(o, d, 1), O.SyntheticModel.make(o, d, 0)
    obs0, acts = 0.2 * rs.randn(o), rs.uniform(-1, 1, (33, h, d))
    other_spec = dataclasses.replace(spec, ctrl_weight=0.7)
    base = roll(mk(o, d, h, om, spec), obs0, acts, observations=False)                       # mode, model, cost
    np.testing.assert_allclose(base, O.rollout_costs(om, spec, obs0, acts), rtol=F64_RTOL, atol=F64_ATOL)
    np.testing.assert_array_equal(roll(mk(o, d, h, om, spec, cost_first=True), obs0, acts, observations=False), base)   # mode, cost, model
    pl = mk(o, d, h, other, other_spec)
    pl.set_cost_spec(device_spec(spec))   # a cost replaced after the model, then the model replaced after the cost
    pl.set_model(om.kind, om.A, om.B)
    np.testing.assert_array_equal(roll(pl, obs0, acts, observations=False), base)
    pl.set_cost_spec(device_spec(other_spec))
    assert not np.array_equal(roll(pl, obs0, acts, observations=False), base)
    pl.set_cost_spec(device_spec(spec))
    np.testing.assert_array_equal(roll(pl, obs0, acts, observations=False), base)
    if o <= 32:   # model and cost set on the chain, the mode switched last
        late = mk(o, d, h, om, spec, arith=None)
        chain = roll(late, obs0, acts, observations=False)
        assert late.set_f64_arith("mfma") == "mfma"
        np.testing.assert_array_equal(roll(late, obs0, acts, observations=False), base)
        late.set_cost_spec(device_spec(other_spec))   # a cost set between two switches
        assert late.set_f64_arith("chain") == "chain" and late.set_f64_arith("mfma") == "mfma"
        late.set_cost_spec(device_spec(spec))
        np.testing.assert_array_equal(roll(late, obs0, acts, observations=False), base)
        np.testing.assert_allclose(chain, base, rtol=F64_RTOL, atol=F64_ATOL)


def test_switching_back_to_the_chain_reproduces_a_twin_that_never_switched():
    o, d, h = 17, 6, 30
    om, spec = O.SyntheticModel.make(o, d, 1), O.CostSpec.halfcheetah(17)
    rs = np.random.RandomState(1)
    obs0, acts = 0.1 * rs.randn(o), rs.uniform(-1, 1, (100, h, d))
    twin = mk(o, d, h, om, spec, arith=None, N=200, opt_iters=3, seed=3)
    sw = mk(o, d, h, om, spec, arith="mfma", N=200, opt_iters=3, seed=3)
    sw.reset()
    sw.plan_step(obs0)
    assert sw.set_f64_arith("chain") == "chain"
    np.testing.assert_array_equal(roll(sw, obs0, acts)[0], roll(twin, obs0, acts)[0])
    np.testing.assert_array_equal(roll(sw, obs0, acts)[1], roll(twin, obs0, acts)[1])
    sw.reset()
    twin.reset()
    for s in range(2):
        ob = 0.1 * np.random.RandomState(20 + s).randn(o)
        np.testing.assert_array_equal(np_(sw.plan_step(ob)), np_(twin.plan_step(ob)))
    np.testing.assert_array_equal(np_(sw.mean), np_(twin.mean))
