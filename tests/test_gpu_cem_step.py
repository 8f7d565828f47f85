"""``icem_plan_step_cem`` (cem_step.hip, k_cem.hip): the MPC step of the truncated-normal CEM baseline (``MpcCemStd.get_action``,
icem/controllers/mpc.py:200-262) as one library call, held bit for bit to its stage-wise twin -- a second planner driven by the
operator loop of ``MpcCemStdHip`` (restated below) on the same seed and episode.  After each of 3 MPC steps ``array_equal`` holds
on the executed action, the best cost, mean, std, lower, upper, the elite set, its costs and indices, and the last pool and its
costs, at the smallest shapes where each kernel can go wrong; bounds are asymmetric (low = -0.7, high = 0.9), so lower != -upper
and the sampler's clamp is live.  Then the controller: fused against stage-wise, fused against the NumPy oracle on the same Philox
uniforms, the launch count, a captured step's replay, and the refusals (nothing touched, the controller falls back to the loop)."""
import dataclasses
import itertools

import numpy as np
import pytest
import torch

from oracle import icem_oracle as O   # checker only

pytestmark = pytest.mark.gpu

LOW, HIGH = -0.7, 0.9
STEPS = 3


def np_(t):
    return t.detach().cpu().numpy().astype(np.float64)


def planner(dtype, N, h, d, o, kind, *, K=10, iters=3, mode="sum", alpha=0.1, rounds=10, wide=None, f64_arith=None, spec=None,
            seed=5, **cfg):
    from icem_amd import DeviceSyntheticModel, IcemConfig, IcemPlanner
    c = dict(horizon=h, act_dim=d, num_traj=N, elites_size=K, opt_iters=iters, cost_mode=mode, use_mean_actions=False,
             keep_previous_elites=False, shift_elites=False, factor_decrease=1.0, alpha=alpha, init_std=0.5, dtype=dtype,
             rng_rounds=rounds, seed=seed)
    c.update(cfg)
    pl = IcemPlanner(IcemConfig(**c), LOW * np.ones(d), HIGH * np.ones(d))
    if f64_arith is not None:
        assert pl.set_f64_arith(f64_arith) == f64_arith   # (before the model: only "mfma" serves o > 32)
    m = DeviceSyntheticModel.make(o, d, kind=kind, seed_a=11, seed_b=12)
    pl.set_model(m.kind, m.A, m.B)
    if spec is None:
        pl.set_cost(0.1, o - 1, -1.0, min(1, o - 1), 10.0, 0.3)
    else:
        pl.set_cost_spec(spec)
    if wide is not None:
        assert pl.set_wide_arith(wide) == wide
    pl.new_episode()
    return pl


class Dist:
    """mean / std / lower / upper of one controller, as ``MpcCemStdHip.beginning_of_rollout`` makes them (mpc.py:158-170)."""

    def __init__(self, pl, like_levine):
        self.mean = torch.empty((pl.h, pl.d), dtype=pl.dt, device=pl.device)
        self.std = torch.empty_like(self.mean)
        pl.reset_distribution(self.mean, self.std)
        self.lower, self.upper = pl.cem_bounds(self.mean, self.std, like_levine)
        pl.mpc_step = 0


def loop_step(pl, s, obs, like_levine, shift_means, execute_best_elite):
    """The stage-wise step: the operator loop of ``MpcCemStdHip._step_stagewise`` (icem_amd/controllers.py) with the default
    ``compute_new_mean``.  -> the buffers the fused step is compared on."""
    N, K, iters = pl.cfg.num_traj, pl.K, pl.cfg.opt_iters
    actions = costs = costs_sorted = idx = elites = None
    for i in range(iters):
        actions = pl.sample_truncnorm(N, s.mean, s.std, s.lower, s.upper, None, offset=pl.noise_offset(pl.mpc_step * iters + i))
        costs = pl.rollout_cost(obs, actions)
        if pl.can_update_in_one_launch(N, K):
            costs_sorted, idx, elites = pl.update_distribution(costs, actions, K, s.mean, s.std)
        else:
            costs_sorted, idx = pl.topk_sorted(costs, K)
            elites = pl.gather_refit(actions, idx, s.mean, s.std)
        s.lower, s.upper = pl.cem_bounds(s.mean, s.std, like_levine)
    executed = (elites[0, 0] if execute_best_elite else s.mean[0]).clone()
    if shift_means:
        last = torch.zeros_like(s.mean[-1]) if like_levine else s.mean[-1].clone()
        s.mean[:-1] = s.mean[1:].clone()
        s.mean[-1] = last
    else:
        s.mean.zero_()
    pl.reset_distribution(torch.empty_like(s.mean), s.std)
    s.lower, s.upper = pl.cem_bounds(s.mean, s.std, like_levine)
    pl.mpc_step += 1
    return dict(executed=executed, best_cost=costs_sorted[:1], mean=s.mean, std=s.std, lower=s.lower, upper=s.upper, elites=elites,
                elite_costs=costs_sorted, elite_idx=idx, actions=actions, costs=costs)


def fused_step(pl, s, obs, like_levine, shift_means, execute_best_elite):
    ex = pl.plan_step_cem(obs, s.mean, s.std, s.lower, s.upper, like_levine=like_levine, shift_means=shift_means,
                          execute_best_elite=execute_best_elite)
    return dict(executed=ex, best_cost=pl.cem_result[pl.d:], mean=s.mean, std=s.std, lower=s.lower, upper=s.upper,
                elites=pl.cem_elites, elite_costs=pl.cem_elite_costs, elite_idx=pl.cem_elite_idx, actions=pl.cem_actions,
                costs=pl.cem_costs)


def observation(o, s):
    return 0.1 * np.random.RandomState(100 + s).randn(o)


def run_against_the_loop(make, o, flags=(False, True, True), steps=STEPS):
    fused, twin = make(), make()
    assert fused.cem_step_ok()
    sf, st = Dist(fused, flags[0]), Dist(twin, flags[0])
    for s in range(steps):
        obs = observation(o, s)
        got, want = fused_step(fused, sf, obs, *flags), loop_step(twin, st, obs, *flags)
        torch.cuda.synchronize()
        for k in want:
            assert np.array_equal(np_(got[k]), np_(want[k])), (s, k)
        assert fused.mpc_step == twin.mpc_step == s + 1
        assert fused.cem_step_launches == 3 * fused.cfg.opt_iters and twin.cem_step_launches == 0
    lo, up = np_(sf.lower), np_(sf.upper)
    if not flags[0]:
        assert not np.array_equal(lo, -up)   # asymmetric action bounds: the two probability tables differ
    return fused, sf


# dtype, N, h, d, o, kind, extra
SHAPES = [
    ("f32", 250, 30, 6, 17, 0, {}),                       # tile kernels, ragged sampler and rollout workgroups
    ("f32", 64, 12, 4, 8, 1, dict(K=40)),                 # generic rollout, K = min(elites, N / 2) = 32
    ("f32", 200, 40, 6, 16, 0, {}),                       # HMAX = 64
    ("f32", 120, 13, 3, 24, 1, dict(rounds=7)),           # rng_rounds 7
    ("f32", 4500, 30, 6, 17, 0, {}),                      # a pool above 4096 keys
    ("f32", 96, 12, 5, 40, 1, dict(wide="f32")),          # GEMM-kernel rollout in exact f32
    ("f64", 250, 30, 6, 17, 0, {}),
    ("f64", 64, 12, 4, 8, 1, {}),
    ("f64", 96, 12, 5, 40, 1, dict(f64_arith="mfma")),
]


@pytest.mark.parametrize("dtype,N,h,d,o,kind,extra", SHAPES)
def test_the_fused_step_equals_the_operator_loop_bit_for_bit(dtype, N, h, d, o, kind, extra):
    fused, _ = run_against_the_loop(lambda: planner(dtype, N, h, d, o, kind, **extra), o)
    if extra.get("K") == 40:
        assert fused.K == 32


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("like_levine,shift_means,execute_best_elite", list(itertools.product((False, True), repeat=3)))
def test_every_flag_combination(dtype, like_levine, shift_means, execute_best_elite):
    run_against_the_loop(lambda: planner(dtype, 250, 30, 6, 17, 0), 17, (like_levine, shift_means, execute_best_elite))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("what", [dict(alpha=0.0), dict(alpha=0.9), dict(K=2), dict(K=32), dict(mode="best"), dict(mode="final")])
def test_momentum_elite_counts_and_cost_modes(dtype, what):
    fused, _ = run_against_the_loop(lambda: planner(dtype, 250, 30, 6, 17, 0, **what), 17)
    if "K" in what:
        assert fused.K == what["K"]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_a_term_list_cost(dtype):
    from icem_amd import reacher_env
    env = reacher_env()
    run_against_the_loop(lambda: planner(dtype, 200, 30, 2, env.obs_dim, 0, spec=env.cost_spec), env.obs_dim)


# ---- the controller -----------------------------------------------------------------------------------------------------------
def controller(fused_step, dtype="f32", N=250, like_levine=False, seed=3, **kw):
    from icem_amd import DeviceSyntheticModel, MpcCemStdHip
    from icem_amd.envs import CostSpec, SyntheticEnv
    env = SyntheticEnv("HalfCheetah", 17, LOW * np.ones(6), HIGH * np.ones(6), CostSpec(0.1, 8, -1.0, 1, 10.0, 0.3))
    return MpcCemStdHip(env=env, forward_model=DeviceSyntheticModel.make(17, 6, kind=0, seed_a=11, seed_b=12), horizon=30,
                        num_simulated_trajectories=N, cost_along_trajectory="sum", verbose=False, dtype=dtype, seed=seed,
                        fused_step=fused_step,
                        action_sampler_params=dict(alpha=0.1, elites_size=10, opt_iterations=3, init_std=0.5, shift_means=True,
                                                   execute_best_elite=True, bounds_like_levine=like_levine), **kw)


def drive(pairs, steps=STEPS, second_episode=True):
    """``get_action`` over 3 steps of one episode and the first of a second one; every pair stays equal."""
    plan = [(0, s) for s in range(steps)] + ([(1, 0)] if second_episode else [])
    for ep, s in plan:
        obs = observation(17, 10 * ep + s)
        if s == 0:
            for c in itertools.chain(*pairs):
                c.beginning_of_rollout(observation=obs, state=None, mode="train")
        for a, b in pairs:
            x, y = a.get_action(obs, None), b.get_action(obs, None)
            assert np.array_equal(x, y), (ep, s)
            assert np.array_equal(a.mean, b.mean) and np.array_equal(a.std, b.std)
            assert np.array_equal(a.elite_samples.as_array("actions"), b.elite_samples.as_array("actions"))
            assert np.array_equal(a.elite_samples.as_array("costs"), b.elite_samples.as_array("costs"))
            assert a.last_min_cost == b.last_min_cost and a.planner.mpc_step == b.planner.mpc_step == s + 1


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("like_levine", [False, True])
def test_the_controller_on_the_fused_step_equals_the_stage_wise_controller(dtype, like_levine):
    a, b, c = (controller(f, dtype, like_levine=like_levine) for f in (True, False, None))
    drive([(a, b)])
    assert a.planner.cem_step_launches == 9 and b.planner.cem_step_launches == 0
    # fused_step=None takes the fused entry where it is served
    c.beginning_of_rollout(observation=observation(17, 0), state=None, mode="train")
    c.get_action(observation(17, 0), None)
    assert c.planner.cem_step_launches == 9


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_the_fused_controller_matches_the_oracle_on_the_same_uniforms(dtype):
    """As tests/test_gpu_parity.py::test_cem_std_device_rng_matches_oracle, at its tolerances, with the controller forced onto
    the fused entry: 2 MPC steps, both bound modes."""
    from golden_util import CEMSTD_CASES, GoldenCemStd
    from icem_amd import DeviceSyntheticModel, MpcCemStdHip
    from icem_amd.envs import CostSpec, SyntheticEnv
    g = GoldenCemStd(CEMSTD_CASES[0])
    npdt = np.float64 if dtype == "f64" else np.float32
    for like_levine in (False, True):
        spec = O.CostSpec.halfcheetah(g.o)
        env = SyntheticEnv("HalfCheetah", g.o, g.low.copy(), g.high.copy(),
                           CostSpec(spec.ctrl_weight, spec.lin_idx, spec.lin_weight, spec.flip_idx, spec.flip_penalty, spec.flip_thresh))
        ctrl = MpcCemStdHip(env=env, forward_model=DeviceSyntheticModel(g.A, g.B, g.kind), horizon=g.h, num_simulated_trajectories=g.N,
                            cost_along_trajectory=g.cost_mode, verbose=False, dtype=dtype, noise_source="philox", fused_step=True,
                            action_sampler_params=dict(alpha=g.alpha, elites_size=g.K, opt_iterations=g.iters, init_std=g.init_std,
                                                       shift_means=True, execute_best_elite=True, bounds_like_levine=like_levine))
        om, oc = O.SyntheticModel(g.A, g.B, g.kind), O.CostSpec.halfcheetah(g.o)
        state = {"call": 0}

        def uniforms(num):
            u = O.philox_uniforms(0, state["call"], num, g.d, g.h, dtype=npdt).astype(np.float64)
            state["call"] += 1
            return u
        orc = O.CemStdOracle(horizon=g.h, num_traj=g.N, opt_iterations=g.iters, elites_size=g.K, alpha=g.alpha,
                             init_std=g.init_std, like_levine=like_levine, shift_means=True, execute_best_elite=True,
                             low=g.low, high=g.high, rollout_cost=lambda ob, ac: O.rollout_costs(om, oc, ob, ac, mode=g.cost_mode),
                             uniforms=uniforms)
        orc.beginning_of_rollout()
        ctrl.beginning_of_rollout(observation=g.obs[0], state=None, mode="train")
        t = dict(rtol=1e-8, atol=1e-9) if dtype == "f64" else dict(rtol=3e-4, atol=3e-5)
        for s in range(2):
            np.testing.assert_allclose(ctrl.get_action(g.obs[s], None), orc.get_action(g.obs[s]), **t)
            assert ctrl.planner.cem_step_launches == 3 * g.iters
        np.testing.assert_allclose(ctrl.mean, orc.mean, **t)


def test_fused_step_true_raises_where_the_step_is_not_served():
    from icem_amd import _lib as L
    c = controller(True)
    obs = observation(17, 0)
    c.beginning_of_rollout(observation=obs, state=None, mode="train")
    L.set_option("cem_step", 0)
    try:
        with pytest.raises(RuntimeError, match="fused_step=True"):
            c.get_action(obs, None)
    finally:
        L.reset_options()
    assert c.planner.mpc_step == 0
    u = controller(True, noise_source=lambda num: np.full((num, 30, 6), 0.5))
    u.beginning_of_rollout(observation=obs, state=None, mode="train")
    with pytest.raises(RuntimeError, match="noise source"):
        u.get_action(obs, None)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_a_captured_step_replays_to_the_same_bits(dtype):
    """One warm-up step outside the capture (the rollout's model upload), then step 1 captured on a side stream: nothing in the
    call synchronises or allocates, and the replay leaves what the eager twin's step 1 leaves."""
    flags = (False, True, True)
    fused, twin = planner(dtype, 250, 30, 6, 17, 0), planner(dtype, 250, 30, 6, 17, 0)
    sf, st = Dist(fused, flags[0]), Dist(twin, flags[0])
    obs = [torch.as_tensor(observation(17, s), dtype=fused.dt, device=fused.device) for s in range(2)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fused_step(fused, sf, obs[0], *flags)
        side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        got = fused_step(fused, sf, obs[1], *flags)
    assert fused.mpc_step == 2 and fused.cem_step_launches == 9
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    loop_step(twin, st, np_(obs[0]), *flags)
    want = loop_step(twin, st, np_(obs[1]), *flags)
    torch.cuda.synchronize()
    for k in want:
        assert np.array_equal(np_(got[k]), np_(want[k])), k


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def _snapshot(pl, s):
    return [np_(x).copy() for x in (s.mean, s.std, s.lower, s.upper, pl.cem_actions, pl.cem_costs, pl.cem_elites, pl.cem_elite_costs,
                                    pl.cem_elite_idx, pl.cem_result)]


REFUSED = ["option", "profiling", "sharded", "pool", "factor_decrease"]


def _refused_planner(case, **kw):
    if case == "sharded":
        return planner("f32", 250, 30, 6, 17, 0, world=2, **kw)
    if case == "pool":
        return planner("f32", 20000, 30, 6, 17, 0, **kw)
    if case == "factor_decrease":
        return planner("f32", 250, 30, 6, 17, 0, factor_decrease=1.25, **kw)
    pl = planner("f32", 250, 30, 6, 17, 0, **kw)
    if case == "profiling":
        pl.profile_enable(True)
    return pl


@pytest.mark.parametrize("case", REFUSED)
def test_a_refused_step_touches_nothing_and_the_controller_falls_back_to_the_loop(case):
    from icem_amd import _lib as L
    try:
        if case == "option":
            L.set_option("cem_step", 0)
        pl = _refused_planner(case)
        assert not pl.cem_step_ok()
        s = Dist(pl, False)
        obs = observation(17, 0)
        if case not in ("option", "pool"):   # a served step first: the buffers hold something a refused step could spoil
            ok = planner("f32", 250, 30, 6, 17, 0)
            fused_step(ok, Dist(ok, False), obs, False, True, True)
            for name in ("actions", "costs", "elites", "elite_costs", "elite_idx", "result"):
                pl._cem_buffers()[name].copy_(ok._cem_buffers()[name])
        before, step = _snapshot(pl, s), pl.mpc_step
        with pytest.raises(L.IcemError) as e:
            pl.plan_step_cem(obs, s.mean, s.std, s.lower, s.upper, like_levine=False, shift_means=True, execute_best_elite=True)
        torch.cuda.synchronize()
        assert e.value.code == L.ICEM_E_UNSUPPORTED
        assert pl.mpc_step == step and pl.cem_step_launches == 0
        for x, y in zip(_snapshot(pl, s), before):
            assert np.array_equal(x, y)
        # the controller: fused_step=None runs the loop on such a handle and gives the loop's result
        N = 20000 if case == "pool" else 250
        a, b = controller(None, N=N), controller(False, N=N)
        if case in ("sharded", "factor_decrease"):
            for c in (a, b):
                c.planner = _refused_planner(case, seed=3)
                c._bind_models()
        if case == "profiling":
            a.planner.profile_enable(True)
        assert not a.planner.cem_step_ok()
        drive([(a, b)], steps=2, second_episode=False)
        assert a.planner.cem_step_launches == 0
    finally:
        L.reset_options()
