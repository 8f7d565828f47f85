"""``icem_plan_step_cem_learned`` / ``icem_plan_step_cem_learned_batch`` (cem_step.hip, k_cem.hip): the MPC step of the truncated-normal
CEM through the learned dynamics (the declared RSSM) as one library call, for one planner or B planners at once.  The step is
DEFINED by the operator loop -- ``sample_truncnorm`` at offset (episode << 32) + step * opt_iters + i, ``DeviceRSSMModel.rollout_cost``,
``update_distribution``, ``cem_bounds``, then the epilogue as tests/test_gpu_cem_step.py::loop_step writes it -- and the new entries
only rearrange its launches, so every comparison in this file is ``np.array_equal``: no tolerance appears.  The solo entry is held to
the loop on all eleven buffers (executed, best cost, mean, std, lower, upper, the elite set, its costs and indices, the last pool and
its costs); a batch to its solo twins on the first nine and on its row of ``results`` (a batch scores its rows in a pool of the first
handle: a problem's own pool is scratch).  Bounds are asymmetric (low = -0.7, high = 0.9), so lower != -upper and the sampler's
clamp is live.  One shared ``DeviceRSSMModel(seed=3)``; shapes (N, h, K, iterations) are the smallest that reach each edge: one
16-row tile; a ragged second tile at a horizon outside the folded sampler's list; several sampler workgroups (42 rows each at
d = 6); K at the update's limit of 32; 257 tiles, past the split launch's one-tile-per-workgroup arrangement (256)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from test_gpu_cem_step import Dist, np_

pytestmark = pytest.mark.gpu

LOW, HIGH = -0.7, 0.9
FLAGS = (False, True, True)   # like_levine, shift_means, execute_best_elite
ALL = ("executed", "best_cost", "mean", "std", "lower", "upper", "elites", "elite_costs", "elite_idx", "actions", "costs")
NINE = ALL[:9]
SHAPES = [(16, 12, 2, 2), (17, 5, 4, 3), (250, 12, 10, 3), (1024, 12, 32, 2), (4100, 10, 10, 2)]
_cache = {}


def model():
    from icem_amd import DeviceRSSMModel
    if "m" not in _cache:
        _cache["m"] = DeviceRSSMModel(seed=3)
    return _cache["m"]


def planner(N, h, K=10, iters=3, *, seed=5, d=6, mode="sum", alpha=0.1, rounds=10, dtype="f32", low=None, high=None, **cfg):
    from icem_amd import IcemConfig, IcemPlanner
    c = dict(horizon=h, act_dim=d, num_traj=N, elites_size=K, opt_iters=iters, cost_mode=mode, use_mean_actions=False,
             keep_previous_elites=False, shift_elites=False, factor_decrease=1.0, alpha=alpha, init_std=0.5, dtype=dtype,
             rng_rounds=rounds, seed=seed)
    c.update(cfg)
    pl = IcemPlanner(IcemConfig(**c), LOW * np.ones(d) if low is None else low, HIGH * np.ones(d) if high is None else high)
    pl.new_episode()
    return pl


def observation(problem, step):
    return (0.3 * np.random.RandomState(1000 * problem + step).randn(230)).astype(np.float32)


def loop_step(pl, s, obs, like_levine, shift_means, execute_best_elite):
    """The operator loop of ``MpcCemStdHip._step_stagewise`` with a ``DeviceRSSMModel``: -> the eleven buffers."""
    from icem_amd import _lib as L
    N, K, iters = pl.cfg.num_traj, pl.K, pl.cfg.opt_iters
    actions = costs = costs_sorted = idx = elites = None
    for i in range(iters):
        actions = pl.sample_truncnorm(N, s.mean, s.std, s.lower, s.upper, None, offset=pl.noise_offset(pl.mpc_step * iters + i))
        costs = model().rollout_cost(obs, actions, L.COST_MODES[pl.cfg.cost_mode])
        costs_sorted, idx, elites = pl.update_distribution(costs, actions, K, s.mean, s.std)
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


def views(pl, s):
    return dict(executed=pl.cem_result[:pl.d], best_cost=pl.cem_result[pl.d:], mean=s.mean, std=s.std, lower=s.lower, upper=s.upper,
                elites=pl.cem_elites, elite_costs=pl.cem_elite_costs, elite_idx=pl.cem_elite_idx, actions=pl.cem_actions, costs=pl.cem_costs)


def fused_step(pl, s, obs, like_levine, shift_means, execute_best_elite):
    ex = pl.plan_step_cem_learned(model(), obs, s.mean, s.std, s.lower, s.upper, like_levine=like_levine, shift_means=shift_means,
                                  execute_best_elite=execute_best_elite)
    assert ex.data_ptr() == pl.cem_result.data_ptr()
    return views(pl, s)


# ---- 1. the raw solo entry against the operator loop --------------------------------------------------------------------------
def run_against_the_loop(make, flags=FLAGS, steps=3, episodes=2):
    fused, twin = make(), make()
    assert fused.cem_learned_step_ok()
    for ep in range(episodes):
        if ep:
            fused.new_episode()
            twin.new_episode()
        sf, st = Dist(fused, flags[0]), Dist(twin, flags[0])
        for k in range(steps):
            obs = observation(0, 10 * ep + k)
            got, want = fused_step(fused, sf, obs, *flags), loop_step(twin, st, obs, *flags)
            torch.cuda.synchronize()
            for name in ALL:
                assert np.array_equal(np_(got[name]), np_(want[name])), (ep, k, name)
            assert fused.mpc_step == twin.mpc_step == k + 1 and fused.episode == twin.episode == ep
            assert fused.cem_step_launches == 3 * fused.cfg.opt_iters and twin.cem_step_launches == 0
        if not flags[0]:
            assert not np.array_equal(np_(sf.lower), -np_(sf.upper))   # asymmetric action bounds: the two probability tables differ
    return fused


@pytest.mark.parametrize("N,h,K,iters", SHAPES)
def test_the_solo_step_equals_the_operator_loop_bit_for_bit(N, h, K, iters):
    fused = run_against_the_loop(lambda: planner(N, h, K, iters))
    assert fused.K == K


@pytest.mark.parametrize("like_levine,shift_means,execute_best_elite", list(itertools.product((False, True), repeat=3)))
def test_every_flag_combination(like_levine, shift_means, execute_best_elite):
    run_against_the_loop(lambda: planner(250, 12, 10, 2), (like_levine, shift_means, execute_best_elite), episodes=1)


PER_DIM = dict(low=np.array([-0.7, -1.0, -0.2, -0.5, -0.9, -0.3]), high=np.array([0.9, 0.4, 1.0, 0.5, 0.1, 0.8]))


@pytest.mark.parametrize("what", [dict(mode="sum"), dict(mode="best"), dict(mode="final"), dict(alpha=0.0), dict(alpha=0.9),
                                  dict(rounds=7), PER_DIM], ids=["sum", "best", "final", "alpha0", "alpha0.9", "rounds7", "per_dim_bounds"])
def test_cost_modes_momentum_the_other_generator_and_bounds_per_dimension(what):
    run_against_the_loop(lambda: planner(250, 12, 10, 2, **what), episodes=1)


# ---- 2. a batch against its solo twins ----------------------------------------------------------------------------------------
class Group:
    """B planners (seed 5 + i) with their distributions: a batch, or its solo twins."""

    def __init__(self, make, B, like_levine=False):
        self.pls = [make(seed=5 + i) for i in range(B)]
        self.dists = [Dist(pl, like_levine) for pl in self.pls]

    def step_batch(self, obs, flags=FLAGS):
        from icem_amd import IcemPlanner
        return IcemPlanner.plan_step_cem_learned_batch(self.pls, model(), obs, [(s.mean, s.std, s.lower, s.upper) for s in self.dists],
                                                       like_levine=flags[0], shift_means=flags[1], execute_best_elite=flags[2])

    def step_solo(self, obs, flags=FLAGS):
        for pl, s, ob in zip(self.pls, self.dists, obs):
            fused_step(pl, s, ob, *flags)

    def step_loop(self, obs, flags=FLAGS):
        """The operator loop; its results go where the fused steps leave theirs (the views are compared there)."""
        for pl, s, ob in zip(self.pls, self.dists, obs):
            out = loop_step(pl, s, ob, *flags)
            pl.cem_result.copy_(torch.cat([out["executed"], out["best_cost"]]))
            for name in ("elites", "elite_costs", "elite_idx", "actions", "costs"):
                getattr(pl, "cem_" + name).copy_(out[name])

    def new_episode(self, i, like_levine=False):
        self.pls[i].new_episode()
        self.dists[i] = Dist(self.pls[i], like_levine)


def assert_equal(batch, twins, where, results=None):
    torch.cuda.synchronize()
    for i, (pb, sb, pt, st) in enumerate(zip(batch.pls, batch.dists, twins.pls, twins.dists)):
        got, want = views(pb, sb), views(pt, st)
        for name in NINE:
            assert np.array_equal(np_(got[name]), np_(want[name])), (where, i, name)
        assert pb.mpc_step == pt.mpc_step, (where, i)
        if results is not None:
            row = np.concatenate([np_(want["executed"]), np_(want["best_cost"])])
            assert np.array_equal(np_(results[i]), row), (where, i, "results")


def run_against_the_twins(make, B, steps=3):
    batch, twins = Group(make, B), Group(make, B)
    iters = batch.pls[0].cfg.opt_iters
    for k in range(steps):
        obs = [observation(i, k) for i in range(B)]
        ex = batch.step_batch(obs)
        twins.step_solo(obs)
        assert_equal(batch, twins, k, batch.pls[0].cem_batch_results)
        assert np.array_equal(np_(ex), np_(batch.pls[0].cem_batch_results[:, :-1]))
        assert batch.pls[0].cem_batch_launches == 3 * iters   # 3 launches per iteration whatever B
        assert all(pl.cem_batch_launches == 0 for pl in batch.pls[1:])
    if B > 1:   # problems of one batch differ (seeds and observations of their own)
        assert not np.array_equal(np_(batch.pls[0].cem_elites), np_(batch.pls[1].cem_elites))
    return batch


@pytest.mark.parametrize("N,h,K,iters", SHAPES[:4])
def test_a_batch_of_three_equals_its_solo_twins_bit_for_bit(N, h, K, iters):
    run_against_the_twins(lambda **kw: planner(N, h, K, iters, **kw), 3)


def test_a_batch_of_one_is_the_solo_step_plus_the_results_row():
    batch = run_against_the_twins(lambda **kw: planner(250, 12, 10, 3, **kw), 1)
    # (one problem steps in its own buffers: its pool is the solo step's too)
    twin = Group(lambda **kw: planner(250, 12, 10, 3, **kw), 1)
    for k in range(3):
        twin.step_solo([observation(0, k)])
    torch.cuda.synchronize()
    assert np.array_equal(np_(batch.pls[0].cem_actions), np_(twin.pls[0].cem_actions))
    assert np.array_equal(np_(batch.pls[0].cem_costs), np_(twin.pls[0].cem_costs))


def test_a_batch_of_thirty_two():
    run_against_the_twins(lambda **kw: planner(16, 12, 2, 2, **kw), 32, steps=2)


def test_a_problem_that_was_reset_later_steps_with_its_neighbours():
    """Problem 1 begins a new episode after step 1: from then on its mpc_steps_host entry and its episode differ from its neighbours'."""
    make = lambda **kw: planner(250, 12, 10, 3, **kw)   # noqa: E731
    batch, twins = Group(make, 3), Group(make, 3)
    for k in range(4):
        if k == 2:
            batch.new_episode(1)
            twins.new_episode(1)
        obs = [observation(i, k) for i in range(3)]
        batch.step_batch(obs)
        twins.step_solo(obs)
        assert_equal(batch, twins, k, batch.pls[0].cem_batch_results)
    assert [pl.mpc_step for pl in batch.pls] == [4, 2, 4] and [pl.episode for pl in batch.pls] == [0, 1, 0]


def test_a_planner_may_alternate_between_the_loop_the_solo_and_the_batched_step():
    make = lambda **kw: planner(250, 12, 10, 3, **kw)   # noqa: E731
    mixed, twins = Group(make, 2), Group(make, 2)
    for k in range(6):
        obs = [observation(i, k) for i in range(2)]
        (mixed.step_loop, mixed.step_solo, mixed.step_batch)[k % 3](obs)
        twins.step_solo(obs)
        assert_equal(mixed, twins, k)


def test_a_steady_batch_uploads_each_slot_once():
    batch = Group(lambda **kw: planner(250, 12, 10, 3, **kw), 3)
    seen = []
    for k in range(5):
        batch.step_batch([observation(i, k) for i in range(3)])
        seen.append(batch.pls[0].batch_uploads)
    assert seen == [1, 2, 2, 2, 2]
    assert all(pl.batch_uploads == 0 for pl in batch.pls[1:])


def _raw_batch(g, obs_ptrs, *, n=None, handles=None, steps=None, results=None):
    """The C entry on the group's planners, every problem's observation wherever ``obs_ptrs`` says."""
    from icem_amd import _lib as L
    pls = g.pls
    cbs = [L.IcemCemBuffersC.from_buffer_copy(pl._cem_cb(None, s.mean, s.std, s.lower, s.upper, obs_ptr=p)) for pl, s, p in zip(pls, g.dists, obs_ptrs)]
    hs = [pl._h for pl in pls] if handles is None else handles
    n = len(hs) if n is None else n
    st = [pl.mpc_step for pl in pls] if steps is None else steps
    prm = L.IcemCemParamsC(*[int(f) for f in FLAGS], 0)
    L.check(pls[0].lib.icem_plan_step_cem_learned_batch((C.c_void_p * len(hs))(*hs), n, (L.IcemCemBuffersC * len(cbs))(*cbs), C.byref(prm),
                                                        C.c_void_p(model().params.data_ptr()), (C.c_int32 * len(st))(*st),
                                                        None if results is None else C.c_void_p(results.data_ptr()), pls[0]._stream()))


def test_observation_buffers_need_not_be_adjacent():
    """The raw entry with every problem's observation in a tensor of its own, in descending address order inside one arena with gaps
    between them: the first sampler launch gathers them into the batch's table."""
    make = lambda **kw: planner(250, 12, 10, 3, **kw)   # noqa: E731
    batch, twins = Group(make, 3), Group(make, 3)
    arena = torch.zeros(4096, dtype=torch.float32, device="cuda")
    slots = [arena[2048:2278], arena[1000:1230], arena[3:233]]
    results = torch.zeros((3, 7), dtype=torch.float32, device="cuda")
    for k in range(2):
        obs = [observation(i, k) for i in range(3)]
        arena.fill_(7.0)
        for slot, ob in zip(slots, obs):
            slot.copy_(torch.as_tensor(ob))
        _raw_batch(batch, [s.data_ptr() for s in slots], results=results)
        for pl in batch.pls:
            pl.mpc_step += 1
        twins.step_solo(obs)
        assert_equal(batch, twins, k, results)
    ptrs = sorted(s.data_ptr() for s in slots)
    assert all(b - a > 230 * 4 for a, b in zip(ptrs, ptrs[1:]))


# ---- 3. the controllers -------------------------------------------------------------------------------------------------------
def controller(fused_step, seed=3, N=250, m=None, iters=3, **kw):
    from icem_amd import MpcCemStdHip, halfcheetah_env
    return MpcCemStdHip(env=halfcheetah_env(17), forward_model=model() if m is None else m, horizon=12, num_simulated_trajectories=N,
                        cost_along_trajectory="sum", verbose=False, seed=seed, fused_step=fused_step,
                        action_sampler_params=dict(alpha=0.1, elites_size=10, opt_iterations=iters, init_std=0.5, shift_means=True,
                                                   execute_best_elite=True, bounds_like_levine=False), **kw)


def same_state(a, b, where):
    assert np.array_equal(a.mean, b.mean) and np.array_equal(a.std, b.std), where
    assert np.array_equal(np_(a._lower), np_(b._lower)) and np.array_equal(np_(a._upper), np_(b._upper)), where
    assert np.array_equal(a.elite_samples.as_array("actions"), b.elite_samples.as_array("actions")), where
    assert np.array_equal(a.elite_samples.as_array("costs"), b.elite_samples.as_array("costs")), where
    assert a.last_min_cost == b.last_min_cost and a.planner.mpc_step == b.planner.mpc_step, where


def test_the_controller_on_the_fused_step_equals_the_stage_wise_controller():
    a, b, c = (controller(f) for f in (True, False, None))
    assert a._fused_step_refusal() is None and a.planner.obs_dim == 0   # (no built-in model is set)
    for ep in range(2):
        for k in range(3):
            obs = observation(0, 10 * ep + k)
            if k == 0:
                for x in (a, b, c):
                    x.beginning_of_rollout(observation=obs, state=None, mode="train")
            got, want, third = a.get_action(obs, None), b.get_action(obs, None), c.get_action(obs, None)
            assert np.array_equal(got, want) and np.array_equal(third, want), (ep, k)
            same_state(a, b, (ep, k))
            same_state(c, b, (ep, k))
            assert a.planner.mpc_step == k + 1
    # fused_step=None takes the library step with the library's RSSM
    assert a.planner.cem_step_launches == 9 and c.planner.cem_step_launches == 9 and b.planner.cem_step_launches == 0


def drive_batch(ctrls, twins, episodes=2, steps=2):
    from icem_amd import MpcCemStdHip
    for ep in range(episodes):
        for k in range(steps):
            obs = [observation(i, 10 * ep + k) for i in range(len(ctrls))]
            if k == 0:
                for c, ob in zip(itertools.chain(ctrls, twins), obs + obs):
                    c.beginning_of_rollout(observation=ob, state=None, mode="train")
            got = MpcCemStdHip.get_action_batch(ctrls, obs)
            want = [t.get_action(ob, None) for t, ob in zip(twins, obs)]
            for i, (a, b) in enumerate(zip(ctrls, twins)):
                assert np.array_equal(got[i], want[i]), (ep, k, i)
                same_state(a, b, (ep, k, i))
                assert a.planner.mpc_step == k + 1


def test_the_controllers_step_together_as_their_twins_step_alone():
    ctrls = [controller(None, seed=3 + i) for i in range(3)]
    twins = [controller(True, seed=3 + i) for i in range(3)]
    drive_batch(ctrls, twins)
    assert ctrls[0].planner.cem_batch_launches == 9 and ctrls[0].planner.cem_step_launches == 0
    stage = [controller(False, seed=3 + i) for i in range(3)]   # ... and as the operator loop steps
    drive_batch([controller(None, seed=3 + i) for i in range(3)], stage, episodes=1)


def test_a_model_with_a_rollout_cost_of_its_own_keeps_the_loop():
    """``rollout_cost`` replaced on the instance (to count the rollouts) or overridden by a subclass: the controller calls it stage
    by stage as it asks to be, ``fused_step=True`` names the reason."""
    from icem_amd import DeviceRSSMModel

    class Counting(DeviceRSSMModel):
        calls = 0

        def rollout_cost(self, obs, actions, cost_mode=0):
            Counting.calls += 1
            return super().rollout_cost(obs, actions, cost_mode)

    patched, calls = DeviceRSSMModel(seed=3), []
    own = patched.rollout_cost
    patched.rollout_cost = lambda obs, actions, cost_mode=0: (calls.append(1), own(obs, actions, cost_mode))[1]
    twin = controller(True)
    obs = observation(0, 0)
    twin.beginning_of_rollout(observation=obs, state=None, mode="train")
    want = twin.get_action(obs, None)
    for m, count in ((patched, lambda: len(calls)), (Counting(seed=3), lambda: Counting.calls)):
        c = controller(None, m=m)
        assert "not the library's own RSSM" in c._fused_step_refusal()
        c.beginning_of_rollout(observation=obs, state=None, mode="train")
        got = c.get_action(obs, None)
        assert count() == 3 and c.planner.cem_step_launches == 0
        assert np.array_equal(got, want)
        same_state(c, twin, type(m).__name__)
        strict = controller(True, m=m)
        strict.beginning_of_rollout(observation=obs, state=None, mode="train")
        with pytest.raises(RuntimeError, match="not the library's own RSSM"):
            strict.get_action(obs, None)
        assert strict.planner.mpc_step == 0


# ---- 4. one captured solo step ------------------------------------------------------------------------------------------------
def test_a_captured_step_replays_to_the_same_bits():
    """One step outside the capture on the capturing stream (the rollout's staging area of this size), then step 1 captured: nothing
    in the call synchronises or allocates, and the replay leaves what the loop twin's step 1 leaves."""
    fused, twin = planner(250, 12, 10, 3), planner(250, 12, 10, 3)
    sf, st = Dist(fused, FLAGS[0]), Dist(twin, FLAGS[0])
    obs = [torch.as_tensor(observation(0, k), device=fused.device) for k in range(2)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fused_step(fused, sf, obs[0], *FLAGS)
        side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        got = fused_step(fused, sf, obs[1], *FLAGS)
    assert fused.mpc_step == 2 and fused.cem_step_launches == 9
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    loop_step(twin, st, np_(obs[0]).astype(np.float32), *FLAGS)
    want = loop_step(twin, st, np_(obs[1]).astype(np.float32), *FLAGS)
    torch.cuda.synchronize()
    for name in ALL:
        assert np.array_equal(np_(got[name]), np_(want[name])), name


# ---- 5. refusals touch nothing ------------------------------------------------------------------------------------------------
def _snapshot(g):
    out = []
    for pl, s in zip(g.pls, g.dists):
        out += [np_(x).copy() for x in views(pl, s).values()]
        out.append(np.array([pl.mpc_step, pl.cem_batch_launches, pl.cem_step_launches, pl.batch_uploads]))
    return out


def _spoilable(g):
    """Something in every buffer that a refused step could spoil."""
    for j, pl in enumerate(g.pls):
        for name in ("actions", "costs", "elites", "elite_costs", "result"):
            getattr(pl, "cem_" + name).fill_(1.5 + j)
        pl.cem_elite_idx.fill_(3 + j)


SOLO_REFUSALS = {
    "an f64 handle": dict(dtype="f64"),
    "act_dim 5": dict(d=5),
    "K = 33": dict(K=33),
    "keep_previous_elites": dict(keep_previous_elites=True),
    "profiling on": dict(),
    "option cem_step = 0": dict(),
}


@pytest.mark.parametrize("case", list(SOLO_REFUSALS))
def test_a_refused_step_touches_nothing(case):
    from icem_amd import _lib as L
    g = Group(lambda **kw: planner(250, 12, **{**dict(K=10, iters=3), **SOLO_REFUSALS[case]}, **kw), 2)
    try:
        if case == "option cem_step = 0":
            L.set_option("cem_step", 0)
        if case == "profiling on":
            for pl in g.pls:
                pl.profile_enable(True)
        if case == "K = 33":
            assert g.pls[0].K == 33
        assert not g.pls[0].cem_learned_step_ok()
        _spoilable(g)
        torch.cuda.synchronize()
        before = _snapshot(g)
        pl, s = g.pls[0], g.dists[0]
        with pytest.raises(L.IcemError) as e:
            pl.plan_step_cem_learned(model(), observation(0, 0), s.mean, s.std, s.lower, s.upper, like_levine=False, shift_means=True,
                                     execute_best_elite=True)
        assert e.value.code == L.ICEM_E_UNSUPPORTED and "icem_plan_step_cem_learned" in str(e.value), str(e.value)
        with pytest.raises(L.IcemError) as e:
            g.step_batch([observation(i, 0) for i in range(2)])
        assert e.value.code == L.ICEM_E_UNSUPPORTED, str(e.value)
        torch.cuda.synchronize()
        for x, y in zip(_snapshot(g), before):
            assert np.array_equal(x, y)
    finally:
        L.reset_options()


def test_a_batch_over_the_tile_limit_is_refused_as_a_whole():
    """rssm_split_max_n = 64 (4 tiles): N = 32 is 2 tiles and steps alone, three of them are 6."""
    from icem_amd import _lib as L
    g = Group(lambda **kw: planner(32, 12, 10, 2, **kw), 3)
    try:
        L.set_option("rssm_split_max_n", 64)
        assert all(pl.cem_learned_step_ok() for pl in g.pls)
        g.step_solo([observation(i, 0) for i in range(3)])
        torch.cuda.synchronize()
        before = _snapshot(g)
        with pytest.raises(L.IcemError) as e:
            g.step_batch([observation(i, 1) for i in range(3)])
        assert e.value.code == L.ICEM_E_UNSUPPORTED and "tiles" in str(e.value)
        torch.cuda.synchronize()
        for x, y in zip(_snapshot(g), before):
            assert np.array_equal(x, y)
    finally:
        L.reset_options()


@pytest.mark.parametrize("case", ["unequal configurations", "a handle twice", "a negative step"])
def test_an_inadmissible_batch_is_refused_before_anything_runs(case):
    from icem_amd import _lib as L
    g = Group.__new__(Group)
    g.pls = [planner(250 + (16 * i if case == "unequal configurations" else 0), 12, 10, 3, seed=5 + i) for i in range(2)]
    g.dists = [Dist(pl, False) for pl in g.pls]
    g.step_solo([observation(i, 0) for i in range(2)])
    obs = torch.as_tensor(np.stack([observation(i, 1) for i in range(2)]), device="cuda")
    torch.cuda.synchronize()
    before = _snapshot(g)
    bent = {"unequal configurations": {}, "a handle twice": dict(handles=[g.pls[0]._h, g.pls[0]._h]), "a negative step": dict(steps=[1, -1])}[case]
    with pytest.raises(L.IcemError) as e:
        _raw_batch(g, [obs[0].data_ptr(), obs[1].data_ptr()], **bent)
    assert e.value.code == L.ICEM_E_INVALID, str(e.value)
    torch.cuda.synchronize()
    for x, y in zip(_snapshot(g), before):
        assert np.array_equal(x, y)


def test_controllers_on_two_models_and_fused_step_true():
    from icem_amd import DeviceRSSMModel, MpcCemStdHip
    from icem_amd import _lib as L
    other = DeviceRSSMModel(seed=4)
    obs = [observation(i, 0) for i in range(2)]

    def pair(fused_step):
        cs = [controller(fused_step, seed=3), controller(fused_step, seed=4, m=other)]
        for c, ob in zip(cs, obs):
            c.beginning_of_rollout(observation=ob, state=None, mode="train")
        return cs
    assert "share one DeviceRSSMModel" in MpcCemStdHip._batch_refusal(pair(None))
    with pytest.raises(RuntimeError, match="share one DeviceRSSMModel"):
        MpcCemStdHip.get_action_batch(pair(True), obs)
    # fused_step=None: each controller's own step, in order, with its own model
    ctrls, twins = pair(None), pair(True)
    got = MpcCemStdHip.get_action_batch(ctrls, obs)
    for i, (c, t) in enumerate(zip(ctrls, twins)):
        assert np.array_equal(got[i], t.get_action(obs[i], None)), i
        same_state(c, t, i)
        assert c.planner.cem_batch_launches == 0 and c.planner.cem_step_launches == 9
    # fused_step=True raises with the reason where the step is not served, and nothing has advanced
    try:
        L.set_option("cem_step", 0)
        c = pair(True)[0]
        with pytest.raises(RuntimeError, match="fused_step=True.*cem_learned_step_ok"):
            c.get_action(obs[0], None)
        assert c.planner.mpc_step == 0
        loop, twin = pair(None)[0], pair(False)[0]   # fused_step=None runs the loop there
        assert np.array_equal(loop.get_action(obs[0], None), twin.get_action(obs[0], None))
        assert loop.planner.cem_step_launches == 0
    finally:
        L.reset_options()
