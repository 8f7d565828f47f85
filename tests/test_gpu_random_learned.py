"""``icem_plan_step_random_learned`` / ``icem_plan_step_random_learned_batch`` (random_step.hip, k_random.hip, k_random_learned.hip):
the random-shooting baseline's MPC step through the learned dynamics (the declared RSSM) as one library call, for one planner or B
planners at once.  The step is DEFINED by the operator chain -- ``sample_piecewise`` at the caller's call offset,
``DeviceRSSMModel.rollout_cost``, ``topk_sorted(costs, 1)`` and the gathers behind it -- and the new entries only rearrange its
launches, so every comparison in this file is ``np.array_equal``: no tolerance appears.  The solo entry is held to the chain on the
pool, its costs, the best row and ``result``; a batch to its solo twins on the same four buffers OF EVERY PROBLEM (a controller keeps
its pool, so a batch mirrors its pool slices into the problems' own buffers) and on its row of ``results``.  Bounds differ per
dimension and are asymmetric.  One shared ``DeviceRSSMModel(seed=3)``; shapes (N, h, hold) are the smallest that reach each edge: one
16-row tile; a ragged tile whose pool (510 elements) is no multiple of 4 and whose slices of a batch start 8 bytes off a 16-byte
boundary, hold 0; hold = h - 1; 1024 rows; 257 tiles, past the split launch's one-tile-per-workgroup arrangement (256), and several
sampler workgroups; 16 400 rows -- two selection slices -- at the shortest horizon a handle takes (2)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LOW = np.array([-0.7, -1.0, -0.2, -0.5, -0.9, -0.3])
HIGH = np.array([0.9, 0.4, 1.0, 0.5, 0.1, 0.8])
NAMES = ("actions", "costs", "best_actions", "result")
SHAPES = [(16, 12, 4), (17, 5, 0), (250, 12, 11), (1024, 12, 1), (4100, 10, 4), (16400, 2, 1)]
_cache = {}


def np_(t):
    return t.detach().cpu().numpy()


def model():
    from icem_amd import DeviceRSSMModel
    if "m" not in _cache:
        _cache["m"] = DeviceRSSMModel(seed=3)
    return _cache["m"]


def planner(N, h, *, seed=5, d=6, mode="sum", rounds=10, dtype="f32", builtin=False, **cfg):
    """A planner configured as ``MpcRandomHip`` configures its own (elites_size 2, one iteration); ``builtin``: with a built-in
    model and cost as well (the handle then serves both kinds of step)."""
    from icem_amd import DeviceSyntheticModel, IcemConfig, IcemPlanner
    c = dict(horizon=h, act_dim=d, num_traj=N, elites_size=2, opt_iters=1, cost_mode=mode, dtype=dtype, rng_rounds=rounds, seed=seed)
    c.update(cfg)
    pl = IcemPlanner(IcemConfig(**c), LOW[:d], HIGH[:d])
    if builtin:
        m = DeviceSyntheticModel.make(17, d, kind=0, seed_a=11, seed_b=12)
        pl.set_model(m.kind, m.A, m.B)
        pl.set_cost(0.1, 16, -1.0, 1, 10.0, 0.3)
    return pl


def observation(problem, step):   # (tests/test_gpu_cem_learned.py::observation)
    return (0.3 * np.random.RandomState(1000 * problem + step).randn(230)).astype(np.float32)


def chain_step(pl, obs, offset, freq):
    """The operator chain of ``MpcRandomHip._step_stagewise`` with a ``DeviceRSSMModel`` -> the four buffers."""
    from icem_amd import _lib as L
    actions = pl.sample_piecewise(pl.cfg.num_traj, offset, freq, None, 0)
    costs = model().rollout_cost(obs, actions, L.COST_MODES[pl.cfg.cost_mode])
    best_cost, idx = pl.topk_sorted(costs, 1)
    best = int(idx[0])
    result = torch.cat([actions[best, 0], best_cost.to(pl.dt), idx.to(pl.dt)])
    return dict(actions=actions, costs=costs, best_actions=actions[best].clone(), result=result)


def views(pl):
    return dict(actions=pl.random_actions, costs=pl.random_costs, best_actions=pl.random_best_actions, result=pl.random_result)


def fused_step(pl, obs, offset, freq):
    ex = pl.plan_step_random_learned(model(), obs, offset, freq)
    assert ex.data_ptr() == pl.random_result.data_ptr()
    return views(pl)


def assert_same(got, want, where):
    torch.cuda.synchronize()
    for k in NAMES:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (where, k)
        assert np.array_equal(np_(got[k]), np_(want[k])), (where, k)


# ---- 1. the solo entry against the operator chain -----------------------------------------------------------------------------
def run_against_the_chain(make, freq, steps=3, episodes=2):
    fused, twin = make(), make()
    assert fused.random_learned_step_ok() and fused.obs_dim == 0   # (no built-in model is set)
    per_step, off = fused.cfg.num_traj * fused.h, 0
    for ep in range(episodes):
        if ep:   # (MpcRandom's call counter runs on across episodes)
            fused.new_episode()
            twin.new_episode()
        for s in range(steps):
            obs = observation(0, 10 * ep + s)
            got, want = fused_step(fused, obs, off, freq), chain_step(twin, obs, off, freq)
            assert_same(got, want, (ep, s))
            costs = np_(got["costs"])
            assert int(np_(got["result"])[-1]) == int(np.argmin(costs)) and np_(got["result"])[-2] == costs.min()
            assert fused.random_step_launches == 3 and twin.random_step_launches == 0
            off += per_step
    return fused


@pytest.mark.parametrize("N,h,hold", SHAPES)
def test_the_solo_step_equals_the_operator_chain_bit_for_bit(N, h, hold):
    run_against_the_chain(lambda: planner(N, h), hold)


@pytest.mark.parametrize("what", [dict(mode="sum"), dict(mode="best"), dict(mode="final"), dict(rounds=7)], ids=["sum", "best", "final", "rounds7"])
def test_cost_modes_and_the_other_generator(what):
    run_against_the_chain(lambda: planner(250, 12, **what), 4, episodes=1)


# ---- 2. a batch against its solo twins ----------------------------------------------------------------------------------------
class Group:
    """B planners (seed 5 + i) with call counters of their own: a batch, or its solo twins."""

    def __init__(self, make, B, start=None):
        self.pls = [make(seed=5 + i) for i in range(B)]
        self.calls = [0 if start is None else start[i] for i in range(B)]
        self.per_step = self.pls[0].cfg.num_traj * self.pls[0].h

    def _advance(self):
        self.calls = [c + self.per_step for c in self.calls]

    def step_batch(self, obs, freq):
        from icem_amd import IcemPlanner
        ex = IcemPlanner.plan_step_random_learned_batch(self.pls, model(), obs, self.calls, freq)
        self._advance()
        return ex

    def step_solo(self, obs, freq):
        for pl, ob, c in zip(self.pls, obs, self.calls):
            fused_step(pl, ob, c, freq)
        self._advance()

    def step_builtin_batch(self, obs17, freq):
        from icem_amd import IcemPlanner
        IcemPlanner.plan_step_random_batch(self.pls, obs17, self.calls, freq)
        self._advance()

    def step_builtin_solo(self, obs17, freq):
        for pl, ob, c in zip(self.pls, obs17, self.calls):
            pl.plan_step_random(ob, c, freq)
        self._advance()


def assert_equal(batch, twins, where, results=None):
    torch.cuda.synchronize()
    assert batch.calls == twins.calls
    for i, (pb, pt) in enumerate(zip(batch.pls, twins.pls)):
        got, want = views(pb), views(pt)
        for k in NAMES:
            assert np.array_equal(np_(got[k]), np_(want[k])), (where, i, k)
        if results is not None:
            assert np.array_equal(np_(results[i]), np_(want["result"])), (where, i, "results")


def run_against_the_twins(make, B, freq, steps=3, start=None):
    batch, twins = Group(make, B, start), Group(make, B, start)
    for s in range(steps):
        obs = [observation(i, s) for i in range(B)]
        ex = batch.step_batch(obs, freq)
        twins.step_solo(obs, freq)
        res = batch.pls[0].random_batch_results
        assert tuple(res.shape) == (B, 8) and np.array_equal(np_(ex), np_(res[:, :-2]))
        assert_equal(batch, twins, s, res)
        assert batch.pls[0].random_batch_launches == 3   # 3 launches whatever B
        assert all(pl.random_batch_launches == 0 for pl in batch.pls[1:])
    if B > 1:   # problems of one batch differ (seeds, observations and offsets of their own)
        assert not np.array_equal(np_(batch.pls[0].random_actions), np_(batch.pls[1].random_actions))
        assert not np.array_equal(np_(batch.pls[0].random_costs), np_(batch.pls[1].random_costs))
    return batch


@pytest.mark.parametrize("N,h,hold", SHAPES)
def test_a_batch_of_three_equals_its_solo_twins_bit_for_bit(N, h, hold):
    """Call offsets that differ per problem.  (17, 5): a slice of the pool starts at i * 17 * 5 * 6 * 4 bytes = 8 mod 16 for odd i,
    the problem's own buffer is aligned -- the 16-byte store is decided per destination."""
    batch = run_against_the_twins(lambda **kw: planner(N, h, **kw), 3, hold, start=[0, 7, 12345])
    if (N, h) == (17, 5):
        assert (N * h * 6 * 4) % 16 == 8 and all(pl.random_actions.data_ptr() % 16 == 0 for pl in batch.pls)


def test_a_batch_of_one_is_the_solo_step_plus_the_results_row():
    run_against_the_twins(lambda **kw: planner(16, 12, **kw), 1, 4)


def test_a_batch_of_thirty_two():
    run_against_the_twins(lambda **kw: planner(16, 12, **kw), 32, 4, steps=2, start=[3 * i for i in range(32)])


def test_a_problem_that_was_reset_later_steps_with_its_neighbours():
    """Problem 1 starts over after step 1 (a controller built later): from then on its call offset differs from its neighbours'."""
    make = lambda **kw: planner(250, 12, **kw)   # noqa: E731
    batch, twins = Group(make, 3), Group(make, 3)
    for s in range(4):
        if s == 2:
            batch.calls[1] = twins.calls[1] = 0
        obs = [observation(i, s) for i in range(3)]
        batch.step_batch(obs, 4)
        twins.step_solo(obs, 4)
        assert_equal(batch, twins, s, batch.pls[0].random_batch_results)
    assert batch.calls == [4 * 3000, 2 * 3000, 4 * 3000]


def test_handles_may_alternate_between_the_learned_batch_the_builtin_batch_and_solo_steps():
    """The learned batch and the built-in batch share the first handle's argument array; solo steps of either kind use none."""
    make = lambda **kw: planner(250, 12, builtin=True, **kw)   # noqa: E731
    mixed, twins = Group(make, 2), Group(make, 2)
    obs17 = lambda i, s: 0.1 * np.random.RandomState(100 + 1000 * i + s).randn(17)   # noqa: E731
    for s in range(8):
        kind = s % 4
        if kind in (0, 2):   # learned: batched, then solo
            obs = [observation(i, s) for i in range(2)]
            (mixed.step_batch if kind == 0 else mixed.step_solo)(obs, 4)
            twins.step_solo(obs, 4)
        else:                # built-in: batched, then solo
            obs = [obs17(i, s) for i in range(2)]
            (mixed.step_builtin_batch if kind == 1 else mixed.step_builtin_solo)(obs, 4)
            twins.step_builtin_solo(obs, 4)
        assert_equal(mixed, twins, s)


def test_a_steady_batch_uploads_its_blocks_once():
    """The call offsets travel by value and the pool's pointers too: nothing in the blocks changes from step to step."""
    batch = Group(lambda **kw: planner(250, 12, **kw), 3)
    seen = []
    for s in range(10):
        batch.step_batch([observation(i, s) for i in range(3)], 4)
        seen.append(batch.pls[0].batch_uploads)
    assert seen == [1] * 10
    assert all(pl.batch_uploads == 0 for pl in batch.pls[1:])


def test_a_captured_batch_replays_to_the_same_bits():
    """One eager step on the capturing stream (the rollout's staging area, the pool, the argument blocks, the results tensor), then
    step 1 captured: nothing in the call synchronises, uploads or allocates, and two replays leave what the eager twins' step 1 leaves."""
    make = lambda **kw: planner(250, 12, **kw)   # noqa: E731
    batch, twins = Group(make, 3), Group(make, 3)
    dev = batch.pls[0].device
    obs = [[torch.as_tensor(observation(i, s), device=dev) for i in range(3)] for s in range(2)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        batch.step_batch(obs[0], 4)
        side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        batch.step_batch(obs[1], 4)
    assert batch.pls[0].batch_uploads == 1 and batch.pls[0].random_batch_launches == 3
    torch.cuda.synchronize()
    for s in range(2):
        twins.step_solo([np_(x) for x in obs[s]], 4)
    for _ in range(2):
        g.replay()
        assert_equal(batch, twins, "replay", batch.pls[0].random_batch_results)


# ---- 3. refusals touch nothing ------------------------------------------------------------------------------------------------
def _snapshot(g):
    out = []
    for pl in g.pls:
        out += [np_(x).copy() for x in views(pl).values()]
        out.append(np.array([pl.mpc_step, pl.random_step_launches, pl.random_batch_launches, pl.batch_uploads]))
    return out


def _unchanged(g, before):
    torch.cuda.synchronize()
    return all(np.array_equal(x, y) for x, y in zip(_snapshot(g), before))


def _spoilable(g):
    """Something in every buffer that a refused step could spoil."""
    for j, pl in enumerate(g.pls):
        for t in views(pl).values():
            t.fill_(1.5 + j)
    torch.cuda.synchronize()


def _raw_batch(g, obs, *, n=None, handles=None, offsets=None, freq=4, params=True, edit=None):
    """The C entry on the group's planners with the arguments bent as a refusal case needs them."""
    from icem_amd import _lib as L
    pls = g.pls
    cbs = [L.IcemRandomBuffersC.from_buffer_copy(pl._random_cb(ob, "obs_rssm")) for pl, ob in zip(pls, obs)]
    if edit:
        edit(cbs)
    hs = [pl._h for pl in pls] if handles is None else handles
    n = len(hs) if n is None else n
    hs_c = (C.c_void_p * max(1, len(hs)))(*hs)
    bs = (L.IcemRandomBuffersC * max(1, len(cbs), n))(*cbs)
    offs = list(g.calls) if offsets is None else offsets
    offs_c = (C.c_int64 * max(1, len(offs), n))(*offs)
    res = torch.zeros((max(1, len(pls)), 8), dtype=torch.float32, device=pls[0].device)
    prm = C.c_void_p(model().params.data_ptr()) if params else None
    L.check(pls[0].lib.icem_plan_step_random_learned_batch(hs_c, n, bs, prm, freq, offs_c, C.c_void_p(res.data_ptr()), pls[0]._stream()))


def _raw_solo(pl, obs, *, offset=0, freq=4, params=True):
    from icem_amd import _lib as L
    cb = pl._random_cb(obs, "obs_rssm")
    prm = C.c_void_p(model().params.data_ptr()) if params else None
    L.check(pl.lib.icem_plan_step_random_learned(pl._h, C.byref(cb), prm, freq, offset, pl._stream()))


# the handle is not served: case -> the planner's configuration
UNSERVED = {
    "an f64 handle": dict(dtype="f64"),
    "act_dim 5": dict(d=5),
    "a population past the split launch": dict(),
    "option random_step = 0": dict(),
    "profiling on": dict(),
}


@pytest.mark.parametrize("case", list(UNSERVED))
def test_a_handle_that_is_not_served_is_refused_and_nothing_is_touched(case):
    from icem_amd import _lib as L
    g = Group(lambda **kw: planner(250, 12, **UNSERVED[case], **kw), 2)
    obs = [observation(i, 0) for i in range(2)]
    try:
        if case == "option random_step = 0":
            L.set_option("random_step", 0)
        if case == "a population past the split launch":
            L.set_option("rssm_split_max_n", 64)
        if case == "profiling on":
            for pl in g.pls:
                pl.profile_enable(True)
        assert not g.pls[0].random_learned_step_ok()
        _spoilable(g)
        before = _snapshot(g)
        with pytest.raises(L.IcemError) as e:
            g.pls[0].plan_step_random_learned(model(), obs[0], 0, 4)
        assert e.value.code == L.ICEM_E_UNSUPPORTED and "icem_plan_step_random_learned: " in str(e.value), str(e.value)
        for B in (1, 2):
            with pytest.raises(L.IcemError) as e:
                from icem_amd import IcemPlanner
                IcemPlanner.plan_step_random_learned_batch(g.pls[:B], model(), obs[:B], [0] * B, 4)
            assert e.value.code == L.ICEM_E_UNSUPPORTED and "icem_plan_step_random_learned_batch: " in str(e.value), str(e.value)
        assert _unchanged(g, before)
    finally:
        L.reset_options()


def test_a_batch_over_the_tile_limit_is_refused_as_a_whole():
    """rssm_split_max_n = 64 (4 tiles): N = 32 is 2 tiles and steps alone, three of them are 6."""
    from icem_amd import _lib as L
    g = Group(lambda **kw: planner(32, 12, **kw), 3)
    try:
        L.set_option("rssm_split_max_n", 64)
        assert all(pl.random_learned_step_ok() for pl in g.pls)
        g.step_solo([observation(i, 0) for i in range(3)], 4)
        torch.cuda.synchronize()
        before = _snapshot(g)
        with pytest.raises(L.IcemError) as e:
            g.step_batch([observation(i, 1) for i in range(3)], 4)
        assert e.value.code == L.ICEM_E_UNSUPPORTED and "tiles" in str(e.value)
        assert _unchanged(g, before)
    finally:
        L.reset_options()


def _null_costs(cbs):
    cbs[1].costs = None


# the call is not admitted: case -> (the second planner's configuration, the call's bent arguments(group))
INADMISSIBLE = {
    "NULL params": (dict(), lambda g: dict(params=False)),
    "change_freq = horizon": (dict(), lambda g: dict(freq=12)),
    "a negative offset": (dict(), lambda g: dict(offsets=[0, -1])),
    "n = 0": (dict(), lambda g: dict(n=0)),
    "n = 33": (dict(), lambda g: dict(n=33, handles=[g.pls[k % 2]._h for k in range(33)])),
    "a handle twice": (dict(), lambda g: dict(handles=[g.pls[0]._h, g.pls[0]._h])),
    "a null handle": (dict(), lambda g: dict(handles=[g.pls[0]._h, None])),
    "a NULL buffer": (dict(), lambda g: dict(edit=_null_costs)),
    "another num_traj": (dict(N=266), lambda g: {}),
    "another cost mode": (dict(mode="best"), lambda g: {}),
}


@pytest.mark.parametrize("case", list(INADMISSIBLE))
def test_an_inadmissible_call_is_refused_before_anything_runs(case):
    from icem_amd import _lib as L
    other, bend = INADMISSIBLE[case]
    g = Group.__new__(Group)
    g.pls = [planner(250, 12, seed=5), planner(other.get("N", 250), 12, seed=6, **{k: v for k, v in other.items() if k != "N"})]
    g.calls, g.per_step = [0, 0], 3000
    obs = [observation(i, 0) for i in range(2)]
    for pl, ob in zip(g.pls, obs):   # a served solo step first: the buffers hold something a refused call could spoil
        fused_step(pl, ob, 0, 4)
    torch.cuda.synchronize()
    before = _snapshot(g)
    with pytest.raises(L.IcemError) as e:
        _raw_batch(g, obs, **bend(g))
    assert e.value.code == L.ICEM_E_INVALID, str(e.value)
    assert _unchanged(g, before)
    solo = {"NULL params": dict(params=False), "change_freq = horizon": dict(freq=12), "a negative offset": dict(offset=-1)}.get(case)
    if solo is not None:   # ... and the solo entry's own
        with pytest.raises(L.IcemError) as e:
            _raw_solo(g.pls[0], obs[0], **solo)
        assert e.value.code == L.ICEM_E_INVALID and "icem_plan_step_random_learned: " in str(e.value), str(e.value)
        assert _unchanged(g, before)


# ---- 4. the controllers -------------------------------------------------------------------------------------------------------
def controller(fused_step, seed=3, N=250, m=None, **kw):
    from icem_amd import MpcRandomHip
    from icem_amd.envs import CostSpec, SyntheticEnv
    env = SyntheticEnv("HalfCheetah", 17, LOW, HIGH, CostSpec(0.1, 8, -1.0, 1, 10.0, 0.3))
    return MpcRandomHip(env=env, forward_model=model() if m is None else m, horizon=12, num_simulated_trajectories=N,
                        cost_along_trajectory="sum", verbose=False, seed=seed, fused_step=fused_step,
                        action_sampler_params=dict(action_change_frequency=4), **kw)


def same_controllers(a, b, where):
    assert a.calls == b.calls and a.best_traj_idx == b.best_traj_idx and a.last_min_cost == b.last_min_cost, where
    assert np.array_equal(np_(a._last_actions), np_(b._last_actions)) and np.array_equal(np_(a._last_costs), np_(b._last_costs)), where


def test_the_controller_on_the_fused_step_equals_the_controller_on_the_chain():
    a, b = controller(True), controller(False)
    assert a._fused_step_refusal() is None and a._steps_through_the_rssm() and a.planner.obs_dim == 0
    for c in (a, b):
        c.beginning_of_rollout(observation=observation(0, 0), state=None, mode="train")
    for s in range(4):
        obs = observation(0, s)
        x, y = a.get_action(obs, None), b.get_action(obs, None)
        assert x.dtype == y.dtype == np.float64 and np.array_equal(x, y), s
        same_controllers(a, b, s)
        assert a.calls == (s + 1) * 250 * 12
    assert a.planner.random_step_launches == 3 and b.planner.random_step_launches == 0


def test_the_controllers_step_together_as_their_twins_step_alone():
    from icem_amd import MpcRandomHip
    ctrls = [controller(True, seed=3 + i) for i in range(3)]
    twins = [controller(True, seed=3 + i) for i in range(3)]
    chain = [controller(False, seed=3 + i) for i in range(3)]
    obs0 = [observation(i, 0) for i in range(3)]
    for c, ob in zip(ctrls + twins + chain, obs0 * 3):
        c.beginning_of_rollout(observation=ob, state=None, mode="train")
    for s in range(3):
        obs = [observation(i, s) for i in range(3)]
        got = MpcRandomHip.get_action_batch(ctrls, obs)
        for i, (c, t, k) in enumerate(zip(ctrls, twins, chain)):
            assert np.array_equal(got[i], t.get_action(obs[i], None)) and np.array_equal(got[i], k.get_action(obs[i], None)), (s, i)
            same_controllers(c, t, (s, i))
            same_controllers(c, k, (s, i))
    assert ctrls[0].planner.random_batch_launches == 3 and ctrls[0].planner.random_step_launches == 0
    assert twins[0].planner.random_step_launches == 3


def test_controllers_on_two_models_and_fused_step_true():
    from icem_amd import DeviceRSSMModel, MpcRandomHip
    other = DeviceRSSMModel(seed=4)
    obs = [observation(i, 0) for i in range(2)]

    def pair(fused_step):
        cs = [controller(fused_step, seed=3), controller(fused_step, seed=4, m=other)]
        for c, ob in zip(cs, obs):
            c.beginning_of_rollout(observation=ob, state=None, mode="train")
        return cs
    assert "share one DeviceRSSMModel" in MpcRandomHip._batch_refusal(pair(True))
    strict = pair(True)
    with pytest.raises(RuntimeError, match="share one DeviceRSSMModel"):
        MpcRandomHip.get_action_batch(strict, obs)
    assert all(c.calls == 0 and c.best_traj_idx is None and c.planner.random_step_launches == 0 for c in strict)
    # fused_step=None: each controller's own step, in order, with its own model
    ctrls, twins = pair(None), pair(False)
    got = MpcRandomHip.get_action_batch(ctrls, obs)
    for i, (c, t) in enumerate(zip(ctrls, twins)):
        assert np.array_equal(got[i], t.get_action(obs[i], None)), i
        same_controllers(c, t, i)
        assert c.planner.random_batch_launches == 0
