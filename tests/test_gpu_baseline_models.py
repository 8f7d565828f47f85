"""``icem_plan_step_cem_learned_models`` / ``icem_plan_step_random_learned_models`` (cem_step.hip + k_cem_members.hip, random_step.hip +
k_random_members.hip): the MPC steps of the two baselines -- truncated-normal CEM, random shooting -- through an ensemble's members or
a model per problem as one library call.  The rollout is ONE launch of n x members problems in member-major order; the launch behind
it (the CEM update, the random-shooting selection) reduces the members' costs itself.  The steps are DEFINED by the stage-wise
operators -- ``sample_truncnorm`` / ``sample_piecewise``, ``DeviceRSSMEnsemble.rollout_cost`` (``icem_rssm_rollout_cost_ensemble``: the
members' launch + ``icem_rssm_ensemble_reduce``), ``update_distribution`` + ``cem_bounds`` / ``topk_sorted(costs, 1)`` and the gathers
-- and the entries only rearrange the launches, so every comparison in this file is ``np.array_equal``: no tolerance appears.  (That
the inputs can tell a wrong cost source from the right one is shown on the CPU: test_baseline_models_sensitivity_cpu.py.)

Members are cached ``DeviceRSSMModel``s of one seed each (test_gpu_learned_models.members).  Shapes are the smallest that reach each
edge.  CEM (N, h, K, iterations): (40, 4, 4, 2) a ragged third tile; (250, 12, 10, 3); (1100, 12, 32, 2) a second pass of the update's
1024-thread key loop.  Random shooting: N = 40, 250 and 16 400 (two selection slices, 2 050 tiles at E = 2), holds 1 and 4.  Member
counts 2 / 3 / 5 (the reduction's group of up to 8 loads), 9 and 32 (its group of up to 32)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import test_gpu_cem_learned as CL
import test_gpu_learned_models as LM
import test_gpu_random_learned as RL
from test_gpu_cem_step import Dist

pytestmark = pytest.mark.gpu

np_ = RL.np_
observation = CL.observation
FLAGS = CL.FLAGS
CEM_SHAPES = [(40, 4, 4, 2), (250, 12, 10, 3), (1100, 12, 32, 2)]


def ensemble(E, reduce="mean", d=6, nan_member=None, first=0):
    """A fresh DeviceRSSMEnsemble on cached members (``first``: skip that many, so that problems get different members)."""
    from icem_amd import DeviceRSSMEnsemble
    if nan_member is not None:
        return LM.ensemble(E, reduce, d, nan_member)
    return DeviceRSSMEnsemble(models=LM.members(E + first, d)[first:], reduce=reduce)


def assert_member_costs_left(batch, stagewise, kind, N, where):
    """What a batched step leaves in the ensembles' ``member_costs``: with an ensemble each, every ensemble holds what its stage-wise
    twin's own ``rollout_cost`` left; a shared ensemble holds the table of all problems, whose last block is what the stage-wise
    twin (called once per problem, in order) holds."""
    torch.cuda.synchronize()
    if kind == "ensemble_each":
        for p, (a, b) in enumerate(zip(batch.each, stagewise.each)):
            assert tuple(a.member_costs.shape) == tuple(b.member_costs.shape) and np.array_equal(np_(a.member_costs), np_(b.member_costs)), (where, p)
    elif kind == "shared":
        assert np.array_equal(np_(batch.models.member_costs)[:, -N:], np_(stagewise.models.member_costs)), where


def flag_kw(flags):
    return dict(like_levine=flags[0], shift_means=flags[1], execute_best_elite=flags[2])


# ================================================================================================ CEM
def cem_loop_step(pl, s, obs, ens, flags=FLAGS):
    """CL.loop_step with the costs of ``ens`` (one launch for all members + the reduction launch) -> the eleven buffers."""
    from icem_amd import _lib as L
    N, K, iters = pl.cfg.num_traj, pl.K, pl.cfg.opt_iters
    like_levine, shift_means, execute_best_elite = flags
    actions = costs = costs_sorted = idx = elites = None
    for i in range(iters):
        actions = pl.sample_truncnorm(N, s.mean, s.std, s.lower, s.upper, None, offset=pl.noise_offset(pl.mpc_step * iters + i))
        costs = ens.rollout_cost(obs, actions, L.COST_MODES[pl.cfg.cost_mode])
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


def cem_fused(pls, dists, models, obs, flags=FLAGS, **kw):
    from icem_amd import IcemPlanner
    return IcemPlanner.plan_step_cem_learned_models(pls, models, obs, [(s.mean, s.std, s.lower, s.upper) for s in dists], **flag_kw(flags), **kw)


def cem_against_the_loop(make, E, reduce, flags=FLAGS, steps=2, d=6, nan_member=None, equal_nan=False):
    fused, twin = make(), make()
    ef, et = ensemble(E, reduce, d, nan_member), ensemble(E, reduce, d, nan_member)
    assert fused._bind_rssm(ef) and fused.cem_learned_models_step_ok(1, E)
    sf, st = Dist(fused, flags[0]), Dist(twin, flags[0])
    for k in range(steps):
        obs = observation(0, k)
        ex = cem_fused([fused], [sf], ef, [obs], flags)
        got, want = CL.views(fused, sf), cem_loop_step(twin, st, obs, et, flags)
        torch.cuda.synchronize()
        for name in CL.ALL:
            assert np.array_equal(np_(got[name]), np_(want[name]), equal_nan=equal_nan), (k, name)
        res = fused.cem_batch_results
        assert np.array_equal(np_(res[0]), np.concatenate([np_(want["executed"]), np_(want["best_cost"])]), equal_nan=equal_nan)
        assert np.array_equal(np_(ex), np_(res[:, :-1]), equal_nan=equal_nan)
        assert np.array_equal(np_(ef.member_costs), np_(et.member_costs), equal_nan=equal_nan), (k, "member_costs")
        assert fused.mpc_step == twin.mpc_step == k + 1
        assert fused.cem_batch_launches == 3 * fused.cfg.opt_iters   # 3 launches per iteration whatever the member count
    return fused, ef


@pytest.mark.parametrize("N,h,K,iters", CEM_SHAPES)
def test_cem_the_fused_step_equals_the_operator_loop(N, h, K, iters):
    cem_against_the_loop(lambda: CL.planner(N, h, K, iters), 2, "mean")


@pytest.mark.parametrize("reduce", ["mean", "max"])
@pytest.mark.parametrize("E", [2, 3, 5, 9, 32])
def test_cem_member_counts_and_reductions(E, reduce):
    cem_against_the_loop(lambda: CL.planner(250, 12, 10, 2), E, reduce, steps=1)


@pytest.mark.parametrize("mode", ["sum", "best", "final"])
def test_cem_cost_modes(mode):
    cem_against_the_loop(lambda: CL.planner(250, 12, 10, 2, mode=mode), 3, "max", steps=1)


@pytest.mark.parametrize("like_levine,shift_means,execute_best_elite", list(itertools.product((False, True), repeat=3)))
def test_cem_every_flag_combination(like_levine, shift_means, execute_best_elite):
    cem_against_the_loop(lambda: CL.planner(40, 4, 4, 2), 2, "mean", (like_levine, shift_means, execute_best_elite))


def test_cem_act_dim_two_runs_the_runtime_width_twins():
    cem_against_the_loop(lambda: CL.planner(250, 12, 10, 2, d=2), 3, "mean", d=2)


@pytest.mark.parametrize("reduce", ["mean", "max"])
@pytest.mark.parametrize("who", [0, 2])
def test_cem_a_nan_member_ends_the_step_as_the_loop_does(who, reduce):
    _, ens = cem_against_the_loop(lambda: CL.planner(250, 12, 10, 2), 3, reduce, steps=1, nan_member=who, equal_nan=True)
    mc = np_(ens.member_costs)
    assert np.isnan(mc[who]).all() and not np.isnan(np.delete(mc, who, 0)).any()


class CemGroup:
    """B planners (seed 5 + i) with their distributions and the models they plan through: ``kind`` "shared" (one ensemble of 2),
    "model_each" (a plain model per planner) or "ensemble_each" (an ensemble of 2 per planner, members of their own)."""

    def __init__(self, B, kind, make=lambda **kw: CL.planner(250, 12, 10, 3, **kw), reduce="mean", E=2):
        self.pls = [make(seed=5 + i) for i in range(B)]
        self.dists = [Dist(pl, False) for pl in self.pls]
        if kind == "shared":
            self.models = ensemble(E, reduce)
            self.each = [self.models] * B
        elif kind == "model_each":
            self.models = LM.members(B)
            self.each = [ensemble(1, first=i) for i in range(B)]   # (the mean of one member is the member: * 1.0f)
        else:
            self.models = self.each = [ensemble(E, reduce, first=i) for i in range(B)]

    def step_batch(self, obs, **kw):
        return cem_fused(self.pls, self.dists, self.models, obs, **kw)

    def step_solo(self, obs):
        for pl, s, ob, m in zip(self.pls, self.dists, obs, self.each):
            cem_fused([pl], [s], m, [ob])

    def step_loop(self, obs):
        for pl, s, ob, m in zip(self.pls, self.dists, obs, self.each):
            out = cem_loop_step(pl, s, ob, m)
            pl.cem_result.copy_(torch.cat([out["executed"], out["best_cost"]]))
            for name in ("elites", "elite_costs", "elite_idx", "actions", "costs"):
                getattr(pl, "cem_" + name).copy_(out[name])

    def new_episode(self, i):
        self.pls[i].new_episode()
        self.dists[i] = Dist(self.pls[i], False)


@pytest.mark.parametrize("kind", ["shared", "model_each", "ensemble_each"])
def test_cem_a_batch_of_three_equals_its_solo_twins_and_the_loop(kind):
    """... with problem 1 reset a step later than its peers (its episode and its step count differ from then on)."""
    batch, twins, loops = CemGroup(3, kind), CemGroup(3, kind), CemGroup(3, kind)
    for k in range(3):
        if k == 1:
            for g in (batch, twins, loops):
                g.new_episode(1)
        obs = [observation(i, k) for i in range(3)]
        batch.step_batch(obs)
        twins.step_solo(obs)
        loops.step_loop(obs)
        CL.assert_equal(batch, twins, (kind, k), batch.pls[0].cem_batch_results)
        CL.assert_equal(batch, loops, (kind, k, "loop"), batch.pls[0].cem_batch_results)
        assert_member_costs_left(batch, loops, kind, 250, (kind, k))
        assert batch.pls[0].cem_batch_launches == 9 and all(pl.cem_batch_launches == 0 for pl in batch.pls[1:])
    assert [pl.mpc_step for pl in batch.pls] == [3, 2, 3]
    assert not np.array_equal(np_(batch.pls[0].cem_elites), np_(batch.pls[2].cem_elites))


@pytest.mark.parametrize("B,E", [(32, 1), (1, 32)])
def test_cem_thirty_two_problems_in_one_rollout(B, E):
    make = lambda **kw: CL.planner(40, 4, 4, 2, **kw)   # noqa: E731
    kind = "model_each" if E == 1 else "shared"
    batch, loops = CemGroup(B, kind, make, E=E), CemGroup(B, kind, make, E=E)
    assert batch.pls[0].cem_learned_models_step_ok(B, E) and not batch.pls[0].cem_learned_models_step_ok(B + 1, E)
    for k in range(2):
        obs = [observation(i, k) for i in range(B)]
        batch.step_batch(obs)
        loops.step_loop(obs)
        CL.assert_equal(batch, loops, (B, E, k), batch.pls[0].cem_batch_results)


def test_cem_one_member_with_equal_pointers_is_the_learned_batch_entry():
    from icem_amd import IcemPlanner
    m = LM.model(3)
    a, b = CemGroup(3, "model_each"), CemGroup(3, "model_each")
    a.models = [m] * 3
    for k in range(2):
        obs = [observation(i, k) for i in range(3)]
        a.step_batch(obs)
        IcemPlanner.plan_step_cem_learned_batch(b.pls, m, obs, [(s.mean, s.std, s.lower, s.upper) for s in b.dists], **flag_kw(FLAGS))
        CL.assert_equal(a, b, k, a.pls[0].cem_batch_results)
    # ... and with one planner the solo entry's, the pool included
    a1, b1 = CemGroup(1, "model_each"), CemGroup(1, "model_each")
    a1.models = [m]
    a1.step_batch([observation(0, 0)])
    sb = b1.dists[0]
    b1.pls[0].plan_step_cem_learned(m, observation(0, 0), sb.mean, sb.std, sb.lower, sb.upper, **flag_kw(FLAGS))
    torch.cuda.synchronize()
    got, want = CL.views(a1.pls[0], a1.dists[0]), CL.views(b1.pls[0], b1.dists[0])
    for name in CL.ALL:
        assert np.array_equal(np_(got[name]), np_(want[name])), name


def test_cem_a_callers_member_costs_holds_the_last_rollout():
    batch, loops = CemGroup(3, "ensemble_each"), CemGroup(3, "ensemble_each")
    N = 250
    mc = torch.full((2 * 3 * N + 5,), -7.0, dtype=torch.float32, device="cuda")
    obs = [observation(i, 0) for i in range(3)]
    batch.step_batch(obs, member_costs=mc)
    loops.step_loop(obs)
    torch.cuda.synchronize()
    got = np_(mc[:2 * 3 * N]).reshape(2, 3 * N)
    for p, ens in enumerate(loops.each):
        assert np.array_equal(got[:, p * N:(p + 1) * N], np_(ens.member_costs)), p
    assert (np_(mc[2 * 3 * N:]) == -7.0).all()


def test_cem_the_steady_state_uploads_nothing_and_entries_alternate():
    """Uploads: one per slot (the two step parities), then none.  Then the same handles alternate between the loop, the solo learned
    entry's sibling (one planner through the models entry), the batch, and the single-model batch entry -- every step the twins'."""
    batch, twins = CemGroup(3, "shared"), CemGroup(3, "shared")
    seen = []
    for k in range(5):
        obs = [observation(i, k) for i in range(3)]
        batch.step_batch(obs)
        twins.step_loop(obs)
        seen.append(batch.pls[0].batch_uploads)
    CL.assert_equal(batch, twins, "steady")
    assert seen == [1, 2, 2, 2, 2] and all(pl.batch_uploads == 0 for pl in batch.pls[1:])
    for k in range(5, 9):
        obs = [observation(i, k) for i in range(3)]
        (batch.step_loop, batch.step_solo, batch.step_batch, batch.step_batch)[k % 4](obs)
        twins.step_loop(obs)
        CL.assert_equal(batch, twins, k)


def test_cem_alternates_with_the_solo_learned_entry_and_the_builtin_batch():
    """One planner steps through: the models entry, the solo learned entry (member 0 alone), the built-in model's batch, the models
    entry again -- a twin that runs only the models steps (with the others' effect on ``mpc_step`` restated) ends in the same bits."""
    from icem_amd import DeviceSyntheticModel, IcemPlanner
    ens_a, ens_b = ensemble(2), ensemble(2)

    def make(seed):
        pl = CL.planner(250, 12, 10, 2, seed=seed)
        m = DeviceSyntheticModel.make(17, 6, kind=0, seed_a=11, seed_b=12)
        pl.set_model(m.kind, m.A, m.B)
        pl.set_cost(0.1, 16, -1.0, 1, 10.0, 0.3)
        return pl
    a, b = [make(5), make(6)], [make(5), make(6)]
    da, db = [Dist(p, False) for p in a], [Dist(p, False) for p in b]
    obs = [observation(i, 0) for i in range(2)]
    cem_fused(a, da, ens_a, obs)
    cem_fused(b, db, ens_b, obs)
    # a detour on handle a[0] / a[1] with distributions of its own: the solo learned entry, then the built-in batch
    side = [Dist(p, False) for p in a]
    for p in a:   # (Dist starts an episode's count: back to where the handles are)
        p.mpc_step = 1
    a[0].plan_step_cem_learned(LM.model(3), obs[0], side[0].mean, side[0].std, side[0].lower, side[0].upper, **flag_kw(FLAGS))
    a[1].mpc_step += 1
    IcemPlanner.plan_step_cem_batch(a, [0.1 * np.ones(17)] * 2, [(s.mean, s.std, s.lower, s.upper) for s in side], **flag_kw(FLAGS))
    for p in b:
        p.mpc_step += 2
    obs = [observation(i, 1) for i in range(2)]
    cem_fused(a, da, ens_a, obs)
    cem_fused(b, db, ens_b, obs)
    torch.cuda.synchronize()
    for i in range(2):
        got, want = CL.views(a[i], da[i]), CL.views(b[i], db[i])
        for name in CL.NINE:
            assert np.array_equal(np_(got[name]), np_(want[name])), (i, name)


def test_cem_a_captured_step_replays_with_a_fresh_observation():
    batch, loops = CemGroup(2, "shared"), CemGroup(2, "shared")
    obs = [torch.as_tensor(np.stack([observation(i, k) for i in range(2)]), device="cuda") for k in range(3)]
    table = obs[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        batch.step_batch(table)   # (outside the capture: the rollout's staging area, the pool, the argument array)
        batch.step_batch(table)   # (... and the other slot of the argument array)
        side.synchronize()
        for pl in batch.pls:       # (the captured step is step 0 of a new episode: slot 0 again)
            pl.mpc_step = 0
        for s, fresh in zip(batch.dists, [Dist(pl, False) for pl in batch.pls]):
            for name in ("mean", "std", "lower", "upper"):
                getattr(s, name).copy_(getattr(fresh, name))
        side.synchronize()
    uploads = batch.pls[0].batch_uploads
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        batch.step_batch(table)
    assert batch.pls[0].batch_uploads == uploads   # (nothing was uploaded under capture)
    torch.cuda.synchronize()
    for s, fresh in zip(batch.dists, [Dist(pl, False) for pl in batch.pls]):
        for name in ("mean", "std", "lower", "upper"):
            getattr(s, name).copy_(getattr(fresh, name))
    for pl in batch.pls:   # (Dist starts an episode's count; the captured call was step 0)
        pl.mpc_step = 1
    table.copy_(obs[2])
    g.replay()
    torch.cuda.synchronize()
    loops.step_loop([np_(obs[2][i]) for i in range(2)])
    CL.assert_equal(batch, loops, "replay", batch.pls[0].cem_batch_results)


# ---- refusals touch nothing
def _raw_cem(g, table, members, *, reduce=0, n=None, handles=None, steps=None, buffers=True, prm=True, null_steps=False):
    from icem_amd import _lib as L
    pls = g.pls
    obs = g.obs_dev
    cbs = [L.IcemCemBuffersC.from_buffer_copy(pl._cem_cb(None, s.mean, s.std, s.lower, s.upper, obs_ptr=obs[i].data_ptr()))
           for i, (pl, s) in enumerate(zip(pls, g.dists))]
    hs = [pl._h for pl in pls] if handles is None else handles
    n = len(hs) if n is None else n
    st = [pl.mpc_step for pl in pls] if steps is None else steps
    p = L.IcemCemParamsC(*[int(f) for f in FLAGS], 0)
    L.check(pls[0].lib.icem_plan_step_cem_learned_models(
        (C.c_void_p * len(hs))(*hs), n, (L.IcemCemBuffersC * len(cbs))(*cbs) if buffers else None, C.byref(p) if prm else None, members,
        None if table is None else (C.c_void_p * len(table))(*table), reduce, None if null_steps else (C.c_int32 * len(st))(*st), None, None,
        pls[0]._stream()))


def _cem_refusal_group(**cfg):
    g = CemGroup(2, "shared", lambda **kw: CL.planner(250, 12, **{**dict(K=10, iters=2), **cfg}, **kw))
    g.obs_dev = torch.as_tensor(np.stack([observation(i, 0) for i in range(2)]), device="cuda")
    return g


CEM_INVALID = {
    "a NULL params table": lambda g, t: dict(table=None),
    "a NULL entry of params_host": lambda g, t: dict(table=t[:3] + [None]),
    "NULL buffers": lambda g, t: dict(buffers=False),
    "NULL flags": lambda g, t: dict(prm=False),
    "NULL steps": lambda g, t: dict(null_steps=True),
    "n = 0": lambda g, t: dict(n=0),
    "n = 33": lambda g, t: dict(n=33),
    "members = 0": lambda g, t: dict(members=0),
    "members = 33": lambda g, t: dict(members=33),
    "a bad reduce": lambda g, t: dict(reduce=2),
    "a handle twice": lambda g, t: dict(handles=[g.pls[0]._h, g.pls[0]._h]),
    "a negative step": lambda g, t: dict(steps=[0, -1]),
}


@pytest.mark.parametrize("case", list(CEM_INVALID))
def test_cem_invalid_arguments_are_refused_before_anything_runs(case):
    from icem_amd import _lib as L
    g = _cem_refusal_group()
    table = [p for _ in range(2) for p in g.models._param_ptrs()]
    kw = dict(table=table, members=2)
    kw.update(CEM_INVALID[case](g, table))
    CL._spoilable(g)
    torch.cuda.synchronize()
    before = CL._snapshot(g)
    with pytest.raises(L.IcemError) as e:
        _raw_cem(g, kw.pop("table"), kw.pop("members"), **kw)
    assert e.value.code == L.ICEM_E_INVALID and "icem_plan_step_cem_learned_models" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    for x, y in zip(CL._snapshot(g), before):
        assert np.array_equal(x, y)


def test_cem_unequal_configurations_and_widths_are_invalid():
    from icem_amd import _lib as L
    g = _cem_refusal_group()
    g.pls[1] = CL.planner(266, 12, 10, 2, seed=6)
    g.dists[1] = Dist(g.pls[1], False)
    table = [p for _ in range(2) for p in g.models._param_ptrs()]
    with pytest.raises(L.IcemError) as e:
        _raw_cem(g, table, 2)
    assert e.value.code == L.ICEM_E_INVALID and "one configuration" in str(e.value)
    g = CemGroup(2, "shared", lambda **kw: CL.planner(250, 12, 10, 2, d=2, **kw))   # one handle bound to width 2, the other never
    g.obs_dev = torch.zeros((2, 230), dtype=torch.float32, device="cuda")
    assert g.pls[0]._bind_rssm(LM.model(11, 2))
    with pytest.raises(L.IcemError) as e:
        _raw_cem(g, table, 2)
    assert e.value.code == L.ICEM_E_INVALID and "one configuration" in str(e.value)


CEM_UNSUPPORTED = {
    "n x members = 34": (dict(), None),
    "an f64 handle": (dict(dtype="f64"), None),
    "K = 33": (dict(K=33), None),
    "keep_previous_elites": (dict(keep_previous_elites=True), None),
    "option cem_step = 0": (dict(), ("cem_step", 0)),
    "option rssm_split = 0": (dict(), ("rssm_split", 0)),
    "the tiles of a rollout": (dict(), ("rssm_split_max_n", 512)),   # 32 tiles: one problem x 1 member is 16, 2 x 2 are 64
}


@pytest.mark.parametrize("case", list(CEM_UNSUPPORTED))
def test_cem_what_is_not_served_is_refused_before_anything_runs(case):
    from icem_amd import _lib as L
    cfg, option = CEM_UNSUPPORTED[case]
    g = _cem_refusal_group(**cfg)
    E = 17 if case == "n x members = 34" else 2
    table = [p for _ in range(2) for p in ensemble(E)._param_ptrs()]
    try:
        if option:
            L.set_option(*option)
        assert not g.pls[0].cem_learned_models_step_ok(2, E)
        CL._spoilable(g)
        torch.cuda.synchronize()
        before = CL._snapshot(g)
        with pytest.raises(L.IcemError) as e:
            _raw_cem(g, table, E)
        assert e.value.code == L.ICEM_E_UNSUPPORTED and "icem_plan_step_cem_learned_models" in str(e.value), str(e.value)
        if case == "the tiles of a rollout":
            assert "tiles" in str(e.value) and g.pls[0].cem_learned_models_step_ok(1, 1)
        torch.cuda.synchronize()
        for x, y in zip(CL._snapshot(g), before):
            assert np.array_equal(x, y)
    finally:
        L.reset_options()


def test_cem_growing_the_rollouts_staging_under_capture_is_a_state_error():
    """The learned-dynamics rollout's staging rule, looked at before the first launch.  A small step sizes this stream's staging
    area (256 tiles at this horizon); under capture on that stream a step of 2 x 129 = 258 tiles would have to grow it, which
    means synchronising: refused with ICEM_E_STATE, nothing launched, every buffer as it was, and the capture goes on."""
    from icem_amd import _lib as L
    small, big = CemGroup(1, "shared"), CemGroup(1, "shared", lambda **kw: CL.planner(2064, 12, 10, 3, **kw))
    obs = torch.as_tensor(observation(0, 0), device="cuda").reshape(1, 230)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        small.step_batch(obs)
        small.step_batch(obs)   # (both slots of its argument array)
        CL._spoilable(big)
        side.synchronize()
    before = CL._snapshot(big)
    assert big.pls[0].cem_learned_models_step_ok(1, 2)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        with pytest.raises(L.IcemError) as e:
            big.step_batch(obs)
        small.step_batch(obs)   # (the capture is intact: a step that fits is recorded)
    assert e.value.code == L.ICEM_E_STATE and "capturing" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    for x, y in zip(CL._snapshot(big), before):
        assert np.array_equal(x, y)


# ================================================================================================ random shooting
def rnd_chain_step(pl, obs, offset, freq, ens):
    """RL.chain_step with the costs of ``ens`` -> the four buffers."""
    from icem_amd import _lib as L
    actions = pl.sample_piecewise(pl.cfg.num_traj, offset, freq, None, 0)
    costs = ens.rollout_cost(obs, actions, L.COST_MODES[pl.cfg.cost_mode])
    best_cost, idx = pl.topk_sorted(costs, 1)
    best = int(idx[0])
    result = torch.cat([actions[best, 0], best_cost.to(pl.dt), idx.to(pl.dt)])
    return dict(actions=actions, costs=costs, best_actions=actions[best].clone(), result=result)


def rnd_fused(pls, models, obs, offsets, freq, **kw):
    from icem_amd import IcemPlanner
    return IcemPlanner.plan_step_random_learned_models(pls, models, obs, offsets, freq, **kw)


def rnd_against_the_chain(make, E, reduce, freq, steps=2, d=6, nan_member=None, equal_nan=False):
    fused, twin = make(), make()
    ef, et = ensemble(E, reduce, d, nan_member), ensemble(E, reduce, d, nan_member)
    assert fused._bind_rssm(ef) and fused.random_learned_models_step_ok(1, E)
    per_step, off = fused.cfg.num_traj * fused.h, 3
    for s in range(steps):
        obs = observation(0, s)
        ex = rnd_fused([fused], ef, [obs], [off], freq)
        got, want = RL.views(fused), rnd_chain_step(twin, obs, off, freq, et)
        torch.cuda.synchronize()
        for k in RL.NAMES:
            assert got[k].shape == want[k].shape and np.array_equal(np_(got[k]), np_(want[k]), equal_nan=equal_nan), (s, k)
        res = fused.random_batch_results
        assert np.array_equal(np_(res[0]), np_(want["result"]), equal_nan=equal_nan) and np.array_equal(np_(ex), np_(res[:, :-2]))
        assert np.array_equal(np_(ef.member_costs), np_(et.member_costs), equal_nan=equal_nan), (s, "member_costs")
        assert fused.random_batch_launches == 3   # 3 launches whatever the member count
        off += per_step
    return fused, ef


@pytest.mark.parametrize("hold", [1, 4])
@pytest.mark.parametrize("N", [40, 250, 16400])
def test_random_the_fused_step_equals_the_operator_chain(N, hold):
    rnd_against_the_chain(lambda: RL.planner(N, 12 if N < 16400 else 5), 2, "mean", hold)


@pytest.mark.parametrize("reduce", ["mean", "max"])
@pytest.mark.parametrize("E", [3, 5, 9, 32])
def test_random_member_counts_and_reductions(E, reduce):
    rnd_against_the_chain(lambda: RL.planner(250, 12), E, reduce, 4, steps=1)


@pytest.mark.parametrize("mode", ["sum", "best", "final"])
def test_random_cost_modes(mode):
    rnd_against_the_chain(lambda: RL.planner(250, 12, mode=mode), 3, "max", 4, steps=1)


def test_random_act_dim_two_runs_the_runtime_width_twins():
    rnd_against_the_chain(lambda: RL.planner(250, 12, d=2), 3, "mean", 4, d=2)


@pytest.mark.parametrize("reduce", ["mean", "max"])
@pytest.mark.parametrize("who", [0, 2])
def test_random_a_nan_member_ends_the_step_as_the_chain_does(who, reduce):
    fused, ens = rnd_against_the_chain(lambda: RL.planner(250, 12), 3, reduce, 4, steps=1, nan_member=who, equal_nan=True)
    assert np.isnan(np_(ens.member_costs)[who]).all() and np.isnan(np_(fused.random_costs)).all()
    assert int(np_(fused.random_result)[-1]) == 0   # every key is (+inf, index): row 0 wins


class RndGroup:
    """B planners (seed 5 + i) with call counters of their own and the models they plan through (``kind`` as CemGroup's)."""

    def __init__(self, B, kind, make=lambda **kw: RL.planner(250, 12, **kw), reduce="mean", E=2, start=None):
        self.pls = [make(seed=5 + i) for i in range(B)]
        self.calls = [7 * i if start is None else start[i] for i in range(B)]
        self.per_step = self.pls[0].cfg.num_traj * self.pls[0].h
        if kind == "shared":
            self.models = ensemble(E, reduce)
            self.each = [self.models] * B
        elif kind == "model_each":
            self.models = LM.members(B)
            self.each = [ensemble(1, first=i) for i in range(B)]
        else:
            self.models = self.each = [ensemble(E, reduce, first=i) for i in range(B)]

    def _advance(self):
        self.calls = [c + self.per_step for c in self.calls]

    def step_batch(self, obs, freq, **kw):
        ex = rnd_fused(self.pls, self.models, obs, self.calls, freq, **kw)
        self._advance()
        return ex

    def step_solo(self, obs, freq):
        for pl, ob, c, m in zip(self.pls, obs, self.calls, self.each):
            rnd_fused([pl], m, [ob], [c], freq)
        self._advance()

    def step_chain(self, obs, freq):
        """The operator chain; its results go where the fused steps leave theirs."""
        for pl, ob, c, m in zip(self.pls, obs, self.calls, self.each):
            out = rnd_chain_step(pl, ob, c, freq, m)
            for k in RL.NAMES:
                getattr(pl, "random_" + k).copy_(out[k])
        self._advance()


@pytest.mark.parametrize("kind", ["shared", "model_each", "ensemble_each"])
def test_random_a_batch_of_three_equals_its_solo_twins_and_the_chain(kind):
    """... with problem 1 an episode (and 1000 calls) ahead of its peers."""
    start = [0, 1000, 14]
    batch, twins, chains = (RndGroup(3, kind, start=start) for _ in range(3))
    for g in (batch, twins, chains):
        g.pls[1].new_episode()
    for s in range(2):
        obs = [observation(i, s) for i in range(3)]
        batch.step_batch(obs, 4)
        twins.step_solo(obs, 4)
        chains.step_chain(obs, 4)
        res = batch.pls[0].random_batch_results
        RL.assert_equal(batch, twins, (kind, s), res)
        RL.assert_equal(batch, chains, (kind, s, "chain"), res)
        assert_member_costs_left(batch, chains, kind, 250, (kind, s))
        assert batch.pls[0].random_batch_launches == 3 and all(pl.random_batch_launches == 0 for pl in batch.pls[1:])
    assert not np.array_equal(np_(batch.pls[0].random_costs), np_(batch.pls[2].random_costs))


def test_random_a_batch_of_two_with_two_selection_slices():
    """(a model each: 2 x 1025 tiles -- two members each would be 4100, past the rollout's 4096)"""
    make = lambda **kw: RL.planner(16400, 2, **kw)   # noqa: E731
    batch, chains = RndGroup(2, "model_each", make), RndGroup(2, "model_each", make)
    assert batch.pls[0].random_learned_models_step_ok(2, 1) and not batch.pls[0].random_learned_models_step_ok(2, 2)
    obs = [observation(i, 0) for i in range(2)]
    batch.step_batch(obs, 1)
    chains.step_chain(obs, 1)
    RL.assert_equal(batch, chains, "two slices", batch.pls[0].random_batch_results)


@pytest.mark.parametrize("B,E", [(32, 1), (1, 32)])
def test_random_thirty_two_problems_in_one_rollout(B, E):
    make = lambda **kw: RL.planner(40, 4, **kw)   # noqa: E731
    kind = "model_each" if E == 1 else "shared"
    batch, chains = RndGroup(B, kind, make, E=E), RndGroup(B, kind, make, E=E)
    assert batch.pls[0].random_learned_models_step_ok(B, E) and not batch.pls[0].random_learned_models_step_ok(B + 1, E)
    for s in range(2):
        obs = [observation(i, s) for i in range(B)]
        batch.step_batch(obs, 1)
        chains.step_chain(obs, 1)
        RL.assert_equal(batch, chains, (B, E, s), batch.pls[0].random_batch_results)


def test_random_one_member_with_equal_pointers_is_the_learned_batch_entry():
    from icem_amd import IcemPlanner
    m = LM.model(3)
    a, b = RndGroup(3, "model_each"), RndGroup(3, "model_each")
    a.models = [m] * 3
    for s in range(2):
        obs = [observation(i, s) for i in range(3)]
        a.step_batch(obs, 4)
        IcemPlanner.plan_step_random_learned_batch(b.pls, m, obs, b.calls, 4)
        b._advance()
        RL.assert_equal(a, b, s, a.pls[0].random_batch_results)
    a1, b1 = RndGroup(1, "model_each"), RndGroup(1, "model_each")
    a1.models = [m]
    a1.step_batch([observation(0, 0)], 4)
    b1.pls[0].plan_step_random_learned(m, observation(0, 0), b1.calls[0], 4)
    b1._advance()
    RL.assert_equal(a1, b1, "solo")


def test_random_a_callers_member_costs_holds_the_rollout():
    batch, chains = RndGroup(3, "ensemble_each"), RndGroup(3, "ensemble_each")
    N = 250
    mc = torch.full((2 * 3 * N + 5,), -7.0, dtype=torch.float32, device="cuda")
    obs = [observation(i, 0) for i in range(3)]
    batch.step_batch(obs, 4, member_costs=mc)
    chains.step_chain(obs, 4)
    torch.cuda.synchronize()
    got = np_(mc[:2 * 3 * N]).reshape(2, 3 * N)
    for p, ens in enumerate(chains.each):
        assert np.array_equal(got[:, p * N:(p + 1) * N], np_(ens.member_costs)), p
    assert (np_(mc[2 * 3 * N:]) == -7.0).all()


def test_random_the_steady_state_uploads_nothing_and_entries_alternate():
    """... on handles that also have a built-in model: the chain, one planner alone, the batch, the single-model learned batch's
    sibling and the built-in batch take turns, and the models steps are the twins'."""
    from icem_amd import IcemPlanner
    make = lambda **kw: RL.planner(250, 12, builtin=True, **kw)   # noqa: E731
    batch, twins = RndGroup(3, "shared", make), RndGroup(3, "shared", make)
    seen = []
    for s in range(4):
        obs = [observation(i, s) for i in range(3)]
        batch.step_batch(obs, 4)
        twins.step_chain(obs, 4)
        seen.append(batch.pls[0].batch_uploads)
    RL.assert_equal(batch, twins, "steady", batch.pls[0].random_batch_results)
    assert seen == [1, 1, 1, 1] and all(pl.batch_uploads == 0 for pl in batch.pls[1:])
    for s in range(4, 8):
        obs = [observation(i, s) for i in range(3)]
        if s % 4 == 2:   # a detour: the solo learned entry and the built-in batch on the same handles (offsets are the caller's)
            batch.pls[0].plan_step_random_learned(LM.model(3), obs[0], 5, 4)
            IcemPlanner.plan_step_random_batch(batch.pls, [0.1 * np.ones(17)] * 3, [0, 1, 2], 4)
        (batch.step_chain, batch.step_solo, batch.step_batch, batch.step_batch)[s % 4](obs, 4)
        twins.step_chain(obs, 4)
        RL.assert_equal(batch, twins, s)


def test_random_a_captured_step_replays_with_a_fresh_observation():
    batch, chains = RndGroup(2, "shared"), RndGroup(2, "shared")
    obs = [[torch.as_tensor(observation(i, s), device="cuda") for i in range(2)] for s in range(2)]
    tables = [o.clone() for o in obs[0]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        batch.step_batch(tables, 4)   # (outside the capture: the rollout's staging area, the pool, the argument array)
        side.synchronize()
    batch.calls = list(chains.calls)
    uploads = batch.pls[0].batch_uploads
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        batch.step_batch(tables, 4)
    assert batch.pls[0].batch_uploads == uploads and batch.pls[0].random_batch_launches == 3
    torch.cuda.synchronize()
    for t, o in zip(tables, obs[1]):
        t.copy_(o)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    chains.step_chain([np_(o) for o in obs[1]], 4)
    RL.assert_equal(batch, chains, "replay", batch.pls[0].random_batch_results)


def _rnd_snapshot(g):
    out = []
    for pl in g.pls:
        out += [np_(x).copy() for x in RL.views(pl).values()]
        out.append(np.array([pl.random_batch_launches, pl.random_step_launches, pl.batch_uploads]))
    return out


def _rnd_spoilable(g):
    for j, pl in enumerate(g.pls):
        for k in RL.NAMES:
            getattr(pl, "random_" + k).fill_(1.5 + j)


def _raw_rnd(g, table, members, *, reduce=0, n=None, handles=None, offsets=None, freq=4, buffers=True, null_offsets=False, null_buffer=False):
    from icem_amd import _lib as L
    pls = g.pls
    cbs = [L.IcemRandomBuffersC.from_buffer_copy(pl._random_cb(observation(i, 0), "obs_rssm")) for i, pl in enumerate(pls)]
    if null_buffer:
        cbs[1].best_actions = None
    hs = [pl._h for pl in pls] if handles is None else handles
    n = len(hs) if n is None else n
    offs = g.calls if offsets is None else offsets
    L.check(pls[0].lib.icem_plan_step_random_learned_models(
        (C.c_void_p * len(hs))(*hs), n, (L.IcemRandomBuffersC * len(cbs))(*cbs) if buffers else None, members,
        None if table is None else (C.c_void_p * len(table))(*table), reduce, freq, None if null_offsets else (C.c_int64 * len(offs))(*offs),
        None, None, pls[0]._stream()))


RND_INVALID = {
    "a NULL params table": lambda g, t: dict(table=None),
    "a NULL entry of params_host": lambda g, t: dict(table=[None] + t[1:]),
    "NULL buffers": lambda g, t: dict(buffers=False),
    "NULL offsets": lambda g, t: dict(null_offsets=True),
    "a NULL buffer": lambda g, t: dict(null_buffer=True),
    "n = 0": lambda g, t: dict(n=0),
    "n = 33": lambda g, t: dict(n=33),
    "members = 0": lambda g, t: dict(members=0),
    "members = 33": lambda g, t: dict(members=33),
    "a bad reduce": lambda g, t: dict(reduce=-1),
    "a handle twice": lambda g, t: dict(handles=[g.pls[1]._h, g.pls[1]._h]),
    "a negative offset": lambda g, t: dict(offsets=[0, -1]),
    "a negative change_freq": lambda g, t: dict(freq=-1),
    "change_freq = horizon": lambda g, t: dict(freq=12),
}


@pytest.mark.parametrize("case", list(RND_INVALID))
def test_random_invalid_arguments_are_refused_before_anything_runs(case):
    from icem_amd import _lib as L
    g = RndGroup(2, "shared")
    table = [p for _ in range(2) for p in g.models._param_ptrs()]
    kw = dict(table=table, members=2)
    kw.update(RND_INVALID[case](g, table))
    _rnd_spoilable(g)
    torch.cuda.synchronize()
    before = _rnd_snapshot(g)
    with pytest.raises(L.IcemError) as e:
        _raw_rnd(g, kw.pop("table"), kw.pop("members"), **kw)
    assert e.value.code == L.ICEM_E_INVALID and "icem_plan_step_random_learned_models" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    for x, y in zip(_rnd_snapshot(g), before):
        assert np.array_equal(x, y)


def test_random_unequal_configurations_and_widths_are_invalid():
    from icem_amd import _lib as L
    g = RndGroup(2, "shared")
    g.pls[1] = RL.planner(266, 12, seed=6)
    table = [p for _ in range(2) for p in g.models._param_ptrs()]
    for g in (g, RndGroup(2, "shared", lambda **kw: RL.planner(250, 12, d=2, **kw))):   # the second: one handle bound to width 2, the other never
        if g.pls[0].d == 2:
            assert g.pls[0]._bind_rssm(LM.model(11, 2)) and g.pls[0].lib.icem_rssm_act_dim(g.pls[0]._h) != g.pls[1].lib.icem_rssm_act_dim(g.pls[1]._h)
        _rnd_spoilable(g)
        torch.cuda.synchronize()
        before = _rnd_snapshot(g)
        with pytest.raises(L.IcemError) as e:
            _raw_rnd(g, table, 2)
        assert e.value.code == L.ICEM_E_INVALID and "one configuration" in str(e.value), str(e.value)
        torch.cuda.synchronize()
        for x, y in zip(_rnd_snapshot(g), before):
            assert np.array_equal(x, y)


def test_random_growing_the_rollouts_staging_under_capture_is_a_state_error():
    """The learned-dynamics rollout's staging rule, looked at before the first launch.  A small step sizes this stream's staging
    area (256 tiles at this horizon); under capture on that stream a step of 2 x 129 = 258 tiles would have to grow it, which
    means synchronising: refused with ICEM_E_STATE, nothing launched, every buffer as it was, and the capture goes on."""
    from icem_amd import _lib as L
    small, big = RndGroup(1, "shared"), RndGroup(1, "shared", lambda **kw: RL.planner(2064, 12, **kw))
    obs = torch.as_tensor(observation(0, 0), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        small.step_batch([obs], 4)
        big.pls[0]._random_cb(obs, "obs_rssm")   # (the planner's buffers exist before the capture)
        _rnd_spoilable(big)
        side.synchronize()
    before = _rnd_snapshot(big)
    assert big.pls[0].random_learned_models_step_ok(1, 2)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        with pytest.raises(L.IcemError) as e:
            big.step_batch([obs], 4)
        small.step_batch([obs], 4)   # (the capture is intact: a step that fits is recorded)
    assert e.value.code == L.ICEM_E_STATE and "capturing" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    for x, y in zip(_rnd_snapshot(big), before):
        assert np.array_equal(x, y)


RND_UNSUPPORTED = {
    "n x members = 34": (dict(), None),
    "an f64 handle": (dict(dtype="f64"), None),
    "act_dim 5, never bound": (dict(d=5), None),
    "option random_step = 0": (dict(), ("random_step", 0)),
    "option rssm_split = 0": (dict(), ("rssm_split", 0)),
    "the tiles of the rollout": (dict(), ("rssm_split_max_n", 512)),
}


@pytest.mark.parametrize("case", list(RND_UNSUPPORTED))
def test_random_what_is_not_served_is_refused_before_anything_runs(case):
    from icem_amd import _lib as L
    cfg, option = RND_UNSUPPORTED[case]
    g = RndGroup(2, "shared", lambda **kw: RL.planner(250, 12, **cfg, **kw))
    E = 17 if case == "n x members = 34" else 2
    table = [p for _ in range(2) for p in ensemble(E)._param_ptrs()]
    try:
        if option:
            L.set_option(*option)
        assert not g.pls[0].random_learned_models_step_ok(2, E)
        _rnd_spoilable(g)
        torch.cuda.synchronize()
        before = _rnd_snapshot(g)
        with pytest.raises(L.IcemError) as e:
            _raw_rnd(g, table, E)
        assert e.value.code == L.ICEM_E_UNSUPPORTED and "icem_plan_step_random_learned_models" in str(e.value), str(e.value)
        if case == "the tiles of the rollout":
            assert "tiles" in str(e.value) and g.pls[0].random_learned_models_step_ok(1, 1)
        torch.cuda.synchronize()
        for x, y in zip(_rnd_snapshot(g), before):
            assert np.array_equal(x, y)
    finally:
        L.reset_options()


# ================================================================================================ the controllers
def cem_controller(m, fused_step=None, seed=3, **kw):
    return CL.controller(fused_step, seed=seed, m=m, **kw)


def rnd_controller(m, fused_step=None, seed=3, N=250):
    from icem_amd import MpcRandomHip, halfcheetah_env
    return MpcRandomHip(env=halfcheetah_env(17), forward_model=m, horizon=12, num_simulated_trajectories=N, cost_along_trajectory="sum",
                        verbose=False, seed=seed, fused_step=fused_step, action_sampler_params=dict(action_change_frequency=4))


def rnd_same_state(a, b, where):
    assert a.calls == b.calls and a.best_traj_idx == b.best_traj_idx and a.last_min_cost == b.last_min_cost, where
    assert np.array_equal(np_(a._last_actions), np_(b._last_actions)) and np.array_equal(np_(a._last_costs), np_(b._last_costs)), where


KINDS = {"cem": (cem_controller, CL.same_state), "random": (rnd_controller, rnd_same_state)}


def launches(c, kind):
    return c.planner.cem_batch_launches if kind == "cem" else c.planner.random_batch_launches


@pytest.mark.parametrize("kind", list(KINDS))
def test_get_action_on_an_ensemble_takes_the_entry_and_equals_the_stage_wise_twin(kind):
    make, same = KINDS[kind]
    a, b, c = make(ensemble(3), True), make(ensemble(3), False), make(ensemble(3), None)
    assert a._fused_step_refusal() is None and a._steps_through_an_ensemble() and not a._steps_through_the_rssm()
    for ep in range(2):
        for k in range(2):
            obs = observation(0, 10 * ep + k)
            if k == 0:
                for x in (a, b, c):
                    x.beginning_of_rollout(observation=obs, state=None, mode="train")
            got, want, third = a.get_action(obs, None), b.get_action(obs, None), c.get_action(obs, None)
            assert np.array_equal(got, want) and np.array_equal(third, want), (ep, k)
            same(a, b, (ep, k))
            same(c, b, (ep, k))
            assert np.array_equal(np_(a.forward_model.member_costs), np_(b.forward_model.member_costs))
    assert launches(a, kind) == (9 if kind == "cem" else 3) and launches(b, kind) == 0


@pytest.mark.parametrize("kind", list(KINDS))
def test_an_instrumented_ensemble_is_still_called_stage_by_stage(kind):
    make, same = KINDS[kind]
    ens, calls = ensemble(3), []
    inner = ens.rollout_cost
    ens.rollout_cost = lambda obs, actions, cost_mode=0: (calls.append(1), inner(obs, actions, cost_mode))[1]
    c, t = make(ens), make(ensemble(3), True)
    assert "not the library's own RSSM" in c._fused_step_refusal()
    obs = observation(0, 0)
    for x in (c, t):
        x.beginning_of_rollout(observation=obs, state=None, mode="train")
    assert np.array_equal(c.get_action(obs, None), t.get_action(obs, None))
    same(c, t, kind)
    assert len(calls) == (3 if kind == "cem" else 1) and launches(c, kind) == 0
    strict = make(ens, True)
    strict.beginning_of_rollout(observation=obs, state=None, mode="train")
    with pytest.raises(RuntimeError, match="fused_step=True"):
        strict.get_action(obs, None)
    assert strict.planner.mpc_step == 0 and getattr(strict, "calls", 0) == 0


def step_together(cls, ctrls, obs, own_models=False):
    """(the baselines spell ``own_models=True`` as a method of its own: ``get_action_batch``'s parameter list is pinned)"""
    return (cls.get_action_batch_own_models if own_models else cls.get_action_batch)(ctrls, obs)


def drive_batch(cls, ctrls, twins, same, steps=2, **kw):
    for k in range(steps):
        obs = [observation(i, k) for i in range(len(ctrls))]
        if k == 0:
            for c, ob in zip(itertools.chain(ctrls, twins), obs + obs):
                c.beginning_of_rollout(observation=ob, state=None, mode="train")
        got = step_together(cls, ctrls, obs, **kw)
        want = [t.get_action(ob, None) for t, ob in zip(twins, obs)]
        for i, (a, b) in enumerate(zip(ctrls, twins)):
            assert np.array_equal(got[i], want[i]), (k, i)
            same(a, b, (k, i))


@pytest.mark.parametrize("models", ["shared", "model_each", "ensemble_each"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_get_action_batch_through_models_equals_twins_stepping_alone(kind, models):
    from icem_amd import MpcCemStdHip, MpcRandomHip
    make, same = KINDS[kind]
    cls = MpcCemStdHip if kind == "cem" else MpcRandomHip
    if models == "shared":
        e1, e2 = ensemble(2), ensemble(2)
        ms, mt = [e1] * 3, [e2] * 3
    elif models == "model_each":
        ms = mt = LM.members(3)
    else:
        ms, mt = [ensemble(2, first=i) for i in range(3)], [ensemble(2, first=i) for i in range(3)]
    ctrls = [make(m, None, seed=3 + i) for i, m in enumerate(ms)]
    twins = [make(m, False, seed=3 + i) for i, m in enumerate(mt)]
    if models != "shared":   # without the keyword: refused with the words the existing tests pin, each controller's own step runs
        for c in ctrls + twins:   # (the twins too: a CEM controller's episode counts its resets)
            c.beginning_of_rollout(observation=observation(0, 0), state=None, mode="train")
        assert "share one DeviceRSSMModel" in cls._batch_refusal(ctrls)
    drive_batch(cls, ctrls, twins, same, own_models=models != "shared")
    assert launches(ctrls[0], kind) == (9 if kind == "cem" else 3) and all(launches(c, kind) == 0 for c in ctrls[1:])


@pytest.mark.parametrize("kind", list(KINDS))
def test_fused_step_true_raises_where_the_step_is_not_served_and_nothing_has_advanced(kind):
    from icem_amd import MpcCemStdHip, MpcRandomHip
    from icem_amd import _lib as L
    make, same = KINDS[kind]
    cls = MpcCemStdHip if kind == "cem" else MpcRandomHip
    obs = [observation(i, 0) for i in range(2)]

    def pair(fused_step, each=True):
        cs = [make(ensemble(2, first=i if each else 0), fused_step, seed=3 + i) for i in range(2)]
        for c, ob in zip(cs, obs):
            c.beginning_of_rollout(observation=ob, state=None, mode="train")
        return cs
    with pytest.raises(RuntimeError, match="share one DeviceRSSMModel"):   # an ensemble each, without the keyword
        cls.get_action_batch(pair(True), obs)
    try:
        L.set_option("cem_step" if kind == "cem" else "random_step", 0)
        c = pair(True)[0]
        with pytest.raises(RuntimeError, match="fused_step=True.*learned_models_step_ok"):
            c.get_action(obs[0], None)
        with pytest.raises(RuntimeError, match="fused_step=True"):
            step_together(cls, pair(True), obs, own_models=True)
        assert c.planner.mpc_step == 0 and getattr(c, "calls", 0) == 0
        ctrls, twins = pair(None), pair(False)   # fused_step=None: each controller's own step, in order -- the loop here
        got = step_together(cls, ctrls, obs, own_models=True)
        for i, (a, t) in enumerate(zip(ctrls, twins)):
            assert np.array_equal(got[i], t.get_action(obs[i], None)), i
            same(a, t, i)
            assert launches(a, kind) == 0
    finally:
        L.reset_options()


def test_icem_controllers_with_an_ensemble_each_step_together():
    """``MpcICemHip.get_action_batch(own_models=True)`` over controllers that each own an ensemble (one size, one reduction) against
    twins stepping alone; without the keyword it is refused as ever."""
    from icem_amd import MpcICemHip
    ctrls = [LM.controller(ensemble(2, first=i), 5 + i) for i in range(3)]
    twins = [LM.controller(ensemble(2, first=i), 5 + i) for i in range(3)]
    obs = LM.TL.observations(3)
    for c, ob in zip(ctrls + twins, list(obs) + list(obs)):
        LM.TL.begin(c, ob)
    with pytest.raises(NotImplementedError, match="own_models=True"):
        MpcICemHip.get_action_batch(ctrls, obs)
    assert all(c.planner.mpc_step == 0 for c in ctrls)
    for k in range(2):
        got = MpcICemHip.get_action_batch(ctrls, obs, own_models=True)
        for i, (c, t) in enumerate(zip(ctrls, twins)):
            assert np.array_equal(got[i], t.get_action(obs[i], None)), (k, i)
            LM.same_state(c, t, (k, i))
            assert np.array_equal(np_(c.forward_model.member_costs), np_(t.forward_model.member_costs)), (k, i, "member_costs")
        assert ctrls[0].planner.learned_step_launches == LM.launches_of(ctrls[0], k)
    mixed = [LM.controller(ensemble(2), 5), LM.controller(ensemble(3), 6)]
    for c, ob in zip(mixed, obs):
        LM.TL.begin(c, ob)
    with pytest.raises(NotImplementedError, match="one size and one reduction"):
        MpcICemHip.get_action_batch(mixed, obs[:2], own_models=True)
