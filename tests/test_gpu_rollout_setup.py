"""The rollout wave's set-up from the start observation -- the wave-wide maximum of |obs0|, the launch's power-of-two scale and
its scalars (icem_amd/csrc/tile_scales.h), the state's first entries -- in the single-launch kernel's merge-prologue launches
(k_iter_small.hip), where the lone rollout wave of the fp16-plane tile runs it AHEAD of the prologue's barriers: in the slack it
has behind its draws, from an observation requested at the kernel's entry.

``plan_step`` takes those launches.  The split API (``icem_plan_iter_local`` + ``icem_plan_iter_merge``, what ``plan_step`` runs
under an ``on_iteration`` callback) merges in a launch of its own, so its rollout kernel has no prologue and does the set-up in
place, behind its last barrier.  Same operations on the same operands: every buffer has to come out bit for bit the same --
for both model kinds and both tile arithmetics (the exact tile has no hoisted set-up: it shares the kernel body), a population
of one full slab (16) and one with a partial last slab (40), start observations over sixty binades and the zero vector (the
scale's exponent then comes from the action bound), solo and as two problems of one batched launch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, D, O = 30, 6, 17
OBS_EXPONENTS = (-30, -8, 0, 8, 30, None)   # obs0 = base x 2^k; None: the zero vector


def np_(t):
    return t.detach().cpu().numpy()


def _planner(N, kind, arith, i=0):
    from icem_amd import DeviceSyntheticModel, IcemConfig, IcemPlanner, halfcheetah_env
    env = halfcheetah_env(O)
    model = DeviceSyntheticModel.make(O, D, kind=kind, seed_a=10 + i, seed_b=20 + i)
    pl = IcemPlanner(IcemConfig(horizon=H, act_dim=D, num_traj=N, opt_iters=2, dtype="f32", seed=11 + 7 * i),
                     env.action_space.low[:D], env.action_space.high[:D])
    pl.set_model(model.kind, model.A, model.B)
    pl.set_cost_spec(env.cost_spec)
    assert pl.set_tile_arith(arith) == arith
    pl.reset()
    return pl


def _obs(k, seed=7):
    base = 0.1 * np.random.RandomState(seed).randn(O)
    return np.zeros(O) if k is None else base * 2.0 ** k


def _state(pl):
    """costs and rows of the last iteration's pool, elite rows and costs, mean, std, the executed action"""
    n_last = pl.population_sizes[-1]
    ea, ec = pl.current_elites()
    return [np_(x).copy() for x in (pl.costs[:n_last], pl.actions[:n_last], ea, ec, pl.mean, pl.std, pl.executed)]


def _split_step(pl, obs):
    pl.plan_step(obs, on_iteration=lambda it: None)


def _same(got, want, where):
    for j, (x, y) in enumerate(zip(got, want)):
        assert np.array_equal(x, y), where + (j,)


@pytest.mark.parametrize("N", [16, 40])
@pytest.mark.parametrize("arith", [0, 1])
@pytest.mark.parametrize("kind", [0, 1])
def test_the_hoisted_set_up_leaves_the_bits_of_the_set_up_in_place(kind, arith, N):
    fused, split = _planner(N, kind, arith), _planner(N, kind, arith)
    for k in OBS_EXPONENTS:
        obs = _obs(k)
        for step in range(2):
            fused.plan_step(obs)
            _split_step(split, obs)
            torch.cuda.synchronize()
            got, want = _state(fused), _state(split)
            assert np.all(np.isfinite(want[0])), (k, step)
            _same(got, want, (k, step))


@pytest.mark.parametrize("N", [16, 40])
@pytest.mark.parametrize("arith", [0, 1])
@pytest.mark.parametrize("kind", [0, 1])
def test_two_problems_of_one_batched_launch_equal_their_split_solo_steps(kind, arith, N):
    from icem_amd import IcemPlanner
    batch = [_planner(N, kind, arith, i) for i in range(2)]
    solo = [_planner(N, kind, arith, i) for i in range(2)]
    # (the two problems' observations lie sixteen binades apart, and one of them is the zero vector in the last round)
    for ka, kb in ((-8, 8), (30, -30), (0, None)):
        obs = [_obs(ka, 7), _obs(kb, 8)]
        for step in range(2):
            IcemPlanner.plan_step_batch(batch, obs)
            for pl, o in zip(solo, obs):
                _split_step(pl, o)
            torch.cuda.synchronize()
            for i in range(2):
                _same(_state(batch[i]), _state(solo[i]), (ka, kb, step, i))
    assert not np.array_equal(np_(batch[0].executed), np_(batch[1].executed))   # (they ARE two problems)
