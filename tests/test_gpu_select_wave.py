"""The seven-wave merge prologue of the single-launch kernel (``sample_rollout_kernel`` at one tile per workgroup, d = 6: six
quad-sampling waves + the selection wave, k_iter_small.hip) at the sizes where its role map can go wrong, whichever wave holds
which role: a row's draw is keyed by the row, not by the thread that draws it, so nothing a caller sees depends on the map.
``plan_step`` (every merge but the last rides in the next iteration's launch) against the split API (one merge launch per
iteration, no prologue), bit for bit -- executed action, mean, std, best cost, elite rows and costs, the last pool's actions and
costs -- at one full slab (every sampling thread live), a partial last slab and seventeen slabs, both model kinds, both tile
arithmetics (the exact tile rolls out on four waves of the same workgroup), three iterations and three MPC steps with kept and
shifted elites; and two problems in one batched launch against their solo steps.  (EXPERIMENTS R13.1: the census of where the seven
waves run, the selection moved to the wave alone on its SIMD -- measured, not kept -- and the kernel's argument lines requested
at entry.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, D, O = 30, 6, 17


def np_(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _make(N, kind, arith, seed=11, i=0):
    from icem_amd import DeviceSyntheticModel, IcemConfig, IcemPlanner, halfcheetah_env
    env = halfcheetah_env(O)
    model = DeviceSyntheticModel.make(O, D, kind=kind, seed_a=10 + i, seed_b=20 + i)
    # factor_decrease = 1 and 2 * elites_size <= N (the smallest population an iteration gets): every iteration -- the
    # merge-prologue launches are iterations 1 and 2 -- has the N rows of the case
    pl = IcemPlanner(IcemConfig(horizon=H, act_dim=D, num_traj=N, opt_iters=3, dtype="f32", seed=seed + 7 * i, factor_decrease=1.0,
                                elites_size=min(10, N // 2), keep_previous_elites=True, shift_elites=True),
                     env.action_space.low[:D], env.action_space.high[:D])
    pl.set_model(model.kind, model.A, model.B)
    c = env.cost_spec
    pl.set_cost(c.ctrl_weight * (1 + 0.1 * i), c.lin_idx, c.lin_weight, c.flip_idx, c.flip_penalty, c.flip_thresh)
    assert pl.set_tile_arith(arith) == arith
    pl.reset()
    assert list(pl.population_sizes) == [N, N, N]
    return pl


def _state(pl):
    n_last = pl.population_sizes[-1]
    ea, ec = pl.current_elites()
    return {"executed": np_(pl.executed).copy(), "mean": np_(pl.mean).copy(), "std": np_(pl.std).copy(),
            "best_cost": np_(pl.best_cost).copy(), "elite rows": np_(ea).copy(), "elite costs": np_(ec).copy(),
            "pool actions": np_(pl.actions[:n_last]).copy(), "pool costs": np_(pl.costs[:n_last]).copy()}


@pytest.mark.parametrize("N", [16, 40, 272])
@pytest.mark.parametrize("arith", [1, 0])   # fp16 planes; the exact tile (T4 rollout through the same body)
@pytest.mark.parametrize("kind", [0, 1])
def test_seven_wave_merge_prologue_equals_the_split_api(kind, arith, N):
    ride, split = _make(N, kind, arith), _make(N, kind, arith)
    rs = np.random.RandomState(2)
    for step in range(3):
        obs = 0.2 * rs.randn(O)
        a0 = np_(ride.plan_step(obs))
        a1 = np_(split.plan_step(obs, on_iteration=lambda it: None))
        torch.cuda.synchronize()
        assert np.array_equal(a0, a1), step
        s0, s1 = _state(ride), _state(split)
        for name in s0:
            assert np.array_equal(s0[name], s1[name]), (step, name)
        assert np.all(np.isfinite(s0["pool costs"])), step   # (two NaN pools would compare unequal; two +inf pools would not)


@pytest.mark.parametrize("arith", [1, 0])
@pytest.mark.parametrize("kind", [0, 1])
def test_two_problems_in_one_launch_equal_two_solo_steps(kind, arith):
    from icem_amd import IcemPlanner
    B, N = 2, 40
    solo = [_make(N, kind, arith, i=i) for i in range(B)]
    batch = [_make(N, kind, arith, i=i) for i in range(B)]
    for step in range(3):
        obs = [0.1 * (1 + i) * np.random.RandomState(100 * step + i).randn(O) for i in range(B)]
        for i in range(B):
            solo[i].plan_step(obs[i])
        IcemPlanner.plan_step_batch(batch, obs)
        torch.cuda.synchronize()
        for i in range(B):
            s0, s1 = _state(batch[i]), _state(solo[i])
            for name in s0:
                assert np.array_equal(s0[name], s1[name]), (step, i, name)
    assert not np.array_equal(np_(batch[0].executed), np_(batch[1].executed))   # two different problems
