"""The merge that every launch of the headline step but the first carries (selection -> gather -> refit; fused_dev.h
``merge_select_shallow`` / ``merge_rows``, refit.h) at the sizes where it takes another path, with the exact-K kernels
(``sample_rollout_exactk_kernel``, ``merge_single_exactk_kernel``, ``merge_noise_exactk_kernel``: K = 10 known at compile
time) and the runtime-K ones.  Shape (h, d, o) = (30, 6, 17), both model kinds, both tile arithmetics, three iterations, two
MPC steps with kept and shifted elites.

Populations: 16 (one candidate list: every elite comes from it, so the selection reads past the three depths it holds in
registers -- the dependent-load path), 17 (a second list of one row and fifteen sentinel keys), 40 (three lists), 272
(seventeen lists).  K: 10 (the exact-K kernels), 4 and 11 (the runtime-K kernels; 11 fills all but one of the twelve register
slots).  A planner's elite count is at most half its population (``IcemConfig.num_elites``, the reference's rule), so at 16
and 17 rows the cases are K = 8 and 4 -- both on the runtime-K kernels, both deeper than the registers.

What is asserted, per case:
 (a) the elite costs of the step's last iteration, and the elite rows (that is: the indices), are the K smallest
     ``(cost, index)`` pairs of the last pool's costs followed by the kept elites' -- selected here with NumPy from the
     buffers the planner exposes, no code shared with the kernels;
 (b) option ``merge_exact_k`` = 1 against 0, bit for bit: executed action, mean, std, best cost, elite rows and costs;
 (c) ``plan_step`` against the split API (a merge launch per iteration, no prologue), and two problems of one batched launch
     against their solo steps, as test_gpu_select_wave.py does;
 (d) ``icem_nonfinite_costs`` is 0.
One more case has every cost tie (a zero model, no control cost): at 272 rows all 170 listed keys are at the threshold -- more than the
64 the compaction holds, so the selection falls back to its streaming form -- and the K best are the K lowest rows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H, D, O = 30, 6, 17
POPS, KS = (16, 17, 40, 272), (10, 4, 11)
# (population, the planner's elite count): K capped at half the population, duplicates dropped
CASES = sorted({(n, min(k, n // 2)) for n in POPS for k in KS})
NAMES = ("executed", "mean", "std", "best_cost", "elite rows", "elite costs")


def np_(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _make(N, K, kind, arith, seed=5, i=0, all_tie=False):
    from icem_amd import DeviceSyntheticModel, IcemConfig, IcemPlanner, halfcheetah_env
    env = halfcheetah_env(O)
    model = DeviceSyntheticModel.make(O, D, kind=kind, seed_a=30 + i, seed_b=40 + i)
    # factor_decrease = 1 and 2 * K <= N: every iteration has the N rows of the case
    pl = IcemPlanner(IcemConfig(horizon=H, act_dim=D, num_traj=N, opt_iters=3, dtype="f32", seed=seed + 7 * i, factor_decrease=1.0,
                                elites_size=K, keep_previous_elites=True, shift_elites=True),
                     env.action_space.low[:D], env.action_space.high[:D])
    c = env.cost_spec
    if all_tie:   # a zero model and no control cost: every trajectory sees the same states and pays the same
        pl.set_model(model.kind, np.zeros_like(model.A), np.zeros_like(model.B))
        pl.set_cost(0.0, c.lin_idx, c.lin_weight, c.flip_idx, c.flip_penalty, c.flip_thresh)
    else:
        pl.set_model(model.kind, model.A, model.B)
        pl.set_cost(c.ctrl_weight * (1 + 0.1 * i), c.lin_idx, c.lin_weight, c.flip_idx, c.flip_penalty, c.flip_thresh)
    assert pl.set_tile_arith(arith) == arith
    pl.reset()
    assert list(pl.population_sizes) == [N, N, N] and pl.K == K
    return pl


def _state(pl):
    ea, ec = pl.current_elites()
    return {"executed": np_(pl.executed).copy(), "mean": np_(pl.mean).copy(), "std": np_(pl.std).copy(),
            "best_cost": np_(pl.best_cost).copy(), "elite rows": np_(ea).copy(), "elite costs": np_(ec).copy()}


def _numpy_selection(pl):
    """(costs [K], rows [K, h, d]) of the K smallest (cost, index) pairs among the last iteration's pool (index = row) and
    the elites it kept from the iteration before (index = pool size + e) -- from the planner's buffers, after a step."""
    n, K = pl.population_sizes[-1], pl.K
    g = (pl.mpc_step * pl.cfg.opt_iters) & 1           # current_elites()' buffer; the other one: the iteration before
    keep_rows, keep_costs = np_(pl.elites_actions[1 - g])[:pl.n_reuse], np_(pl.elites_costs[1 - g])[:pl.n_reuse]
    costs = np.concatenate([np_(pl.costs[:n]), keep_costs])
    rows = np.concatenate([np_(pl.actions[:n]).reshape(n, H, D), keep_rows.reshape(-1, H, D)])
    order = np.lexsort((np.arange(costs.size), costs))[:K]   # by cost, then by index
    return costs[order], rows[order], order


def _two_steps(pl, split=False):
    rs, out = np.random.RandomState(3), []
    for _ in range(2):
        obs = 0.2 * rs.randn(O)
        if split:
            pl.plan_step(obs, on_iteration=lambda it: None)
        else:
            pl.plan_step(obs)
        torch.cuda.synchronize()
        out.append(_state(pl))
    return out


@pytest.mark.parametrize("N,K", CASES)
@pytest.mark.parametrize("arith", [1, 0])   # fp16 planes (the headline's); the exact tile
@pytest.mark.parametrize("kind", [0, 1])
def test_merge_chain_selects_gathers_and_refits(kind, arith, N, K):
    from icem_amd import _lib as L
    L.set_option("merge_exact_k", 1)
    exact = _make(N, K, kind, arith)
    s_exact = _two_steps(exact)
    # (a) after the second step: kept elites (iterations 1, 2) and shifted elites (iteration 0) have been through the merge
    want_c, want_rows, order = _numpy_selection(exact)
    print(f"\nN={N} K={K} kind={kind} arith={arith}: selected indices {order.tolist()} (>= {N}: kept elites)")
    assert np.all(np.isfinite(want_c))
    assert np.array_equal(s_exact[-1]["elite costs"], want_c)
    assert np.array_equal(s_exact[-1]["elite rows"].reshape(K, H, D), want_rows)
    assert np.array_equal(s_exact[-1]["best_cost"].ravel(), want_c[:1])
    assert exact.nonfinite_costs() == 0   # (d)
    # (b) the runtime-K kernels for every K
    L.set_option("merge_exact_k", 0)
    runtime = _make(N, K, kind, arith)
    s_runtime = _two_steps(runtime)
    for step, (s0, s1) in enumerate(zip(s_exact, s_runtime)):
        for name in NAMES:
            assert np.array_equal(s0[name], s1[name]), ("merge_exact_k 1 / 0", step, name)
    assert runtime.nonfinite_costs() == 0
    # (c) the split API: every merge a launch of its own (merge_single[_exactk]_kernel), none in a prologue
    L.set_option("merge_exact_k", 1)
    split = _make(N, K, kind, arith)
    s_split = _two_steps(split, split=True)
    for step, (s0, s1) in enumerate(zip(s_exact, s_split)):
        for name in NAMES:
            assert np.array_equal(s0[name], s1[name]), ("plan_step / split API", step, name)
    assert split.nonfinite_costs() == 0


@pytest.mark.parametrize("arith", [1, 0])
@pytest.mark.parametrize("kind", [0, 1])
def test_two_problems_in_one_launch_equal_two_solo_steps(kind, arith):
    from icem_amd import IcemPlanner
    B, N, K = 2, 40, 10
    solo = [_make(N, K, kind, arith, i=i) for i in range(B)]
    batch = [_make(N, K, kind, arith, i=i) for i in range(B)]
    for step in range(2):
        obs = [0.1 * (1 + i) * np.random.RandomState(100 * step + i).randn(O) for i in range(B)]
        for i in range(B):
            solo[i].plan_step(obs[i])
        IcemPlanner.plan_step_batch(batch, obs)
        torch.cuda.synchronize()
        for i in range(B):
            s0, s1 = _state(batch[i]), _state(solo[i])
            for name in NAMES:
                assert np.array_equal(s0[name], s1[name]), (step, i, name)
    assert not np.array_equal(np_(batch[0].executed), np_(batch[1].executed))   # two different problems
    assert all(p.nonfinite_costs() == 0 for p in solo + batch)


@pytest.mark.parametrize("N", [40, 272])   # 30 and 170 keys at the threshold: within the compaction's 64, and past them
@pytest.mark.parametrize("exact_k", [1, 0])
def test_all_costs_tie(exact_k, N):
    from icem_amd import _lib as L
    K = 10
    L.set_option("merge_exact_k", exact_k)
    ride, split = _make(N, K, 0, 1, all_tie=True), _make(N, K, 0, 1, all_tie=True)
    s_ride, s_split = _two_steps(ride), _two_steps(split, split=True)
    pool = ride.costs[:N].detach().cpu().numpy()
    assert np.all(pool.view(np.int32) == pool.view(np.int32)[0]), "the case needs every cost to be the same bits"
    want_c, want_rows, order = _numpy_selection(ride)
    print(f"\nN={N} merge_exact_k={exact_k}: selected indices {order.tolist()}")
    assert order.tolist() == list(range(K))   # ties: the lowest rows
    assert np.array_equal(s_ride[-1]["elite costs"], want_c)
    assert np.array_equal(s_ride[-1]["elite rows"].reshape(K, H, D), want_rows)
    for step, (s0, s1) in enumerate(zip(s_ride, s_split)):
        for name in NAMES:
            assert np.array_equal(s0[name], s1[name]), (step, name)
    assert ride.nonfinite_costs() == 0 and split.nonfinite_costs() == 0
