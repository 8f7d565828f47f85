"""``icem_plan_step_batch`` on the TileHN shapes -- Door (d = 28, o = 39; icem/environments/mjenvs.py:57-78), Relocate (d = 30,
o = 39; mjenvs.py:155-174), FetchPickAndPlace (d = 4, o = 28; icem/environments/robotics.py:150-164), h = 30: the reference's
parallel episodes (icem/misc/rollout_utils.py:46-58, 129-152), each controller its own ``get_action`` (icem/controllers/icem.py:
106-189), with the three launches of their two-kernel iterations -- sampler (shifted elites in its extra workgroup), sampler with
the previous merge in its prologue, one-wave-per-tile rollout -- and the last merge ONE launch each for all problems
(grid.y = the problem, argument blocks in a device array).  Held here: every problem's outputs are bit for bit those of its own
``icem_plan_step``; a batch's last pools against the float64 oracle under the criterion of
``test_gpu_hn_shapes.py::test_whole_mpc_steps_on_tilehn``; leaving and rejoining a batch; no upload in the steady state; what is
refused is refused before anything runs; the controllers' ``get_action_batch``.
"""
import dataclasses

import numpy as np
import pytest
import torch

import cost_term_cases as CC
from oracle import icem_oracle as O

pytestmark = pytest.mark.gpu


def np_(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _env(name):
    from icem_amd import envs as E
    return {"door": (E.door_env, O.CostSpec.door), "relocate": (E.relocate_env, O.CostSpec.relocate),
            "fpp": (E.fetch_pick_and_place_env, O.CostSpec.fetch_pick_and_place)}[name]


def _problem(name, i, kind):
    """Problem i of a batch: (env, the device model, the planner's cost spec, the oracle's): model seeds and the control weight are
    its own."""
    from icem_amd import DeviceSyntheticModel
    mk, spec_fn = _env(name)
    env = mk()
    model = DeviceSyntheticModel.make(env.obs_dim, env.action_space.shape[0], kind=kind, seed_a=10 + i, seed_b=20 + i)
    w = env.cost_spec.ctrl_weight * (1 + 0.1 * i)
    return env, model, dataclasses.replace(env.cost_spec, ctrl_weight=w), dataclasses.replace(spec_fn(), ctrl_weight=w)


def _make(name, i, N, iters, kind=1, mode="sum", elites=10, terms=True):
    """... and its planner: bound scale and seed are its own too."""
    from icem_amd import IcemConfig, IcemPlanner
    env, model, spec, _ = _problem(name, i, kind)
    bound = 1.0 if i % 2 == 0 else 0.5
    pl = IcemPlanner(IcemConfig(horizon=30, act_dim=env.action_space.shape[0], num_traj=N, opt_iters=iters, dtype="f32", seed=100 + 7 * i,
                                cost_mode=mode, elites_size=elites), bound * env.action_space.low, bound * env.action_space.high)
    pl.set_model(model.kind, model.A, model.B)
    pl.set_cost_spec(spec if terms else dataclasses.replace(spec, terms=()))
    pl.reset()
    return pl


def _obs(name, s, i):
    o = _env(name)[0]().obs_dim
    return 0.1 * (1 + i) * np.random.RandomState(1000 * s + i).randn(o)


def _state(pl):
    n_last = pl.population_sizes[-1]
    ea, ec = pl.current_elites()
    return [np_(pl.executed).copy(), np_(pl.best_cost).copy(), np_(pl.mean).copy(), np_(pl.std).copy(), np_(ea).copy(), np_(ec).copy(),
            np_(pl.costs[:n_last]).copy(), np_(pl.actions[:n_last]).copy()]


def _same(a, b, where):
    for k, (x, y) in enumerate(zip(_state(a), _state(b))):
        assert np.array_equal(x, y, equal_nan=True), where + (k,)


@pytest.mark.parametrize("name,B,N,iters,kind,mode", [
    ("door", 3, 200, 3, 1, "sum"),        # ragged last tile; 13 / 10 / 8 tiles per iteration; 203 rows with the shifted elites
    ("relocate", 2, 528, 2, 1, "best"),   # 33 tiles: more than one round per wave
    ("fpp", 5, 100, 3, 0, "final"),
    ("fpp", 16, 64, 2, 1, "sum"),         # many problems of four tiles
    ("door", 4, 4096, 2, 1, "sum"),       # the arrangement the benchmark's batch takes: > 1024 tiles, four waves per workgroup
])
def test_every_problem_of_a_batch_equals_its_solo_twin_bit_for_bit(name, B, N, iters, kind, mode):
    from icem_amd import IcemPlanner
    solo = [_make(name, i, N, iters, kind, mode) for i in range(B)]
    batch = [_make(name, i, N, iters, kind, mode) for i in range(B)]
    assert all(pl.tile_arith == 1 for pl in batch)   # the TileHN kernel serves them
    for s in range(4):   # (shifted and kept elites are in play from the second step)
        obs = [_obs(name, s, i) for i in range(B)]
        for i in range(B):
            solo[i].plan_step(obs[i])
        IcemPlanner.plan_step_batch(batch, obs)
        torch.cuda.synchronize()
        for i in range(B):
            _same(batch[i], solo[i], (s, i))
        assert np.all(np.isfinite(np_(batch[0].executed)))
        assert not np.array_equal(np_(batch[0].executed), np_(batch[1].executed))   # the problems ARE different problems


def test_a_batch_against_the_float64_oracle():
    """Door, B = 3, N = 200: every problem's last pool of every step re-scored by ``oracle.icem_oracle.rollout_costs`` from ITS
    model, spec and observation: within 1e-5 of the magnitude of the sum for more than 99 % of the rows, every excused row within
    ``cost_term_cases.NEAR`` of an indicator term's threshold (the criterion of test_whole_mpc_steps_on_tilehn).
    The 99 % cap with these seeds, checked without a GPU on the oracle pair (float32 against float64 arithmetic from the f32-rounded
    observation; each problem's model, spec, bounds and observations of the three steps, 128 rows drawn from its reset
    distribution): all 1152 rows within 1e-5 x magnitude, none near a threshold -- the cap's 1 % is all headroom."""
    from icem_amd import IcemPlanner
    B, N, iters = 3, 200, 3
    batch = [_make("door", i, N, iters) for i in range(B)]
    probs = [_problem("door", i, 1) for i in range(B)]
    for s in range(3):
        obs = [_obs("door", s, i) for i in range(B)]
        IcemPlanner.plan_step_batch(batch, obs)
        torch.cuda.synchronize()
        for i, pl in enumerate(batch):
            _, model, _, spec = probs[i]
            om = O.SyntheticModel(model.A, model.B, model.kind)
            n_last = pl.population_sizes[-1]
            pool, dev = np_(pl.actions[:n_last]), np_(pl.costs[:n_last])
            ob = obs[i].astype(np.float32).astype(np.float64)
            want = O.rollout_costs(om, spec, ob, pool).astype(np.float64)
            mag = O.rollout_cost_magnitudes(om, spec, ob, pool)
            ok = np.abs(dev - want) <= 1e-5 * mag
            print(f"step {s} problem {i}: {ok.mean():.4f} of {n_last} rows within 1e-5 x magnitude, max |diff| / mag {np.max(np.abs(dev - want) / mag):.3g}")
            assert ok.mean() > 0.99, (s, i, ok.mean())
            near = O.threshold_margins(om, spec, obs[i], pool) <= CC.NEAR   # the excused rows are near a threshold
            assert np.all(ok | near), (s, i, np.nonzero(~(ok | near))[0][:8])


def test_a_member_steps_alone_on_odd_steps_and_rejoins_on_even_ones():
    from icem_amd import IcemPlanner
    name, B, N, iters = "fpp", 3, 300, 3
    ref = [_make(name, i, N, iters) for i in range(B)]
    mix = [_make(name, i, N, iters) for i in range(B)]
    for s in range(6):
        obs = [_obs(name, s, i) for i in range(B)]
        for i in range(B):
            ref[i].plan_step(obs[i])
        if s % 2 == 0:
            IcemPlanner.plan_step_batch(mix, obs)
        else:
            for i in range(B):
                mix[i].plan_step(obs[i])
        torch.cuda.synchronize()
        for i in range(B):
            _same(mix[i], ref[i], (s, i))


def test_the_steady_state_uploads_nothing():
    """The argument blocks of step s are those of step s - 6 byte for byte (the elite buffers alternate per iteration; offsets
    are stored relative to the step's base, which travels in the kernel arguments): after twelve steps, twelve more upload nothing."""
    from icem_amd import IcemPlanner
    name, B = "relocate", 3
    batch = [_make(name, i, 200, 3) for i in range(B)]
    for s in range(12):
        IcemPlanner.plan_step_batch(batch, [_obs(name, s, i) for i in range(B)])
    before = batch[0].batch_uploads
    assert before > 0
    for s in range(12, 24):
        IcemPlanner.plan_step_batch(batch, [_obs(name, s, i) for i in range(B)])
    torch.cuda.synchronize()
    assert batch[0].batch_uploads == before, (before, batch[0].batch_uploads)


def test_what_a_tilehn_batch_cannot_do_is_refused_before_anything_runs():
    from icem_amd import IcemPlanner, _lib as L
    N, iters = 200, 2
    door = [_make("door", i, N, iters) for i in range(2)]
    relocate = _make("relocate", 1, N, iters)
    no_terms = _make("door", 1, N, iters, terms=False)       # another term program
    exact = _make("door", 1, N, iters)
    assert exact.set_tile_arith("f32") == 0                  # the exact-f32 GEMM kernel
    k12 = [_make("door", i, N, iters, elites=12) for i in range(2)]
    # one step of their own first, so that every planner holds elites, a distribution and a pool to compare
    everyone = door + [relocate, no_terms, exact] + k12
    for pl in everyone:
        pl.plan_step(0.1 * np.ones(pl.obs_dim))
    torch.cuda.synchronize()
    held = [(pl.mpc_step, _state(pl)) for pl in everyone]
    for group, code in (([door[0], relocate], L.ICEM_E_INVALID), ([door[0], no_terms], L.ICEM_E_INVALID),
                        ([door[0], exact], L.ICEM_E_UNSUPPORTED), (k12, L.ICEM_E_UNSUPPORTED)):
        with pytest.raises(L.IcemError) as e:
            IcemPlanner.plan_step_batch(group, None)
        assert e.value.code == code, (e.value.code, str(e.value))
    torch.cuda.synchronize()
    for pl, (step, st) in zip(everyone, held):
        assert pl.mpc_step == step
        for x, y in zip(_state(pl), st):
            assert np.array_equal(x, y)
    # ... and a proper batch afterwards equals solo
    ref = [_make("door", i, N, iters) for i in range(2)]
    for pl in ref:
        pl.plan_step(0.1 * np.ones(pl.obs_dim))
    obs = [_obs("door", 7, i) for i in range(2)]
    for i in range(2):
        ref[i].plan_step(obs[i])
    IcemPlanner.plan_step_batch(door, obs)
    torch.cuda.synchronize()
    for i in range(2):
        _same(door[i], ref[i], (i,))


def test_door_controllers_get_action_batch_equals_their_own_get_action():
    from icem_amd import DeviceSyntheticModel, MpcICemHip, envs as E

    def make(i):
        env = E.door_env()
        o, d = env.obs_dim, env.action_space.shape[0]
        c = MpcICemHip(env=env, forward_model=DeviceSyntheticModel.make(o, d, kind=1, seed_a=30 + i, seed_b=40 + i), horizon=30,
                       num_simulated_trajectories=256, factor_decrease_num=1.25, cost_along_trajectory="sum", seed=9 + i,
                       action_sampler_params=dict(alpha=0.1, elites_size=10, opt_iterations=3, init_std=0.5, use_mean_actions=True,
                                                  keep_previous_elites=True, shift_elites_over_time=True, fraction_elites_reused=0.3,
                                                  noise_beta=0.25))
        c.beginning_of_rollout(observation=np.zeros(o), state=None, mode="train")
        return c
    solo = [make(i) for i in range(4)]
    batch = [make(i) for i in range(4)]
    assert all(c.planner.tile_arith == 1 for c in batch)
    rs = np.random.RandomState(3)
    for s in range(4):
        obs = [0.1 * rs.randn(39) for _ in range(4)]
        want = [c.get_action(ob, None) for c, ob in zip(solo, obs)]
        got = MpcICemHip.get_action_batch(batch, obs)
        for w, g in zip(want, got):
            assert g.dtype == np.float64 and np.array_equal(w, g)
        for a, b in zip(solo, batch):
            assert np.array_equal(a.mean, b.mean) and a.last_min_cost == b.last_min_cost
    assert not np.array_equal(got[0], got[1])
