"""``icem_plan_step_batch_f64``: B planners of one configuration in the strict-parity arithmetic (dtype f64, the generic kernels)
advanced together -- the reference's parallel episodes (icem/misc/rollout_utils.py:46-58, 129-152), each controller its own
``get_action`` (icem/controllers/icem.py:106-189), in the reference's own float64.  Held here: every problem's outputs are bit for
bit those of its own ``icem_plan_step`` (executed action, best cost, mean, std, both elite halves and their costs, the last pool and
its costs) over several MPC steps, at the shapes where each batched kernel can go wrong; one problem of a batch against the NumPy
oracle on the same Philox stream; a step launches what a solo step launches whatever B, and a steady-state step uploads nothing;
what is refused is refused before anything runs."""
import itertools

import numpy as np
import pytest
import torch

from oracle import icem_oracle as O   # checker only

pytestmark = pytest.mark.gpu


def np_(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _make(i, N, iters, h=30, d=6, o=17, kind=0, mode="sum", beta=0.25, rounds=10, dtype="f64", **flags):
    from icem_amd import DeviceSyntheticModel, IcemConfig, IcemPlanner, halfcheetah_env
    env = halfcheetah_env(17)
    model = DeviceSyntheticModel.make(o, d, kind=kind, seed_a=10 + i, seed_b=20 + i)
    bound = 1.0 if i % 2 == 0 else 0.5
    pl = IcemPlanner(IcemConfig(horizon=h, act_dim=d, num_traj=N, opt_iters=iters, dtype=dtype, seed=100 + 7 * i, cost_mode=mode,
                                noise_beta=beta, rng_rounds=rounds, **flags), bound * env.action_space.low[:d], bound * env.action_space.high[:d])
    pl.set_model(model.kind, model.A, model.B)
    c = env.cost_spec
    pl.set_cost(c.ctrl_weight * (1 + 0.1 * i), min(c.lin_idx, o - 1), c.lin_weight, min(c.flip_idx, o - 1), c.flip_penalty, c.flip_thresh)
    pl.reset()
    return pl


def _state(pl):
    n_last = pl.population_sizes[-1]
    out = [np_(pl.executed).copy(), np_(pl.best_cost).copy(), np_(pl.mean).copy(), np_(pl.std).copy()]
    out += [np_(x).copy() for x in pl.current_elites()]
    out += [np_(x).copy() for g in (0, 1) for x in (pl.elites_actions[g], pl.elites_costs[g])]   # both elite halves
    return out + [np_(pl.costs[:n_last]).copy(), np_(pl.actions[:n_last]).copy()]


def _obs(B, o, s):
    return [0.1 * (1 + i) * np.random.RandomState(1000 * s + i).randn(o) for i in range(B)]


def _run_against_twins(make, B, o, steps):
    from icem_amd import IcemPlanner
    solo, batch = [make(i) for i in range(B)], [make(i) for i in range(B)]
    for s in range(steps):
        obs = _obs(B, o, s)
        for i in range(B):
            solo[i].plan_step(obs[i])
        IcemPlanner.plan_step_batch_f64(batch, obs)
        torch.cuda.synchronize()
        for i in range(B):
            for k, (x, y) in enumerate(zip(_state(batch[i]), _state(solo[i]))):
                assert np.array_equal(x, y, equal_nan=True), (s, i, k)
        assert not np.array_equal(np_(batch[0].executed), np_(batch[1].executed))   # the problems ARE different problems
    return solo, batch


@pytest.mark.parametrize("B,N,iters,h,d,o,kind,mode,rounds", [
    (3, 250, 3, 30, 6, 17, 0, "sum", 10),     # N no multiple of the sampler's 10 rows per workgroup or the rollout's 8
    (2, 253, 2, 30, 6, 18, 1, "best", 10),
    (4, 64, 4, 12, 4, 8, 0, "final", 10),     # decays onto the 2 * elites floor
    (2, 200, 2, 40, 6, 16, 0, "sum", 10),     # the HMAX = 64 sampler and the 16-lane rollout
    (2, 120, 2, 13, 3, 24, 1, "sum", 7),      # rng_rounds 7
    (2, 300, 2, 30, 6, 32, 0, "sum", 10),
    (2, 4500, 2, 30, 6, 17, 0, "sum", 10),    # a pool above 4096 keys: select_refit's second pass
    (32, 40, 2, 10, 2, 8, 0, "sum", 10),      # the batch limit
])
def test_every_problem_of_an_f64_batch_equals_its_solo_run_bit_for_bit(B, N, iters, h, d, o, kind, mode, rounds):
    _run_against_twins(lambda i: _make(i, N, iters, h, d, o, kind, mode, rounds=rounds), B, o, 4)   # steps >= 1 carry shifted elites


def test_white_noise_batch_equals_its_solo_runs():
    _run_against_twins(lambda i: _make(i, 250, 3, beta=0.0), 3, 17, 4)


@pytest.mark.parametrize("keep,shift,mean_actions", list(itertools.product((False, True), repeat=3)))
def test_every_flag_combination_batches_bit_for_bit(keep, shift, mean_actions):
    _run_against_twins(lambda i: _make(i, 250, 3, keep_previous_elites=keep, shift_elites=shift, use_mean_actions=mean_actions), 3, 17, 3)


def _make_terms(i, env, N=200, iters=3, with_terms=True):
    from icem_amd import DeviceSyntheticModel, IcemConfig, IcemPlanner
    import dataclasses
    o, d = env.obs_dim, env.action_space.shape[0]
    model = DeviceSyntheticModel.make(o, d, seed_a=30 + i, seed_b=40 + i)   # (linear: a batch shares the model kind)
    pl = IcemPlanner(IcemConfig(horizon=30, act_dim=d, num_traj=N, opt_iters=iters, dtype="f64", seed=50 + i), env.action_space.low, env.action_space.high)
    pl.set_model(model.kind, model.A, model.B)
    spec = env.cost_spec
    if not with_terms:   # the parametric part alone
        spec = type(spec)(0.1, 0, -1.0, -1, 0.0, 0.0)
    else:
        spec = dataclasses.replace(spec, ctrl_weight=spec.ctrl_weight + 0.01 * i)
    pl.set_cost_spec(spec)
    pl.reset()
    return pl


@pytest.mark.parametrize("envname", ["reacher", "hopper"])
def test_term_list_costs_batch_on_the_thread_form_rollout(envname):
    """Handles with ``icem_cost_terms`` keep the thread-per-trajectory rollout (Reacher: o = 11, a norm term; Hopper: the health
    range, the state box and the difference term)."""
    from icem_amd import hopper_env, reacher_env
    env = reacher_env() if envname == "reacher" else hopper_env()
    _run_against_twins(lambda i: _make_terms(i, env), 2, env.obs_dim, 3)


def test_a_planner_with_a_term_list_beside_one_without_is_refused():
    """include/icem_hip.h: either every handle carries icem_cost_terms or none -- the term list decides the rollout kernel."""
    from icem_amd import IcemPlanner, reacher_env, _lib as L
    env = reacher_env()
    a, b = _make_terms(0, env), _make_terms(1, env, with_terms=False)
    with pytest.raises(L.IcemError) as e:
        IcemPlanner.plan_step_batch_f64([a, b], [np.zeros(env.obs_dim)] * 2)
    assert e.value.code == L.ICEM_E_INVALID
    assert a.mpc_step == 0 and b.mpc_step == 0


def test_one_problem_of_a_batch_against_the_float64_oracle():
    """As tests/test_gpu_parity.py::test_strict_parity_path_at_unusual_shapes_against_the_oracle: the oracle restates the planner's
    Philox stream; executed action, mean and std to rtol 1e-9, atol 1e-11."""
    from icem_amd import IcemConfig, IcemPlanner
    B, N, iters, h, d, o, which = 3, 256, 3, 30, 6, 17, 1
    low, high = -0.7 * np.ones(d), 0.9 * np.ones(d)
    pls, models, specs = [], [], []
    for i in range(B):
        m = O.SyntheticModel.make(o, d, 0, seed_a=60 + i, seed_b=70 + i)   # a model of its own per problem
        spec = O.CostSpec(0.1 * (1 + i), o - 1, -1.0, 1, 10.0, 0.3)
        pl = IcemPlanner(IcemConfig(horizon=h, act_dim=d, num_traj=N, opt_iters=iters, dtype="f64", seed=17 + i), low, high)
        pl.set_model(0, m.A, m.B)
        pl.set_cost(spec.ctrl_weight, spec.lin_idx, spec.lin_weight, spec.flip_idx, spec.flip_penalty, spec.flip_thresh)
        pl.reset()
        pls.append(pl), models.append(m), specs.append(spec)
    sched = O.PhiloxNoiseSchedule(17 + which, iters, d, h, dtype=np.float64)
    orc = O.IcemOracle(O.IcemParams(horizon=h, num_simulated_trajectories=N, opt_iterations=iters), low, high,
                       lambda ob, ac: O.rollout_costs(models[which], specs[which], ob, ac, mode="sum"),
                       lambda num: tuple(z.astype(np.float64) for z in sched(num)))
    orc.beginning_of_rollout()
    rs = np.random.RandomState(4)
    for step in range(3):
        obs = [0.2 * rs.randn(o) for _ in range(B)]
        if step:
            sched.begin_step()
        IcemPlanner.plan_step_batch_f64(pls, obs)
        want = orc.get_action(obs[which])
        np.testing.assert_allclose(np_(pls[which].executed), want, rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(np_(pls[which].mean), orc.mean, rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(np_(pls[which].std), orc.std, rtol=1e-9, atol=1e-11)


def test_a_batch_member_can_step_alone_and_rejoin():
    from icem_amd import IcemPlanner
    B, N, iters, o = 3, 250, 3, 17
    ref, mix = [_make(i, N, iters) for i in range(B)], [_make(i, N, iters) for i in range(B)]
    rs = np.random.RandomState(5)
    for s in range(6):
        obs = [0.2 * rs.randn(o) for _ in range(B)]
        for i in range(B):
            ref[i].plan_step(obs[i])
        if s % 2 == 0:
            IcemPlanner.plan_step_batch_f64(mix, obs)
        else:
            for i in range(B):
                mix[i].plan_step(obs[i])
        torch.cuda.synchronize()
        for i in range(B):
            for k, (x, y) in enumerate(zip(_state(mix[i]), _state(ref[i]))):
                assert np.array_equal(x, y, equal_nan=True), (s, i, k)


def test_a_step_launches_what_a_solo_step_launches_and_a_steady_state_step_uploads_nothing():
    from icem_amd import IcemPlanner
    iters, o = 3, 17
    for B in (2, 8):
        batch = [_make(i, 128, iters) for i in range(B)]
        ups = []
        for s in range(14):
            IcemPlanner.plan_step_batch_f64(batch, _obs(B, o, s))
            # sampler + rollout + selection per iteration; the shifted elites' copy and their last action's sampler in front
            assert batch[0].batch_f64_launches == 3 * iters + (2 if s > 0 else 0), (B, s, batch[0].batch_f64_launches)
            ups.append(batch[0].batch_uploads)
        torch.cuda.synchronize()
        # six slots by the step modulo 6; slot 0 is written at step 0 and once more at step 6, the first time it carries shifted elites
        assert ups[0] == 1 and ups[5] == 6 and ups[6] == 7, ups
        assert ups[7:] == [ups[6]] * 7, ups


def test_what_an_f64_batch_cannot_do_is_refused_before_anything_runs():
    from icem_amd import IcemPlanner, _lib as L
    o = 17
    a, b = _make(0, 250, 3), _make(1, 250, 3)
    zeros = [np.zeros(o)] * 2

    def refused(pls, code):
        with pytest.raises(L.IcemError) as e:
            IcemPlanner.plan_step_batch_f64(pls, zeros)
        assert e.value.code == code, e.value
        for pl in pls:
            assert pl.mpc_step == 0
    refused([_make(0, 250, 3, dtype="f32"), _make(1, 250, 3, dtype="f32")], L.ICEM_E_UNSUPPORTED)
    refused([a, _make(1, 250, 3, dtype="f32")], L.ICEM_E_INVALID)
    refused([a, _make(2, 200, 3)], L.ICEM_E_INVALID)              # another population
    refused([a, a], L.ICEM_E_INVALID)
    refused([_make(0, 16384, 2), _make(1, 16384, 2)], L.ICEM_E_UNSUPPORTED)
    try:
        for name, val in (("gk_select", 0), ("gk_rollout_thread", 1), ("gk_sample", 0)):
            L.reset_options()
            L.set_option(name, val)
            refused([a, b], L.ICEM_E_UNSUPPORTED)
    finally:
        L.reset_options()
    a.profile_enable(True)
    try:
        refused([a, b], L.ICEM_E_UNSUPPORTED)
    finally:
        a.profile_enable(False)
    with pytest.raises(L.IcemError):     # the f32 entry is as it was: f64 handles are not its
        IcemPlanner.plan_step_batch([a, b], zeros)
    assert a.mpc_step == 0 and b.mpc_step == 0
    # ... and the planners are still good for a proper batch
    ref = [_make(0, 250, 3), _make(1, 250, 3)]
    obs = [0.1 * np.ones(o), -0.1 * np.ones(o)]
    for i in range(2):
        ref[i].plan_step(obs[i])
    IcemPlanner.plan_step_batch_f64([a, b], obs)
    torch.cuda.synchronize()
    for x, y in zip(_state(a) + _state(b), _state(ref[0]) + _state(ref[1])):
        assert np.array_equal(x, y)


def test_f64_controllers_get_action_batch_equals_their_own_get_action():
    from icem_amd import DeviceSyntheticModel, MpcICemHip, halfcheetah_env

    def make(i):
        env = halfcheetah_env(17)
        c = MpcICemHip(env=env, forward_model=DeviceSyntheticModel.make(17, 6, seed_a=30 + i, seed_b=40 + i), horizon=30,
                       num_simulated_trajectories=128, factor_decrease_num=1.25, cost_along_trajectory="sum", seed=9 + i, dtype="f64",
                       action_sampler_params=dict(alpha=0.1, elites_size=10, opt_iterations=2, init_std=0.5, use_mean_actions=True,
                                                  keep_previous_elites=True, shift_elites_over_time=True, fraction_elites_reused=0.3,
                                                  noise_beta=0.25))
        c.beginning_of_rollout(observation=np.zeros(17), state=None, mode="train")
        return c
    solo, batch = [make(i) for i in range(3)], [make(i) for i in range(3)]
    assert all(c.planner.cfg.dtype == "f64" for c in batch)
    rs = np.random.RandomState(3)
    for s in range(3):
        obs = [0.1 * rs.randn(17) for _ in range(3)]
        want = [c.get_action(ob, None) for c, ob in zip(solo, obs)]
        got = MpcICemHip.get_action_batch(batch, obs)
        for w, g in zip(want, got):
            assert g.dtype == np.float64 and np.array_equal(w, g)
        for a, b in zip(solo, batch):
            assert np.array_equal(a.mean, b.mean) and a.last_min_cost == b.last_min_cost
            for x, y in zip(_state(a.planner), _state(b.planner)):
                assert np.array_equal(x, y)
