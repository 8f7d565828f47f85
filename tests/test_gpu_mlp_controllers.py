"""MpcICemHip, MpcCemStdHip and MpcRandomHip plan through a DeviceMLPModel on a HalfCheetah-shaped environment (N = 128,
h = 12, 3 iterations, 3 MPC steps): the controllers take the duck-typed learned-dynamics path (``rollout_cost`` + ``params``)
stage by stage -- one ``rollout_cost`` per iteration, no fused ``*_learned`` entry --, two equal controllers execute the same
actions bit for bit, ``last_min_cost`` is the minimum of a direct ``rollout_cost`` over the recorded pools, and a
``compute_new_mean`` override is handed a finite observation of the model's width."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, H, ITERS, STEPS = 128, 12, 3, 3
KINDS = ["icem", "cem", "random"]


def np_(t):
    return t.detach().cpu().numpy()


def model(seed=3, layers=2, activation="swish"):
    from icem_amd import DeviceMLPModel, halfcheetah_env
    return DeviceMLPModel(17, 6, layers=layers, activation=activation, seed=seed, env=halfcheetah_env(17), device=DEV)


def controller(kind, m, seed=5, cls=None):
    from icem_amd import MpcCemStdHip, MpcICemHip, MpcRandomHip, halfcheetah_env
    env = halfcheetah_env(17)
    if kind == "icem":
        asp = dict(alpha=0.1, elites_size=10, opt_iterations=ITERS, init_std=0.5, use_mean_actions=True, keep_previous_elites=True,
                   shift_elites_over_time=True, fraction_elites_reused=0.3, noise_beta=0.25)
        return (cls or MpcICemHip)(env=env, forward_model=m, horizon=H, num_simulated_trajectories=N, factor_decrease_num=1.25,
                                   cost_along_trajectory="sum", dtype="f32", seed=seed, action_sampler_params=asp)
    if kind == "cem":
        asp = dict(alpha=0.1, elites_size=10, opt_iterations=ITERS, init_std=0.5, shift_means=True, execute_best_elite=True,
                   bounds_like_levine=False)
        return (cls or MpcCemStdHip)(env=env, forward_model=m, horizon=H, num_simulated_trajectories=N, cost_along_trajectory="sum",
                                     verbose=False, seed=seed, action_sampler_params=asp)
    return (cls or MpcRandomHip)(env=env, forward_model=m, horizon=H, num_simulated_trajectories=N, cost_along_trajectory="sum",
                                 verbose=False, seed=seed, action_sampler_params=dict(action_change_frequency=2))


def record(m):
    """Replace the instance's rollout_cost by one that keeps (obs, actions, costs) of every call."""
    calls, inner = [], m.rollout_cost

    def recording(obs, actions, cost_mode=0, **kw):
        out = inner(obs, actions, cost_mode, **kw)
        calls.append((np.asarray(obs, np.float32).copy(), actions.clone(), out.clone(), cost_mode))
        return out
    m.rollout_cost = recording
    return calls, inner


def observations():
    rs = np.random.RandomState(7)
    ob = 0.3 * rs.randn(17)
    return [ob + 0.02 * k * rs.randn(17) for k in range(STEPS)]


@pytest.mark.parametrize("kind", KINDS)
def test_the_controllers_plan_stage_by_stage_through_the_model(kind):
    m, twin_m = model(), model()
    calls, inner = record(m)
    a, b = controller(kind, m), controller(kind, twin_m)
    for c in (a, b):
        assert c.rssm_path and not c.device_path and not c.torch_path
        assert not c._model_is_the_library_rssm() and not c._model_is_the_library_ensemble()   # no fused *_learned entry
    obs = observations()
    for c in (a, b):
        c.beginning_of_rollout(observation=obs[0], state=None, mode="train")
    per_step = ITERS if kind != "random" else 1
    for k, ob in enumerate(obs):
        before = len(calls)
        act = a.get_action(ob, None)
        assert act.shape == (6,) and np.isfinite(act).all()
        assert np.array_equal(act, b.get_action(ob, None)), (kind, k)      # two equal controllers: the same bits
        assert a.last_min_cost == b.last_min_cost, (kind, k)
        mine = calls[before:]
        assert len(mine) == per_step, (kind, k, len(mine))                  # one launch per iteration: stage by stage
        for o, acts, _, mode in mine:
            assert np.array_equal(o, ob.astype(np.float32)) and acts.shape[1:] == (H, 6) and mode == 0
        # a direct rollout_cost over the recorded pools: the recorded costs again, and last_min_cost is their minimum -- of the
        # last pool (CEM, random shooting), or of the last pool and the elites kept from the pools before it (iCEM: the best
        # row of every earlier pool of the step is among the kept elites)
        direct = [inner(o, acts, mode) for o, acts, _, mode in mine]
        for d, (_, _, out, _) in zip(direct, mine):
            assert torch.equal(d, out)
        pools = direct if kind == "icem" else direct[-1:]
        assert a.last_min_cost == float(min(np_(d).min() for d in pools)), (kind, k)
        assert mine[-1][1].shape[0] <= N


@pytest.mark.parametrize("kind", ["icem", "cem"])
def test_a_compute_new_mean_override_gets_an_observation_of_the_models_width(kind):
    from icem_amd import MpcCemStdHip, MpcICemHip
    seen = []

    def override(self, obs):
        seen.append(np.asarray(obs, dtype=np.float64).copy())
        return self.mean[-1] * 0 + 0.25

    base = MpcICemHip if kind == "icem" else MpcCemStdHip
    cls = type("Overriding" + base.__name__, (base,), dict(compute_new_mean=override))
    m = model(seed=4, activation="relu")
    c = controller(kind, m, cls=cls)
    obs = observations()
    c.beginning_of_rollout(observation=obs[0], state=None, mode="train")
    for k, ob in enumerate(obs):
        c.get_action(ob, None)
        assert len(seen) == k + 1 and seen[-1].shape == (17,) and np.isfinite(seen[-1]).all(), (kind, k, seen[-1:])
    # the observation in front of the best trajectory's last action: index h - 1 of the model's own states s_0 .. s_h
    assert np.allclose(np.asarray(c.mean)[-1], 0.25)


def test_a_batch_of_controllers_is_refused_with_the_existing_message():
    from icem_amd import MpcICemHip
    m = model()
    ctrls = [controller("icem", m, seed=s) for s in (1, 2)]
    obs = observations()[:2]
    for c, ob in zip(ctrls, obs):
        c.beginning_of_rollout(observation=ob, state=None, mode="train")
    with pytest.raises(NotImplementedError, match="get_action_batch: the learned-dynamics model has no rollout_cost_batch"):
        MpcICemHip.get_action_batch(ctrls, obs)
    assert [c.planner.mpc_step for c in ctrls] == [0, 0]
