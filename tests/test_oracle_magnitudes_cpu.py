"""oracle.rollout_cost_magnitudes -- the scale every f32 cost is held to 1e-5 of -- counts every addend of the cost,
the term list's diff and health terms included.  CPU only."""
import dataclasses

import numpy as np

from oracle import icem_oracle as O


def test_magnitude_bounds_every_sum_and_counts_diff_and_health_terms():
    spec = O.CostSpec.hopper(healthy_z_range=(-0.05, float("inf")), healthy_state_range=(-0.45, 0.45))
    assert spec.diff_idx >= 0 and spec.health_idx >= 0
    o, d, h, n = 11, 3, 12, 400
    m = O.SyntheticModel.make(o, d, O.MODEL_TANH)
    rs = np.random.RandomState(0)
    obs0 = 0.2 * rs.randn(o)
    act = rs.uniform(-1, 1, (n, h, d))
    cost = O.rollout_costs(m, spec, obs0, act)
    mag = O.rollout_cost_magnitudes(m, spec, obs0, act)
    assert np.all(mag >= np.abs(cost) * (1 - 1e-12))
    # each group on its own: the magnitude of a cost made of one term is that term's sum of absolute values
    only_diff = dataclasses.replace(spec, ctrl_weight=0.0, health_idx=-1, box_from=-1, lin_weight=0.0, flip_idx=-1)
    obs = O.rollout_observations(m, obs0, act)
    nxt = np.concatenate([obs[:, 1:], m.predict(obs[:, -1], act[:, -1])[:, None]], axis=1)
    want = abs(spec.diff_weight) * (np.abs(obs[..., spec.diff_idx]) + np.abs(nxt[..., spec.diff_idx])).sum(axis=1)
    np.testing.assert_allclose(O.rollout_cost_magnitudes(m, only_diff, obs0, act), want, rtol=1e-12)
    only_health = dataclasses.replace(spec, ctrl_weight=0.0, diff_idx=-1, lin_weight=0.0, flip_idx=-1)
    unhealthy_steps = O.rollout_costs(m, dataclasses.replace(only_health, health_penalty=1.0), obs0, act)
    assert 0 < unhealthy_steps.mean() < h   # (healthy and unhealthy steps both occur)
    np.testing.assert_allclose(O.rollout_cost_magnitudes(m, only_health, obs0, act),
                               abs(spec.health_penalty) * unhealthy_steps, rtol=1e-12)
