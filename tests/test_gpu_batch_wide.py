"""``icem_plan_step_batch`` on the GEMM-kernel shapes -- HumanoidStandup at its real width (o = 378, d = 17;
icem/environments/mujoco.py:241-277), Humanoid (o = 376), Ant (o = 113, d = 8, with its difference and health terms;
mujoco.py:146-171), and the narrow shapes no tile kernel serves (Hopper o = 12, Reacher o = 11), h = 30: the reference's parallel
episodes (icem/misc/rollout_utils.py:46-58, 129-152), each controller its own ``get_action`` (icem/controllers/icem.py:106-189),
with the launches of their two-kernel iterations -- sampler, sampler with the previous merge in its prologue, the GEMM rollout
(16-bit planes, or exact f32 tiles and the row-by-row tail behind them) -- and the last merge ONE launch each for all problems
(grid.y = the problem, argument blocks in a device array).  Held here: every problem's outputs are bit for bit those of its own
``icem_plan_step``; a batch's last pools against the float64 oracle; leaving and rejoining a batch; no upload in the steady state;
what is refused is refused before anything runs; the controllers' ``get_action_batch``.  Modelled on tests/test_gpu_batch_hn.py:
the same per-problem seeds, control weights and bound scales.
"""
import dataclasses

import numpy as np
import pytest
import torch

import cost_term_cases as CC
from oracle import icem_oracle as O

pytestmark = pytest.mark.gpu

FLIP = dict(ctrl_weight=0.1, lin_idx=8, lin_weight=-1.0, flip_idx=1, flip_penalty=10.0, flip_thresh=0.1)   # (a flip term that trips)


def np_(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _env(name):
    """(the env of the planner's side, the oracle's cost spec)"""
    from icem_amd import envs as E
    if name == "standup":
        return E.humanoid_standup_env(378), O.CostSpec.humanoid_standup()
    if name == "humanoid":
        return E.humanoid_env(376), O.CostSpec.humanoid()
    if name == "standup_terms":   # HumanoidStandup's width and actions with Humanoid's health term: a term list at o = 378
        return (E.SyntheticEnv("HumanoidStandupTerms", 378, -0.4 * np.ones(17), 0.4 * np.ones(17), E.humanoid_env(378).cost_spec),
                O.CostSpec.humanoid())
    if name == "ant":
        return E.ant_env(), O.CostSpec.ant()
    if name == "hopper":
        return E.hopper_env(), O.CostSpec.hopper()
    if name == "reacher":
        return E.reacher_env(11), O.CostSpec.reacher(11)
    if name == "syn200":          # a middle width: o = 200, d = 3, the parametric cost with a flip term
        return E.SyntheticEnv("Synthetic200", 200, -np.ones(3), np.ones(3), E.CostSpec(**FLIP)), O.CostSpec(**FLIP)
    if name == "door":
        return E.door_env(), O.CostSpec.door()
    raise KeyError(name)


def _problem(name, i, kind):
    """Problem i of a batch: (env, the device model, the planner's cost spec, the oracle's): model seeds and the control weight are
    its own."""
    from icem_amd import DeviceSyntheticModel
    env, ospec = _env(name)
    model = DeviceSyntheticModel.make(env.obs_dim, env.action_space.shape[0], kind=kind, seed_a=10 + i, seed_b=20 + i)
    w = env.cost_spec.ctrl_weight * (1 + 0.1 * i)
    return env, model, dataclasses.replace(env.cost_spec, ctrl_weight=w), dataclasses.replace(ospec, ctrl_weight=w)


def _make(name, i, N, iters, kind=1, mode="sum", elites=10, arith=None, horizon=30):
    """... and its planner: bound scale and seed are its own too.  arith: None (the default arithmetic of the shape), "exact"
    (``set_wide_exact(1)``: the exact-f32 kernel) or "bf16" (``set_wide_exact(2)``: the bf16 planes)."""
    from icem_amd import IcemConfig, IcemPlanner
    env, model, spec, _ = _problem(name, i, kind)
    bound = 1.0 if i % 2 == 0 else 0.5
    pl = IcemPlanner(IcemConfig(horizon=horizon, act_dim=env.action_space.shape[0], num_traj=N, opt_iters=iters, dtype="f32", seed=100 + 7 * i,
                                cost_mode=mode, elites_size=elites), bound * env.action_space.low, bound * env.action_space.high)
    pl.set_model(model.kind, model.A, model.B)
    pl.set_cost_spec(spec)
    if arith is not None:
        pl.set_wide_exact({"exact": 1, "bf16": 2}[arith])
    pl.reset()
    return pl


def _obs(name, s, i):
    o = _env(name)[0].obs_dim
    return 0.1 * (1 + i) * np.random.RandomState(1000 * s + i).randn(o)


def _state(pl):
    n_last = pl.population_sizes[-1]
    ea, ec = pl.current_elites()
    return [np_(pl.executed).copy(), np_(pl.best_cost).copy(), np_(pl.mean).copy(), np_(pl.std).copy(), np_(ea).copy(), np_(ec).copy(),
            np_(pl.costs[:n_last]).copy(), np_(pl.actions[:n_last]).copy()]


def _same(a, b, where):
    for k, (x, y) in enumerate(zip(_state(a), _state(b))):
        assert np.array_equal(x, y, equal_nan=True), where + (k,)


@pytest.mark.parametrize("name,arith,B,N,iters,kind,mode,expect", [
    ("standup", None, 3, 64, 2, 1, "sum", "f16x2"),      # four tiles in one workgroup; from step 1 the shifted elites open the fifth (FIVE)
    ("standup", None, 2, 300, 3, 0, "best", "f16x2"),    # 19 tiles over 4 workgroups with remainders, a ragged last tile, decayed populations
    ("standup", "bf16", 2, 100, 2, 1, "final", "bf16x3"),  # the bf16 planes, parametric cost
    ("standup", "exact", 3, 64, 2, 1, "sum", "f32"),     # the row-wise tail kernel from step 1 (64 sampled rows = whole tiles)
    ("standup", "exact", 2, 200, 2, 0, "sum", "f32"),    # ragged: all rows in tiles (NT = 24)
    ("ant", None, 4, 200, 3, 1, "sum", "f16x2"),         # the term list (finite / health sweep, difference term) on the plane kernel, NCT = 1
    ("ant", "exact", 4, 200, 2, 1, "sum", "f32"),        # ... and on the exact kernel, NT = 8
    ("syn200", None, 2, 129, 2, 1, "sum", "f16x2"),      # a middle width: NCT = 2
    ("syn200", "exact", 2, 129, 2, 0, "best", "f32"),    # ... NT = 16
    ("hopper", None, 16, 64, 2, 1, "sum", "f32"),        # the narrow GEMM shapes: NT = 4, the next step's actions held in registers
    ("reacher", None, 5, 100, 3, 0, "sum", "f32"),
    ("standup", None, 32, 64, 2, 1, "sum", "f16x2"),     # the widest batch
    ("standup", None, 8, 4096, 2, 1, "sum", "f16x2"),    # 8 x 64 workgroups: more than the chip has CUs
])
def test_every_problem_of_a_batch_equals_its_solo_twin_bit_for_bit(name, arith, B, N, iters, kind, mode, expect):
    from icem_amd import IcemPlanner
    solo = [_make(name, i, N, iters, kind, mode, arith=arith) for i in range(B)]
    batch = [_make(name, i, N, iters, kind, mode, arith=arith) for i in range(B)]
    assert all(pl.wide_arith == expect for pl in batch)   # the GEMM kernel this case is about serves them
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


@pytest.mark.parametrize("name", ["standup", "ant"])
def test_a_batch_against_the_float64_oracle(name):
    """HumanoidStandup o = 378 and Ant (tanh models), B = 3, N = 200, three steps: every problem's last pool of every step re-scored by
    ``oracle.icem_oracle.rollout_costs`` from ITS model, spec and f32-rounded observation: within 1e-5 of the magnitude of the sum
    for more than 99 % of the rows, every excused row within ``cost_term_cases.NEAR`` of a threshold (the criterion of
    test_gpu_batch_hn.py::test_a_batch_against_the_float64_oracle).  HumanoidStandup's cost has no threshold: there every row must
    pass.  The cap with these seeds, checked without a GPU on the oracle pair (float32 against float64 arithmetic, 128 rows per step
    from each problem's reset distribution): all rows within 1e-5 x magnitude, worst 4.6e-6 (HumanoidStandup) / 2.7e-7 (Ant), none
    near a threshold.  The device's plane arithmetic is not f32; the solo path at this shape passes the same bound in
    test_gpu_parity_sizes.py (c3wide_*).
    Observed on an MI355X (EXPERIMENTS.md R9.1): every row of every problem and step within the bound (share 1.0000 of 128 rows,
    18 pools); worst |diff| / magnitude 1.41e-6 on HumanoidStandup (problem 1, step 0), 2.64e-7 on Ant; no row needed the excuse."""
    from icem_amd import IcemPlanner
    B, N, iters = 3, 200, 3
    batch = [_make(name, i, N, iters) for i in range(B)]
    probs = [_problem(name, i, 1) for i in range(B)]
    for s in range(3):
        obs = [_obs(name, s, i) for i in range(B)]
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
            print(f"{name} step {s} problem {i}: {ok.mean():.4f} of {n_last} rows within 1e-5 x magnitude, max |diff| / mag {np.max(np.abs(dev - want) / mag):.3g}")
            assert ok.mean() > 0.99, (s, i, ok.mean())
            near = O.threshold_margins(om, spec, obs[i], pool) <= CC.NEAR   # the excused rows are near a threshold (HumanoidStandup: none is)
            assert np.all(ok | near), (s, i, np.nonzero(~(ok | near))[0][:8])


def test_a_member_steps_alone_on_odd_steps_and_rejoins_on_even_ones():
    from icem_amd import IcemPlanner
    name, B, N, iters = "hopper", 3, 300, 3
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
    """The argument blocks of step s are those of step s - 6 byte for byte (the elite buffers alternate per iteration; the sampling
    offsets are stored relative to the step's base, the rollout blocks carry no offset and no padding byte that is not zero): after
    twelve steps, twelve more upload nothing."""
    from icem_amd import IcemPlanner
    name, B = "standup", 3
    batch = [_make(name, i, 200, 3) for i in range(B)]
    for s in range(12):
        IcemPlanner.plan_step_batch(batch, [_obs(name, s, i) for i in range(B)])
    before = batch[0].batch_uploads
    assert before > 0
    for s in range(12, 24):
        IcemPlanner.plan_step_batch(batch, [_obs(name, s, i) for i in range(B)])
    torch.cuda.synchronize()
    assert batch[0].batch_uploads == before, (before, batch[0].batch_uploads)


def test_what_a_gemm_batch_cannot_do_is_refused_before_anything_runs():
    from icem_amd import IcemPlanner, _lib as L
    N, iters = 200, 2
    standup = [_make("standup", i, N, iters) for i in range(2)]
    humanoid = _make("humanoid", 1, N, iters)                      # o = 376, the same d
    terms = _make("standup_terms", 1, N, iters)                    # a term list beside none at the same width
    exact = _make("standup", 1, N, iters, arith="exact")           # exact beside default
    k12 = [_make("standup", i, N, iters, elites=12) for i in range(2)]
    big = [_make("standup", i, 16384, iters) for i in range(2)]
    h12 = [_make("standup", i, N, iters, horizon=12) for i in range(2)]
    door = _make("door", 0, N, iters)                              # the TileHN kernel ...
    door_exact = _make("door", 1, N, iters)
    assert door.tile_arith == 1 and door_exact.set_tile_arith("f32") == 0   # ... beside the exact-f32 GEMM kernel at the same shape
    # (no instantiation of the rollout kernels was left without a batched twin for its registers: nothing to refuse on that account;
    #  the one candidate, the bf16 planes with a term list at o > 256, is the last group below and must be SERVED)
    bf16_terms = [_make("standup_terms", i, N, iters, arith="bf16") for i in range(2)]
    assert all(pl.wide_arith == "bf16x3" for pl in bf16_terms)
    # one step of their own first, so that every planner holds elites, a distribution and a pool to compare
    everyone = standup + [humanoid, terms, exact] + k12 + big + h12 + [door, door_exact] + bf16_terms
    for pl in everyone:
        pl.plan_step(0.1 * np.ones(pl.obs_dim))
    torch.cuda.synchronize()
    held = [(pl.mpc_step, _state(pl)) for pl in everyone]
    for group, code in (([standup[0], humanoid], L.ICEM_E_INVALID), ([standup[0], terms], L.ICEM_E_INVALID), ([standup[0], exact], L.ICEM_E_INVALID),
                        (k12, L.ICEM_E_UNSUPPORTED), (big, L.ICEM_E_UNSUPPORTED), (h12, L.ICEM_E_UNSUPPORTED),
                        ([door, door_exact], L.ICEM_E_UNSUPPORTED)):
        with pytest.raises(L.IcemError) as e:
            IcemPlanner.plan_step_batch(group, None)
        assert e.value.code == code, (e.value.code, str(e.value))
    torch.cuda.synchronize()
    for pl, (step, st) in zip(everyone, held):
        assert pl.mpc_step == step
        for x, y in zip(_state(pl), st):
            assert np.array_equal(x, y)
    # ... and a proper batch afterwards equals solo
    ref = [_make("standup", i, N, iters) for i in range(2)]
    for pl in ref:
        pl.plan_step(0.1 * np.ones(pl.obs_dim))
    obs = [_obs("standup", 7, i) for i in range(2)]
    for i in range(2):
        ref[i].plan_step(obs[i])
    IcemPlanner.plan_step_batch(standup, obs)
    torch.cuda.synchronize()
    for i in range(2):
        _same(standup[i], ref[i], (i,))
    ref = [_make("standup_terms", i, N, iters, arith="bf16") for i in range(2)]
    for pl in ref:
        pl.plan_step(0.1 * np.ones(pl.obs_dim))
    for i in range(2):
        ref[i].plan_step(obs[i])
    IcemPlanner.plan_step_batch(bf16_terms, obs)
    torch.cuda.synchronize()
    for i in range(2):
        _same(bf16_terms[i], ref[i], ("bf16 planes with a term list", i))


def test_humanoid_standup_controllers_get_action_batch_equals_their_own_get_action():
    from icem_amd import DeviceSyntheticModel, MpcICemHip, envs as E

    def make(i):
        env = E.humanoid_standup_env(378)
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
    assert all(c.planner.wide_arith == "f16x2" for c in batch)
    rs = np.random.RandomState(3)
    for s in range(4):
        obs = [0.1 * rs.randn(378) for _ in range(4)]
        want = [c.get_action(ob, None) for c, ob in zip(solo, obs)]
        got = MpcICemHip.get_action_batch(batch, obs)
        for w, g in zip(want, got):
            assert g.dtype == np.float64 and np.array_equal(w, g)
        for a, b in zip(solo, batch):
            assert np.array_equal(a.mean, b.mean) and a.last_min_cost == b.last_min_cost
    assert not np.array_equal(got[0], got[1])
