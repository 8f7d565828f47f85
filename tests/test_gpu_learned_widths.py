"""The three one-call MPC steps through the learned dynamics at action widths other than six: icem_plan_step_learned*,
icem_plan_step_cem_learned*, icem_plan_step_random_learned* on handles bound to their model's width (icem_set_rssm_act_dim).

Every step is DEFINED by its operator loop, which at these widths runs through ``DeviceRSSMModel(act_dim=d).rollout_cost``
(held to the float64 emulation in test_gpu_rssm_widths.py), and the entries only rearrange its launches: every comparison here is
``np.array_equal``.  The loops, planners and comparisons are those of test_gpu_learned_step.py, test_gpu_cem_learned.py and
test_gpu_random_learned.py, called with ``d`` and with the shared model of those modules exchanged for one of that width.
Widths 1, 2 (the reference's own small environments), 5 (a partial group of four) and 32 (the whole action K block).
Refusals -- a binding of the wrong width, widths the layout does not hold, an f64 handle, a batch of mixed bindings, a handle
never bound -- leave every buffer as it was."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_cem_learned as TC
import test_gpu_learned_step as TL
import test_gpu_random_learned as TR

pytestmark = pytest.mark.gpu

WIDTHS = [1, 2, 5, 32]
_models = {}


def np_(t):
    return t.detach().cpu().numpy()


def model(d):
    from icem_amd import DeviceRSSMModel
    if d not in _models:
        _models[d] = DeviceRSSMModel(seed=3, act_dim=d)
    return _models[d]


@contextlib.contextmanager
def shared_model(d):
    """The helper modules' one shared model (their ``model()``) is the width-d one inside."""
    saved = [(mod, mod._cache.get("m")) for mod in (TC, TL, TR)]
    for mod, _ in saved:
        mod._cache["m"] = model(d)
    try:
        yield model(d)
    finally:
        for mod, old in saved:
            if old is None:
                mod._cache.pop("m", None)
            else:
                mod._cache["m"] = old


def bound(pl, d):
    assert pl._bind_rssm(model(d)) and pl.lib.icem_rssm_act_dim(pl._h) == d == pl.d
    return pl


# ---- 1. icem_plan_step_learned ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(64, 2), (250, 10)])
@pytest.mark.parametrize("d", WIDTHS)
def test_the_icem_step_equals_the_operator_loop(d, N, K):
    """test_gpu_learned_step.py::test_raw_entry_against_the_operators at width d: mean, std, executed, best cost and both elite
    halves over three steps (K = 10: three kept and, from the second step on, three shifted elites; K = 2: none)."""
    m = model(d)
    p, q = TL.planner(11, n=N, act_dim=d, elites_size=K), TL.planner(11, n=N, act_dim=d, elites_size=K)
    assert not p.learned_step_ok() and p.learned_step_ok(m)   # (served once it is bound to the model's width)
    assert (p.n_reuse > 0) == (K == 10)
    ob0 = TL.observations(1, seed=4)[0]
    elites = None
    for k in range(3):
        ob = ob0 + 0.02 * k
        p.plan_step_learned(m, ob)
        want, elites, before = TL.operator_step(q, m, ob, elites)
        assert p.learned_step_launches > 0 and p.mpc_step == q.mpc_step == k + 1
        assert np.array_equal(np_(torch.cat([p.executed, p.best_cost])), want), k
        assert np.array_equal(np_(p.mean), np_(q.mean)) and np.array_equal(np_(p.std), np_(q.std)), k
        g = (p.mpc_step * p.cfg.opt_iters) & 1
        assert np.array_equal(np_(p.elites_actions[g]), np_(elites[0])) and np.array_equal(np_(p.elites_costs[g]), np_(elites[1])), k
        assert np.array_equal(np_(p.elites_actions[g ^ 1]), np_(before[0])) and np.array_equal(np_(p.elites_costs[g ^ 1]), np_(before[1])), k


@pytest.mark.parametrize("B,N", [(3, 64), (32, 16)])
@pytest.mark.parametrize("d", WIDTHS)
def test_the_icem_batch_equals_its_solo_twins(d, B, N):
    from icem_amd import IcemPlanner
    m = model(d)
    batch = [TL.planner(31 + i, n=N, act_dim=d) for i in range(B)]
    twins = [TL.planner(31 + i, n=N, act_dim=d) for i in range(B)]
    obs0 = np.stack(TL.observations(B, seed=7))
    steps = 8 if B == 3 else 2
    uploads = []
    for k in range(steps):
        obs = obs0 + 0.01 * k
        res = IcemPlanner.plan_step_learned_batch(batch, m, obs)
        assert tuple(res.shape) == (B, d + 1)
        for i, (p, t) in enumerate(zip(batch, twins)):
            t.plan_step_learned(m, obs[i])
            for name in ("mean", "std", "executed", "best_cost", "elites_actions", "elites_costs"):
                assert np.array_equal(np_(getattr(p, name)), np_(getattr(t, name))), (k, i, name)
            assert np.array_equal(np_(res[i]), np_(torch.cat([t.executed, t.best_cost]))), (k, i)
        uploads.append(batch[0].batch_uploads)
    if B == 3:   # the steady state uploads nothing (test_gpu_learned_step.py: the blocks settle after the third step)
        assert uploads[3] > 0 and uploads[3:] == [uploads[3]] * (steps - 3), uploads


# ---- 2. icem_plan_step_cem_learned --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,h,K,iters", [(17, 5, 4, 3), (250, 12, 10, 3)])
@pytest.mark.parametrize("d", WIDTHS)
def test_the_cem_step_equals_its_operator_loop(d, N, h, K, iters):
    with shared_model(d):
        assert not TC.planner(N, h, K, iters, d=d).cem_learned_step_ok()
        TC.run_against_the_loop(lambda: bound(TC.planner(N, h, K, iters, d=d), d), episodes=1)


@pytest.mark.parametrize("B", [3, 32])
@pytest.mark.parametrize("d", WIDTHS)
def test_the_cem_batch_equals_its_solo_twins(d, B):
    with shared_model(d):
        batch = TC.run_against_the_twins(lambda **kw: TC.planner(16, 12, 2, 2, d=d, **kw), B, steps=2)   # (the step binds the handles)
        assert tuple(batch.pls[0].cem_batch_results.shape) == (B, d + 1)
        if B == 3:
            seen = []
            for k in range(2, 5):
                batch.step_batch([TC.observation(i, k) for i in range(B)])
                seen.append(batch.pls[0].batch_uploads)
            assert seen == [2, 2, 2], seen   # (test_gpu_cem_learned.py: each of the two slots once)


# ---- 3. icem_plan_step_random_learned -----------------------------------------------------------------------------------------
def random_planner(N, h, d, seed=5, **cfg):
    from icem_amd import IcemConfig, IcemPlanner
    c = dict(horizon=h, act_dim=d, num_traj=N, elites_size=2, opt_iters=1, cost_mode="sum", dtype="f32", seed=seed)
    c.update(cfg)
    lo, hi = np.resize(TR.LOW, d), np.resize(TR.HIGH, d)   # (the six per-dimension bounds of test_gpu_random_learned.py, repeated)
    return IcemPlanner(IcemConfig(**c), lo, hi)


@pytest.mark.parametrize("N,h,hold", [(17, 5, 0), (250, 12, 4)])
@pytest.mark.parametrize("d", WIDTHS)
def test_the_random_step_equals_its_operator_chain(d, N, h, hold):
    with shared_model(d):
        assert not random_planner(N, h, d).random_learned_step_ok()
        fused = TR.run_against_the_chain(lambda: bound(random_planner(N, h, d), d), hold, episodes=1)
        assert tuple(fused.random_result.shape) == (d + 2,)


@pytest.mark.parametrize("B", [3, 32])
@pytest.mark.parametrize("d", WIDTHS)
def test_the_random_batch_equals_its_solo_twins(d, B):
    with shared_model(d):
        make = lambda **kw: random_planner(16, 12, d, **kw)   # noqa: E731
        start = [7 * i for i in range(B)]
        batch, twins = TR.Group(make, B, start), TR.Group(make, B, start)
        seen = []
        for s in range(3):
            obs = [TR.observation(i, s) for i in range(B)]
            ex = batch.step_batch(obs, 4)
            twins.step_solo(obs, 4)
            res = batch.pls[0].random_batch_results
            assert tuple(res.shape) == (B, d + 2) and np.array_equal(np_(ex), np_(res[:, :d]))
            TR.assert_equal(batch, twins, s, res)
            assert batch.pls[0].random_batch_launches == 3
            seen.append(batch.pls[0].batch_uploads)
        assert seen == [1, 1, 1], seen


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------
def _cem_call(pl, m, s):
    return lambda: pl.plan_step_cem_learned(m, TC.observation(0, 0), s.mean, s.std, s.lower, s.upper, like_levine=False, shift_means=True,
                                            execute_best_elite=True)


def test_bindings_that_are_refused_and_steps_behind_them_touch_nothing():
    from icem_amd import IcemPlanner, _lib as L
    m2, m6 = model(2), model(6)
    ob = TL.observations(1, seed=12)[0]
    # bind with the wrong width, and with widths the layout does not hold: the binding stays what it was
    p = TL.planner(3, act_dim=2)
    lib = p.lib
    assert lib.icem_rssm_act_dim(p._h) == 6
    for bad in (6, 3, 33):
        assert lib.icem_set_rssm_act_dim(p._h, bad) == L.ICEM_E_INVALID and lib.icem_rssm_act_dim(p._h) == 6, bad
    for d in (33, 64):
        wide = TL.planner(3, act_dim=d)
        assert lib.icem_set_rssm_act_dim(wide._h, d) == L.ICEM_E_UNSUPPORTED and lib.icem_rssm_act_dim(wide._h) == 6, d
        assert not wide._bind_rssm(type("M", (), {"act_dim": d})()) and not wide.learned_step_ok()
    # a d = 2 handle never bound is refused by all three solo entries, with the six-wide model and with a raw call on the two-wide one's params
    snap = TL.snapshot(p)
    assert not p.learned_step_ok() and not p.learned_step_ok(m6)
    with pytest.raises(L.IcemError) as e:
        p.plan_step_learned(m6, ob)
    assert e.value.code == L.ICEM_E_UNSUPPORTED
    cb = p._learned_buffers(p.obs_rssm.data_ptr())
    assert lib.icem_plan_step_learned(p._h, C.byref(cb), C.c_void_p(m2.params.data_ptr()), 0, p._stream()) == L.ICEM_E_UNSUPPORTED
    assert b"6 action dimensions" in lib.icem_last_error()
    TL.assert_untouched(p, snap, "an unbound d = 2 handle")
    with shared_model(2):
        c = TC.planner(250, 12, d=2)
        s = TC.Dist(c, False)
        before = [np_(x).copy() for x in TC.views(c, s).values()]
        cb = c._cem_cb(TC.observation(0, 0), s.mean, s.std, s.lower, s.upper, "obs_rssm")
        prm = L.IcemCemParamsC(0, 1, 1, 0)
        assert lib.icem_plan_step_cem_learned(c._h, C.byref(cb), C.byref(prm), C.c_void_p(m2.params.data_ptr()), 0, c._stream()) == L.ICEM_E_UNSUPPORTED
        r = random_planner(250, 12, 2)
        TR._spoilable(TR.Group(lambda **kw: r, 1))
        rb = [np_(x).copy() for x in TR.views(r).values()]
        cb = r._random_cb(TR.observation(0, 0), "obs_rssm")
        assert lib.icem_plan_step_random_learned(r._h, C.byref(cb), C.c_void_p(m2.params.data_ptr()), 4, 0, r._stream()) == L.ICEM_E_UNSUPPORTED
        torch.cuda.synchronize()
        assert all(np.array_equal(np_(x), y) for x, y in zip(TC.views(c, s).values(), before))
        assert all(np.array_equal(np_(x), y) for x, y in zip(TR.views(r).values(), rb))
    # an f64 handle binds (the binding knows no dtype) and is still refused by the step
    f = TL.planner(3, act_dim=2, dtype="f64")
    assert f._bind_rssm(m2) and lib.icem_rssm_act_dim(f._h) == 2 and not f.learned_step_ok(m2)
    snap = TL.snapshot(f)
    with pytest.raises(L.IcemError) as e:
        f.plan_step_learned(m2, ob)
    assert e.value.code == L.ICEM_E_UNSUPPORTED
    TL.assert_untouched(f, snap, "a bound f64 handle")
    # a batch of mixed bindings: ICEM_E_INVALID from all three batch entries, nothing touched, and the bound planner still steps
    a, b = bound(TL.planner(21, act_dim=2), 2), TL.planner(22, act_dim=2)
    sa, sb = TL.snapshot(a), TL.snapshot(b)
    hs = (C.c_void_p * 2)(a._h, b._h)
    obs = torch.zeros((2, 230), dtype=torch.float32, device="cuda")
    res = torch.zeros((2, 4), dtype=torch.float32, device="cuda")
    bs = (L.IcemPlanBuffersC * 2)(a._learned_buffers(obs[0].data_ptr()), b._learned_buffers(obs[1].data_ptr()))
    prm2 = C.c_void_p(m2.params.data_ptr())
    assert lib.icem_plan_step_learned_batch(hs, 2, bs, prm2, (C.c_int32 * 2)(0, 0), C.c_void_p(res.data_ptr()), a._stream()) == L.ICEM_E_INVALID
    assert b"one configuration" in lib.icem_last_error()
    TL.assert_untouched(a, sa, "mixed bindings")
    TL.assert_untouched(b, sb, "mixed bindings")
    with shared_model(2):
        ca, cb_ = bound(TC.planner(16, 12, 2, 2, d=2, seed=5), 2), TC.planner(16, 12, 2, 2, d=2, seed=6)
        g = TC.Group(lambda seed: {5: ca, 6: cb_}[seed], 2)
        with pytest.raises(L.IcemError) as e:
            TC._raw_batch(g, [obs[0].data_ptr(), obs[1].data_ptr()])
        assert e.value.code == L.ICEM_E_INVALID
        ra, rb_ = bound(random_planner(16, 12, 2, seed=5), 2), random_planner(16, 12, 2, seed=6)
        cbs = (L.IcemRandomBuffersC * 2)(ra._random_cb(TR.observation(0, 0), "obs_rssm"), rb_._random_cb(TR.observation(1, 0), "obs_rssm"))
        assert lib.icem_plan_step_random_learned_batch((C.c_void_p * 2)(ra._h, rb_._h), 2, cbs, prm2, 4, (C.c_int64 * 2)(0, 0),
                                                       C.c_void_p(res.data_ptr()), ra._stream()) == L.ICEM_E_INVALID
    a.plan_step_learned(m2, ob)
    t = TL.planner(21, act_dim=2)
    t.plan_step_learned(m2, ob)
    for x, y in zip(TL.snapshot(a), TL.snapshot(t)):
        assert np.array_equal(x, y)
    assert isinstance(IcemPlanner.__dict__["plan_step_learned_batch"], staticmethod)


# ---- 5. the controllers ---------------------------------------------------------------------------------------------------------
def env(d):
    from icem_amd.envs import CostSpec, SyntheticEnv
    return SyntheticEnv("Pendulum" if d == 1 else "Reacher", 230, -np.ones(d), np.ones(d), CostSpec(0.1, 8, -1.0, 1, 10.0, 0.3))


def icem_controller(d, seed, n=64):
    from icem_amd import MpcICemHip
    return MpcICemHip(env=env(d), forward_model=model(d), horizon=12, num_simulated_trajectories=n, factor_decrease_num=1.25,
                      cost_along_trajectory="sum", seed=seed, action_sampler_params=dict(TL.ASP), dtype="f32")


def cem_controller(d, seed, fused_step, n=64):
    from icem_amd import MpcCemStdHip
    return MpcCemStdHip(env=env(d), forward_model=model(d), horizon=12, num_simulated_trajectories=n, cost_along_trajectory="sum",
                        verbose=False, seed=seed, fused_step=fused_step,
                        action_sampler_params=dict(alpha=0.1, elites_size=10, opt_iterations=3, init_std=0.5, shift_means=True,
                                                   execute_best_elite=True, bounds_like_levine=False))


def random_controller(d, seed, fused_step, n=64):
    from icem_amd import MpcRandomHip
    return MpcRandomHip(env=env(d), forward_model=model(d), horizon=12, num_simulated_trajectories=n, cost_along_trajectory="sum",
                        verbose=False, seed=seed, fused_step=fused_step, action_sampler_params=dict(action_change_frequency=4))


def _begin(ctrls, obs):
    for c, ob in zip(ctrls, obs):
        c.beginning_of_rollout(observation=ob, state=None, mode="train")


@pytest.mark.parametrize("d", [1, 2])
def test_the_icem_controller_at_the_small_widths(d):
    from icem_amd import MpcICemHip
    obs0 = TL.observations(3)
    c, t = icem_controller(d, 5), icem_controller(d, 5)
    _begin([c, t], [obs0[0]] * 2)
    for k in range(4):
        got = c.get_action(obs0[0] + 0.01 * k, None)
        with TL.stagewise():
            want = t.get_action(obs0[0] + 0.01 * k, None)
        assert got.shape == (d,) and np.array_equal(got, want), k
        assert c.planner.learned_step_launches > 0 and t.planner.learned_step_launches == 0
        TL.assert_same_state(c, t, k)
    ctrls, solos = [icem_controller(d, i + 1) for i in range(3)], [icem_controller(d, i + 1) for i in range(3)]
    _begin(ctrls + solos, obs0 + obs0)
    for k in range(4):
        got = MpcICemHip.get_action_batch(ctrls, obs0)
        assert ctrls[0].planner.learned_step_launches > 0
        for i in range(3):
            assert np.array_equal(got[i], solos[i].get_action(obs0[i], None)), (k, i)
            TL.assert_same_state(ctrls[i], solos[i], (k, i))


@pytest.mark.parametrize("d", [1, 2])
def test_the_cem_controller_at_the_small_widths(d):
    from icem_amd import MpcCemStdHip
    a, b = cem_controller(d, 3, True), cem_controller(d, 3, False)
    assert a._fused_step_refusal() is None
    for k in range(4):
        obs = TC.observation(0, k)
        if k == 0:
            _begin([a, b], [obs, obs])
        got, want = a.get_action(obs, None), b.get_action(obs, None)
        assert got.shape == (d,) and np.array_equal(got, want), k
        TC.same_state(a, b, k)
    assert a.planner.cem_step_launches == 9 and b.planner.cem_step_launches == 0
    ctrls, twins = [cem_controller(d, 3 + i, True) for i in range(3)], [cem_controller(d, 3 + i, True) for i in range(3)]
    for k in range(4):
        obs = [TC.observation(i, k) for i in range(3)]
        if k == 0:
            _begin(ctrls + twins, obs + obs)
        got = MpcCemStdHip.get_action_batch(ctrls, obs)
        for i in range(3):
            assert np.array_equal(got[i], twins[i].get_action(obs[i], None)), (k, i)
            TC.same_state(ctrls[i], twins[i], (k, i))
    assert ctrls[0].planner.cem_batch_launches == 9


@pytest.mark.parametrize("d", [1, 2])
def test_the_random_controller_at_the_small_widths(d):
    from icem_amd import MpcRandomHip
    a, b = random_controller(d, 3, True), random_controller(d, 3, False)
    assert a._fused_step_refusal() is None and a._steps_through_the_rssm()
    _begin([a, b], [TR.observation(0, 0)] * 2)
    for s in range(4):
        obs = TR.observation(0, s)
        x, y = a.get_action(obs, None), b.get_action(obs, None)
        assert x.shape == (d,) and np.array_equal(x, y), s
        TR.same_controllers(a, b, s)
    assert a.planner.random_step_launches == 3 and b.planner.random_step_launches == 0
    ctrls, twins = [random_controller(d, 3 + i, True) for i in range(3)], [random_controller(d, 3 + i, True) for i in range(3)]
    _begin(ctrls + twins, [TR.observation(i, 0) for i in range(3)] * 2)
    for s in range(4):
        obs = [TR.observation(i, s) for i in range(3)]
        got = MpcRandomHip.get_action_batch(ctrls, obs)
        for i in range(3):
            assert np.array_equal(got[i], twins[i].get_action(obs[i], None)), (s, i)
            TR.same_controllers(ctrls[i], twins[i], (s, i))
    assert ctrls[0].planner.random_batch_launches == 3
