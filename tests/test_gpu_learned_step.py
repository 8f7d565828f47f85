"""icem_plan_step_learned / icem_plan_step_learned_batch (learned_step.hip): the MPC step of the learned-dynamics
configuration as one library call, for one planner or B planners at once.  The step is DEFINED by the stage-wise loop of the
controllers (MpcICemHip._get_action_stagewise + _stage_finish), and the new entries only rearrange its launches, so every
comparison in this file is ``np.array_equal``: no tolerance appears.

Shapes: one shared DeviceRSSMModel(seed=3), N = 128, factor_decrease_num = 1.25, elites_size = 10, 3 iterations -- rows
128 (+ 3 shifted elites from the second step on), 102, 81: the last 16-row tile of every rollout is ragged, the sampler's
last workgroup (42 rows at d = 6) is partial (N = 126 fills it exactly), a batch's problems start off a multiple of 16 rows.
h = 12 and h = 10 are two of the folded sampler's horizons, h = 30 the one at which its batched kernel also serves
icem_plan_step_batch; h = 4 is none of them (refused, the controller falls back)."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_cache = {}
ASP = dict(alpha=0.1, elites_size=10, opt_iterations=3, init_std=0.5, use_mean_actions=True, keep_previous_elites=True,
           shift_elites_over_time=True, fraction_elites_reused=0.3, noise_beta=0.25)


def np_(t):
    return t.detach().cpu().numpy()


def model():
    from icem_amd import DeviceRSSMModel
    if "m" not in _cache:
        _cache["m"] = DeviceRSSMModel(seed=3)
    return _cache["m"]


def controller(seed, horizon=12, n=128, cost="sum", asp=None, **kw):
    from icem_amd import MpcICemHip, halfcheetah_env
    a = dict(ASP)
    a.update(asp or {})
    kw.setdefault("dtype", "f32")
    return MpcICemHip(env=halfcheetah_env(17), forward_model=model(), horizon=horizon, num_simulated_trajectories=n,
                      factor_decrease_num=1.25, cost_along_trajectory=cost, seed=seed, action_sampler_params=a, **kw)


def begin(c, ob):
    c.beginning_of_rollout(observation=ob, state=None, mode="train")


@contextlib.contextmanager
def stagewise():
    """The library's switch between the two bit-identical arrangements: inside, the new entries refuse and a controller
    runs the stage-wise loop."""
    from icem_amd import _lib as L
    L.set_option("learned_step", 0)
    try:
        yield
    finally:
        L.set_option("learned_step", 1)


def state(c):
    ea, ec = c._elite_actions, c._elite_costs
    return dict(last_min_cost=c.last_min_cost, mpc_step=c.planner.mpc_step, mean=c.mean, std=c.std,
                elite_actions=np_(ea).copy(), elite_costs=np_(ec).copy())


def assert_same_state(a, b, what):
    sa, sb = state(a), state(b)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), (what, k)


def observations(n, seed=9):
    rs = np.random.RandomState(seed)
    return [0.3 * rs.randn(230) for _ in range(n)]


VARIANTS = {
    "h12": dict(),
    "h10": dict(horizon=10),
    "n126_full_last_workgroup": dict(n=126),
    "no_keep": dict(asp=dict(keep_previous_elites=False)),
    "no_shift": dict(asp=dict(shift_elites_over_time=False)),
    "no_mean_row": dict(asp=dict(use_mean_actions=False)),
    "best": dict(cost="best"),
    "final": dict(cost="final"),
    "white": dict(asp=dict(noise_beta=0)),
}


# ---- 1. fused equals stage-wise, one controller ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(VARIANTS))
def test_fused_step_equals_the_stagewise_step(name):
    """5 MPC steps of a controller on the new entry against a twin under learned_step = 0, driven alternately: executed
    action, last_min_cost, mean, std, elite actions, elite costs and mpc_step.  Step 0 shifts no elites, the later ones do."""
    kw = VARIANTS[name]
    c, t = controller(5, **kw), controller(5, **kw)
    ob0 = observations(1)[0]
    begin(c, ob0)
    begin(t, ob0)
    assert c.planner.learned_step_ok()
    for k in range(5):
        ob = ob0 + 0.01 * k
        got = c.get_action(ob, None)
        with stagewise():
            assert not t.planner.learned_step_ok()
            want = t.get_action(ob, None)
        assert c.planner.learned_step_launches > 0 and t.planner.learned_step_launches == 0, "which path each of them took"
        assert np.array_equal(got, want), (name, k, got, want)
        assert_same_state(c, t, (name, k))


def test_the_seven_round_generator_is_refused_and_falls_back():
    """The batched sampler is compiled for the default generator: a rng_rounds = 7 handle is not served, its controller
    steps stage-wise (the same bits as a twin under learned_step = 0)."""
    from icem_amd import _lib as L
    c, t = controller(5, rng_rounds=7), controller(5, rng_rounds=7)
    ob0 = observations(1)[0]
    begin(c, ob0)
    begin(t, ob0)
    assert not c.planner.learned_step_ok()
    with pytest.raises(L.IcemError) as e:
        c.planner.plan_step_learned(model(), ob0)
    assert e.value.code == L.ICEM_E_UNSUPPORTED and c.planner.mpc_step == 0
    for k in range(2):
        got = c.get_action(ob0, None)
        with stagewise():
            want = t.get_action(ob0, None)
        assert np.array_equal(got, want) and c.planner.learned_step_launches == 0
        assert_same_state(c, t, k)


# ---- 2. the raw entry against the operators -------------------------------------------------------------------------------
def planner(seed, horizon=12, n=128, **kw):
    from icem_amd import IcemConfig, IcemPlanner
    cfg = IcemConfig(horizon=horizon, act_dim=kw.pop("act_dim", 6), num_traj=n, elites_size=kw.pop("elites_size", 10), opt_iters=3,
                     factor_decrease=1.25, seed=seed, **kw)
    d = cfg.act_dim
    p = IcemPlanner(cfg, -np.ones(d), np.ones(d))
    p._ensure_buffers(learned=True)
    p.reset_distribution(p.mean, p.std)
    return p


def operator_step(p, m, ob, elites):
    """_get_action_stagewise's operators in its order, called from here on planner ``p``; elites = (actions, costs) of the
    step before or None.  -> (executed | best cost, elites of the last iteration, elites of the one before)."""
    it_n = p.cfg.opt_iters
    base = p.noise_offset(p.mpc_step * (it_n + 1))
    before = None
    for i, n_i in enumerate(p.population_sizes):
        shift = i == 0 and elites is not None and p.n_reuse > 0
        acts = torch.empty((n_i + (p.n_reuse if shift else 0), p.h, p.d), dtype=p.dt, device=p.device)
        p.sample_clip(n_i, p.mean, p.std, offset=base + i, row0_mean=i == it_n - 1, out=acts[:n_i])
        if shift:
            acts[n_i:, :-1] = elites[0][:p.n_reuse, 1:]
            p.sample_clip(p.n_reuse, p.mean, p.std, offset=base + it_n, t_begin=p.h - 1, out=acts[n_i:])
        costs = m.rollout_cost(ob, acts, 0)
        keep = i > 0 and p.n_reuse > 0
        before = elites
        ec, _, ea = p.update_distribution(costs, acts, p.K, p.mean, p.std, elites[1][:p.n_reuse] if keep else None,
                                          elites[0][:p.n_reuse] if keep else None)
        elites = (ea, ec)
    p.shift(p.mean, p.std)
    p.mpc_step += 1
    return np_(torch.cat([elites[0][0, 0], elites[1][:1]])), elites, before


def test_raw_entry_against_the_operators():
    """plan_step_learned through IcemPlanner alone against the operators called one by one: mean, std, executed, best_cost
    and BOTH elite halves (the last iteration's set and the one before it) over 3 steps."""
    m = model()
    p, q = planner(11), planner(11)
    ob0 = observations(1, seed=4)[0]
    elites = None
    for k in range(3):
        ob = ob0 + 0.02 * k
        p.plan_step_learned(m, ob)
        want, elites, before = operator_step(q, m, ob, elites)
        assert p.mpc_step == q.mpc_step == k + 1
        assert np.array_equal(np_(torch.cat([p.executed, p.best_cost])), want), k
        assert np.array_equal(np_(p.mean), np_(q.mean)) and np.array_equal(np_(p.std), np_(q.std)), k
        g = (p.mpc_step * p.cfg.opt_iters) & 1
        assert np.array_equal(np_(p.elites_actions[g]), np_(elites[0])) and np.array_equal(np_(p.elites_costs[g]), np_(elites[1])), k
        assert np.array_equal(np_(p.elites_actions[g ^ 1]), np_(before[0])) and np.array_equal(np_(p.elites_costs[g ^ 1]), np_(before[1])), k
        a, c = p.current_elites()
        assert a.data_ptr() == p.elites_actions[g].data_ptr() and c.data_ptr() == p.elites_costs[g].data_ptr()


# ---- 3. batch equals solo ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("horizon", [12, 10, 30])
def test_batch_equals_solo_and_stagewise(horizon):
    """B = 3 (distinct seeds and observations) through get_action_batch against twins stepping alone on the new entry and
    twins on the stage-wise path: 3 steps; 2 more after controller 1 alone was reset (128 rows against its peers' 131, its
    own mpc_step); then one solo get_action each."""
    from icem_amd import MpcICemHip
    obs0 = observations(3)
    ctrls = [controller(i + 1, horizon=horizon) for i in range(3)]
    solos = [controller(i + 1, horizon=horizon) for i in range(3)]
    stage = [controller(i + 1, horizon=horizon) for i in range(3)]
    for group in (ctrls, solos, stage):
        for c, ob in zip(group, obs0):
            begin(c, ob)

    def step(k):
        obs = [ob + 0.01 * k for ob in obs0]
        got = MpcICemHip.get_action_batch(ctrls, obs)
        assert ctrls[0].planner.learned_step_launches > 0
        for i in range(3):
            alone = solos[i].get_action(obs[i], None)
            with stagewise():
                want = stage[i].get_action(obs[i], None)
            assert np.array_equal(got[i], alone) and np.array_equal(got[i], want), (k, i)
            assert_same_state(ctrls[i], solos[i], ("solo", k, i))
            assert_same_state(ctrls[i], stage[i], ("stage-wise", k, i))

    for k in range(3):
        step(k)
    for group in (ctrls, solos, stage):
        begin(group[1], obs0[1])
    r = [c._stage_rows(0) for c in ctrls]
    assert r[1] == 128 < r[0] == r[2] == 131, r
    assert [c.planner.mpc_step for c in ctrls] == [3, 0, 3]
    for k in range(3, 5):
        step(k)
    for i in range(3):
        got = ctrls[i].get_action(obs0[i], None)
        with stagewise():
            want = stage[i].get_action(obs0[i], None)
        assert np.array_equal(got, want), i
        assert_same_state(ctrls[i], stage[i], ("after the batches", i))


def test_batch_of_32():
    """The largest batch once, at N = 32 (rows 32 (+ 3), 25, 20): every problem against its twin stepping alone, 2 steps."""
    from icem_amd import MpcICemHip
    obs0 = observations(32, seed=2)
    ctrls = [controller(i + 1, n=32) for i in range(32)]
    solos = [controller(i + 1, n=32) for i in range(32)]
    for group in (ctrls, solos):
        for c, ob in zip(group, obs0):
            begin(c, ob)
    for k in range(2):
        got = MpcICemHip.get_action_batch(ctrls, obs0)
        assert ctrls[0].planner.learned_step_launches > 0
        for i in range(32):
            assert np.array_equal(got[i], solos[i].get_action(obs0[i], None)), (k, i)
            assert_same_state(ctrls[i], solos[i], (k, i))


# ---- 4. alternation ---------------------------------------------------------------------------------------------------------
def test_a_controller_alternates_between_the_two_steps():
    """Fused on the even steps, stage-wise on the odd ones, against a twin that is stage-wise throughout: the elites cross
    between the planner's buffer halves and the controller's own tensors in both directions."""
    c, t = controller(8), controller(8)
    ob0 = observations(1, seed=6)[0]
    begin(c, ob0)
    begin(t, ob0)
    for k in range(6):
        ob = ob0 + 0.01 * k
        if k % 2 == 0:
            got = c.get_action(ob, None)
            assert c.planner.learned_step_launches > 0
        else:
            with stagewise():
                got = c.get_action(ob, None)
        with stagewise():
            want = t.get_action(ob, None)
        assert np.array_equal(got, want), k
        assert_same_state(c, t, k)


# ---- 5. launch count ----------------------------------------------------------------------------------------------------------
def test_launch_count_does_not_grow_with_the_batch():
    """At most 3 launches per iteration + 1, whatever B is: the same count at B = 1, 3 and 8, in a step without shifted
    elites and in one with them."""
    from icem_amd import MpcICemHip
    counts = {}
    for B in (1, 3, 8):
        obs0 = observations(B, seed=B)
        ctrls = [controller(i + 1) for i in range(B)]
        for c, ob in zip(ctrls, obs0):
            begin(c, ob)
        counts[B] = []
        for k in range(2):
            if B == 1:
                ctrls[0].get_action(obs0[0], None)
            else:
                MpcICemHip.get_action_batch(ctrls, obs0)
            counts[B].append(ctrls[0].planner.learned_step_launches)
    print("launches per step (first step, later steps) by batch size:", counts)
    for B, per_step in counts.items():
        assert all(0 < x <= 3 * 3 + 1 for x in per_step), counts
    assert counts[1] == counts[3] == counts[8], counts


# ---- 6. steady state ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
def test_the_steady_state_uploads_nothing(B):
    """learned_step.hip's claim: the argument blocks of a step are those of the step two before it (the elite halves alternate
    per iteration, 3 iterations: per step), the stream offsets travel in the kernel arguments.  The blocks change at step 0,
    at step 1 and at step 2 (shifted elites first appear in slot 0); after 4 warm-up steps 4 more upload nothing.
    B = 1: a controller.  B = 3: the raw entry on planners stepped by hand, with ONE results tensor and ONE observation
    array for all steps -- both pointers sit inside the blocks."""
    m = model()
    if B == 1:
        c = controller(5)
        ob0 = observations(1)[0]
        begin(c, ob0)
        lead = c.planner

        def step(k):
            c.get_action(ob0 + 0.01 * k, None)
            assert lead.learned_step_launches > 0
    else:
        from icem_amd import _lib as L
        pls = [planner(31 + i) for i in range(B)]
        lead = pls[0]
        obs = torch.as_tensor(np.stack(observations(B, seed=7)), dtype=torch.float32, device="cuda")
        res = torch.zeros((B, 7), dtype=torch.float32, device="cuda")
        hs = (C.c_void_p * B)(*[pl._h for pl in pls])

        def step(k):
            obs.add_(0.01)
            bs = (L.IcemPlanBuffersC * B)(*[pl._learned_buffers(obs[i].data_ptr()) for i, pl in enumerate(pls)])
            st = (C.c_int32 * B)(*[pl.mpc_step for pl in pls])
            L.check(lead.lib.icem_plan_step_learned_batch(hs, B, bs, C.c_void_p(m.params.data_ptr()), st, C.c_void_p(res.data_ptr()),
                                                          lead._stream()))
            for pl in pls:
                pl.mpc_step += 1
    for k in range(4):
        step(k)
    before = lead.batch_uploads
    assert before > 0
    for k in range(4, 8):
        step(k)
    torch.cuda.synchronize()
    print("argument uploads: %d in 4 warm-up steps, %d in the 4 steps behind them" % (before, lead.batch_uploads - before))
    assert lead.batch_uploads == before, (before, lead.batch_uploads)


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------
def snapshot(p):
    return [p.mpc_step] + [np_(x).copy() for x in (p.mean, p.std, p.elites_actions, p.elites_costs, p.executed, p.best_cost)]


def assert_untouched(p, snap, what):
    torch.cuda.synchronize()
    now = snapshot(p)
    assert now[0] == snap[0], what
    for a, b in zip(now[1:], snap[1:]):
        assert np.array_equal(a, b), what


def raw_batch(pls, m, steps=None, n=None, z_r=None):
    from icem_amd import _lib as L
    k = len(pls)
    obs = torch.zeros((k, 230), dtype=torch.float32, device="cuda")
    cbs = [pl._learned_buffers(obs[i].data_ptr()) for i, pl in enumerate(pls)]
    if z_r is not None:
        cbs[0].z_r = z_r.data_ptr()
    hs = (C.c_void_p * k)(*[pl._h for pl in pls])
    bs = (L.IcemPlanBuffersC * k)(*cbs)
    st = (C.c_int32 * k)(*(steps or [pl.mpc_step for pl in pls]))
    res = torch.zeros((k, 7), dtype=torch.float32, device="cuda")
    return pls[0].lib.icem_plan_step_learned_batch(hs, k if n is None else n, bs, C.c_void_p(m.params.data_ptr()), st,
                                                   C.c_void_p(res.data_ptr()), pls[0]._stream())


def test_refusals_happen_before_anything_runs():
    from icem_amd import _lib as L
    m = model()
    ob = observations(1, seed=12)[0]
    good, twin = planner(21), planner(21)
    good.plan_step_learned(m, ob)
    twin.plan_step_learned(m, ob)
    # handles that are not served: ICEM_E_UNSUPPORTED from the solo entry, the handle's buffers as they were
    unserved = {"f64": planner(3, dtype="f64"), "act_dim 4": planner(3, act_dim=4), "world 2": planner(3, world=2),
                "K = 40": planner(3, elites_size=40), "h = 4": planner(3, horizon=4)}
    for what, p in unserved.items():
        assert not p.learned_step_ok(), what
        snap = snapshot(p)
        with pytest.raises(L.IcemError) as e:
            p.plan_step_learned(m, ob)
        assert e.value.code == L.ICEM_E_UNSUPPORTED, what
        assert_untouched(p, snap, what)
    # calls that are refused although the handle is served
    snap = snapshot(good)
    z = torch.zeros((128, 6, 7), dtype=torch.float32, device="cuda")
    other = planner(22, horizon=10)
    snap_other = snapshot(other)
    cases = [("z_r", lambda: raw_batch([good], m, z_r=z), L.ICEM_E_UNSUPPORTED),
             ("two configurations", lambda: raw_batch([good, other], m), L.ICEM_E_INVALID),
             ("the same handle twice", lambda: raw_batch([good, good], m), L.ICEM_E_INVALID),
             ("n = 0", lambda: raw_batch([good], m, n=0), L.ICEM_E_INVALID),
             ("n = 33", lambda: raw_batch([good] * 33, m), L.ICEM_E_INVALID)]
    for what, call, code in cases:
        assert call() == code, (what, good.lib.icem_last_error())
        assert_untouched(good, snap, what)
        assert_untouched(other, snap_other, what)
    with pytest.raises(L.IcemError):
        type(good).plan_step_learned_batch([], m, [])
    # ... and a proper step behind all that is the fresh twin's
    good.plan_step_learned(m, ob)
    twin.plan_step_learned(m, ob)
    for a, b in zip(snapshot(good), snapshot(twin)):
        assert np.array_equal(a, b)


def test_a_controller_at_an_unserved_horizon_falls_back():
    """h = 4: the entry refuses (ICEM_E_UNSUPPORTED), get_action and get_action_batch still return the stage-wise action."""
    from icem_amd import MpcICemHip
    obs0 = observations(2, seed=3)
    ctrls = [controller(i + 1, horizon=4) for i in range(2)]
    twins = [controller(i + 1, horizon=4) for i in range(2)]
    for c, ob in zip(ctrls + twins, obs0 + obs0):
        begin(c, ob)
    assert not ctrls[0].planner.learned_step_ok()
    for k in range(2):
        got = MpcICemHip.get_action_batch(ctrls, obs0) if k else [c.get_action(ob, None) for c, ob in zip(ctrls, obs0)]
        for i in range(2):
            with stagewise():
                want = twins[i].get_action(obs0[i], None)
            assert np.array_equal(got[i], want), (k, i)
            assert_same_state(ctrls[i], twins[i], (k, i))
        assert ctrls[0].planner.learned_step_launches == 0


def test_an_instrumented_rollout_is_still_called():
    """A model whose rollout_cost was replaced on the instance (a timing or counting wrapper) is not the library's own
    rollout any more: the controller calls it stage by stage, once per CEM iteration, and computes the same bits."""
    from icem_amd import DeviceRSSMModel
    m = DeviceRSSMModel(seed=3)
    c, t = controller(5), controller(5)
    c.forward_model = m
    calls, orig = [], m.rollout_cost
    m.rollout_cost = lambda ob, a, mode=0: (calls.append(a.shape[0]), orig(ob, a, mode))[1]
    ob0 = observations(1)[0]
    begin(c, ob0)
    begin(t, ob0)
    for k in range(2):
        assert np.array_equal(c.get_action(ob0, None), t.get_action(ob0, None)), k
        assert_same_state(c, t, k)
    assert calls == [128, 102, 81, 131, 102, 81] and c.planner.learned_step_launches == 0 < t.planner.learned_step_launches
