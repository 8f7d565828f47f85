"""icem_plan_step_learned_models (learned_step.hip): the learned-dynamics MPC step through an ensemble's members or a model per
problem as one library call -- sample, (shift), ONE launch_rssm_split_models of n x members problems in member-major order, and
update_small_members_batch_kernel (k_merge.hip), the one-launch update that reduces the members' costs while it builds its keys.
The step is DEFINED by the stage-wise loop of the controllers around DeviceRSSMEnsemble.rollout_cost / rollout_cost_batch /
rssm_rollout_cost_models, and the entry only rearranges its launches, so every comparison in this file is ``np.array_equal``:
no tolerance appears.  (That the inputs can tell a wrong cost source from the right one is shown on the CPU:
test_learned_models_sensitivity_cpu.py, on the shape of the batch test below.)

Shapes: h = 12, N = 128, factor_decrease_num = 1.25, K = 10, 3 iterations -- rows 128 (+ 3 shifted elites from a problem's
second step on), 102, 81: every rollout's last 16-row tile is ragged, a batch's problems start off a multiple of 16 rows,
and with one problem reset a step later than its peers (131 | 128 | 131) row offsets and the member stride (390) differ
between steps.  Members are cached DeviceRSSMModel(seed=...)s of rssm_models_cases.MEMBER_SEEDS."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import learned_models_cases as LC
import rssm_models_cases as MC
import test_gpu_learned_step as TL

pytestmark = pytest.mark.gpu

ITERS = 3
SENTINEL = -12345.0
_models = {}
np_ = TL.np_
stagewise = TL.stagewise


def model(seed, d=6):
    from icem_amd import DeviceRSSMModel
    if (seed, d) not in _models:
        _models[(seed, d)] = DeviceRSSMModel(seed=seed, act_dim=d)
    return _models[(seed, d)]


def members(E, d=6):
    seeds = (MC.MEMBER_SEEDS * 7)[:E]   # (more than five members: the five models again, every member a buffer of its own)
    return [model(s, d) for s in seeds]


def ensemble(E, reduce="mean", d=6, nan_member=None):
    """A fresh DeviceRSSMEnsemble on the cached members (twins get an object each: member_costs is theirs)."""
    from icem_amd import DeviceRSSMEnsemble, DeviceRSSMModel
    ms = members(E, d)
    if nan_member is not None:
        import copy
        net = copy.deepcopy(ms[nan_member].reference)
        with torch.no_grad():
            net.rew3.bias.fill_(float("nan"))
        ms[nan_member] = DeviceRSSMModel(module=net)
    return DeviceRSSMEnsemble(models=ms, reduce=reduce)


def controller(m, seed, horizon=12, n=128, cost="sum", asp=None, **kw):
    from icem_amd import MpcICemHip, halfcheetah_env
    a = dict(TL.ASP)
    a.update(asp or {})
    kw.setdefault("dtype", "f32")
    return MpcICemHip(env=halfcheetah_env(17), forward_model=m, horizon=horizon, num_simulated_trajectories=n,
                      factor_decrease_num=1.25, cost_along_trajectory=cost, seed=seed, action_sampler_params=a, **kw)


def launches_of(c, step):
    """3 launches per iteration, + 1 in a step that shifts elites."""
    p = c.planner
    return 3 * len(p.population_sizes) + (1 if step > 0 and c.shift_elites_over_time and p.n_reuse > 0 else 0)


def same_state(a, b, what, equal_nan=False):
    sa, sb = TL.state(a), TL.state(b)
    for k in sa:
        assert np.array_equal(sa[k], sb[k], equal_nan=equal_nan), (what, k)


def drive_twins(c, t, steps, what, ob0=None, equal_nan=False):
    """c on the new entry against t under learned_step = 0, alternately: action, state, member costs, path and launch count."""
    ob0 = TL.observations(1)[0] if ob0 is None else ob0
    TL.begin(c, ob0)
    TL.begin(t, ob0)
    assert c._model_is_the_library_ensemble() and not c._model_is_the_library_rssm()
    assert c._learned_models_ok(None, 1), what
    for k in range(steps):
        ob = ob0 + 0.01 * k
        got = c.get_action(ob, None)
        with stagewise():
            assert not t._learned_models_ok(None, 1)
            want = t.get_action(ob, None)
        assert c.planner.learned_step_launches == launches_of(c, k) and t.planner.learned_step_launches == 0, (what, k, "which path")
        assert np.array_equal(got, want, equal_nan=equal_nan), (what, k, got, want)
        same_state(c, t, (what, k), equal_nan)
        mc, mt = np_(c.forward_model.member_costs), np_(t.forward_model.member_costs)
        assert mc.shape == mt.shape == (c.forward_model.members, c.planner.population_sizes[-1]), (what, k, mc.shape, mt.shape)
        assert np.array_equal(mc, mt, equal_nan=equal_nan), (what, k, "member_costs")


# ---- 1. fused against stage-wise, one controller on an ensemble ----------------------------------------------------------------
@pytest.mark.parametrize("cost", ["sum", "best", "final"])
@pytest.mark.parametrize("reduce", ["mean", "max"])
@pytest.mark.parametrize("E", [2, 3, 5])
def test_fused_step_equals_the_stagewise_step(E, reduce, cost):
    drive_twins(controller(ensemble(E, reduce), 5, cost=cost), controller(ensemble(E, reduce), 5, cost=cost), 4, (E, reduce, cost))


FLAG_VARIANTS = ["no_keep", "no_shift", "no_mean_row", "white", "n126_full_last_workgroup", "h10"]


@pytest.mark.parametrize("name", FLAG_VARIANTS + ["h30"])
def test_fused_step_equals_the_stagewise_step_under_every_flag(name):
    kw = dict(horizon=30) if name == "h30" else TL.VARIANTS[name]
    E, reduce = (2, "max") if name in ("h10", "h30") else (3, "mean")
    drive_twins(controller(ensemble(E, reduce), 5, **kw), controller(ensemble(E, reduce), 5, **kw), 4, name)


def test_the_runtime_width_twins():
    """d = 2: the rollout's runtime-width kernels.  The raw entry on a planner bound to the width against the operators called
    one by one through the ensemble (TL.operator_step), 3 steps."""
    from icem_amd import IcemPlanner
    ens, ref = ensemble(2, "mean", d=2), ensemble(2, "mean", d=2)
    p, q = TL.planner(11, act_dim=2), TL.planner(11, act_dim=2)
    ob0 = TL.observations(1, seed=4)[0]
    elites = None
    assert p._bind_rssm(ens) and p.learned_models_step_ok(1, 2)
    for k in range(3):
        ob = ob0 + 0.02 * k
        res = IcemPlanner.plan_step_learned_models([p], ens, [ob])
        want, elites, _ = TL.operator_step(q, ref, ob, elites)
        assert p.mpc_step == q.mpc_step == k + 1 and p.learned_step_launches == 3 * ITERS + (k > 0)
        assert np.array_equal(np_(res[0]), want) and np.array_equal(np_(torch.cat([p.executed, p.best_cost])), want), k
        assert np.array_equal(np_(p.mean), np_(q.mean)) and np.array_equal(np_(p.std), np_(q.std)), k
        a, c = p.current_elites()
        assert np.array_equal(np_(a), np_(elites[0])) and np.array_equal(np_(c), np_(elites[1])), k
        assert np.array_equal(np_(ens.member_costs), np_(ref.member_costs)), k


# ---- 2. batch against solo twins -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["one ensemble", "a model each"])
def test_batch_equals_solo_and_stagewise(kind):
    """B = 3 through get_action_batch on the new entry against twins stepping alone on the fused entries (their own n == 1
    call with their members) and twins on the stage-wise loop: 2 steps; 3 more after controller 1 alone was reset (128 rows
    against its peers' 131: offsets 0, 131, 259, stride 390)."""
    from icem_amd import MpcICemHip
    obs0 = TL.observations(3)
    shared = kind == "one ensemble"
    if shared:
        eb, es, et = ensemble(3), ensemble(3), ensemble(3)
        groups = [[controller(e, i + 1) for i in range(3)] for e in (eb, es, et)]
    else:
        ms = [model(s) for s in MC.MEMBER_SEEDS[:3]]
        groups = [[controller(ms[i], i + 1) for i in range(3)] for _ in range(3)]
    ctrls, solos, stage = groups
    for group in groups:
        for c, ob in zip(group, obs0):
            TL.begin(c, ob)
    E = 3 if shared else 1
    assert all(c._learned_models_ok(None, 3) for c in ctrls)

    def step(k):
        obs = [ob + 0.01 * k for ob in obs0]
        rows_last = [c._stage_rows(ITERS - 1) for c in ctrls]
        shifting = any(c.planner.mpc_step > 0 for c in ctrls)
        got = MpcICemHip.get_action_batch(ctrls, obs, own_models=not shared)
        assert ctrls[0].planner.learned_step_launches == 3 * ITERS + (1 if shifting else 0), k
        if shared:
            batch_mc = np_(eb.member_costs).copy()
            assert batch_mc.shape == (E, sum(rows_last))
        for i in range(3):
            alone = solos[i].get_action(obs[i], None)
            assert solos[i].planner.learned_step_launches > 0
            with stagewise():
                want = stage[i].get_action(obs[i], None)
            assert stage[i].planner.learned_step_launches == 0
            assert np.array_equal(got[i], alone) and np.array_equal(got[i], want), (k, i)
            same_state(ctrls[i], solos[i], ("solo", k, i))
            same_state(ctrls[i], stage[i], ("stage-wise", k, i))
            if shared:
                r0 = sum(rows_last[:i])
                assert np.array_equal(batch_mc[:, r0:r0 + rows_last[i]], np_(et.member_costs)), (k, i, "member_costs")
                assert np.array_equal(np_(es.member_costs), np_(et.member_costs)), (k, i, "solo member_costs")

    for k in range(2):
        step(k)
    for group in groups:
        TL.begin(group[1], obs0[1])
    assert [c._stage_rows(0) for c in ctrls] == LC.ROWS_LATE_RESET and [c.planner.mpc_step for c in ctrls] == [2, 0, 2]
    for k in range(2, 5):
        step(k)


def raw_models(pls, table, obs, reduce=0, member_costs=None, res=None, steps=None, n=None, z_r=None, members=None):
    """The entry itself on planners ``pls``: table [n][members] of parameter pointers (None: a NULL entry) -> return code."""
    from icem_amd import _lib as L
    k = len(pls)
    cbs = [pl._learned_buffers(obs[i].data_ptr()) for i, pl in enumerate(pls)]
    if z_r is not None:
        cbs[0].z_r = z_r.data_ptr()
    hs = (C.c_void_p * k)(*[pl._h for pl in pls])
    bs = (L.IcemPlanBuffersC * k)(*cbs)
    st = (C.c_int32 * k)(*(steps or [pl.mpc_step for pl in pls]))
    flat = [p for row in table for p in row]
    ptrs = (C.c_void_p * len(flat))(*flat)
    E = len(table[0]) if members is None else members
    return pls[0].lib.icem_plan_step_learned_models(hs, k if n is None else n, bs, E, ptrs, reduce, st,
                                                    None if member_costs is None else C.c_void_p(member_costs.data_ptr()),
                                                    None if res is None else C.c_void_p(res.data_ptr()), pls[0]._stream())


def test_the_raw_entry_with_an_ensemble_each():
    """B = 2, E = 2, four distinct models, reduce = max, through the C entry: every buffer of both problems (mean, std, BOTH elite
    halves, executed, best_cost, the results row) is its own n == 1 call's, and the operators' called one by one through a
    two-member ensemble of its models.  Problem 1 is reset after two steps: rows 131 | 128."""
    from icem_amd import DeviceRSSMEnsemble, IcemPlanner
    ms = [model(s) for s in MC.MEMBER_SEEDS[:4]]
    own = [[ms[0], ms[1]], [ms[2], ms[3]]]
    refs = [DeviceRSSMEnsemble(models=o, reduce="max") for o in own]
    batch, solo, ops = ([TL.planner(41 + i) for i in range(2)] for _ in range(3))
    obs0 = TL.observations(2, seed=8)
    elites = [None, None]
    for k in range(4):
        if k == 2:
            for group in (batch, solo, ops):
                group[1].mpc_step = 0
                group[1].reset_distribution(group[1].mean, group[1].std)
            elites[1] = None
        obs = [ob + 0.01 * k for ob in obs0]
        res = np_(IcemPlanner.plan_step_learned_models(batch, own, obs, reduce="max")).copy()
        assert batch[0].learned_step_launches == 3 * ITERS + (k > 0)
        for i in range(2):
            alone = np_(IcemPlanner.plan_step_learned_models([solo[i]], [own[i]], [obs[i]], reduce="max")).copy()
            want, elites[i], _ = TL.operator_step(ops[i], refs[i], obs[i], elites[i])
            assert np.array_equal(res[i], alone[0]) and np.array_equal(res[i], want), (k, i)
            for x, y in zip(TL.snapshot(batch[i]), TL.snapshot(solo[i])):
                assert np.array_equal(x, y), (k, i)
            assert np.array_equal(np_(batch[i].mean), np_(ops[i].mean)) and np.array_equal(np_(batch[i].std), np_(ops[i].std)), (k, i)
            a, c = batch[i].current_elites()
            assert np.array_equal(np_(a), np_(elites[i][0])) and np.array_equal(np_(c), np_(elites[i][1])), (k, i)


# ---- 3. edges of the new kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,E,reduce", [(1100, 2, "mean"), (40, 3, "max"), (40, 32, "mean"), (40, 32, "max"), (40, 9, "mean")],
                         ids=["pool-above-1024", "pool-of-40", "E32-mean", "E32-max", "E9-the-wide-group"])
def test_pool_sizes_and_member_counts(n, E, reduce):
    """n = 1100: the update's second pass over the pool reads member costs too (rows 1100 + 3, 880, 704).  n = 40: a pool of at
    most 64 (40 + 3, 32, 25).  E = 32: the launch's whole table at B = 1, and the 32-wide group of the reduction; E = 9: that
    group with slots behind the last member."""
    drive_twins(controller(ensemble(E, reduce), 7, n=n), controller(ensemble(E, reduce), 7, n=n), 2, (n, E, reduce))


def test_exactly_32_problems():
    """B = 4 controllers on one 8-member ensemble: 32 problems, the rollout's whole table; against stage-wise twins, 2 steps."""
    from icem_amd import MpcICemHip
    eb, et = ensemble(8), ensemble(8)
    obs0 = TL.observations(4, seed=5)
    ctrls, stage = [controller(eb, i + 1, n=40) for i in range(4)], [controller(et, i + 1, n=40) for i in range(4)]
    for c, ob in zip(ctrls + stage, obs0 + obs0):
        TL.begin(c, ob)
    assert ctrls[0].planner.learned_models_step_ok(4, 8) and not ctrls[0].planner.learned_models_step_ok(5, 8)
    for k in range(2):
        got = MpcICemHip.get_action_batch(ctrls, obs0)
        assert ctrls[0].planner.learned_step_launches == 3 * ITERS + (k > 0)
        with stagewise():
            want = MpcICemHip.get_action_batch(stage, obs0)
        assert stage[0].planner.learned_step_launches == 0
        for i in range(4):
            assert np.array_equal(got[i], want[i]), (k, i)
            same_state(ctrls[i], stage[i], (k, i))
        assert np.array_equal(np_(eb.member_costs), np_(et.member_costs)), k


def test_one_member_with_equal_pointers_is_the_shared_model_step():
    """members == 1 and the same pointer for every problem: bit for bit icem_plan_step_learned_batch (B = 3, one reset late), and
    with n == 1 icem_plan_step_learned."""
    from icem_amd import IcemPlanner
    m = model(3)
    a, b = [TL.planner(31 + i) for i in range(3)], [TL.planner(31 + i) for i in range(3)]
    obs0 = TL.observations(3, seed=7)
    for k in range(4):
        if k == 2:
            for group in (a, b):
                group[1].mpc_step = 0
                group[1].reset_distribution(group[1].mean, group[1].std)
        obs = [ob + 0.01 * k for ob in obs0]
        got = np_(IcemPlanner.plan_step_learned_models(a, [m, m, m], obs)).copy()
        want = np_(IcemPlanner.plan_step_learned_batch(b, m, obs)).copy()
        assert np.array_equal(got, want) and a[0].learned_step_launches == b[0].learned_step_launches, k
        for p, q in zip(a, b):
            for x, y in zip(TL.snapshot(p), TL.snapshot(q)):
                assert np.array_equal(x, y), k
    p, q = TL.planner(51), TL.planner(51)
    for k in range(2):
        IcemPlanner.plan_step_learned_models([p], [m], [obs0[0]])
        q.plan_step_learned(m, obs0[0])
        for x, y in zip(TL.snapshot(p), TL.snapshot(q)):
            assert np.array_equal(x, y), k


@pytest.mark.parametrize("reduce", ["mean", "max"])
@pytest.mark.parametrize("who", [0, 2])
def test_a_nan_member_ends_the_step_as_the_stagewise_loop_does(who, reduce):
    """A NaN in the last reward bias of member ``who``'s packed buffer: its costs are NaN, so is every reduced row, every key is
    (+inf, index), and the step ends exactly as the stage-wise twin's does (NaN compared as equal to NaN)."""
    c, t = controller(ensemble(3, reduce, nan_member=who), 5), controller(ensemble(3, reduce, nan_member=who), 5)
    drive_twins(c, t, 2, ("nan", who, reduce), equal_nan=True)
    mc = np_(c.forward_model.member_costs)
    assert np.isnan(mc[who]).all() and not np.isnan(np.delete(mc, who, 0)).any()
    assert np.isnan(c.last_min_cost) or np.isinf(c.last_min_cost)


# ---- 4. refusals leave everything untouched ------------------------------------------------------------------------------------
def test_refusals_happen_before_anything_runs():
    from icem_amd import IcemPlanner
    from icem_amd import _lib as L
    ms = [model(s) for s in MC.MEMBER_SEEDS[:3]]
    ptr = [m.params.data_ptr() for m in ms]
    ob = TL.observations(1, seed=12)[0]
    good, mate, twin = TL.planner(21), TL.planner(22), TL.planner(21)
    IcemPlanner.plan_step_learned_models([good], [ms], [ob])
    IcemPlanner.plan_step_learned_models([twin], [ms], [ob])
    other = TL.planner(23, act_dim=2)   # (another configuration, and once bound another RSSM width)
    assert other._bind_rssm(model(3, d=2))
    obs = torch.zeros((3, 230), dtype=torch.float32, device="cuda")
    z = torch.zeros((128, 6, 7), dtype=torch.float32, device="cuda")
    mc = torch.full((3 * 3 * 131,), SENTINEL, dtype=torch.float32, device="cuda")
    res = torch.full((3, 7), SENTINEL, dtype=torch.float32, device="cuda")
    third = TL.planner(24)
    snaps = [(p, TL.snapshot(p)) for p in (good, mate, other, third)]

    def option(name, value, call):
        def run():
            L.set_option(name, value)
            try:
                return call()
            finally:
                L.reset_options()
        return run

    kw = dict(member_costs=mc, res=res)
    cases = [
        ("3 x 11 = 33 problems", lambda: raw_models([good, mate, third], [[ptr[e % 3] for e in range(11)]] * 3, obs, **kw), L.ICEM_E_UNSUPPORTED),
        ("a NULL table entry", lambda: raw_models([good, mate], [ptr[:2], [ptr[0], None]], obs, **kw), L.ICEM_E_INVALID),
        ("reduce = 2", lambda: raw_models([good, mate], [ptr[:2]] * 2, obs, reduce=2, **kw), L.ICEM_E_INVALID),
        ("members = 0", lambda: raw_models([good], [ptr[:1]], obs, members=0, **kw), L.ICEM_E_INVALID),
        ("members = 33", lambda: raw_models([good], [[ptr[0]] * 33], obs, **kw), L.ICEM_E_INVALID),
        ("tiles beyond the limit", option("rssm_split_max_n", 256, lambda: raw_models([good, mate], [ptr] * 2, obs, **kw)), L.ICEM_E_UNSUPPORTED),
        ("learned_step = 0", option("learned_step", 0, lambda: raw_models([good, mate], [ptr] * 2, obs, **kw)), L.ICEM_E_UNSUPPORTED),
        ("external noise", lambda: raw_models([good, mate], [ptr] * 2, obs, z_r=z, **kw), L.ICEM_E_UNSUPPORTED),
        ("mixed widths", lambda: raw_models([good, other], [ptr[:2]] * 2, obs, **kw), L.ICEM_E_INVALID),
        ("the same handle twice", lambda: raw_models([good, good], [ptr[:2]] * 2, obs, **kw), L.ICEM_E_INVALID),
        ("n = 0", lambda: raw_models([good], [ptr[:2]], obs, n=0, **kw), L.ICEM_E_INVALID),
    ]
    for what, call, code in cases:
        launches = good.learned_step_launches
        assert call() == code, (what, good.lib.icem_last_error())
        assert b"icem_plan_step_learned" in good.lib.icem_last_error(), what
        torch.cuda.synchronize()
        for p, snap in snaps:
            TL.assert_untouched(p, snap, what)
        assert bool((mc == SENTINEL).all()) and bool((res == SENTINEL).all()), what
        assert good.learned_step_launches == launches, what
    # (rssm_split_max_n = 256 is 16 tiles: one problem's nine pass the handle's own check, two problems x three members x nine do not)
    assert good.learned_models_step_ok(2, 3) and not good.learned_models_step_ok(3, 11) and not good.learned_models_step_ok(1, 33)
    # ... and a proper step behind all that is the fresh twin's
    IcemPlanner.plan_step_learned_models([good], [ms], [ob])
    IcemPlanner.plan_step_learned_models([twin], [ms], [ob])
    for a, b in zip(TL.snapshot(good), TL.snapshot(twin)):
        assert np.array_equal(a, b)


def test_the_controllers_refuse_in_the_same_words_and_fall_back_to_the_same_bits():
    from icem_amd import MpcICemHip
    ms = [model(s) for s in MC.MEMBER_SEEDS[:2]]
    obs0 = TL.observations(2, seed=3)
    # a batch of controllers with a model each, without own_models: refused as ever, before any controller has advanced
    ctrls = [controller(ms[i], i + 1) for i in range(2)]
    for c, ob in zip(ctrls, obs0):
        TL.begin(c, ob)
    with pytest.raises(NotImplementedError, match="own_models=True"):
        MpcICemHip.get_action_batch(ctrls, obs0)
    assert [c.planner.mpc_step for c in ctrls] == [0, 0]
    # 11 planners x 3 members: no launch holds 33 problems; the stage-wise loop's words
    ens = ensemble(3)
    eleven = [controller(ens, i + 1, n=32) for i in range(11)]
    obs11 = TL.observations(11, seed=4)
    for c, ob in zip(eleven, obs11):
        TL.begin(c, ob)
    assert not eleven[0]._learned_models_ok(None, 11) and eleven[0]._learned_models_ok(None, 10)
    with pytest.raises(ValueError, match="11 planners x 3 members = 33 problems"):
        MpcICemHip.get_action_batch(eleven, obs11)
    # an unserved horizon (h = 4: none of the folded sampler's): solo and batch fall back to the stage-wise bits
    ea, eb = ensemble(2), ensemble(2)
    c4, t4 = [controller(ea, i + 1, horizon=4) for i in range(2)], [controller(eb, i + 1, horizon=4) for i in range(2)]
    for c, ob in zip(c4 + t4, obs0 + obs0):
        TL.begin(c, ob)
    assert not c4[0]._learned_models_ok(None, 1)
    for k in range(2):
        got = MpcICemHip.get_action_batch(c4, obs0) if k else [c.get_action(ob, None) for c, ob in zip(c4, obs0)]
        for i in range(2):
            with stagewise():
                want = t4[i].get_action(obs0[i], None)
            assert np.array_equal(got[i], want), (k, i)
            same_state(c4[i], t4[i], (k, i))
        assert c4[0].planner.learned_step_launches == 0
    # the entry refusing a batch its controllers asked for (the option goes off between the question and the call): stage-wise bits
    ec, et = ensemble(2), ensemble(2)
    cs, ts = [controller(ec, i + 1) for i in range(2)], [controller(et, i + 1) for i in range(2)]
    for c, ob in zip(cs + ts, obs0 + obs0):
        TL.begin(c, ob)
    with stagewise():
        got = MpcICemHip._get_action_batch_learned_models(cs, obs0, ec)
        want = MpcICemHip._get_action_batch_rssm(ts, obs0)
    assert np.array_equal(got, want) and cs[0].planner.learned_step_launches == 0


# ---- 5. steady state, alternation, capture -------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
def test_the_steady_state_uploads_nothing(B):
    """As test_gpu_learned_step.py reads it: the argument blocks of a step are those of the step two before it, the parameter
    pointers travel by value in the rollout's table.  After 4 warm-up steps 4 more upload nothing.  B = 1: a controller on an
    ensemble.  B = 3: planners with an ensemble each (E = 2) through IcemPlanner.plan_step_learned_models, member costs in the
    first handle's scratch."""
    from icem_amd import IcemPlanner
    if B == 1:
        c = controller(ensemble(3), 5)
        ob0 = TL.observations(1)[0]
        TL.begin(c, ob0)
        lead = c.planner

        def step(k):
            c.get_action(ob0 + 0.01 * k, None)
            assert lead.learned_step_launches > 0
    else:
        ms = members(5)
        own = [[ms[0], ms[1]], [ms[2], ms[3]], [ms[4], ms[0]]]
        pls = [TL.planner(31 + i) for i in range(B)]
        lead = pls[0]
        obs0 = np.stack(TL.observations(B, seed=7))

        def step(k):
            IcemPlanner.plan_step_learned_models(pls, own, obs0 + 0.01 * k)
    for k in range(4):
        step(k)
    before = lead.batch_uploads
    assert before > 0
    for k in range(4, 8):
        step(k)
    torch.cuda.synchronize()
    print("argument uploads: %d in 4 warm-up steps, %d in the 4 steps behind them" % (before, lead.batch_uploads - before))
    assert lead.batch_uploads == before, (before, lead.batch_uploads)


def test_a_controller_alternates_between_the_two_steps():
    """The new entry on the even steps, the stage-wise loop on the odd ones, against a twin that is stage-wise throughout."""
    c, t = controller(ensemble(3, "max"), 8), controller(ensemble(3, "max"), 8)
    ob0 = TL.observations(1, seed=6)[0]
    TL.begin(c, ob0)
    TL.begin(t, ob0)
    for k in range(6):
        ob = ob0 + 0.01 * k
        if k % 2 == 0:
            got = c.get_action(ob, None)
            assert c.planner.learned_step_launches == launches_of(c, k)
        else:
            with stagewise():
                got = c.get_action(ob, None)
        with stagewise():
            want = t.get_action(ob, None)
        assert np.array_equal(got, want), k
        same_state(c, t, k)
        assert np.array_equal(np_(c.forward_model.member_costs), np_(t.forward_model.member_costs)), k


def test_a_captured_call_replays_with_fresh_observations():
    """Steps 0, 1, 2 outside the capture on the capturing stream (the rollout's staging area, the step's scratch and the argument
    blocks of both slots), then step 3 captured -- nothing in the call synchronises, allocates or uploads -- and replayed three
    times, each time on a fresh observation: what a twin's uncaptured calls at mpc_step = 3 leave, bit for bit."""
    ms = members(3)
    table = [[m.params.data_ptr() for m in ms]]
    p, t = TL.planner(61), TL.planner(61)
    rs = np.random.RandomState(2)
    fresh = [torch.as_tensor((0.3 * rs.randn(1, 230)).astype(np.float32), device="cuda") for _ in range(6)]
    bufs = {}
    for pl in (p, t):
        bufs[pl] = (torch.zeros((1, 230), dtype=torch.float32, device="cuda"), torch.zeros((3 * 131,), dtype=torch.float32, device="cuda"),
                    torch.zeros((1, 7), dtype=torch.float32, device="cuda"))

    def call(pl, step):
        obs, mc, res = bufs[pl]
        assert raw_models([pl], table, obs, reduce=1, member_costs=mc, res=res, steps=[step]) == 0, pl.lib.icem_last_error()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for k in range(3):
            bufs[p][0].copy_(fresh[k])
            call(p, k)
        side.synchronize()
    uploads = p.batch_uploads
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        call(p, 3)
    assert p.batch_uploads == uploads and p.learned_step_launches == 3 * ITERS + 1
    for k in range(3):
        bufs[t][0].copy_(fresh[k])
        call(t, k)
    for rep in range(3):
        bufs[p][0].copy_(fresh[3 + rep])
        torch.cuda.synchronize()
        g.replay()
        bufs[t][0].copy_(fresh[3 + rep])
        call(t, 3)
        torch.cuda.synchronize()
        for x, y in zip(TL.snapshot(p)[1:], TL.snapshot(t)[1:]):
            assert np.array_equal(x, y), rep
        assert np.array_equal(np_(bufs[p][1]), np_(bufs[t][1])) and np.array_equal(np_(bufs[p][2]), np_(bufs[t][2])), rep
        assert not np.array_equal(np_(bufs[p][2]), np.zeros((1, 7), np.float32))


# ---- 6. an instrumented ensemble is still called stage by stage ----------------------------------------------------------------
def test_an_instrumented_ensemble_is_still_called():
    """rollout_cost replaced on the instance (a recording wrapper, as test_the_baselines_plan_through_an_ensemble's): not the
    library's own ensemble any more -- the controller calls it once per CEM iteration and computes the fused twin's bits."""
    ens, ref = ensemble(3), ensemble(3)
    calls, inner = [], ens.rollout_cost
    ens.rollout_cost = lambda ob, a, mode=0: (calls.append(a.shape[0]), inner(ob, a, mode))[1]
    c, t = controller(ens, 5), controller(ref, 5)
    assert not c._model_is_the_library_ensemble() and t._model_is_the_library_ensemble()
    ob0 = TL.observations(1)[0]
    TL.begin(c, ob0)
    TL.begin(t, ob0)
    for k in range(2):
        assert np.array_equal(c.get_action(ob0, None), t.get_action(ob0, None)), k
        same_state(c, t, k)
    assert calls == [128, 102, 81, 131, 102, 81] and c.planner.learned_step_launches == 0 < t.planner.learned_step_launches
