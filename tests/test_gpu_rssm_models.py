"""Problems with a MODEL EACH in one learned-dynamics launch (rssm_split_models_kernel, icem_rssm_split.hip):
icem_rssm_rollout_cost_models, the ensemble entry with its reduction, and the controllers on top of them.  A trajectory's
cost depends on its problem's weights, its problem's observation, its own actions and its row position inside its 16-row
tile, and the launch cuts every problem into tiles of its own -- so every comparison is BIT EQUALITY with
``DeviceRSSMModel.rollout_cost`` of the problem's own model on that problem alone ("solo"), and with the NumPy float32
restatement of the reduction (rssm_models_cases.py).  No tolerance appears in this file.  That the inputs can tell the models
apart -- on every row, for every single parameter tensor -- is shown on the CPU (test_rssm_models_sensitivity_cpu.py).
Shapes are the smallest at which the arrangement can go wrong: ragged last tiles, lone-tile and two-tile recurrence
workgroups, the 513th tile (reward workgroups that walk the tiles and reload a head across a model boundary), 32 problems."""
import ctypes as C

import numpy as np
import pytest
import torch

import rssm_models_cases as MC

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
_cache = {}


def np_(t):
    return t.detach().cpu().numpy()


def model(seed, tensor=None, d=6):
    """DeviceRSSMModel of declared_rssm(seed) (d = 6: rssm_models_cases' module, ``tensor`` taken from the donor seed)."""
    from icem_amd import DeviceRSSMModel
    key = (seed, tensor, d)
    if key not in _cache:
        _cache[key] = DeviceRSSMModel(module=MC.module(seed, tensor)) if d == 6 else DeviceRSSMModel(seed=seed, act_dim=d)
    return _cache[key]


def problems(rows, h, seed, d=6):
    """A distinct observation per problem (0.3 N(0, 1)) and distinct actions: (obs [B, 230] device, actions device)."""
    rs = np.random.RandomState(seed)
    obs = (0.3 * rs.randn(len(rows), 230)).astype(np.float32)
    acts = rs.uniform(-1, 1, (sum(rows), h, d)).astype(np.float32)
    return torch.as_tensor(obs, device="cuda"), torch.as_tensor(acts, device="cuda")


def pool_rows(n):
    """(obs [230], actions [n, 2, 6] device): the pool of rssm_models_cases, its 16 rows repeated up to n."""
    ob, acts = MC.pool()
    reps = -(-n // MC.POOL_ROWS)
    return ob, torch.as_tensor(np.tile(acts, (reps, 1, 1))[:n].copy(), device="cuda")


def solo_costs(ms, obs, acts, rows, mode, row0=None):
    """``rollout_cost`` of every problem alone, through its own model."""
    out, r0 = [], 0
    for p, r in enumerate(rows):
        a = r0 if row0 is None else row0[p]
        out.append(np_(ms[p].rollout_cost(np_(obs[p]), acts[a:a + r], mode)).copy())
        r0 += r
    return out


def raw_models(ms, obs, acts, rows, mode, costs, row0=None):
    """The entry point itself, writing into the caller's ``costs``: -> return code."""
    from icem_amd import _lib as L
    r0 = [sum(rows[:p]) for p in range(len(rows))] if row0 is None else row0
    arr = (L.IcemRssmProblemC * len(rows))(*[L.IcemRssmProblemC(ms[p].params.data_ptr(), r0[p], rows[p], p) for p in range(len(rows))])
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return ms[0].lib.icem_rssm_rollout_cost_models(len(rows), arr, acts.shape[1], acts.shape[2], mode, C.c_void_p(obs.data_ptr()), len(rows),
                                                   C.c_void_p(acts.data_ptr()), acts.shape[0], C.c_void_p(costs.data_ptr()), st)


def assert_equal_per_problem(got, want, rows, what=""):
    r0 = 0
    for p, r in enumerate(rows):
        assert np.array_equal(got[r0:r0 + r], want[p]), (what, "problem", p, "rows", r, np.flatnonzero(got[r0:r0 + r] != want[p])[:8])
        r0 += r


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [6, 2])
@pytest.mark.parametrize("tt", [0, 2], ids=["default", "tt2"])
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["sum", "best", "final"])
@pytest.mark.parametrize("h", [1, 3])
def test_every_problem_costs_what_it_costs_alone(h, mode, tt, d):
    """B = 4, rows 1 / 16 / 17 / 40, four models of which problems 1 and 2 name the SAME object, distinct observations; the
    compiled-in width and the runtime-width twin; three launches in a row into a sentinel-filled buffer with a guard entry
    behind it (the tile flags are back at zero behind each); then a same-model batch and a solo launch on the same stream."""
    from icem_amd import _lib as L, rssm_rollout_cost_models
    rows = [1, 16, 17, 40]
    a, b, c = model(5, d=d), model(6, d=d), model(7, d=d)
    ms = [a, b, b, c]
    if tt:
        L.set_option("rssm_split_tt", tt)
    obs, acts = problems(rows, h, 10 * h + mode, d)
    want = solo_costs(ms, obs, acts, rows, mode)
    assert not np.array_equal(want[1], solo_costs([a], obs[1:2], acts[1:17], [16], mode)[0]), "the models cannot be told apart here"
    total = sum(rows)
    for rep in range(3):
        costs = torch.full((total + 1,), SENTINEL, dtype=torch.float32, device="cuda")
        assert raw_models(ms, obs, acts, rows, mode, costs) == 0, a.lib.icem_last_error()
        got = np_(costs)
        assert got[total] == SENTINEL, "the guard entry behind the last problem was written"
        assert not np.any(got[:total] == SENTINEL), ("rows never written", np.flatnonzero(got[:total] == SENTINEL))
        assert_equal_per_problem(got, want, rows, f"launch {rep}")
    assert_equal_per_problem(np_(rssm_rollout_cost_models(ms, obs, acts, rows, None, mode)), want, rows, "the wrapper")
    same = np_(c.rollout_cost_batch(obs, acts, rows, mode))
    assert_equal_per_problem(same, solo_costs([c] * 4, obs, acts, rows, mode), rows, "a same-model batch behind the launches")
    assert np.array_equal(np_(c.rollout_cost(np_(obs[3]), acts[total - 40:], mode)), want[3]), "a solo launch behind them"


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,seeds,mode", [
    ([1400, 1399, 1401], [5, 6, 7], 0),        # 88 + 88 + 88 = 264 tiles: two tiles per recurrence workgroup, ragged last tiles
    ([4100, 4099], [5, 6], 1),                 # 257 + 257 = 514 tiles: walking heads 0 and 1 cross the model boundary
    ([8200, 16], [5, 6], 2),                   # 513 + 1: head 0's two tiles are in problem 0, head 1 crosses: no reload beside reload
    ([5] * 32, [5, 6] * 16, 0),                # the largest table, the models alternating
    ([333], [7], 0),                           # B = 1 is the solo launch
], ids=["264tiles", "514tiles", "513+1", "32x5", "one"])
def test_the_arrangements_by_size(rows, seeds, mode):
    from icem_amd import rssm_rollout_cost_models
    ms = [model(s) for s in seeds]
    obs, acts = problems(rows, 2, len(rows))
    want = solo_costs(ms, obs, acts, rows, mode)
    for rep in range(2):
        got = np_(rssm_rollout_cost_models(ms, obs, acts, rows, None, mode))
        assert got.shape == (sum(rows),)
        assert_equal_per_problem(got, want, rows, f"launch {rep}")


def test_walking_heads_come_back_to_a_model_they_held_before():
    """Three problems of 6000 rows (375 tiles each, 1125 tiles) on models A, B, A: head k walks tiles k, k + 512 and k + 1024
    -- A, then B (k < 238) or A, then A again: reload, reload back, and no reload, side by side."""
    from icem_amd import rssm_rollout_cost_models
    rows, ms = [6000] * 3, [model(5), model(6), model(5)]
    obs, acts = problems(rows, 2, 33)
    want = solo_costs(ms, obs, acts, rows, 1)
    assert_equal_per_problem(np_(rssm_rollout_cost_models(ms, obs, acts, rows, None, 1)), want, rows)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tensor", MC.TENSORS)
def test_one_tensor_pairs_in_the_walking_arrangement(tensor):
    """Rows [8200, 16], problem 0 on the base model and problem 1 on its twin that differs in ONE parameter tensor, the same
    observation, the pool's action rows: head 1 walks from tile 1 (problem 0) to tile 513 (problem 1).  A head that reloads
    only a part of what it holds -- or a recurrence that reads one tensor from the wrong buffer -- leaves a row of problem 1
    at the base model's cost, which differs from the twin's on every row in every mode (shown on the CPU)."""
    from icem_amd import rssm_rollout_cost_models
    rows, ms = [8200, 16], [model(MC.BASE), model(MC.BASE, tensor)]
    ob, acts = pool_rows(sum(rows))
    obs = torch.as_tensor(np.stack([ob, ob]), device="cuda")
    for name, mode in MC.MODES.items():
        want = solo_costs(ms, obs, acts, rows, mode)
        base_on_twins_rows = np_(ms[0].rollout_cost(ob, acts[8200:], mode))
        assert not np.any(base_on_twins_rows == want[1]), (tensor, name, "the pair cannot be told apart on the device")
        got = np_(rssm_rollout_cost_models(ms, obs, acts, rows, None, mode))
        assert_equal_per_problem(got, want, rows, (tensor, name))
        # and the other way round: the twin first, the walking head reloads towards the base model
        got = np_(rssm_rollout_cost_models(ms[::-1], obs, acts, rows, None, mode))
        assert_equal_per_problem(got, solo_costs(ms[::-1], obs, acts, rows, mode), rows, (tensor, name, "reversed"))


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
def test_problems_may_share_their_action_rows():
    """E = 3 problems that all name rows 0 .. 40 of one actions buffer (and one that names rows 8 .. 40 of it): slice e of the
    costs is member e alone; the actions are only read."""
    from icem_amd import rssm_rollout_cost_models
    ms = [model(s) for s in MC.MEMBER_SEEDS[:3]]
    ob, acts = pool_rows(40)
    obs = torch.as_tensor(np.stack([ob] * 3), device="cuda")
    before = np_(acts).copy()
    for mode in (0, 1, 2):
        got = np_(rssm_rollout_cost_models(ms, obs, acts, [40, 40, 40], [0, 0, 0], mode))
        assert got.shape == (120,)
        for e, m in enumerate(ms):
            assert np.array_equal(got[40 * e:40 * (e + 1)], np_(m.rollout_cost(ob, acts, mode))), (mode, e)
        got = np_(rssm_rollout_cost_models(ms, obs, acts, [40, 32, 1], [0, 8, 39], mode))
        assert_equal_per_problem(got, solo_costs(ms, obs, acts, [40, 32, 1], mode, row0=[0, 8, 39]), [40, 32, 1], mode)
    assert np.array_equal(np_(acts), before)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
def ensemble(E, reduce="mean", nan_member=None):
    from icem_amd import DeviceRSSMEnsemble, DeviceRSSMModel
    ms = [model(s) for s in MC.MEMBER_SEEDS[:E]]
    if nan_member is not None:
        import copy
        net = copy.deepcopy(MC.module(MC.MEMBER_SEEDS[nan_member]))
        with torch.no_grad():
            net.rew3.bias.fill_(float("nan"))
        ms[nan_member] = DeviceRSSMModel(module=net)
    return DeviceRSSMEnsemble(models=ms, reduce=reduce), ms


@pytest.mark.parametrize("E,n", [(1, 40), (3, 40), (5, 2048)], ids=["E1", "E3", "E5-640tiles"])
def test_the_ensemble_entry(E, n):
    """member_costs row e is member e alone; costs is the restated reduction of those rows, mean and max (in `sum`, where no
    single member holds the maximum: asserted on the device's own member costs); E = 5 at n = 2048 is 640 tiles, heads that
    walk from one member's tiles into another's."""
    ob, acts = pool_rows(n)
    for reduce in ("mean", "max"):
        ens, ms = ensemble(E, reduce)
        for mode in (0, 1, 2):
            costs = np_(ens.rollout_cost(ob, acts, mode))
            mc = np_(ens.member_costs)
            assert mc.shape == (E, n) and costs.shape == (n,)
            for e, m in enumerate(ms):
                assert np.array_equal(mc[e], np_(m.rollout_cost(ob, acts, mode))), (reduce, mode, e)
            assert np.array_equal(costs, MC.reduce_members(mc, reduce)), (reduce, mode)
            if E == 1:
                assert np.array_equal(costs, mc[0])
            elif mode == 0:
                assert len(set(mc.argmax(0).tolist())) >= 2, "one member is the worst on every row: max would say nothing"


def test_a_nan_member_makes_every_row_nan():
    ob, acts = pool_rows(40)
    for reduce in ("mean", "max"):
        for who in (0, 2):
            ens, ms = ensemble(3, reduce, nan_member=who)
            costs = np_(ens.rollout_cost(ob, acts, 0))
            mc = np_(ens.member_costs)
            assert np.isnan(mc[who]).all() and not np.isnan(np.delete(mc, who, 0)).any()
            assert np.isnan(costs).all(), (reduce, who)


def test_ensemble_refusals_leave_the_outputs_untouched():
    """33 members (ICEM_E_INVALID); members x tiles beyond the limit (rssm_split_max_n = 64: four tiles, three members of two
    tiles each are six: ICEM_E_UNSUPPORTED): sentinel-filled outputs stay as they are; then a good call on the same stream."""
    from icem_amd import _lib as L
    ens, ms = ensemble(3)
    ob, acts = pool_rows(17)
    obs = torch.as_tensor(ob, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(E):
        mc = torch.full((E, 17), SENTINEL, dtype=torch.float32, device="cuda")
        k = torch.full((17,), SENTINEL, dtype=torch.float32, device="cuda")
        ptrs = (C.c_void_p * E)(*[ms[e % 3].params.data_ptr() for e in range(E)])
        rc = ens.lib.icem_rssm_rollout_cost_ensemble(E, ptrs, 17, 2, 6, 0, 0, C.c_void_p(obs.data_ptr()), C.c_void_p(acts.data_ptr()),
                                                     C.c_void_p(mc.data_ptr()), C.c_void_p(k.data_ptr()), st)
        torch.cuda.synchronize()
        return rc, np_(mc), np_(k)

    rc, mc, k = call(33)
    assert rc == L.ICEM_E_INVALID and np.all(mc == SENTINEL) and np.all(k == SENTINEL)
    L.set_option("rssm_split_max_n", 64)
    rc, mc, k = call(3)
    assert rc == L.ICEM_E_UNSUPPORTED and np.all(mc == SENTINEL) and np.all(k == SENTINEL)
    L.reset_options()
    rc, mc, k = call(3)
    assert rc == 0
    for e in range(3):
        assert np.array_equal(mc[e], np_(ms[e].rollout_cost(ob, acts, 0))), e
    assert np.array_equal(k, MC.reduce_members(mc, "mean"))


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
def test_a_captured_ensemble_call_replays():
    """One call outside the capture on the side stream (it sizes the staging area), the capture of one ensemble call on that
    stream alone (a linear graph: the split launch, then the reduction), replays on fresh actions: the new solo bits."""
    ens, ms = ensemble(3, "max")
    ob, acts = pool_rows(100)
    rs = np.random.RandomState(6)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ens.rollout_cost(ob, acts)
        side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        out = ens.rollout_cost(ob, acts)
        members = ens.member_costs
    for rep in range(3):
        fresh = torch.as_tensor(rs.uniform(-1, 1, (100, 2, 6)), dtype=torch.float32, device="cuda")
        acts.copy_(fresh)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        mc = np_(members)
        for e, m in enumerate(ms):
            assert np.array_equal(mc[e], np_(m.rollout_cost(ob, fresh, 0))), (rep, e)
        assert np.array_equal(np_(out), MC.reduce_members(mc, "max")), rep


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
def icem(m, seed, horizon=4, **kw):
    from icem_amd import MpcICemHip, halfcheetah_env
    asp = dict(alpha=0.1, elites_size=10, opt_iterations=3, init_std=0.5, use_mean_actions=True, keep_previous_elites=True,
               shift_elites_over_time=True, fraction_elites_reused=0.3, noise_beta=0.25)
    return MpcICemHip(env=halfcheetah_env(17), forward_model=m, horizon=horizon, num_simulated_trajectories=128,
                      factor_decrease_num=1.25, cost_along_trajectory="sum", dtype="f32", seed=seed, action_sampler_params=asp, **kw)


def assert_same_state(a, b, what):
    assert a.last_min_cost == b.last_min_cost, what
    assert a.planner.mpc_step == b.planner.mpc_step, what
    assert np.array_equal(a.mean, b.mean) and np.array_equal(a.std, b.std), what
    assert np.array_equal(a.elite_samples.as_array("actions"), b.elite_samples.as_array("actions")), what


def test_controllers_with_a_model_each_step_together_as_they_step_alone():
    """Two MpcICemHip with DIFFERENT DeviceRSSMModels through get_action_batch for three MPC steps against twins stepping
    alone: executed actions, best costs, mean, std and elites bit for bit.  Asked for with ``own_models=True``: without the
    keyword the batch is refused as it always was ("must share one parameter buffer"), before any controller has advanced."""
    from icem_amd import MpcICemHip
    ms = [model(5), model(6)]
    rs = np.random.RandomState(9)
    obs0 = [0.3 * rs.randn(230) for _ in range(2)]
    ctrls = [icem(ms[i], seed=i + 1) for i in range(2)]
    twins = [icem(ms[i], seed=i + 1) for i in range(2)]
    for c, ob in zip(ctrls + twins, obs0 + obs0):
        c.beginning_of_rollout(observation=ob, state=None, mode="train")
    with pytest.raises(NotImplementedError, match="own_models=True"):
        MpcICemHip.get_action_batch(ctrls, obs0)
    assert [c.planner.mpc_step for c in ctrls] == [0, 0]
    for k in range(3):
        obs = [ob + 0.01 * k for ob in obs0]
        got = MpcICemHip.get_action_batch(ctrls, obs, own_models=True)
        for i, (c, t) in enumerate(zip(ctrls, twins)):
            assert np.array_equal(got[i], t.get_action(obs[i], None)), (k, i)
            assert_same_state(c, t, (k, i))
    # the twins' models really differ: controller 0 on model 1 executes something else
    other = icem(ms[1], seed=1)
    other.beginning_of_rollout(observation=obs0[0], state=None, mode="train")
    first = icem(ms[0], seed=1)
    first.beginning_of_rollout(observation=obs0[0], state=None, mode="train")
    assert not np.array_equal(other.get_action(obs0[0], None), first.get_action(obs0[0], None))


def test_a_one_member_ensemble_plans_as_its_member():
    from icem_amd import DeviceRSSMEnsemble
    m = model(5)
    ens = DeviceRSSMEnsemble(models=[m])
    ob = 0.3 * np.random.RandomState(3).randn(230)
    a, b = icem(ens, seed=4), icem(m, seed=4)
    assert a.rssm_path and not a._model_is_the_library_rssm() and b._model_is_the_library_rssm()
    for c in (a, b):
        c.beginning_of_rollout(observation=ob, state=None, mode="train")
    for k in range(3):
        assert np.array_equal(a.get_action(ob + 0.01 * k, None), b.get_action(ob + 0.01 * k, None)), k
        assert_same_state(a, b, k)


def test_planners_share_an_ensemble_in_one_launch():
    """Two MpcICemHip on ONE three-member ensemble through get_action_batch (2 x 3 problems per scoring launch) against twins
    alone; eleven planners would be 33 problems: a ValueError that says so."""
    from icem_amd import MpcICemHip
    ens, _ = ensemble(3)
    rs = np.random.RandomState(11)
    obs0 = [0.3 * rs.randn(230) for _ in range(2)]
    ctrls, twins = [icem(ens, seed=i + 1) for i in range(2)], [icem(ens, seed=i + 1) for i in range(2)]
    for c, ob in zip(ctrls + twins, obs0 + obs0):
        c.beginning_of_rollout(observation=ob, state=None, mode="train")
    for k in range(2):
        got = MpcICemHip.get_action_batch(ctrls, obs0)
        for i, (c, t) in enumerate(zip(ctrls, twins)):
            assert np.array_equal(got[i], t.get_action(obs0[i], None)), (k, i)
            assert_same_state(c, t, (k, i))
    with pytest.raises(ValueError, match="11 planners x 3 members = 33 problems"):
        ens.rollout_cost_batch(np.zeros((11, 230), np.float32), torch.zeros((11, 2, 6), device="cuda"), [1] * 11)


@pytest.mark.parametrize("kind,reduce", [("cem", "mean"), ("random", "max")])
def test_the_baselines_plan_through_an_ensemble(kind, reduce):
    """One step of MpcCemStdHip / MpcRandomHip on a three-member ensemble (their stage-wise loops: the model is no
    DeviceRSSMModel): last_min_cost is the restated reduction of the members' SOLO costs of the winning row of the last
    pool, and no row of that pool is cheaper."""
    from icem_amd import MpcCemStdHip, MpcRandomHip, halfcheetah_env
    ens, ms = ensemble(3, reduce)
    pools = []
    inner = ens.rollout_cost

    def recording(obs, actions, cost_mode=0):
        pools.append((np.asarray(obs, np.float32).copy(), actions.clone()))
        return inner(obs, actions, cost_mode)

    ens.rollout_cost = recording
    if kind == "cem":
        c = MpcCemStdHip(env=halfcheetah_env(17), forward_model=ens, horizon=4, num_simulated_trajectories=128,
                         cost_along_trajectory="sum", verbose=False, seed=3,
                         action_sampler_params=dict(alpha=0.1, elites_size=10, opt_iterations=2, init_std=0.5, shift_means=True,
                                                    execute_best_elite=True, bounds_like_levine=False))
    else:
        c = MpcRandomHip(env=halfcheetah_env(17), forward_model=ens, horizon=4, num_simulated_trajectories=128,
                         cost_along_trajectory="sum", verbose=False, seed=3, action_sampler_params=dict(action_change_frequency=2))
    ob = 0.3 * np.random.RandomState(5).randn(230)
    c.beginning_of_rollout(observation=ob, state=None, mode="train")
    c.get_action(ob, None)
    assert len(pools) == (2 if kind == "cem" else 1)
    o, acts = pools[-1]
    solo = np.stack([np_(m.rollout_cost(o, acts, 0)) for m in ms])
    want = MC.reduce_members(solo, reduce)
    assert c.last_min_cost == float(want.min())
    assert np.array_equal(np_(ens.member_costs), solo)
