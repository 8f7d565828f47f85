"""icem_rssm_rollout_cost_batch (rssm_split_batch_kernel, icem_rssm_split.hip): B planners' populations through the
declared RSSM in one launch, each problem with its own start state.  A trajectory's cost depends on the weights, its
problem's observation, its own actions and its row position inside its 16-row tile, and a batch cuts every problem into
tiles of its own -- so the criterion is BIT EQUALITY per problem with icem_rssm_rollout_cost on that problem alone; no
tolerance appears in this file except rssm_cases' own (the float64 emulation, test 3).  Shapes are the smallest at which
the indexing can go wrong: problems that start off a multiple of 16 rows, ragged last tiles, lone-tile and two-tile
recurrence workgroups, the 257th tile (two tiles per workgroup by the launcher's own rule), the 513th (reward workgroups
that walk the tiles, across a problem boundary), 32 problems."""
import ctypes as C

import numpy as np
import pytest
import torch

import rssm_cases as RC

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
_cache = {}


def np_(t):
    return t.detach().cpu().numpy()


def model():
    from icem_amd import DeviceRSSMModel
    if "m" not in _cache:
        _cache["m"] = DeviceRSSMModel(seed=3)
    return _cache["m"]


def problems(rows, h, seed):
    """A distinct observation per problem (0.3 N(0, 1)) and distinct actions: (obs [B, 230] device, actions device)."""
    rs = np.random.RandomState(seed)
    obs = (0.3 * rs.randn(len(rows), 230)).astype(np.float32)
    acts = rs.uniform(-1, 1, (sum(rows), h, 6)).astype(np.float32)
    return torch.as_tensor(obs, device="cuda"), torch.as_tensor(acts, device="cuda")


def solo_costs(m, obs, acts, rows, mode):
    """icem_rssm_rollout_cost on every problem alone."""
    out, r0 = [], 0
    for p, r in enumerate(rows):
        out.append(np_(m.rollout_cost(np_(obs[p]), acts[r0:r0 + r], mode)).copy())
        r0 += r
    return out


def raw_batch(m, obs, acts, rows, mode, costs):
    """The entry point itself, writing into the caller's ``costs``: -> return code."""
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return m.lib.icem_rssm_rollout_cost_batch(len(rows), (C.c_int32 * len(rows))(*rows), acts.shape[1], mode,
                                              C.c_void_p(m.params.data_ptr()), C.c_void_p(obs.data_ptr()),
                                              C.c_void_p(acts.data_ptr()), C.c_void_p(costs.data_ptr()), st)


def assert_equal_per_problem(got, want, rows, what=""):
    r0 = 0
    for p, r in enumerate(rows):
        assert np.array_equal(got[r0:r0 + r], want[p]), (what, "problem", p, "rows", r,
                                                        np.flatnonzero(got[r0:r0 + r] != want[p])[:8])
        r0 += r


@pytest.mark.parametrize("tt", [0, 2], ids=["default", "tt2"])
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["sum", "best", "final"])
@pytest.mark.parametrize("h", [1, 3])
def test_every_problem_costs_what_it_costs_alone(h, mode, tt):
    """B = 4, rows 1 / 16 / 17 / 40 (tiles 1, 1, 2, 3: under rssm_split_tt = 2 lone-tile and two-tile workgroups), three
    launches in a row (the tile flags are back at zero behind each), exactly sum(rows) costs written, then a launch of one
    problem on the same stream."""
    from icem_amd import _lib as L
    m, rows = model(), [1, 16, 17, 40]
    if tt:
        L.set_option("rssm_split_tt", tt)
    obs, acts = problems(rows, h, 10 * h + mode)
    want = solo_costs(m, obs, acts, rows, mode)
    total = sum(rows)
    for rep in range(3):
        costs = torch.full((total + 1,), SENTINEL, dtype=torch.float32, device="cuda")
        assert raw_batch(m, obs, acts, rows, mode, costs) == 0, m.lib.icem_last_error()
        got = np_(costs)
        assert got[total] == SENTINEL, "the guard entry behind the last problem was written"
        assert not np.any(got[:total] == SENTINEL), ("rows never written", np.flatnonzero(got[:total] == SENTINEL))
        assert_equal_per_problem(got, want, rows, f"launch {rep}")
    again = np_(m.rollout_cost(np_(obs[3]), acts[total - 40:], mode))
    assert np.array_equal(again, want[3]), "a launch of one problem behind the batches"
    assert np.array_equal(np_(m.rollout_cost_batch(obs, acts, rows, mode)), np.concatenate(want))


@pytest.mark.parametrize("rows,h,mode", [
    ([1400, 1399, 1401], 2, 0),   # 88 + 88 + 88 = 264 tiles: two tiles per recurrence workgroup, ragged last tiles
    ([4100, 4099], 2, 1),         # 257 + 257 = 514 tiles: 512 walking reward workgroups, tiles 512 / 513 in the second problem
    ([5] * 32, 1, 2),             # the largest table
    ([333], 2, 0),                # B = 1 is icem_rssm_rollout_cost
], ids=["264tiles", "514tiles", "32x5", "one"])
def test_the_arrangements_by_size(rows, h, mode):
    m = model()
    obs, acts = problems(rows, h, len(rows))
    want = solo_costs(m, obs, acts, rows, mode)
    for rep in range(2):
        got = np_(m.rollout_cost_batch(obs, acts, rows, mode))
        assert got.shape == (sum(rows),)
        assert_equal_per_problem(got, want, rows, f"launch {rep}")


@pytest.mark.parametrize("case", [c for c in RC.FULL_CASES if c.launches > 1], ids=lambda c: c.name)
def test_batches_against_the_float64_emulation(case):
    """rssm_cases' pooled cases -- their launches already are problems with an observation each -- as batches of up to 32
    problems, held to the emulation of the kernel's rounding points by rssm_cases' own criterion and bounds."""
    from icem_amd import DeviceRSSMModel
    m = DeviceRSSMModel(module=RC.module(case))
    launches = RC.launches(case)
    got = []
    for b0 in range(0, len(launches), 32):
        part = launches[b0:b0 + 32]
        obs = np.stack([ob for ob, _ in part])
        acts = torch.as_tensor(np.concatenate([a for _, a in part], 0), dtype=torch.float32, device="cuda")
        got.append(np_(m.rollout_cost_batch(obs, acts, [a.shape[0] for _, a in part], RC.MODES[case.mode])).astype(np.float64))
    got, want = np.concatenate(got), RC.want(case)
    print(case.name, RC.errors(got, want))
    assert got.shape == want.shape
    assert RC.agree(got, want), (RC.violations(got, want), RC.errors(got, want))


def test_refusals_launch_nothing():
    """More tiles than the split launch takes (rssm_split_max_n = 64: four tiles, the batch has seven), or the split
    launch switched off: ICEM_E_UNSUPPORTED, the costs untouched; then a good batch on the same stream."""
    from icem_amd import _lib as L
    m, rows, h, mode = model(), [1, 16, 17, 40], 3, 0
    obs, acts = problems(rows, h, 77)
    want = solo_costs(m, obs, acts, rows, mode)
    for name, value in (("rssm_split_max_n", 64), ("rssm_split", 0)):
        L.set_option(name, value)
        costs = torch.full((sum(rows) + 1,), SENTINEL, dtype=torch.float32, device="cuda")
        assert raw_batch(m, obs, acts, rows, mode, costs) == L.ICEM_E_UNSUPPORTED, name
        torch.cuda.synchronize()
        assert np.all(np_(costs) == SENTINEL), name
        L.reset_options()
    assert_equal_per_problem(np_(m.rollout_cost_batch(obs, acts, rows, mode)), want, rows)


def test_a_captured_batch_replays():
    """One call outside the capture on the side stream (it sizes the staging area), the capture of one batched call on
    that stream alone (a linear graph), replays on fresh actions: what a direct call gives, bit for bit."""
    m, rows, h = model(), [100, 37], 3
    obs, acts = problems(rows, h, 5)
    rs = np.random.RandomState(6)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.rollout_cost_batch(obs, acts, rows)
        side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        out = m.rollout_cost_batch(obs, acts, rows)
    for rep in range(3):
        fresh = torch.as_tensor(rs.uniform(-1, 1, (sum(rows), h, 6)), dtype=torch.float32, device="cuda")
        acts.copy_(fresh)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        direct = m.rollout_cost_batch(obs, fresh, rows)
        torch.cuda.synchronize()
        assert np.array_equal(np_(out), np_(direct)), rep
        assert_equal_per_problem(np_(out), solo_costs(m, obs, fresh, rows, 0), rows, f"replay {rep}")


# ---- controllers ------------------------------------------------------------------------------------------------------------
def controller(m, seed, horizon=4, **kw):
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


def test_controllers_step_together_as_they_step_alone():
    """Three MpcICemHip over one DeviceRSSMModel (the third through a second model object on the same parameter storage)
    through get_action_batch against three twins stepping alone: executed actions, last_min_cost, mean, std and the elites
    bit-equal over 3 steps; over 2 more after controller 1 alone was reset (no shifted elites at its iteration 0: its row
    count differs from its peers'); and over one solo get_action of every controller of the former batch (the Philox
    offsets went on as they would have alone)."""
    from icem_amd import DeviceRSSMModel, MpcICemHip
    m = model()
    m2 = DeviceRSSMModel(seed=3)
    m2.params = m.params
    rs = np.random.RandomState(9)
    obs0 = [0.3 * rs.randn(230) for _ in range(3)]
    ctrls = [controller(m2 if i == 2 else m, seed=i + 1) for i in range(3)]
    twins = [controller(m, seed=i + 1) for i in range(3)]
    for c, ob in zip(ctrls + twins, obs0 + obs0):
        c.beginning_of_rollout(observation=ob, state=None, mode="train")

    def step(k):
        obs = [ob + 0.01 * k for ob in obs0]
        got = MpcICemHip.get_action_batch(ctrls, obs)
        for i, (c, t) in enumerate(zip(ctrls, twins)):
            assert np.array_equal(got[i], t.get_action(obs[i], None)), (k, i)
            assert_same_state(c, t, (k, i))

    for k in range(3):
        step(k)
    for c in (ctrls[1], twins[1]):
        c.beginning_of_rollout(observation=obs0[1], state=None, mode="train")
    r = [c._stage_rows(0) for c in ctrls]
    assert r[1] == 128 < r[0] == r[2], r
    for k in range(3, 5):
        step(k)
    for i, (c, t) in enumerate(zip(ctrls, twins)):
        assert np.array_equal(c.get_action(obs0[i], None), t.get_action(obs0[i], None)), i
        assert_same_state(c, t, ("solo", i))

    # what a batch refuses, before any controller has advanced
    others = [controller(m, seed=7, horizon=5), controller(m, seed=7, noise_source="numpy_legacy"),
              controller(DeviceRSSMModel(seed=4), seed=7)]
    for o in others:
        o.beginning_of_rollout(observation=obs0[0], state=None, mode="train")
        before = ctrls[0].planner.mpc_step
        with pytest.raises(NotImplementedError, match="get_action_batch"):
            MpcICemHip.get_action_batch([ctrls[0], o], [obs0[0], obs0[0]])
        assert ctrls[0].planner.mpc_step == before and o.planner.mpc_step == 0
