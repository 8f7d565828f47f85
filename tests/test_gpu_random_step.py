"""``icem_plan_step_random`` (random_step.hip, k_random.hip): the MPC step of the random-shooting baseline (``MpcRandom.get_action``,
icem/controllers/mpc.py:114-138) as one library call, held bit for bit to the operator chain it replaces -- ``sample_piecewise``,
``rollout_cost``, ``topk_sorted(costs, 1)`` and the gathers, restated below -- on the SAME planner (the entry keeps no step state,
so the two may alternate): the pool, its costs, the best row and ``result`` compare equal as bytes over three consecutive steps
with a running call offset, at one shape per rollout family, at pool sizes from 2 rows to several sampler workgroups and at hold
lengths whose blocks straddle rows, workgroups and steps.  A planted minimum holds the selection launch to every slice edge;
ties and non-finite costs go the way ``icem_topk_sorted`` sends them.  Then the controller: fused against the operator chain,
against the NumPy oracle on the same Philox uniforms, the launch count, a captured step's replay, and the refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import icem_oracle as O   # checker only

pytestmark = pytest.mark.gpu

LOW, HIGH = -0.7, 0.9
STEPS = 3
NAMES = ("actions", "costs", "best_actions", "result")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def np_(t):
    return t.detach().cpu().numpy().astype(np.float64)


def bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def planner(dtype, N, h, d, o, kind, *, mode="sum", rounds=10, wide=None, f64_arith=None, tile=None, spec=None, seed=5, model=None,
            low=LOW, high=HIGH, model_seed=11, **cfg):
    """A planner configured as ``MpcRandomHip`` configures its own (elites_size 2, one iteration)."""
    from icem_amd import DeviceSyntheticModel, IcemConfig, IcemPlanner
    c = dict(horizon=h, act_dim=d, num_traj=N, elites_size=2, opt_iters=1, cost_mode=mode, dtype=dtype, rng_rounds=rounds, seed=seed)
    c.update(cfg)
    pl = IcemPlanner(IcemConfig(**c), low * np.ones(d), high * np.ones(d))
    if f64_arith is not None:
        assert pl.set_f64_arith(f64_arith) == f64_arith
    m = model if model is not None else DeviceSyntheticModel.make(o, d, kind=kind, seed_a=model_seed, seed_b=model_seed + 1)
    pl.set_model(m.kind, m.A, m.B)
    if spec is None:
        pl.set_cost(0.1, o - 1, -1.0, min(1, o - 1), 10.0, 0.3)
    else:
        pl.set_cost_spec(spec)
    if wide is not None:
        assert pl.set_wide_arith(wide) == wide
    if tile is not None:
        pl.set_tile_arith(tile)
    return pl


def chain_step(pl, obs, offset, freq, u=None, first=0):
    """The operator chain of ``MpcRandomHip._step_stagewise`` (icem_amd/controllers.py) -> the buffers the fused step is compared on."""
    actions = pl.sample_piecewise(pl.cfg.num_traj, offset, freq, u, first)
    costs = pl.rollout_cost(obs, actions)
    best_cost, idx = pl.topk_sorted(costs, 1)
    best = int(idx[0])
    result = torch.cat([actions[best, 0], best_cost.to(pl.dt), idx.to(pl.dt)])
    return dict(actions=actions, costs=costs, best_actions=actions[best].clone(), result=result)


def views(pl):
    return dict(actions=pl.random_actions, costs=pl.random_costs, best_actions=pl.random_best_actions, result=pl.random_result)


def fused_step(pl, obs, offset, freq, u=None, first=0):
    ex = pl.plan_step_random(obs, offset, freq, u, first)
    assert ex.data_ptr() == pl.random_result.data_ptr()
    return views(pl)


def observation(o, s):
    return 0.1 * np.random.RandomState(100 + s).randn(o)


def assert_same_bits(got, want, where):
    torch.cuda.synchronize()
    for k in NAMES:
        assert got[k].dtype == want[k].dtype and bits(got[k]) == bits(want[k]), (where, k)


def run_against_the_chain(pl, o, freq, steps=STEPS, start=0):
    assert pl.random_step_ok()
    per_step = pl.cfg.num_traj * pl.h
    for s in range(steps):
        obs, off = observation(o, s), start + s * per_step
        want = chain_step(pl, obs, off, freq)
        got = fused_step(pl, obs, off, freq)
        assert_same_bits(got, want, (freq, s))
        assert pl.random_step_launches == 3
    return pl


def _fpp(N, **kw):
    from icem_amd import fetch_pick_and_place_env
    env = fetch_pick_and_place_env()
    return planner("f32", N, 30, env.action_space.shape[0], env.obs_dim, 0, spec=env.cost_spec, low=-1.0, high=1.0, **kw)


def _reacher64(N, **kw):
    from icem_amd import reacher_env
    env = reacher_env()
    return planner("f64", N, 30, 2, env.obs_dim, 0, spec=env.cost_spec, **kw)


# one shape per rollout family: name -> (make(N, **kw), horizon)
FAMILIES = {
    "f32 tile, linear model": (lambda N, **kw: planner("f32", N, 30, 6, 17, 0, **kw), 30),
    "f32 tile, tanh model": (lambda N, **kw: planner("f32", N, 30, 6, 17, 1, **kw), 30),
    "f32 tile h12": (lambda N, **kw: planner("f32", N, 12, 6, 17, 1, **kw), 12),
    "f32 FetchPickAndPlace on TileHN": (_fpp, 30),
    "f32 GEMM kernel o = 40": (lambda N, **kw: planner("f32", N, 12, 5, 40, 1, **kw), 12),
    "f32 narrow generic shape": (lambda N, **kw: planner("f32", N, 13, 3, 11, 1, **kw), 13),
    "f64 chain o = 17": (lambda N, **kw: planner("f64", N, 30, 6, 17, 0, **kw), 30),
    "f64 term list": (_reacher64, 30),
}
POOLS = (2, 17, 100, 4096)


@pytest.mark.parametrize("N", POOLS)
@pytest.mark.parametrize("name", list(FAMILIES))
def test_the_fused_step_equals_the_operator_chain_bit_for_bit(name, N):
    make, h = FAMILIES[name]
    pl = make(N)
    start = 0
    for freq in (0, 1, 3, h - 1):
        run_against_the_chain(pl, pl.obs_dim, freq, start=start)
        start += STEPS * N * h + 1   # (a counter that has run on: the next hold length starts off any block's edge)
    if name == "f32 FetchPickAndPlace on TileHN":
        assert pl.cfg.act_dim == 4


@pytest.mark.parametrize("rounds", [7, 10])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_both_generators_and_a_large_call_offset(dtype, rounds):
    """rng_rounds 7 and 10, and a counter past 2^32 sample() calls (the block index no longer fits 32 bits)."""
    pl = planner(dtype, 100, 30, 6, 17, 0, rounds=rounds)
    run_against_the_chain(pl, 17, 3)
    run_against_the_chain(pl, 17, 4, steps=1, start=(1 << 35) + 12345)


@pytest.mark.parametrize("mode", ["sum", "best", "final"])
def test_all_three_cost_modes(mode):
    run_against_the_chain(planner("f32", 100, 30, 6, 17, 0, mode=mode), 17, 3)


def test_exact_tile_arithmetic_and_the_generic_top_k():
    """The exact-f32 tile kernels; and a pool above the f32 one-launch top-k's 16 384 rows, where ``icem_topk_sorted`` is the generic
    pair of launches (its cost is reported as it stands) and the selection launch has two workgroups."""
    run_against_the_chain(planner("f32", 100, 30, 6, 17, 0, tile="f32"), 17, 3)
    run_against_the_chain(planner("f32", 16500, 12, 6, 17, 1), 17, 5, steps=2)
    run_against_the_chain(planner("f64", 16500, 12, 6, 17, 1), 17, 5, steps=2)


# ---- the planted minimum: the selection launch at every slice edge -------------------------------------------------------------
def _slice():
    src = open(os.path.join(ROOT, "icem_amd", "csrc", "random_step.h")).read()
    return int(re.search(r"constexpr int RANDOM_SLICE = (\d+);", src).group(1))


SLICE = _slice()
PLANTED = {N: (0, 1, N // 2, N - 2, N - 1) for N in (2, 63, 64, 65, 1023, 1025, 65536)}
# the selection kernel's own edges: pools that end one row before, at and one row behind a slice; rows on both sides of every edge
PLANTED.update({N: (0, SLICE - 1, min(SLICE, N - 1), N - 1) for N in (SLICE - 1, SLICE, SLICE + 1, 2 * SLICE + 1)})
PLANTED[65536] += tuple(k * SLICE + e for k in range(1, 65536 // SLICE) for e in (-1, 0))
PLANTED_H = 5


def _zero_model(o, d):
    from icem_amd import DeviceSyntheticModel
    return DeviceSyntheticModel(np.zeros((o, o)), np.zeros((d, o)), 0)


def _block(c, freq):
    return 0 if c < freq else 1 + (c - freq) // (freq + 1)


@pytest.mark.parametrize("dtype,N", [("f32", N) for N in PLANTED] + [("f64", 1025), ("f64", 2 * SLICE + 1)])
def test_a_planted_minimum_is_found_at_every_slice_edge(dtype, N):
    """Zero model, HalfCheetah cost, bounds +-1, a hold of h calls: u = 1 everywhere (action 1: cost 0.1 * d per step) but 0.5 on
    the two blocks that cover row r of step s (action 0).  Row r costs 0 exactly; its neighbours share one of its blocks each and
    cost at least one step of 0.1 * d = 0.6; everyone else h * 0.6."""
    h, d, o, freq = PLANTED_H, 6, 17, PLANTED_H - 1
    pl = planner(dtype, N, h, d, o, 0, model=_zero_model(o, d), low=-1.0, high=1.0)
    pl.set_cost()   # HalfCheetah's
    obs = np.zeros(o)
    rows = sorted(set(r for r in PLANTED.get(N, (0, 1, SLICE - 1, SLICE, N - 1)) if 0 <= r < N))
    for s in range(3):
        off = s * N * h
        first, last = _block(off, freq), _block(off + N * h - 1, freq)
        for r in rows:
            u = np.ones((last - first + 1, d))
            for c in (off + r * h, off + r * h + h - 1):
                u[_block(c, freq) - first] = 0.5
            got = fused_step(pl, obs, off, freq, u, first)
            torch.cuda.synchronize()
            res, costs = np_(got["result"]), np_(got["costs"])
            assert int(res[-1]) == r == int(np.argmin(costs)), (s, r, res)
            assert (res[:d] == 0).all() and res[d] == 0 and costs[r] == 0, (s, r, res)
            assert (np_(got["best_actions"]) == 0).all(), (s, r)
            assert np.partition(costs, 1)[1] >= 0.5, (s, r)


# ---- ties and non-finite costs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,N", [("f32", 100), ("f32", 2 * SLICE + 7), ("f64", 100), ("f64", 2 * SLICE + 7)])
def test_a_pool_of_equal_rows_selects_row_zero(dtype, N):
    h, d, o, freq = 12, 6, 17, 3
    pl = planner(dtype, N, h, d, o, 1)
    n_blocks = _block(N * h - 1, freq) + 1
    u = np.full((n_blocks, d), 0.3)
    obs = observation(o, 0)
    want, got = chain_step(pl, obs, 0, freq, u, 0), fused_step(pl, obs, 0, freq, u, 0)
    assert_same_bits(got, want, "ties")
    assert int(np_(got["result"])[-1]) == 0 and len(np.unique(np_(got["costs"]))) == 1


@pytest.mark.parametrize("dtype,N", [("f32", 100), ("f32", 2 * SLICE + 7), ("f64", 100), ("f64", 2 * SLICE + 7)])
@pytest.mark.parametrize("bad", ["nan", "inf"])
def test_non_finite_costs_go_the_way_of_the_operators(dtype, N, bad):
    """An observation of NaN / +inf: every cost of the pool is non-finite and the chain's answer (row 0 at +inf where all are NaN)
    is the step's.  Then NaN uniforms on the blocks of the pool's first half: those rows cost NaN and count as +inf -- the best row
    lies in the second half."""
    h, d, o, freq = 12, 6, 17, 3
    pl = planner(dtype, N, h, d, o, 0)
    obs = np.full(o, np.nan if bad == "nan" else np.inf)
    want, got = chain_step(pl, obs, 0, freq), fused_step(pl, obs, 0, freq)
    assert_same_bits(got, want, bad)
    assert not np.isfinite(np_(got["costs"])).any()
    n_blocks = _block(N * h - 1, freq) + 1
    u = np.random.RandomState(3).uniform(size=(n_blocks, d))
    u[:n_blocks // 2] = np.nan
    obs = observation(o, 1)
    want, got = chain_step(pl, obs, 0, freq, u, 0), fused_step(pl, obs, 0, freq, u, 0)
    assert_same_bits(got, want, "half nan")
    costs = np_(got["costs"])
    assert np.isnan(costs[:N // 2 - 1]).all() and int(np_(got["result"])[-1]) >= N // 2 - 1
    assert np.isfinite(np_(got["result"])).all()


# ---- the controller -----------------------------------------------------------------------------------------------------------
def controller(fused_step, dtype="f32", N=250, freq=4, seed=3, **kw):
    from icem_amd import DeviceSyntheticModel, MpcRandomHip
    from icem_amd.envs import CostSpec, SyntheticEnv
    env = SyntheticEnv("HalfCheetah", 17, LOW * np.ones(6), HIGH * np.ones(6), CostSpec(0.1, 8, -1.0, 1, 10.0, 0.3))
    return MpcRandomHip(env=env, forward_model=DeviceSyntheticModel.make(17, 6, kind=0, seed_a=11, seed_b=12), horizon=30,
                        num_simulated_trajectories=N, cost_along_trajectory="sum", verbose=False, dtype=dtype, seed=seed,
                        fused_step=fused_step, action_sampler_params=dict(action_change_frequency=freq), **kw)


def same_controllers(a, b, where):
    assert a.calls == b.calls and a.best_traj_idx == b.best_traj_idx and a.last_min_cost == b.last_min_cost, where
    assert bits(a._last_actions) == bits(b._last_actions) and bits(a._last_costs) == bits(b._last_costs), where


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_the_controller_on_the_fused_step_equals_the_controller_on_the_chain(dtype):
    a, b, c = (controller(f, dtype) for f in (True, False, None))
    for ctrl in (a, b, c):
        ctrl.beginning_of_rollout(observation=observation(17, 0), state=None, mode="train")
    for s in range(5):
        obs = observation(17, s)
        x, y, z = (ctrl.get_action(obs, None) for ctrl in (a, b, c))
        assert x.dtype == y.dtype == np.float64 and np.array_equal(x, y) and np.array_equal(z, y), s
        same_controllers(a, b, s)
        same_controllers(c, b, s)
        assert a.calls == (s + 1) * 250 * 30
    assert a.planner.random_step_launches == 3 and b.planner.random_step_launches == 0
    assert (c.planner.random_step_launches == 3) == (c._fused_step_refusal() is None)


def test_the_fused_f64_controller_matches_the_oracle_on_the_same_uniforms():
    """tests/test_gpu_parity.py::test_random_shooting_device_rng_matches_oracle, at its f64 tolerances, with the controller forced
    onto the fused entry."""
    from icem_amd import DeviceSyntheticModel, MpcRandomHip, halfcheetah_env
    env = halfcheetah_env(17)
    model = DeviceSyntheticModel.make(17, 6, kind=1)
    N, h, freq, seed = 3000, 30, 4, 17
    ctrl = MpcRandomHip(env=env, forward_model=model, horizon=h, num_simulated_trajectories=N, cost_along_trajectory="sum",
                        dtype="f64", seed=seed, fused_step=True, action_sampler_params=dict(action_change_frequency=freq))
    om, oc = O.SyntheticModel(model.A, model.B, model.kind), O.CostSpec.halfcheetah(17)
    orc = O.RandomShootingOracle(horizon=h, num_traj=N, freq=freq, low=env.action_space.low, high=env.action_space.high,
                                 rollout_cost=lambda ob, ac: O.rollout_costs(om, oc, ob, ac),
                                 uniforms=lambda b0, nb: O.philox_block_uniforms(seed, b0, nb, 6, dtype=np.float64))
    ctrl.beginning_of_rollout(observation=np.zeros(17), state=None, mode="train")
    t = dict(rtol=1e-12, atol=1e-13)
    for s in range(3):
        ob = 0.1 * np.random.RandomState(s).randn(17)
        a, want = ctrl.get_action(ob, None), orc.get_action(ob)
        np.testing.assert_allclose(np_(ctrl._last_actions), orc.actions, **t)
        assert ctrl.best_traj_idx == orc.best
        np.testing.assert_allclose(a, want, **t)
        np.testing.assert_allclose(ctrl.last_min_cost, orc.costs[orc.best], rtol=1e-10, atol=1e-12)
        assert ctrl.planner.random_step_launches == 3


@pytest.mark.parametrize("dtype,N", [("f32", 250), ("f64", 250), ("f32", 2 * SLICE + 7)])
def test_a_captured_step_replays_to_the_same_bits(dtype, N):
    """One warm-up step outside the capture (the rollout's model upload, the selection's words), then the next step captured on a
    side stream: nothing in the call synchronises or allocates, and the replay leaves what the chain leaves for that step."""
    h, freq = 12, 3
    pl, twin = planner(dtype, N, h, 6, 17, 1), planner(dtype, N, h, 6, 17, 1)
    obs = [torch.as_tensor(observation(17, s), dtype=pl.dt, device=pl.device) for s in range(2)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fused_step(pl, obs[0], 0, freq)
        side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        got = fused_step(pl, obs[1], N * h, freq)
    assert pl.random_step_launches == 3
    torch.cuda.synchronize()
    for _ in range(2):   # (the selection leaves its ticket as it found it: a second replay is the first)
        g.replay()
        torch.cuda.synchronize()
        want = chain_step(twin, np_(obs[1]), N * h, freq)
        assert_same_bits(got, want, "replay")


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def _snapshot(pl):
    return [bits(x) for x in views(pl).values()] + [pl.random_step_launches, pl.random_batch_launches, pl.batch_uploads]


def _raw(pl, obs_t, *, freq=3, offset=0, null=None):
    """The C entry on the planner's own buffers with the arguments bent as a refusal case needs them."""
    from icem_amd import _lib as L
    cb = L.IcemRandomBuffersC.from_buffer_copy(pl._random_cb(obs_t))
    if null:
        setattr(cb, null, None)
    L.check(pl.lib.icem_plan_step_random(pl._h, C.byref(cb), freq, offset, 0, None, pl._stream()))


ARGUMENTS = {
    "a negative change_freq": dict(freq=-1), "change_freq = horizon": dict(freq=12), "a negative call_offset": dict(offset=-1),
    "a null pool": dict(null="actions"), "a null result": dict(null="result"), "a null observation": dict(null="obs0"),
}


@pytest.mark.parametrize("case", list(ARGUMENTS))
def test_a_bad_argument_is_invalid_and_touches_nothing(case):
    from icem_amd import _lib as L
    pl = planner("f32", 100, 12, 6, 17, 1)
    obs = torch.as_tensor(observation(17, 0), dtype=pl.dt, device=pl.device)
    fused_step(pl, obs, 0, 3)   # a served step first: the buffers hold something a refused step could spoil
    torch.cuda.synchronize()
    before = _snapshot(pl)
    with pytest.raises(L.IcemError) as e:
        _raw(pl, obs, **ARGUMENTS[case])
    torch.cuda.synchronize()
    assert e.value.code == L.ICEM_E_INVALID, str(e.value)
    assert _snapshot(pl) == before


def test_a_handle_without_model_or_cost_is_a_state_error():
    from icem_amd import IcemConfig, IcemPlanner
    from icem_amd import _lib as L
    pl = IcemPlanner(IcemConfig(horizon=12, act_dim=6, num_traj=100, elites_size=2, opt_iters=1), LOW * np.ones(6), HIGH * np.ones(6))
    new = lambda *shape: torch.zeros(shape, dtype=pl.dt, device=pl.device)   # noqa: E731
    bufs = dict(obs0=new(17), actions=new(100, 12, 6), costs=new(100), best_actions=new(12, 6), result=new(8))
    cb = L.IcemRandomBuffersC(low=pl.low.data_ptr(), high=pl.high.data_ptr(), **{k: v.data_ptr() for k, v in bufs.items()})
    assert pl.random_step_ok()   # (the handle's configuration is served: what is missing is state)
    with pytest.raises(L.IcemError) as e:
        L.check(pl.lib.icem_plan_step_random(pl._h, C.byref(cb), 3, 0, 0, None, pl._stream()))
    torch.cuda.synchronize()
    assert e.value.code == L.ICEM_E_STATE and pl.random_step_launches == 0
    assert all(not np_(v).any() for v in bufs.values())


UNSERVED = ["option", "profiling", "sharded"]


def _unserved_planner(case, **kw):
    pl = planner("f32", 250, 30, 6, 17, 0, **(dict(world=2) if case == "sharded" else {}), **kw)
    if case == "profiling":
        pl.profile_enable(True)
    return pl


@pytest.mark.parametrize("case", UNSERVED)
def test_an_unserved_handle_is_refused_untouched_and_the_controller_falls_back_to_the_chain(case):
    from icem_amd import _lib as L
    try:
        if case == "option":
            L.set_option("random_step", 0)
        pl = _unserved_planner(case)
        assert not pl.random_step_ok()
        obs = observation(17, 0)
        for v in views(pl).values():
            v.fill_(0.25)   # (something a refused step could spoil)
        torch.cuda.synchronize()
        before = _snapshot(pl)
        with pytest.raises(L.IcemError) as e:
            pl.plan_step_random(obs, 0, 4)
        torch.cuda.synchronize()
        assert e.value.code == L.ICEM_E_UNSUPPORTED, str(e.value)
        assert _snapshot(pl) == before and pl.random_step_launches == 0
        # the controller: fused_step=None runs the chain on such a handle and gives the chain's result; True raises
        a, b, t = controller(None), controller(False), controller(True)
        for c in (a, t):
            if case == "sharded":
                c.planner = _unserved_planner(case, seed=3)
                c._bind_models()
            if case == "profiling":
                c.planner.profile_enable(True)
        assert not a.planner.random_step_ok() and a._fused_step_refusal() is not None
        for c in (a, b, t):
            c.beginning_of_rollout(observation=obs, state=None, mode="train")
        if case != "sharded":   # (a sharded handle's operators draw the same pool: the chain's results are the twin's)
            for s in range(2):
                ob = observation(17, s)
                assert np.array_equal(a.get_action(ob, None), b.get_action(ob, None))
                same_controllers(a, b, s)
        assert a.planner.random_step_launches == 0
        with pytest.raises(RuntimeError, match="fused_step=True"):
            t.get_action(obs, None)
        assert t.calls == 0
    finally:
        L.reset_options()


def test_fused_step_true_raises_on_external_uniforms():
    u = controller(True, noise_source=lambda first, n: np.full((n, 6), 0.5))
    obs = observation(17, 0)
    u.beginning_of_rollout(observation=obs, state=None, mode="train")
    with pytest.raises(RuntimeError, match="noise source"):
        u.get_action(obs, None)
    with pytest.raises(ValueError):
        controller("yes")
