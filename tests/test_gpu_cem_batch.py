"""``icem_plan_step_cem_batch`` (cem_step.hip, k_cem.hip, k_rollout.hip): the CEM baseline's MPC step for B planners in one library
call -- 3 launches per CEM iteration whatever B -- held bit for bit to ``icem_plan_step_cem``: every problem of a batch has a solo
twin on the same seed and episode (seeds differ across problems), each problem gets an observation of its own on every step, and
after each of 3 MPC steps ``array_equal`` holds on all eleven buffers of every problem (executed, best cost, mean, std, lower, upper,
the elite set, its costs and indices, the last pool and its costs) and on the batch's ``results`` rows against executed | best_cost.
Bounds are asymmetric (low = -0.7, high = 0.9) as in tests/test_gpu_cem_step.py, whose helpers are used.  Both sides run the same
device code (the batched kernels call the solo kernels' bodies), so every comparison is an exact equality."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from test_gpu_cem_step import Dist, controller, fused_step, np_, observation, planner

pytestmark = pytest.mark.gpu

STEPS = 3
FLAGS = (False, True, True)   # like_levine, shift_means, execute_best_elite
NAMES = ("executed", "best_cost", "mean", "std", "lower", "upper", "elites", "elite_costs", "elite_idx", "actions", "costs")


def views(pl, s):
    """The eleven buffers of one problem."""
    return dict(executed=pl.cem_result[:pl.d], best_cost=pl.cem_result[pl.d:], mean=s.mean, std=s.std, lower=s.lower, upper=s.upper,
                elites=pl.cem_elites, elite_costs=pl.cem_elite_costs, elite_idx=pl.cem_elite_idx, actions=pl.cem_actions, costs=pl.cem_costs)


def obs_of(o, problem, step):
    return observation(o, 1000 * problem + step)


class Group:
    """B planners (seed 5 + i) with their distributions: a batch, or its solo twins."""

    def __init__(self, make, B, like_levine=False):
        self.pls = [make(seed=5 + i) for i in range(B)]
        self.dists = [Dist(pl, like_levine) for pl in self.pls]

    def step_batch(self, obs, flags=FLAGS):
        from icem_amd import IcemPlanner
        return IcemPlanner.plan_step_cem_batch(self.pls, obs, [(s.mean, s.std, s.lower, s.upper) for s in self.dists],
                                               like_levine=flags[0], shift_means=flags[1], execute_best_elite=flags[2])

    def step_solo(self, obs, flags=FLAGS, only=None):
        for i, (pl, s) in enumerate(zip(self.pls, self.dists)):
            if only is None or i in only:
                fused_step(pl, s, obs[i], *flags)

    def new_episode(self, i, like_levine=False):
        self.pls[i].new_episode()
        self.dists[i] = Dist(self.pls[i], like_levine)


def assert_equal(batch, twins, where, results=None):
    torch.cuda.synchronize()
    for i, (pb, sb, pt, st) in enumerate(zip(batch.pls, batch.dists, twins.pls, twins.dists)):
        got, want = views(pb, sb), views(pt, st)
        assert set(got) == set(NAMES)
        for k in NAMES:
            assert np.array_equal(np_(got[k]), np_(want[k])), (where, i, k)
        assert pb.mpc_step == pt.mpc_step, (where, i)
        if results is not None:
            row = np.concatenate([np_(want["executed"]), np_(want["best_cost"])])
            assert np.array_equal(np_(results[i]), row), (where, i, "results")


def run_against_the_twins(make, o, B, flags=FLAGS, steps=STEPS):
    batch, twins = Group(make, B, flags[0]), Group(make, B, flags[0])
    iters = batch.pls[0].cfg.opt_iters
    for s in range(steps):
        obs = [obs_of(o, i, s) for i in range(B)]
        ex = batch.step_batch(obs, flags)
        twins.step_solo(obs, flags)
        assert_equal(batch, twins, s, batch.pls[0].cem_batch_results)
        assert np.array_equal(np_(ex), np_(batch.pls[0].cem_batch_results[:, :-1]))
        # 3 launches per iteration whatever B (the GEMM path's row tail needs shifted rows, which a CEM step never has)
        assert batch.pls[0].cem_batch_launches == 3 * iters
    # problems of one batch differ (seeds and observations of their own)
    if B > 1:
        assert not np.array_equal(np_(batch.pls[0].cem_actions), np_(batch.pls[1].cem_actions))
    return batch


def _tile_f32(make):
    def made(**kw):
        pl = make(**kw)
        assert pl.set_tile_arith("f32") == 0
        return pl
    return made


def _door(**kw):
    from icem_amd import door_env
    return planner("f32", 64, 30, 28, 39, 0, spec=door_env().cost_spec, **kw)


# name -> (make(seed=...), observation width)
SHAPES = {
    "f32 tile, default arithmetic": (lambda **kw: planner("f32", 250, 30, 6, 17, 0, **kw), 17),
    "f32 tile, exact f32": (_tile_f32(lambda **kw: planner("f32", 250, 30, 6, 17, 0, **kw)), 17),
    "f32 two-tile shape, waves capped at 8": (lambda **kw: planner("f32", 100, 30, 17, 24, 1, **kw), 24),
    "f32 rng_rounds 7": (lambda **kw: planner("f32", 120, 13, 4, 17, 1, rounds=7, **kw), 17),
    "f32 GEMM kernel, exact f32": (lambda **kw: planner("f32", 96, 12, 5, 40, 1, wide="f32", **kw), 40),
    "f32 Door on TileHN": (_door, 39),
    # (a narrow shape no tile kernel serves rolls out on the exact-f32 GEMM kernel in f32: it has a batched twin.  The f32
    #  thread-per-trajectory kernel is reached only with the fast path off, which the solo entry refuses already)
    "f32 narrow shape on the GEMM kernel": (lambda **kw: planner("f32", 64, 12, 4, 8, 1, **kw), 8),
    "f64 rows rollout": (lambda **kw: planner("f64", 250, 30, 6, 17, 0, **kw), 17),
    "f64 narrow tanh": (lambda **kw: planner("f64", 64, 12, 4, 8, 1, **kw), 8),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_a_batch_of_three_equals_its_solo_twins_bit_for_bit(name):
    make, o = SHAPES[name]
    batch = run_against_the_twins(make, o, 3)
    if name == "f32 tile, default arithmetic":
        assert batch.pls[0].tile_arith == 1   # (the other arithmetic is the next case)
    if name == "f32 Door on TileHN":
        assert batch.pls[0].cfg.act_dim == 28


def test_a_pool_above_4096_keys():
    run_against_the_twins(lambda **kw: planner("f32", 4500, 30, 6, 17, 0, **kw), 17, 2)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("like_levine,shift_means,execute_best_elite", list(itertools.product((False, True), repeat=3)))
def test_every_flag_combination(dtype, like_levine, shift_means, execute_best_elite):
    run_against_the_twins(lambda **kw: planner(dtype, 250, 30, 6, 17, 0, **kw), 17, 2, (like_levine, shift_means, execute_best_elite))


@pytest.mark.parametrize("what", [dict(K=2), dict(K=32), dict(alpha=0.0), dict(alpha=0.9), dict(mode="best"), dict(mode="final")])
def test_elite_counts_momentum_and_cost_modes(what):
    batch = run_against_the_twins(lambda **kw: planner("f32", 250, 30, 6, 17, 0, **what, **kw), 17, 2)
    if "K" in what:
        assert batch.pls[0].K == what["K"]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_a_batch_of_one_equals_the_solo_entry(dtype):
    run_against_the_twins(lambda **kw: planner(dtype, 250, 30, 6, 17, 0, **kw), 17, 1)


def test_a_batch_of_thirty_two():
    run_against_the_twins(lambda **kw: planner("f32", 64, 12, 6, 17, 0, **kw), 17, 32, steps=2)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_a_problem_that_was_reset_later_steps_with_its_neighbours(dtype):
    """Problem 1 begins a new episode after step 1: from then on its mpc_steps_host entry and its episode differ from its neighbours'."""
    make = lambda **kw: planner(dtype, 250, 30, 6, 17, 0, **kw)   # noqa: E731
    batch, twins = Group(make, 3), Group(make, 3)
    for s in range(4):
        if s == 2:
            batch.new_episode(1)
            twins.new_episode(1)
        obs = [obs_of(17, i, s) for i in range(3)]
        batch.step_batch(obs)
        twins.step_solo(obs)
        assert_equal(batch, twins, s, batch.pls[0].cem_batch_results)
    assert [pl.mpc_step for pl in batch.pls] == [4, 2, 4] and [pl.episode for pl in batch.pls] == [0, 1, 0]


def test_a_planner_may_alternate_between_batched_and_solo_steps():
    make = lambda **kw: planner("f32", 250, 30, 6, 17, 0, **kw)   # noqa: E731
    batch, twins = Group(make, 2), Group(make, 2)
    for s in range(4):
        obs = [obs_of(17, i, s) for i in range(2)]
        if s % 2 == 0:
            batch.step_batch(obs)
        else:
            batch.step_solo(obs)
        twins.step_solo(obs)
        assert_equal(batch, twins, s)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_a_steady_batch_uploads_each_slot_once(dtype):
    make = lambda **kw: planner(dtype, 250, 30, 6, 17, 0, **kw)   # noqa: E731
    batch = Group(make, 3)
    seen = []
    for s in range(5):
        batch.step_batch([obs_of(17, i, s) for i in range(3)])
        seen.append(batch.pls[0].batch_uploads)
    assert seen == [1, 2, 2, 2, 2]
    assert all(pl.batch_uploads == 0 for pl in batch.pls[1:])


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_a_captured_batch_replays_to_the_same_bits(dtype):
    """Two warm steps outside the capture (the model uploads, both argument slots, the results tensor), then step 2 captured on a side
    stream: nothing in the call synchronises, uploads or allocates, and the replay leaves what the eager twins' step 2 leaves."""
    make = lambda **kw: planner(dtype, 250, 30, 6, 17, 0, **kw)   # noqa: E731
    batch, twins = Group(make, 3), Group(make, 3)
    dev, dt = batch.pls[0].device, batch.pls[0].dt
    obs = [[torch.as_tensor(obs_of(17, i, s), dtype=dt, device=dev) for i in range(3)] for s in range(3)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        batch.step_batch(obs[0])
        batch.step_batch(obs[1])
        side.synchronize()
    uploads = batch.pls[0].batch_uploads
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        batch.step_batch(obs[2])
    assert batch.pls[0].batch_uploads == uploads and batch.pls[0].cem_batch_launches == 9
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for s in range(3):
        twins.step_solo([np_(x) for x in obs[s]])
    assert_equal(batch, twins, "replay", batch.pls[0].cem_batch_results)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def _snapshot(g):
    out = []
    for pl, s in zip(g.pls, g.dists):
        out += [np_(x).copy() for x in views(pl, s).values()] + [np.array([pl.mpc_step, pl.cem_batch_launches, pl.cem_step_launches, pl.batch_uploads])]
    return out


def _raw_call(g, obs, *, n=None, handles=None, steps=None, edit=None):
    """The C entry on the group's planners with the arguments bent as a refusal case needs them."""
    from icem_amd import _lib as L
    pls = g.pls
    cbs = [L.IcemCemBuffersC.from_buffer_copy(pl._cem_cb(ob, s.mean, s.std, s.lower, s.upper)) for pl, ob, s in zip(pls, obs, g.dists)]
    if edit:
        edit(cbs)
    hs = [pl._h for pl in pls] if handles is None else handles
    n = len(hs) if n is None else n
    hs_c = (C.c_void_p * max(1, len(hs)))(*hs)
    bs = (L.IcemCemBuffersC * max(1, len(cbs)))(*cbs)
    st = [pl.mpc_step for pl in pls] if steps is None else steps
    st_c = (C.c_int32 * max(1, len(st), n))(*st)
    prm = L.IcemCemParamsC(0, 1, 1, 0)
    res = torch.zeros((max(1, len(pls)), pls[0].d + 1), dtype=pls[0].dt, device=pls[0].device)
    L.check(pls[0].lib.icem_plan_step_cem_batch(hs_c, n, bs, C.byref(prm), st_c, C.c_void_p(res.data_ptr()), pls[0]._stream()))


def _tile(**kw):
    return planner("f32", 250, 30, 6, 17, 0, **kw)


def _null_costs(cbs):
    cbs[1].costs = None


# case -> (make(i, seed=...) of problem i, the call's bent arguments(group), the code)
REFUSALS = {
    "n = 0": (lambda i, **kw: _tile(**kw), lambda g: dict(n=0), "ICEM_E_INVALID"),
    "n = 33": (lambda i, **kw: _tile(**kw), lambda g: dict(n=33, handles=[g.pls[k % 2]._h for k in range(33)]), "ICEM_E_INVALID"),
    "a null handle": (lambda i, **kw: _tile(**kw), lambda g: dict(handles=[g.pls[0]._h, None]), "ICEM_E_INVALID"),
    "the same handle twice": (lambda i, **kw: _tile(**kw), lambda g: dict(handles=[g.pls[0]._h, g.pls[0]._h]), "ICEM_E_INVALID"),
    "another num_traj": (lambda i, **kw: planner("f32", 250 + 16 * i, 30, 6, 17, 0, **kw), lambda g: {}, "ICEM_E_INVALID"),
    # (the problems' rollout launches differ: the code and wording of icem_plan_step_batch for unequal keys)
    "another tile arithmetic": (lambda i, **kw: (_tile_f32(_tile) if i else _tile)(**kw), lambda g: {}, "ICEM_E_STATE"),
    "keep_previous_elites": (lambda i, **kw: _tile(keep_previous_elites=True, **kw), lambda g: {}, "ICEM_E_UNSUPPORTED"),
    "option cem_step = 0": (lambda i, **kw: _tile(**kw), lambda g: {}, "ICEM_E_UNSUPPORTED"),
    "a NULL buffer": (lambda i, **kw: _tile(**kw), lambda g: dict(edit=_null_costs), "ICEM_E_INVALID"),
    "a negative step": (lambda i, **kw: _tile(**kw), lambda g: dict(steps=[0, -1]), "ICEM_E_INVALID"),
    "profiling on": (lambda i, **kw: _tile(**kw), lambda g: {}, "ICEM_E_UNSUPPORTED"),
    # h * d = 3072 doubles: the sampler's three tables and one row would need 96 KB of LDS (cem_sample_ok false; the solo step draws
    # with the operator's kernel, which has no batched twin)
    "a row that does not fit the sampler": (lambda i, **kw: planner("f64", 64, 64, 48, 8, 1, **kw), lambda g: {}, "ICEM_E_UNSUPPORTED"),
    # a rollout without a batched form: the float64 matrix-core rollout
    "the f64 matrix-core rollout": (lambda i, **kw: planner("f64", 96, 12, 5, 40, 1, f64_arith="mfma", **kw), lambda g: {}, "ICEM_E_UNSUPPORTED"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_a_refused_batch_launches_nothing_and_touches_nothing(case):
    from icem_amd import _lib as L
    make, bend, code = REFUSALS[case]
    g = Group.__new__(Group)
    g.pls = [make(i, seed=5 + i) for i in range(2)]
    g.dists = [Dist(pl, False) for pl in g.pls]
    o = g.pls[0].obs_dim
    # a served solo step first where the handle takes one: the buffers hold something a refused batch could spoil
    for i, (pl, s) in enumerate(zip(g.pls, g.dists)):
        if pl.cem_step_ok():
            fused_step(pl, s, obs_of(o, i, 0), *FLAGS)
    try:
        if case == "option cem_step = 0":
            L.set_option("cem_step", 0)
        if case == "profiling on":
            g.pls[1].profile_enable(True)
        torch.cuda.synchronize()
        before = _snapshot(g)
        with pytest.raises(L.IcemError) as e:
            _raw_call(g, [obs_of(o, i, 1) for i in range(2)], **bend(g))
        torch.cuda.synchronize()
        assert e.value.code == getattr(L, code), str(e.value)
        for x, y in zip(_snapshot(g), before):
            assert np.array_equal(x, y)
        if case not in ("n = 0", "n = 33", "a null handle", "the same handle twice", "a NULL buffer", "a negative step"):
            # ... and through the wrapper: no planner has advanced
            with pytest.raises(L.IcemError):
                g.step_batch([obs_of(o, i, 1) for i in range(2)])
            torch.cuda.synchronize()
            for x, y in zip(_snapshot(g), before):
                assert np.array_equal(x, y)
    finally:
        L.reset_options()


# ---- the controllers ----------------------------------------------------------------------------------------------------------
def drive_batch(ctrls, twins, episodes=2, steps=2):
    from icem_amd import MpcCemStdHip
    for ep in range(episodes):
        for s in range(steps):
            obs = [obs_of(17, i, 10 * ep + s) for i in range(len(ctrls))]
            if s == 0:
                for c, ob in zip(itertools.chain(ctrls, twins), obs + obs):
                    c.beginning_of_rollout(observation=ob, state=None, mode="train")
            got = MpcCemStdHip.get_action_batch(ctrls, obs)
            want = [t.get_action(ob, None) for t, ob in zip(twins, obs)]
            for i, (a, b) in enumerate(zip(ctrls, twins)):
                assert np.array_equal(got[i], want[i]), (ep, s, i)
                assert a.last_min_cost == b.last_min_cost and a.planner.mpc_step == b.planner.mpc_step == s + 1
                assert np.array_equal(a.mean, b.mean) and np.array_equal(a.std, b.std)
                assert np.array_equal(np_(a._lower), np_(b._lower)) and np.array_equal(np_(a._upper), np_(b._upper))
                assert np.array_equal(a.elite_samples.as_array("actions"), b.elite_samples.as_array("actions"))
                assert np.array_equal(a.elite_samples.as_array("costs"), b.elite_samples.as_array("costs"))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("like_levine", [False, True])
def test_the_controllers_step_together_as_their_twins_step_alone(dtype, like_levine):
    ctrls = [controller(None, dtype, like_levine=like_levine, seed=3 + i) for i in range(3)]
    twins = [controller(True, dtype, like_levine=like_levine, seed=3 + i) for i in range(3)]
    drive_batch(ctrls, twins)
    assert ctrls[0].planner.cem_batch_launches == 9 and ctrls[0].planner.cem_step_launches == 0


def test_fused_step_true_raises_and_none_falls_back_where_a_controller_is_refused():
    from icem_amd import MpcCemStdHip
    from icem_amd import _lib as L
    try:
        L.set_option("cem_step", 0)
        ctrls = [controller(True, seed=3 + i) for i in range(3)]
        obs = [obs_of(17, i, 0) for i in range(3)]
        for c, ob in zip(ctrls, obs):
            c.beginning_of_rollout(observation=ob, state=None, mode="train")
        with pytest.raises(RuntimeError, match="fused_step=True"):
            MpcCemStdHip.get_action_batch(ctrls, obs)
        assert all(c.planner.mpc_step == 0 for c in ctrls)
        # fused_step=None: every controller's own step, in order -- here the stage-wise loop -- and the twins' results
        ctrls = [controller(None, seed=3 + i) for i in range(3)]
        twins = [controller(False, seed=3 + i) for i in range(3)]
        drive_batch(ctrls, twins, episodes=1)
        assert all(c.planner.cem_batch_launches == 0 and c.planner.cem_step_launches == 0 for c in ctrls)
    finally:
        L.reset_options()
    # controllers that differ in a flag are not one batch: fused_step=None steps them one by one (each on its own fused step)
    ctrls = [controller(None, like_levine=bool(i % 2), seed=3 + i) for i in range(2)]
    twins = [controller(True, like_levine=bool(i % 2), seed=3 + i) for i in range(2)]
    drive_batch(ctrls, twins, episodes=1)
    assert all(c.planner.cem_batch_launches == 0 and c.planner.cem_step_launches == 9 for c in ctrls)
