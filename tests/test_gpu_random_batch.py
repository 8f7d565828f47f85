"""``icem_plan_step_random_batch`` (random_step.hip, k_random.hip): the random-shooting baseline's MPC step for B planners in one
library call -- the solo step's launch count whatever B -- held bit for bit to ``icem_plan_step_random``: every problem of a batch
has a solo twin on the same seed, model and call offset (seeds, models, observations and offsets differ across problems), and after
each of 3 steps the pool, its costs, the best row and ``result`` of every problem, and its row of the batch's ``results``, compare
equal as bytes.  Both sides run the same device code (the batched kernels call the solo kernels' bodies).  The helpers are
tests/test_gpu_random_step.py's."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_random_step import FAMILIES, NAMES, SLICE, bits, controller, fused_step, np_, observation, planner, same_controllers, views

pytestmark = pytest.mark.gpu

STEPS = 3
FREQ = 3


def obs_of(o, problem, step):
    return observation(o, 1000 * problem + step)


class Group:
    """B planners (seed 5 + i, model seed 11 + 2 i) with call counters of their own: a batch, or its solo twins."""

    def __init__(self, make, B, start=None):
        self.pls = [make(seed=5 + i, model_seed=11 + 2 * i) for i in range(B)]
        self.calls = [0 if start is None else start[i] for i in range(B)]
        self.per_step = self.pls[0].cfg.num_traj * self.pls[0].h

    def step_batch(self, obs, freq=FREQ):
        from icem_amd import IcemPlanner
        ex = IcemPlanner.plan_step_random_batch(self.pls, obs, self.calls, freq)
        self.calls = [c + self.per_step for c in self.calls]
        return ex

    def step_solo(self, obs, freq=FREQ):
        for i, pl in enumerate(self.pls):
            fused_step(pl, obs[i], self.calls[i], freq)
            self.calls[i] += self.per_step


def assert_equal(batch, twins, where, results=None):
    torch.cuda.synchronize()
    assert batch.calls == twins.calls
    for i, (pb, pt) in enumerate(zip(batch.pls, twins.pls)):
        got, want = views(pb), views(pt)
        for k in NAMES:
            assert bits(got[k]) == bits(want[k]), (where, i, k)
        if results is not None:
            assert bits(results[i]) == bits(want["result"]), (where, i, "results")


def run_against_the_twins(make, B, freq=FREQ, steps=STEPS, start=None):
    batch, twins = Group(make, B, start), Group(make, B, start)
    o = batch.pls[0].obs_dim
    for s in range(steps):
        obs = [obs_of(o, i, s) for i in range(B)]
        ex = batch.step_batch(obs, freq)
        twins.step_solo(obs, freq)
        res = batch.pls[0].random_batch_results
        assert tuple(res.shape) == (B, batch.pls[0].d + 2) and bits(ex) == bits(res[:, :-2])
        assert_equal(batch, twins, s, res)
        # the solo step's launch count whatever B
        assert batch.pls[0].random_batch_launches == twins.pls[0].random_step_launches == 3
    if B > 1:   # problems of one batch differ (seeds, models and observations of their own)
        assert bits(batch.pls[0].random_actions) != bits(batch.pls[1].random_actions)
        assert bits(batch.pls[0].random_costs) != bits(batch.pls[1].random_costs)
    return batch


def _family(name, N):
    make, h = FAMILIES[name]
    return (lambda **kw: make(N, **kw)), h


@pytest.mark.parametrize("name", list(FAMILIES))
def test_a_batch_of_three_equals_its_solo_twins_bit_for_bit(name):
    make, h = _family(name, 100)
    run_against_the_twins(make, 3, freq=3, start=[0, 7, 12345])
    run_against_the_twins(make, 3, freq=h - 1, steps=1, start=[5, 0, 1])


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_a_batch_of_one_equals_the_solo_entry(dtype):
    run_against_the_twins(lambda **kw: planner(dtype, 250, 30, 6, 17, 0, **kw), 1)


def test_a_batch_of_thirty_two():
    run_against_the_twins(lambda **kw: planner("f32", 64, 12, 6, 17, 0, **kw), 32, steps=2)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_pools_of_several_selection_slices(dtype):
    """Every problem's selection has three workgroups and a ticket of its own."""
    run_against_the_twins(lambda **kw: planner(dtype, 2 * SLICE + 7, 12, 6, 17, 1, **kw), 3, steps=2)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_a_problem_that_was_reset_later_steps_with_its_neighbours(dtype):
    """Problem 1 starts over after step 1 (a controller built later): from then on its call offset differs from its neighbours'."""
    make = lambda **kw: planner(dtype, 250, 30, 6, 17, 0, **kw)   # noqa: E731
    batch, twins = Group(make, 3), Group(make, 3)
    for s in range(4):
        if s == 2:
            batch.calls[1] = twins.calls[1] = 0
        obs = [obs_of(17, i, s) for i in range(3)]
        batch.step_batch(obs)
        twins.step_solo(obs)
        assert_equal(batch, twins, s, batch.pls[0].random_batch_results)
    assert batch.calls == [4 * 7500, 2 * 7500, 4 * 7500]


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
def test_a_steady_batch_uploads_its_blocks_once(dtype):
    """The call offsets travel by value: nothing in the blocks changes from step to step."""
    batch = Group(lambda **kw: planner(dtype, 250, 30, 6, 17, 0, **kw), 3)
    seen = []
    for s in range(5):
        batch.step_batch([obs_of(17, i, s) for i in range(3)])
        seen.append(batch.pls[0].batch_uploads)
    assert seen == [1, 1, 1, 1, 1]
    assert all(pl.batch_uploads == 0 for pl in batch.pls[1:])


@pytest.mark.parametrize("dtype,N", [("f32", 250), ("f64", 250), ("f32", 2 * SLICE + 7)])
def test_a_captured_batch_replays_to_the_same_bits(dtype, N):
    """One warm step outside the capture (the model uploads, the argument blocks, the results tensor), then step 1 captured on a
    side stream: nothing in the call synchronises, uploads or allocates, and the replay leaves what the eager twins' step 1 leaves."""
    make = lambda **kw: planner(dtype, N, 12, 6, 17, 1, **kw)   # noqa: E731
    batch, twins = Group(make, 3), Group(make, 3)
    dev, dt = batch.pls[0].device, batch.pls[0].dt
    obs = [[torch.as_tensor(obs_of(17, i, s), dtype=dt, device=dev) for i in range(3)] for s in range(2)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        batch.step_batch(obs[0])
        side.synchronize()
    uploads = batch.pls[0].batch_uploads
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        batch.step_batch(obs[1])
    assert batch.pls[0].batch_uploads == uploads == 1 and batch.pls[0].random_batch_launches == 3
    torch.cuda.synchronize()
    for s in range(2):
        twins.step_solo([np_(x) for x in obs[s]])
    for _ in range(2):
        g.replay()
        assert_equal(batch, twins, "replay", batch.pls[0].random_batch_results)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def _snapshot(g):
    out = []
    for pl in g.pls:
        out += [bits(x) for x in views(pl).values()] + [pl.random_step_launches, pl.random_batch_launches, pl.batch_uploads]
    return out


def _raw_call(g, obs, *, n=None, handles=None, offsets=None, freq=FREQ, edit=None):
    """The C entry on the group's planners with the arguments bent as a refusal case needs them."""
    from icem_amd import _lib as L
    pls = g.pls
    cbs = [L.IcemRandomBuffersC.from_buffer_copy(pl._random_cb(ob)) for pl, ob in zip(pls, obs)]
    if edit:
        edit(cbs)
    hs = [pl._h for pl in pls] if handles is None else handles
    n = len(hs) if n is None else n
    hs_c = (C.c_void_p * max(1, len(hs)))(*hs)
    bs = (L.IcemRandomBuffersC * max(1, len(cbs), n))(*cbs)
    offs = list(g.calls) if offsets is None else offsets
    offs_c = (C.c_int64 * max(1, len(offs), n))(*offs)
    res = torch.zeros((max(1, len(pls)), pls[0].d + 2), dtype=pls[0].dt, device=pls[0].device)
    L.check(pls[0].lib.icem_plan_step_random_batch(hs_c, n, bs, freq, offs_c, C.c_void_p(res.data_ptr()), pls[0]._stream()))


def _tile(**kw):
    return planner("f32", 250, 30, 6, 17, 0, **kw)


def _tile_f32(**kw):
    return planner("f32", 250, 30, 6, 17, 0, tile="f32", **kw)


def _null_costs(cbs):
    cbs[1].costs = None


# case -> (make(i, seed=...) of problem i, the call's bent arguments(group), the code)
REFUSALS = {
    "n = 0": (lambda i, **kw: _tile(**kw), lambda g: dict(n=0), "ICEM_E_INVALID"),
    "n = 33": (lambda i, **kw: _tile(**kw), lambda g: dict(n=33, handles=[g.pls[k % 2]._h for k in range(33)]), "ICEM_E_INVALID"),
    "a null handle": (lambda i, **kw: _tile(**kw), lambda g: dict(handles=[g.pls[0]._h, None]), "ICEM_E_INVALID"),
    "the same handle twice": (lambda i, **kw: _tile(**kw), lambda g: dict(handles=[g.pls[0]._h, g.pls[0]._h]), "ICEM_E_INVALID"),
    "another num_traj": (lambda i, **kw: planner("f32", 250 + 16 * i, 30, 6, 17, 0, **kw), lambda g: {}, "ICEM_E_INVALID"),
    "another cost mode": (lambda i, **kw: _tile(mode="best" if i else "sum", **kw), lambda g: {}, "ICEM_E_INVALID"),
    # (the problems' rollout launches differ in shape: the code and wording of icem_plan_step_cem_batch for unequal keys)
    "another tile arithmetic": (lambda i, **kw: (_tile_f32 if i else _tile)(**kw), lambda g: {}, "ICEM_E_STATE"),
    "option random_step = 0": (lambda i, **kw: _tile(**kw), lambda g: {}, "ICEM_E_UNSUPPORTED"),
    "a NULL buffer": (lambda i, **kw: _tile(**kw), lambda g: dict(edit=_null_costs), "ICEM_E_INVALID"),
    "a negative offset": (lambda i, **kw: _tile(**kw), lambda g: dict(offsets=[0, -1]), "ICEM_E_INVALID"),
    "change_freq = horizon": (lambda i, **kw: _tile(**kw), lambda g: dict(freq=30), "ICEM_E_INVALID"),
    "profiling on": (lambda i, **kw: _tile(**kw), lambda g: {}, "ICEM_E_UNSUPPORTED"),
    # a rollout without a batched twin: the float64 matrix-core rollout
    "the f64 matrix-core rollout": (lambda i, **kw: planner("f64", 96, 12, 5, 40, 1, f64_arith="mfma", **kw), lambda g: {}, "ICEM_E_UNSUPPORTED"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_a_refused_batch_launches_nothing_and_touches_nothing(case):
    from icem_amd import _lib as L
    make, bend, code = REFUSALS[case]
    g = Group.__new__(Group)
    g.pls = [make(i, seed=5 + i) for i in range(2)]
    g.calls = [0, 0]
    g.per_step = g.pls[0].cfg.num_traj * g.pls[0].h
    o = g.pls[0].obs_dim
    for i, pl in enumerate(g.pls):   # a served solo step first: the buffers hold something a refused batch could spoil
        fused_step(pl, obs_of(o, i, 0), 0, FREQ)
    try:
        if case == "option random_step = 0":
            L.set_option("random_step", 0)
        if case == "profiling on":
            g.pls[1].profile_enable(True)
        torch.cuda.synchronize()
        before = _snapshot(g)
        with pytest.raises(L.IcemError) as e:
            _raw_call(g, [obs_of(o, i, 0) for i in range(2)], **bend(g))
        torch.cuda.synchronize()
        assert e.value.code == getattr(L, code), str(e.value)
        assert _snapshot(g) == before
        if not bend(g):   # ... and through the wrapper
            with pytest.raises(L.IcemError):
                g.step_batch([obs_of(o, i, 0) for i in range(2)])
            torch.cuda.synchronize()
            assert _snapshot(g) == before
    finally:
        L.reset_options()


# ---- the controllers ----------------------------------------------------------------------------------------------------------
def drive_batch(ctrls, twins, steps=3):
    from icem_amd import MpcRandomHip
    obs0 = [obs_of(17, i, 0) for i in range(len(ctrls))]
    for c, ob in zip(list(ctrls) + list(twins), obs0 + obs0):
        c.beginning_of_rollout(observation=ob, state=None, mode="train")
    for s in range(steps):
        obs = [obs_of(17, i, s) for i in range(len(ctrls))]
        got = MpcRandomHip.get_action_batch(ctrls, obs)
        want = [t.get_action(ob, None) for t, ob in zip(twins, obs)]
        for i, (a, b) in enumerate(zip(ctrls, twins)):
            assert np.array_equal(got[i], want[i]), (s, i)
            same_controllers(a, b, (s, i))
            assert a.calls == (s + 1) * 250 * 30


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_the_controllers_step_together_as_their_twins_step_alone(dtype):
    ctrls = [controller(None, dtype, seed=3 + i) for i in range(3)]
    twins = [controller(False, dtype, seed=3 + i) for i in range(3)]
    drive_batch(ctrls, twins)
    served = all(c._fused_step_refusal() is None for c in ctrls)
    assert (ctrls[0].planner.random_batch_launches == 3) == served
    assert all(c.planner.random_step_launches == 0 for c in ctrls)
    from icem_amd import MpcRandomHip
    assert MpcRandomHip.get_action_batch([], []) == []


def test_fused_step_true_raises_and_none_falls_back_where_the_batch_is_refused():
    from icem_amd import MpcRandomHip
    from icem_amd import _lib as L
    try:
        L.set_option("random_step", 0)
        ctrls = [controller(True, seed=3 + i) for i in range(3)]
        obs = [obs_of(17, i, 0) for i in range(3)]
        for c, ob in zip(ctrls, obs):
            c.beginning_of_rollout(observation=ob, state=None, mode="train")
        with pytest.raises(RuntimeError, match="fused_step=True"):
            MpcRandomHip.get_action_batch(ctrls, obs)
        assert all(c.calls == 0 for c in ctrls)
        # fused_step=None: every controller's own step, in order -- here the operator chain -- and the twins' results
        ctrls = [controller(None, seed=3 + i) for i in range(3)]
        twins = [controller(False, seed=3 + i) for i in range(3)]
        drive_batch(ctrls, twins, steps=2)
        assert all(c.planner.random_batch_launches == 0 and c.planner.random_step_launches == 0 for c in ctrls)
    finally:
        L.reset_options()
    # controllers that differ in action_change_frequency are not one batch: each steps on its own fused step
    ctrls = [controller(None, freq=3 + i, seed=3 + i) for i in range(2)]
    twins = [controller(False, freq=3 + i, seed=3 + i) for i in range(2)]
    drive_batch(ctrls, twins, steps=2)
    assert all(c.planner.random_batch_launches == 0 for c in ctrls)
    strict = [controller(True, freq=3 + i, seed=3 + i) for i in range(2)]
    obs = [obs_of(17, i, 0) for i in range(2)]
    for c, ob in zip(strict, obs):
        c.beginning_of_rollout(observation=ob, state=None, mode="train")
    with pytest.raises(RuntimeError, match="fused_step=True"):
        MpcRandomHip.get_action_batch(strict, obs)
