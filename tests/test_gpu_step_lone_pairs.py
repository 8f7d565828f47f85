"""The lone rollout wave's shortened model step (Tile16H::step_lone_pairs, icem_amd/csrc/fused_dev.h) in the single-launch
kernel: the step's two extra entries come from ONE paired LDS read at lane-uniform offsets, so a padding entry (weight 0,
scale 0) no longer re-reads the step's first action but whatever lies up to six floats behind the step's last action -- the
next step's actions, the next row's, and for the last step of the tile's last row the words behind the tile, which the
workgroup zeroes in front of its barrier.  A value there that is not finite would poison the row's cost (0 x inf).

What this test holds and what it does not.  ``plan_step`` (merge-prologue launches) and the split API (``icem_plan_iter_local``
+ ``icem_plan_iter_merge``: the same rollout without prologue) BOTH roll out with the shortened step, so their equality, bit
for bit, says that the step gives the same bits in both launches -- prologue or not, whatever LDS held before -- not that those
are the bits of the step it replaced.  The arithmetic itself is held by tests/test_gpu_tile_arith.py and tests/test_gpu_parity.py
(these three shapes against the float64 oracle) and by the byte-identical benchmark outputs of EXPERIMENTS R19.1.  What bears on
the paired read here: every cost is finite and the handle's count of non-finite costs stays 0, over the three shapes the step
is compiled for -- (13, 4, 17) has three of four lane groups padding in the second entry --, both model kinds, the three cost
modes, populations of one full tile (16: row 15 reads behind the tile) and partly filled tiles (17, 40: rows past the end), two
iterations and two MPC steps, with other kernels between the launches that leave LDS dirty: another shape's planner step, whose
observation is large, and a generator kernel.  (Nothing here can PLACE a NaN in the eight words behind the tile: a missing
zeroing shows only if what ran before left one there.)  Then two problems of one batched launch against their solo steps."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(30, 6, 17), (12, 6, 17), (13, 4, 17)]
POPULATIONS = (16, 17, 40)
MODES = ("sum", "best", "final")


def np_(t):
    return t.detach().cpu().numpy()


def _planner(N, h, d, o, kind, mode, i=0):
    from icem_amd import DeviceSyntheticModel, IcemConfig, IcemPlanner, halfcheetah_env
    env = halfcheetah_env(o)
    model = DeviceSyntheticModel.make(o, d, kind=kind, seed_a=10 + i, seed_b=20 + i)
    pl = IcemPlanner(IcemConfig(horizon=h, act_dim=d, num_traj=N, opt_iters=2, dtype="f32", seed=11 + 7 * i, cost_mode=mode),
                     env.action_space.low[:d], env.action_space.high[:d])
    pl.set_model(model.kind, model.A, model.B)
    pl.set_cost_spec(env.cost_spec)
    assert pl.set_tile_arith(1) == 1
    pl.reset()
    return pl


def _obs(o, seed):
    return 0.3 * np.random.RandomState(seed).randn(o)


def _state(pl):
    """costs and rows of the last iteration's pool, elite rows and costs, mean, std, the executed action"""
    n_last = pl.population_sizes[-1]
    ea, ec = pl.current_elites()
    return [np_(x).copy() for x in (pl.costs[:n_last], pl.actions[:n_last], ea, ec, pl.mean, pl.std, pl.executed)]


def _same(got, want, where):
    for j, (x, y) in enumerate(zip(got, want)):
        assert np.array_equal(x, y), where + (j,)


class _Dirt:
    """Kernels of other shapes between the launches under test: whatever they leave in LDS is what the next launch finds."""

    def __init__(self):
        self.pl = _planner(64, 30, 6, 18, 1, "sum", i=3)   # (o = 18: a tile with other strides, and no paired read)
        self.obs = 5.0 * _obs(18, 99)
        self.junk = torch.empty(1 << 20, device=self.pl.device)

    def __call__(self):
        self.pl.plan_step(self.obs)
        self.junk.normal_()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("h,d,o", SHAPES)
def test_the_paired_read_leaves_the_bits_of_the_split_step(h, d, o, kind, mode):
    dirt = _Dirt()
    for N in POPULATIONS:
        fused, split = _planner(N, h, d, o, kind, mode), _planner(N, h, d, o, kind, mode)
        for step in range(2):
            obs = _obs(o, 7 + step)
            dirt()
            fused.plan_step(obs)
            dirt()
            split.plan_step(obs, on_iteration=lambda it: None)
            torch.cuda.synchronize()
            got, want = _state(fused), _state(split)
            assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(want[0])), (N, step)
            _same(got, want, (N, step))
        assert fused.nonfinite_costs() == 0 and split.nonfinite_costs() == 0, N


@pytest.mark.parametrize("N", POPULATIONS)
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("h,d,o", SHAPES)
def test_two_problems_of_one_batched_launch_equal_their_solo_steps(h, d, o, kind, N):
    from icem_amd import IcemPlanner
    mode = MODES[(POPULATIONS.index(N) + kind) % 3]
    dirt = _Dirt()
    batch = [_planner(N, h, d, o, kind, mode, i) for i in range(2)]
    solo = [_planner(N, h, d, o, kind, mode, i) for i in range(2)]
    for step in range(2):
        obs = [_obs(o, 7 + step), 4.0 * _obs(o, 17 + step)]
        dirt()
        IcemPlanner.plan_step_batch(batch, obs)
        for pl, ob in zip(solo, obs):
            dirt()
            pl.plan_step(ob)
        torch.cuda.synchronize()
        for i in range(2):
            got, want = _state(batch[i]), _state(solo[i])
            assert np.all(np.isfinite(got[0])), (step, i)
            _same(got, want, (step, i))
    assert all(pl.nonfinite_costs() == 0 for pl in batch + solo)
    assert not np.array_equal(np_(batch[0].executed), np_(batch[1].executed))   # (they ARE two problems)
