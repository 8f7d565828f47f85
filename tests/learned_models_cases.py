"""Shared by test_learned_models_sensitivity_cpu.py and test_gpu_learned_models.py (a plain module, no fixtures): the shape of the
batched models step both files use, and the NumPy float32 restatement of the cost source of update_small_members_batch_kernel
(k_merge.hip) -- the update of problem p reads member e's cost of its row i at ``member_costs[e * stride + row0 + i]`` and
reduces the members as rssm_ensemble_reduce_kernel does (rssm_models_cases.reduce_members).

The shape: B = 3 controllers on one E = 3 ensemble, N = 128, factor_decrease 1.25, K = 10 elites, 3 iterations, fraction
reused 0.3 -- populations 128, 102, 81, and 3 shifted elites at iteration 0 of every step but a problem's first.  With
problem 1 reset a step later than its peers, iteration 0 scores 131 | 128 | 131 rows: row offsets 0, 131, 259 and the member
stride 390 are no multiples of 16 (the rollout's tile) and differ from the steps in which every problem has 131 rows."""
import numpy as np

from rssm_models_cases import reduce_members

B, E, K = 3, 3, 10
POPULATIONS = [128, 102, 81]
N_REUSE = 3
ROWS_LATE_RESET = [131, 128, 131]   # iteration 0 with problem 1 in its first step
BIG = np.float32(2.0 ** 25)


def row_offsets(rows):
    return [int(sum(rows[:p])) for p in range(len(rows))]


def member_source(member_costs, members, stride, row0, n, reduce):
    """The new update's cost source: ``member_costs`` flat f32, -> the n reduced costs of the problem whose rows start at row0."""
    flat = np.asarray(member_costs, dtype=np.float32).reshape(-1)
    idx = np.arange(members)[:, None] * stride + row0 + np.arange(n)[None, :]
    return reduce_members(flat[idx], reduce)


def elite_set(costs, k=K):
    """The index set the update selects from a pool's costs: the k smallest (cost, index) keys, NaN = +inf."""
    c = np.where(np.isnan(costs), np.inf, np.asarray(costs, dtype=np.float32))
    order = np.lexsort((np.arange(c.size), c))
    return frozenset(order[:k].tolist())


def designed_member_costs(rows=ROWS_LATE_RESET, members=E, seed=0):
    """member_costs ``[members, sum rows]`` f32 on which every single fault of the cost source moves an elite set.

    Everywhere: uniform [1, 2) plus a level per member (0, 0.5, 0.25, ...), every entry its own value -- an offset that reads
    another problem's, another member's or another row's entry reads another number.  On top of that three designed groups
    of 2 K rows each, the cheapest rows of their problem under ``mean``:
      problem 0, rows 20 .. 39: (2^25, -2^25, x), x falling from just under 2 to just above 1 -- in member order the sum is x
        exactly and the LAST ten rows win; summed in reverse every row is 2 and the first ten win on their indices;
      problem 1, rows 30 .. 49: three multiples of 1/8 that sum to -30 exactly, split differently on every row -- one product
        with inv ties them all (the first ten win), a product per member does not;
      problem 2, rows 5 .. 24: uniform [0, 0.5) in every member and NaN in member 1 on the even rows -- NaN = +inf keeps those rows
        out under both reductions, a maximum that ignores NaN lets them in."""
    rs = np.random.RandomState(seed)
    total, r0 = int(sum(rows)), row_offsets(rows)
    level = 0.25 * ((2 * np.arange(members)) % 3)   # 0, 0.5, 0.25, ...
    mc = (rs.uniform(1.0, 2.0, (members, total)) + level[:, None]).astype(np.float32)
    g = 2 * K
    x = np.linspace(1.95, 1.05, g).astype(np.float32)
    mc[:, r0[0] + 20:r0[0] + 20 + g] = 0.0
    mc[0, r0[0] + 20:r0[0] + 20 + g] = BIG
    mc[1, r0[0] + 20:r0[0] + 20 + g] = -BIG
    mc[members - 1, r0[0] + 20:r0[0] + 20 + g] = x
    if len(rows) > 1:
        j = np.arange(g, dtype=np.float32)
        a = (-10.0 - 0.375 * j).astype(np.float32)
        b = (-10.0 + 0.125 * j * ((-1.0) ** j)).astype(np.float32)
        mc[:, r0[1] + 30:r0[1] + 30 + g] = 0.0
        mc[0, r0[1] + 30:r0[1] + 30 + g] = a
        mc[1, r0[1] + 30:r0[1] + 30 + g] = b
        mc[members - 1, r0[1] + 30:r0[1] + 30 + g] = (np.float32(-30.0) - a - b).astype(np.float32)
    if len(rows) > 2:
        mc[:, r0[2] + 5:r0[2] + 5 + g] = rs.uniform(0.0, 0.5, (members, g)).astype(np.float32)
        mc[1, r0[2] + 5:r0[2] + 5 + g:2] = np.nan
    return mc
