"""Can the inputs of test_gpu_learned_models.py's batch test tell a wrong cost source from the right one?  The update kernel of
icem_plan_step_learned_models (update_small_members_batch_kernel, k_merge.hip) builds problem p's selection keys from
``reduce_e member_costs[e * stride + row0 + i]``; the GPU tests compare its elites bit for bit with the stage-wise loop's.  Here
the cost source is restated in NumPy float32 (learned_models_cases.member_source, on rssm_models_cases.reduce_members) and run
on member-cost arrays of that test's shape -- B = 3 problems, E = 3 members, 131 | 128 | 131 rows (one problem reset a step
later), K = 10 -- and every single fault below must change the selected elite index SET of at least one problem.  No device."""
import numpy as np
import pytest

import learned_models_cases as LC
from rssm_models_cases import reduce_members

ROWS = LC.ROWS_LATE_RESET
R0 = LC.row_offsets(ROWS)
STRIDE = sum(ROWS)
E = LC.E


def right(mc, p, reduce):
    return LC.member_source(mc, E, STRIDE, R0[p], ROWS[p], reduce)


def gather(mc, offsets):
    """[E, n] member costs of one problem through a (possibly wrong) offset table [E, n]."""
    return np.asarray(mc, dtype=np.float32).reshape(-1)[offsets]


def offsets(p, stride=STRIDE, row0=None, members=E):
    r0 = R0[p] if row0 is None else row0
    return np.arange(members)[:, None] * stride + r0 + np.arange(ROWS[p])[None, :]


def _inv_per_member(c):
    inv = np.float32(1.0 / c.shape[0])
    acc = (c[0] * inv).astype(np.float32)
    for e in range(1, c.shape[0]):
        acc = (acc + (c[e] * inv).astype(np.float32)).astype(np.float32)
    return acc


def _mean_fixed_inv(c, members):
    acc = c[0].copy()
    for e in range(1, c.shape[0]):
        acc = (acc + c[e]).astype(np.float32)
    return (acc * np.float32(1.0 / members)).astype(np.float32)


# name -> (reduce it is a fault of, fn(mc, p) -> the problem's reduced costs under the fault)
FAULTS = {
    "problem-major instead of member-major": ("mean", lambda mc, p: reduce_members(
        gather(mc, E * R0[p] + np.arange(E)[:, None] * ROWS[p] + np.arange(ROWS[p])[None, :]), "mean")),
    "stride = the problem's own rows": ("mean", lambda mc, p: reduce_members(gather(mc, offsets(p, stride=ROWS[p])), "mean")),
    "row0 dropped": ("mean", lambda mc, p: reduce_members(gather(mc, offsets(p, row0=0)), "mean")),
    "a member dropped": ("mean", lambda mc, p: _mean_fixed_inv(gather(mc, offsets(p, members=E - 1)), E)),
    "a member dropped (max)": ("max", lambda mc, p: reduce_members(gather(mc, offsets(p, members=E - 1)), "max")),
    "members summed in reverse order": ("mean", lambda mc, p: reduce_members(gather(mc, offsets(p))[::-1], "mean")),
    "inv applied per member": ("mean", lambda mc, p: _inv_per_member(gather(mc, offsets(p)))),
    "max for mean": ("mean", lambda mc, p: reduce_members(gather(mc, offsets(p)), "max")),
    "mean for max": ("max", lambda mc, p: reduce_members(gather(mc, offsets(p)), "mean")),
    "NaN ignored by max": ("max", lambda mc, p: np.fmax.reduce(gather(mc, offsets(p)), axis=0)),
}


@pytest.fixture(scope="module")
def mc():
    return LC.designed_member_costs()


def test_the_shape_is_the_gpu_tests(mc):
    assert (LC.B, LC.E, LC.K) == (3, 3, 10) and ROWS == [131, 128, 131] and R0 == [0, 131, 259] and STRIDE == 390
    assert all(r % 16 for r in R0[1:]) and STRIDE % 16, "offsets and stride off the rollout's 16-row tiles"
    assert mc.shape == (E, STRIDE) and mc.dtype == np.float32
    assert all(r == LC.POPULATIONS[0] + (LC.N_REUSE if p != 1 else 0) for p, r in enumerate(ROWS))


@pytest.mark.parametrize("reduce", ["mean", "max"])
def test_the_restatement_is_the_offset_followed_by_the_reduction(mc, reduce):
    """member_source against a scalar loop that spells the offset e * stride + row0 + i out, member by member."""
    flat = mc.reshape(-1)
    for p in range(LC.B):
        got = right(mc, p, reduce)
        for i in (0, 1, ROWS[p] // 2, ROWS[p] - 1):
            acc = flat[0 * STRIDE + R0[p] + i]
            for e in range(1, E):
                c = flat[e * STRIDE + R0[p] + i]
                acc = np.float32(acc + c) if reduce == "mean" else (c if (c > acc or c != c) else acc)
            want = np.float32(acc * np.float32(1.0 / E)) if reduce == "mean" else acc
            assert np.array_equal(got[i], want, equal_nan=True), (p, i)
    # a NaN member makes the row NaN under both reductions, and NaN rows are never elites while K finite rows exist
    nan_rows = np.flatnonzero(np.isnan(mc[1, R0[2]:R0[2] + ROWS[2]]))
    assert nan_rows.size == LC.K and np.isnan(right(mc, 2, reduce)[nan_rows]).all()
    assert not (LC.elite_set(right(mc, 2, reduce)) & set(nan_rows.tolist()))


@pytest.mark.parametrize("name", list(FAULTS))
def test_every_single_fault_moves_an_elite_set(mc, name):
    reduce, fn = FAULTS[name]
    moved = []
    for p in range(LC.B):
        want, got = LC.elite_set(right(mc, p, reduce)), LC.elite_set(fn(mc, p))
        assert len(want) == LC.K
        if want != got:
            moved.append(p)
    print(f"{name} ({reduce}): elite sets of problems {moved} move")
    assert moved, name


def test_the_designed_groups_do_what_they_were_designed_for(mc):
    """The order of the sum, the place of inv and the NaN rule are visible in ONE designed group each: say which."""
    assert [p for p in range(3) if LC.elite_set(right(mc, p, "mean")) != LC.elite_set(FAULTS["members summed in reverse order"][1](mc, p))] == [0]
    assert LC.elite_set(right(mc, 0, "mean")) == frozenset(range(30, 40))
    assert [p for p in range(3) if LC.elite_set(right(mc, p, "mean")) != LC.elite_set(FAULTS["inv applied per member"][1](mc, p))] == [1]
    assert LC.elite_set(right(mc, 1, "mean")) == frozenset(range(30, 40))
    assert [p for p in range(3) if LC.elite_set(right(mc, p, "max")) != LC.elite_set(FAULTS["NaN ignored by max"][1](mc, p))] == [2]
