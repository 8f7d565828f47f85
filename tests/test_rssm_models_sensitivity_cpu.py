"""The condition on the inputs of test_gpu_rssm_models.py, without a device (rssm_models_cases.py): every one-tensor pair
is told apart on every row of the pool in every cost mode, so a launch that reads ANY single tensor of a problem from the
other problem's buffer cannot pass the bit comparison; the members of the ensembles differ on every row; and the NumPy
float32 restatement of the two reductions rejects each single fault of a reduction."""
import numpy as np
import pytest

import rssm_models_cases as MC


@pytest.fixture(scope="module")
def base_costs():
    ob, acts = MC.pool()
    P = MC.params(MC.BASE)
    return {mode: MC.emulated(P, ob, acts, mode) for mode in MC.MODES}


def test_there_is_a_pair_for_every_parameter_tensor():
    assert sorted(MC.TENSORS) == sorted(MC.module(MC.BASE).state_dict().keys()) and len(MC.TENSORS) == 16
    for t in MC.TENSORS:
        a, b = MC.module(MC.BASE).state_dict(), MC.module(MC.BASE, t).state_dict()
        for k in a:
            assert (not np.array_equal(a[k].numpy(), b[k].numpy())) == (k == t), (t, k)


@pytest.mark.parametrize("tensor", MC.TENSORS)
def test_swapping_one_tensor_changes_every_row_in_every_mode(tensor, base_costs):
    ob, acts = MC.pool()
    P = MC.params(MC.BASE, tensor)
    for mode in MC.MODES:
        got = MC.emulated(P, ob, acts, mode)
        assert got.dtype == np.float32 and got.shape == (MC.POOL_ROWS,)
        same = np.flatnonzero(got == base_costs[mode])
        assert same.size == 0, (tensor, mode, "rows that cannot tell the pair apart", same)


def member_costs(E, mode="sum"):
    ob, acts = MC.pool()
    return np.stack([MC.emulated(MC.params(s), ob, acts, mode) for s in MC.MEMBER_SEEDS[:E]]).astype(np.float32)


def test_the_members_differ_on_every_row():
    for mode in MC.MODES:
        c = member_costs(5, mode)
        for i in range(5):
            for j in range(i):
                assert not np.any(c[i] == c[j]), (mode, i, j)


def test_the_restatement_is_the_three_float32_operations():
    c = member_costs(5)
    want = ((((c[0] + c[1]) + c[2]) + c[3]) + c[4]) * np.float32(0.2)
    assert want.dtype == np.float32 and np.array_equal(MC.reduce_members(c, "mean"), want)
    assert np.array_equal(MC.reduce_members(c, "max"), c.max(0))
    assert np.array_equal(MC.reduce_members(c[:1], "mean"), c[0]) and np.array_equal(MC.reduce_members(c[:1], "max"), c[0])
    # a float64 mean rounded once is NOT the kernel's arithmetic on this pool: the restatement has to be the f32 chain
    assert not np.array_equal(want, c.astype(np.float64).mean(0).astype(np.float32))


@pytest.mark.parametrize("fault,reduces", [
    ("a member dropped", ("mean",)),
    ("a member counted twice", ("mean",)),
    ("1 / (E - 1)", ("mean",)),
    ("max for mean", ("mean", "max")),
    ("the members visited in reverse", ("mean",)),
])
def test_the_restatement_rejects_single_faults(fault, reduces):
    c = member_costs(5)
    for r in reduces:
        want, got = MC.reduce_members(c, r), MC.REDUCTION_FAULTS[fault](c, r)
        assert got.shape == want.shape
        assert not np.array_equal(got, want), (fault, r)


def test_a_nan_member_makes_the_row_nan_and_a_max_that_swallows_it_is_rejected():
    c = member_costs(3)
    for e in range(3):   # wherever the NaN member stands in the order
        k = c.copy()
        k[e, ::2] = np.nan
        for r in ("mean", "max"):
            got = MC.reduce_members(k, r)
            assert np.isnan(got[::2]).all() and np.array_equal(got[1::2], MC.reduce_members(c, r)[1::2]), (e, r)
        swallowed = MC.REDUCTION_FAULTS["a NaN member swallowed by max"](k, "max")
        assert not np.isnan(swallowed).any()
        assert not np.array_equal(swallowed, MC.reduce_members(k, "max"), equal_nan=True), e


@pytest.mark.parametrize("E", [3, 5])
def test_a_dropped_member_is_missed_by_max_where_it_was_the_worst(E):
    """Under max a dropped member shows on the rows on which it was the worst one, and on this pool (mode `sum`) at least two
    members are the worst of some row: the maximum is no single member's costs."""
    c = member_costs(E)
    worst = sorted(set(c.argmax(0).tolist()))
    assert len(worst) >= 2, worst
    for e in worst:
        got = MC.REDUCTION_FAULTS["a member dropped"](c, "max", e)
        rows = np.flatnonzero(got != MC.reduce_members(c, "max"))
        assert np.array_equal(rows, np.flatnonzero(c.argmax(0) == e)), e
