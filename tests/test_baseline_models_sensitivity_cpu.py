"""Can the comparisons of test_gpu_baseline_models.py tell a wrong member reduction from the right one?  The two new kernels build
their keys from ``reduce_e member_costs[e * stride + row0 + i]`` and write the reduced cost back: cem_update_members_batch_kernel
selects the K smallest (cost + 0, index) keys with NaN = +inf, random_select_members_batch_kernel the smallest one (the reported cost
-0 -> +0).  The GPU tests compare the elite indices and costs / the winning row and its cost AND the costs buffer bit for bit with
the stage-wise operators.  Here both selections are restated in NumPy float32 (on learned_models_cases.member_source and
rssm_models_cases.reduce_members) and run on member-cost arrays of the GPU batch tests' shape -- B = 3 problems of N = 250 rows,
E = 3 members, stride 750, K = 10 -- and that comparison must accept the restatement and reject every single fault below, on at
least one problem.  No device."""
import numpy as np
import pytest

import learned_models_cases as LC
from rssm_models_cases import reduce_members

B, E, N, K = 3, 3, 250, 10
ROWS = [N] * B
R0 = LC.row_offsets(ROWS)
STRIDE = B * N
INV = np.float32(1.0 / E)


# ---- the restatements ----------------------------------------------------------------------------------------------------------
def keys(costs):
    """(cost, index) order of the selections: NaN = +inf, -0 = +0, ties by index -> the row indices, best first."""
    costs = np.asarray(costs)   # (float32; a fault may hand over float64 -- products that were never rounded)
    c = np.where(np.isnan(costs), costs.dtype.type(np.inf), costs) + costs.dtype.type(0.0)
    return np.lexsort((np.arange(c.size), c)), c


def cem_outputs(reduced):
    """What the GPU test compares of a CEM update: the costs buffer, the K elite indices in key order and their key costs."""
    order, c = keys(reduced)
    return dict(costs=np.asarray(reduced, dtype=np.float32), elite_idx=order[:K].astype(np.int32), elite_costs=c[order[:K]])


def random_outputs(reduced):
    """... of a random-shooting selection: the costs buffer, the winning row and the cost reported for it."""
    order, c = keys(reduced)
    return dict(costs=np.asarray(reduced, dtype=np.float32), best=order[:1].astype(np.int32), best_cost=c[order[:1]])


def same(a, b):
    """The GPU tests' comparison: np.array_equal on every buffer (NaN costs compare equal where the test says equal_nan)."""
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def right(mc, p, reduce):
    return LC.member_source(mc, E, STRIDE, R0[p], N, reduce)


# ---- the faults: fn(mc, p) -> (the reduced costs the selection keys on, the costs buffer it leaves) ------------------------------
def gather(mc, offsets):
    return np.asarray(mc, dtype=np.float32).reshape(-1)[offsets]


def offsets(p, stride=STRIDE, row0=None, members=E):
    r0 = R0[p] if row0 is None else row0
    return np.arange(members)[:, None] * stride + r0 + np.arange(N)[None, :]


def _sum(c):
    acc = c[0].copy()
    for e in range(1, c.shape[0]):
        acc = (acc + c[e]).astype(np.float32)
    return acc


def _mean_unrounded(c):
    """The multiply without a rounding of its own: the product stays exact (float64 holds a float32 product exactly) on its way
    into the comparison."""
    return _sum(c).astype(np.float64) * np.float64(INV)


STALE = np.float32(-12345.0)   # what the costs buffer held before the step (test_gpu_learned_models.SENTINEL)
both = lambda r: (r, r)   # noqa: E731
FAULTS = {
    "wrong stride (the problem's own rows)": ("mean", lambda mc, p: both(reduce_members(gather(mc, offsets(p, stride=N)), "mean"))),
    "row0 dropped": ("mean", lambda mc, p: both(reduce_members(gather(mc, offsets(p, row0=0)), "mean"))),
    "the last member skipped": ("mean", lambda mc, p: both((_sum(gather(mc, offsets(p, members=E - 1))) * INV).astype(np.float32))),
    "the last member skipped (max)": ("max", lambda mc, p: both(reduce_members(gather(mc, offsets(p, members=E - 1)), "max"))),
    "mean without the rounding of its own multiply": ("mean", lambda mc, p: (_mean_unrounded(gather(mc, offsets(p))), right(mc, p, "mean"))),
    "max without the NaN clause": ("max", lambda mc, p: both(np.fmax.reduce(gather(mc, offsets(p)), axis=0))),
    "the reduced cost not written back": ("mean", lambda mc, p: (right(mc, p, "mean"), np.full(N, STALE))),
    "max for mean": ("mean", lambda mc, p: both(right(mc, p, "max"))),
    "mean for max": ("max", lambda mc, p: both(right(mc, p, "mean"))),
    "members read problem-major": ("mean", lambda mc, p: both(reduce_members(
        gather(mc, E * R0[p] + np.arange(E)[:, None] * N + np.arange(N)[None, :]), "mean"))),
}


def faulty_outputs(outputs, fn, mc, p):
    keyed, buffer = fn(mc, p)
    out = outputs(keyed)
    out["costs"] = np.asarray(buffer, dtype=np.float32)
    for k in out:   # (a selection on unrounded costs still reports float32)
        out[k] = out[k].astype(np.float32) if out[k].dtype == np.float64 else out[k]
    return out


# ---- the inputs ----------------------------------------------------------------------------------------------------------------
def merged_pair():
    """Two sums a_lo < a_hi (adjacent float32) whose products with inv = float32(1 / 3) round to the SAME float32: rounded they tie
    and the index decides, unrounded a_lo wins."""
    a = np.float32(-29.0)
    for _ in range(64):
        lo = np.nextafter(a, np.float32(-np.inf))
        if np.float32(lo * INV) == np.float32(a * INV):
            return lo, a
        a = lo
    raise AssertionError("no merging pair near -29")


def designed(rank):
    """LC.designed_member_costs on this shape, plus a pair of rows of problem 0 whose sums are merged_pair() -- the larger sum at
    the LOWER index -- with ``rank - 1`` rows cheaper than both: the pair straddles the boundary of the ``rank`` best."""
    mc = LC.designed_member_costs(ROWS, E)
    lo, hi = merged_pair()
    r = R0[0]
    for j, total in ((200, hi), (210, lo)):
        mc[:, r + j] = 0.0
        mc[0, r + j] = total   # (0 + 0 adds nothing: the sum is `total` exactly)
    for j in range(rank - 1):
        mc[:, r + 220 + j] = np.float32(-20.0 - j)   # mean -20 - j: cheaper than the pair's -9.67
    # (the designed group of problem 0, mean x / 3 > 0, and every other row, mean > 1, cost more than the pair)
    return mc


@pytest.fixture(scope="module")
def inputs():
    return {"cem": designed(K), "random": designed(1)}


OUTPUTS = {"cem": cem_outputs, "random": random_outputs}


def test_the_shape_is_the_gpu_tests(inputs):
    assert (B, E, N, K, STRIDE, R0) == (3, 3, 250, 10, 750, [0, 250, 500])
    assert N % 16 and STRIDE % 16, "offsets and stride off the rollout's 16-row tiles"
    for mc in inputs.values():
        assert mc.shape == (E, STRIDE) and mc.dtype == np.float32
    lo, hi = merged_pair()
    assert lo < hi and np.float32(lo * INV) == np.float32(hi * INV)


@pytest.mark.parametrize("which", list(OUTPUTS))
@pytest.mark.parametrize("reduce", ["mean", "max"])
def test_the_restatement_is_the_offset_the_reduction_and_the_key_order(inputs, which, reduce):
    """member_source against a scalar loop that spells the offset e * stride + row0 + i and rssm_ensemble_reduce_kernel's operations
    out; the selection against a scalar scan of (nan_to_inf(cost) + 0, index) keys; and the comparison accepts it."""
    mc = inputs[which]
    flat = mc.reshape(-1)
    for p in range(B):
        got = right(mc, p, reduce)
        for i in (0, 1, 24, 200, 210, N - 1):
            acc = flat[0 * STRIDE + R0[p] + i]
            for e in range(1, E):
                c = flat[e * STRIDE + R0[p] + i]
                acc = np.float32(acc + c) if reduce == "mean" else (c if (c > acc or c != c) else acc)
            want = np.float32(acc * INV) if reduce == "mean" else acc
            assert np.array_equal(got[i], want, equal_nan=True), (p, i)
        out = OUTPUTS[which](got)
        ranked = sorted(range(N), key=lambda i: (np.inf if np.isnan(got[i]) else float(got[i]) + 0.0, i))
        if which == "cem":
            assert out["elite_idx"].tolist() == ranked[:K] and not np.isnan(out["elite_costs"]).any()
        else:
            assert int(out["best"][0]) == ranked[0] and np.array_equal(out["best_cost"][0], np.nan_to_num(got[ranked[0]], nan=np.inf) + np.float32(0))
        assert same(out, OUTPUTS[which](right(mc, p, reduce)))
    # a NaN member makes the row NaN under both reductions, and a NaN row is never selected while finite rows exist
    nan_rows = np.flatnonzero(np.isnan(mc[1, R0[2]:R0[2] + N]))
    assert nan_rows.size == K and np.isnan(right(mc, 2, reduce)[nan_rows]).all()
    assert not set(cem_outputs(right(mc, 2, reduce))["elite_idx"].tolist()) & set(nan_rows.tolist())


def test_minus_zero_wins_as_plus_zero_and_ties_go_to_the_lower_index():
    c = np.full(N, 1.0, dtype=np.float32)
    c[[7, 3]] = np.float32(-0.0), np.float32(0.0)
    out = random_outputs(c)
    assert int(out["best"][0]) == 3 and out["best_cost"][0] == 0 and not np.signbit(out["best_cost"][0])
    c[:] = np.nan
    assert int(random_outputs(c)["best"][0]) == 0 and np.isinf(random_outputs(c)["best_cost"][0])   # every key (+inf, index)


@pytest.mark.parametrize("which", list(OUTPUTS))
@pytest.mark.parametrize("name", list(FAULTS))
def test_every_single_fault_is_rejected(inputs, which, name):
    reduce, fn = FAULTS[name]
    mc, outputs = inputs[which], OUTPUTS[which]
    selection = "elite_idx" if which == "cem" else "best"
    moved, seen = [], []
    for p in range(B):
        want, got = outputs(right(mc, p, reduce)), faulty_outputs(outputs, fn, mc, p)
        if not same(want, got):
            seen.append(p)
        if not np.array_equal(np.sort(want[selection]), np.sort(got[selection])):
            moved.append(p)
    print(f"{which}: {name} ({reduce}): rejected on problems {seen}, the selection moves on {moved}")
    assert seen, name
    if name != "the reduced cost not written back":   # (that one leaves the selection alone: the costs buffer shows it)
        assert moved, name


def test_the_designed_pair_does_what_it_was_designed_for(inputs):
    """Rounded, the pair's means tie and row 200 is the last of the K best (the winner); unrounded, row 210 takes its place."""
    fn = FAULTS["mean without the rounding of its own multiply"][1]
    assert 200 in cem_outputs(right(inputs["cem"], 0, "mean"))["elite_idx"] and 210 not in cem_outputs(right(inputs["cem"], 0, "mean"))["elite_idx"]
    assert 210 in faulty_outputs(cem_outputs, fn, inputs["cem"], 0)["elite_idx"] and 200 not in faulty_outputs(cem_outputs, fn, inputs["cem"], 0)["elite_idx"]
    assert int(random_outputs(right(inputs["random"], 0, "mean"))["best"][0]) == 200
    assert int(faulty_outputs(random_outputs, fn, inputs["random"], 0)["best"][0]) == 210
