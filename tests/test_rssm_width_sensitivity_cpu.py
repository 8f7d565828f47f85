"""The test of the action-width tests (no GPU): with the CPU emulation standing in for the kernel, rssm_cases.py's criterion
-- bounds unchanged -- passes the reference pair on every case of rssm_width_cases.py, and rejects every single fault in how
an action row is staged: the stand-in is handed the action tensor as a wrong staging would see it (an entry dropped, two
swapped, an entry of the neighbouring step, step 0 for ever, the declared width's row stride) at 128 rows per launch."""
import numpy as np
import pytest

import rssm_cases as RC
import rssm_width_cases as WC

ROWS = 128


@pytest.mark.parametrize("case", WC.CASES, ids=lambda c: c.name)
def test_reference_pair_agrees_at_every_width(case):
    """float32 / K-blocked / +-2 ulp against float64, both on the kernel's rounding points: inside the bounds rssm_cases.py
    measured at width six, at every width and shape of the new table."""
    want = WC.want(case)
    got = WC.kernel_standin(case)
    print(case.name, WC.errors(got, want))
    assert WC.agree(got, want), (WC.violations(got, want), WC.errors(got, want))


# ---- the mutants: action tensor [n, h, d] -> what the faulty staging hands the model -----------------------------------------
def _drop(k):
    def see(a):
        a = a.copy()
        a[:, :, k] = 0
        return a
    return see


def _swap(k):
    def see(a):
        a = a.copy()
        a[:, :, [k, k + 1]] = a[:, :, [k + 1, k]]
        return a
    return see


def _from_step(k, dt):   # entry k of step t taken from step t + dt (where that step exists)
    def see(a):
        out = a.copy()
        if dt > 0:
            out[:, :-1, k] = a[:, 1:, k]
        else:
            out[:, 1:, k] = a[:, :-1, k]
        return out
    return see


def _step0_for_ever(a):
    return np.repeat(a[:, :1], a.shape[1], 1)


def _stride_of_six(a):   # row i read from i * h * 6 on instead of i * h * d (zeros past the end of the tensor)
    n, h, d = a.shape
    flat = np.concatenate([a.reshape(-1), np.zeros(n * h * max(6 - d, 0))])
    return np.stack([flat[i * h * 6:i * h * 6 + h * d].reshape(h, d) for i in range(n)])


def _mutants():
    out = []
    for d in WC.MUTANT_WIDTHS:
        out += [(d, f"entry {k} dropped", _drop(k)) for k in range(d)]
        if d > 1:
            out += [(d, f"entries {k} and {k + 1} swapped", _swap(k)) for k in sorted({0, d // 2 - 1, d - 2}) if k >= 0]
        out += [(d, f"entry {d - 1} from step t + 1", _from_step(d - 1, 1)), (d, f"entry {d - 1} from step t - 1", _from_step(d - 1, -1)),
                (d, "entry 0 from step t + 1", _from_step(0, 1)), (d, "step 0's action at every step", _step0_for_ever),
                (d, "row stride 6", _stride_of_six)]
    return out


MUTANTS = _mutants()
_want = {}


def small_want(case):
    if case.name not in _want:
        _want[case.name] = WC.want(case, rows=ROWS)
    return _want[case.name]


@pytest.mark.parametrize("d,name,see", MUTANTS, ids=[f"d{d}-{name.replace(' ', '_')}" for d, name, _ in MUTANTS])
def test_every_staging_fault_fails_some_case_tenfold(d, name, see):
    """The median part or the share part (the factor by which ROW_BOUND can grow with more than SHARE_CAP of the rows still
    above it) is missed by a factor of at least 10 on one of the width's 1007 x 12 cases, cut to 128 rows."""
    best = (0.0, None)
    for case in (c for c in WC.WIDE_CASES if c.d == d):
        s = WC.errors(WC.kernel_standin(case, rows=ROWS, actions=see), small_want(case))
        f = max(s["median"] / RC.MEDIAN_BOUND, s["quantile"] / RC.ROW_BOUND)
        if f > best[0]:
            best = (f, case.name)
        if f >= 10:
            return
    pytest.fail(f"width {d}, {name}: best case {best[1]} misses by {best[0]:.3g} only")


def test_the_unfaulted_stand_in_passes_at_128_rows():
    """... and the same stand-in with nothing wrong passes on those cut cases, so the mutants fail for their fault alone."""
    for case in (c for c in WC.WIDE_CASES if c.d in WC.MUTANT_WIDTHS):
        got = WC.kernel_standin(case, rows=ROWS)
        assert WC.agree(got, small_want(case)), (case.name, WC.errors(got, small_want(case)))
