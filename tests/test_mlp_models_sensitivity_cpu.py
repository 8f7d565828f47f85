"""What test_gpu_mlp_models.py's comparison is worth, on the CPU: mlp_models_cases' NumPy stand-in of the models launch (the
kernel's walk over problems and tiles on mlp_cases.kernel_standin's arithmetic) is accepted by the comparison the GPU test uses,
and every single-fault mutant of it is rejected -- on the layouts the GPU test runs, so that each of them is known to change at
least one compared value there."""
import numpy as np
import pytest

import mlp_cases as MC
import mlp_models_cases as MM

SHAPE = MM.SHAPE_BY_NAME["o17d6-L1-swish-h2"]   # the smallest: h = 2, one hidden layer (the stand-in computes row by row)
# the layouts on which each launch fault has to show: every layout of the GPU test on which it can
_ALL = [l.name for l in MM.LAYOUTS]
_MANY = [n for n in _ALL if n != "one-17"]   # (a launch of one problem has no neighbour, no table and no second cost base)
WHERE = {
    "params-of-problem-0": _MANY,
    "obs-row-ignored": _MANY,
    "action-row0-ignored": [n for n in _MANY if n != "three-coincide"],   # (whose problems all start at row 0)
    "cost-base-16": _MANY,
    "padding-from-neighbour": _MANY,
    "last-tile-dropped": _ALL,
    "states-stride-h": _ALL,
}
_standins = {}


def standin(layout, mode="sum", shape=SHAPE, spec=None):
    key = (layout.name, mode, shape.name)
    if key not in _standins:
        obs, acts = MM.inputs(shape.case.o, shape.case.d, shape.h, layout)
        params = [MC.params_of(MM.shape_module(shape, k)) for k in range(layout.n_models)]
        _standins[key] = MM.Standin(params, spec or MM.plain_spec(shape.case.o), obs, acts, mode)
    return _standins[key]


def test_the_fault_table_names_every_fault():
    assert sorted(WHERE) == sorted(MM.LAUNCH_FAULTS)


@pytest.mark.parametrize("layout", MM.LAYOUTS, ids=lambda l: l.name)
def test_the_faithful_standin_is_accepted(layout):
    s = standin(layout)
    costs, states = s.launch(layout.problems)
    assert costs.shape == (sum(q[3] for q in layout.problems),) and np.isfinite(costs).all() and np.isfinite(states).all()
    assert MM.launch_mismatches(costs, states, layout.problems, s.solo(layout.problems)) == []
    assert MM.launch_mismatches(costs, None, layout.problems, s.solo(layout.problems)) == []
    assert len(np.unique(costs)) > 0.9 * len(costs) or layout.name == "three-coincide"   # the rows spread: a compared value is a row's own
    if layout.name == "three-coincide":   # one model for problems 0 and 2, another observation; another model for problem 1
        a, b, c = np.split(costs, 3)
        assert (a != b).all() and (a != c).all()


@pytest.mark.parametrize("mode", MM.MODE_NAMES)
def test_the_faithful_standin_is_accepted_in_every_cost_mode_and_with_the_term_list(mode):
    layout = MM.LAYOUT_BY_NAME["two-17-5"]
    s = standin(layout, mode)
    costs, states = s.launch(layout.problems)
    assert MM.launch_mismatches(costs, states, layout.problems, s.solo(layout.problems)) == []
    env = MM.HOPPER
    obs, acts = MM.inputs(env.o, env.d, 2, layout, seed=3)
    h = MM.Standin([MC.params_of(MM.hopper_module(k)) for k in range(2)], env.spec, 0.2 * obs, acts, mode)
    costs, states = h.launch(layout.problems)
    assert np.isfinite(costs).all() and MM.launch_mismatches(costs, states, layout.problems, h.solo(layout.problems)) == []


@pytest.mark.parametrize("fault", MM.LAUNCH_FAULTS)
def test_every_launch_fault_is_rejected(fault):
    for name in WHERE[fault]:
        layout = MM.LAYOUT_BY_NAME[name]
        s = standin(layout)
        costs, states = s.launch(layout.problems, fault=fault)
        found = MM.launch_mismatches(costs, states, layout.problems, s.solo(layout.problems))
        assert found, (fault, name)
        if fault != "states-stride-h":   # the costs alone show it: the launches without `observations` are covered too
            assert MM.launch_mismatches(costs, None, layout.problems, s.solo(layout.problems)), (fault, name)
        else:
            assert not MM.launch_mismatches(costs, None, layout.problems, s.solo(layout.problems)) and all("states" in f for f in found)


# ---- the ensemble ---------------------------------------------------------------------------------------------------------------------
def _member_costs(E, n):
    layout = MM._layout("ens", [n] * E, action_row0=[0] * E, obs_rows=[0] * E)
    s = standin(layout._replace(name=f"ens-{E}-{n}"))
    return s.launch(layout.problems)[0].reshape(E, n)


@pytest.mark.parametrize("E,n", [(1, 17), (2, 17), (5, 40)])
@pytest.mark.parametrize("reduce", ["mean", "max"])
def test_the_reduction_is_accepted_and_its_faults_rejected(E, n, reduce):
    mc = _member_costs(E, n)
    assert MM.ensemble_mismatches(mc, MM.standin_reduce(mc, reduce), mc, reduce) == []
    if E == 1:
        assert np.array_equal(MM.standin_reduce(mc, reduce), mc[0])   # one member: the solo bits
    if E == 5 and reduce == "mean":   # (at E = 2 the factor is a power of two: dividing first changes nothing)
        bad = MM.standin_reduce(mc, "mean", fault="mean-divides-first")
        assert MM.ensemble_mismatches(mc, bad, mc, "mean") == ["costs are not the restated mean of the members"]
        np.testing.assert_allclose(bad, mc.astype(np.float64).mean(0), rtol=1e-5)   # (a fault of rounding only)
    if E > 1:
        swapped = mc[::-1].copy()   # member rows in another order
        assert MM.ensemble_mismatches(swapped, MM.standin_reduce(swapped, reduce), mc, reduce)
        nan = mc.copy()
        nan[1] = np.nan             # a member whose parameters hold a NaN
        good = MM.standin_reduce(nan, reduce)
        assert np.isnan(good).all() and MM.ensemble_mismatches(nan, good, nan, reduce) == []
        if reduce == "max":
            bad = MM.standin_reduce(nan, "max", fault="max-ignores-nan")
            assert np.isfinite(bad).all() and MM.ensemble_mismatches(nan, bad, nan, "max") == ["costs are not the restated max of the members"]


def test_problem_major_order_is_rejected():
    """rollout_cost_batch's launch is member-major: member_costs [E, sum rows] is the launch's cost vector as it stands."""
    rows, E = [5, 17, 9], 3
    layout = MM._layout("batch", rows, models=[0, 1, 2])   # (three models, three observations, the planners' rows back to back)
    s = standin(layout)
    row0 = MM._back_to_back(rows)
    want = np.stack([np.concatenate([s.launch([(e, b, row0[b], rows[b])])[0] for b in range(len(rows))]) for e in range(E)])
    assert np.array_equal(s.batch(rows, E), want)
    assert not np.array_equal(s.batch(rows, E, fault="problem-major"), want)
    for reduce in ("mean", "max"):
        assert MM.ensemble_mismatches(s.batch(rows, E), MM.standin_reduce(want, reduce), want, reduce) == []
        assert MM.ensemble_mismatches(s.batch(rows, E, fault="problem-major"), MM.standin_reduce(want, reduce), want, reduce)
