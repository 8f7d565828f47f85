"""The test of the feed-forward learned-dynamics tests (no GPU): with the CPU emulation standing in for the kernel, (a) the
acceptance criterion of mlp_cases.py passes the reference pair on every case and the pair's worst values are the ones the bounds
were derived from, (b) every deliberately wrong variant of the rollout fails it on some case by a factor of ten, (c) the cost
criterion (cost_term_cases.py's, on the states the kernel itself would hand out) passes the f32 cost arithmetic and rejects
single faults of the cost, and the tables keep the properties that make them discriminating."""
import dataclasses

import numpy as np
import pytest

import cost_term_cases as CT
import mlp_cases as MC
from oracle import icem_oracle as O

ROWS = 128   # rows per launch for the mutants


# ---- (a) the reference pair ---------------------------------------------------------------------------------------------------
_pair = {}


def pair(case):
    if case.name not in _pair:
        want = MC.want(case)
        _pair[case.name] = [(MC.kernel_standin(case, seed=seed), want) for seed in (0, 1)]
    return _pair[case.name]


@pytest.mark.parametrize("case", MC.CASES, ids=lambda c: c.name)
def test_reference_pair_agrees(case):
    """The float32, K-blocked emulation with perturbed sigmoids against the float64 one: what the bounds were measured on passes
    them, with the pair's own numbers inside the constants of mlp_cases.py (so the bounds carry the factors they state)."""
    for got, want in pair(case):
        s = MC.errors(got, want)
        assert MC.agree(got, want), (MC.violations(got, want), s)
        assert s["median"] <= MC.PAIR_MEDIAN and s["share"] <= MC.PAIR_SHARE <= 0.16 and s["max"] <= MC.PAIR_MAX, s


def test_the_bounds_are_the_pairs_worst_values_with_their_factors():
    worst = dict(median=0.0, share=0.0, max=0.0)
    for case in MC.CASES:
        for got, want in pair(case):
            s = MC.errors(got, want)
            worst = {k: max(v, s[k]) for k, v in worst.items()}
    # the constants are the measurements rounded up, by no more than a tenth
    assert MC.PAIR_MEDIAN / 1.1 <= worst["median"] <= MC.PAIR_MEDIAN, worst
    assert MC.PAIR_SHARE / 1.1 <= worst["share"] <= MC.PAIR_SHARE, worst
    assert MC.PAIR_MAX / 1.1 <= worst["max"] <= MC.PAIR_MAX, worst
    assert MC.MEDIAN_BOUND == 4 * MC.PAIR_MEDIAN and MC.SHARE_CAP == 2 * MC.PAIR_SHARE <= 0.32 and MC.MAX_BOUND == 4 * MC.PAIR_MAX
    assert MC.ROW_BOUND == 2e-5


def test_every_relu_unit_is_active_somewhere_in_the_table():
    active = {}
    for case in MC.CASES:
        if case.act != "relu":
            continue
        P, seen = MC.params(case), {}
        MC.over_launches(case, lambda ob, a: MC.emulated_states(P, ob, a, q=MC.bf16, active=seen))
        for k, on in seen.items():
            active[k] = active.get(k, False) | on
    assert set(active) == {0, 1, 2, 3}
    for layer, on in active.items():
        assert on.shape == (200,) and on.all(), (layer, np.flatnonzero(~on))


def test_the_table_covers_the_edges_the_issue_names():
    cs = MC.CASES
    assert {c.o for c in cs} >= {1, 3, 16, 17, 32, 33, 39, 64} and {c.d for c in cs} == {1, 6, 32}
    assert {(c.L, c.act) for c in cs} >= {(L, a) for L in (1, 2, 4) for a in ("relu", "swish")}
    assert {c.n for c in cs} == {1, 13, 16, 17, 333, 1007} and {c.h for c in cs} == {1, 2, 12, 30}
    assert all(c.n * c.launches >= 96 for c in cs)   # a median over fewer rows says nothing


# ---- (b) the mutants of the rollout ---------------------------------------------------------------------------------------------
def _edit(fn):
    """fn(P, case) edits a copy of the parameters in place, or returns False where the case has no such entry."""
    def params(P, case):
        P = dict(P, W=[w.copy() for w in P["W"]], b=[b.copy() for b in P["b"]], Wout=P["Wout"].copy(), bout=P["bout"].copy())
        return None if fn(P, case) is False else P
    return params


def _hidden_unit(u):
    """Hidden unit u of the last hidden layer: its output row dropped / its column in the output layer dropped; and, where there is
    a second hidden layer, unit u of the first as a contraction column."""
    def row(P, case):
        P["W"][-1][u] = 0
        P["b"][-1][u] = 0

    def out_col(P, case):
        P["Wout"][:, u] = 0

    def k_col(P, case):
        if len(P["W"]) < 2:
            return False
        P["W"][1][:, u] = 0
    return {f"hidden unit {u}: output row dropped": dict(params=_edit(row)), f"hidden unit {u}: dropped from the output layer": dict(params=_edit(out_col)),
            f"hidden unit {u}: dropped from the second layer's contraction": dict(params=_edit(k_col))}


def _state_col(c):   # c: a column index, or -1 for obs_dim - 1
    def fn(P, case):
        k = case.o - 1 if c < 0 else c
        if k >= case.o or (c >= 0 and case.o <= 32 and c > 0):
            return False   # columns 31 / 32 are asked of the two-K-block cases
        P["W"][0][:, k] = 0
    return _edit(fn)


def _action_col(c):
    def fn(P, case):
        P["W"][0][:, case.o + (case.d - 1 if c < 0 else c)] = 0
    return _edit(fn)


def _out_unit(u):
    def fn(P, case):
        if u >= case.o:
            return False
        P["Wout"][u] = 0
        P["bout"][u] = 0
    return _edit(fn)


def _bias(layer):   # layer: 0 .. 3 hidden, -1 output; the last valid entry
    def fn(P, case):
        if layer >= len(P["b"]):
            return False
        if layer < 0:
            P["bout"][case.o - 1] = 0
        else:
            P["b"][layer][199] = 0
    return _edit(fn)


MUTANTS = {}
for _u in (0, 15, 16, 191, 192, 199):
    MUTANTS.update(_hidden_unit(_u))
MUTANTS.update({
    "state column 0 dropped": dict(params=_state_col(0)),
    "state column obs_dim - 1 dropped": dict(params=_state_col(-1)),
    "state column 31 dropped": dict(params=_state_col(31)),
    "state column 32 dropped": dict(params=_state_col(32)),
    "action column 0 dropped": dict(params=_action_col(0)),
    "action column act_dim - 1 dropped": dict(params=_action_col(-1)),
})
MUTANTS.update({f"output unit {u} not produced": dict(params=_out_unit(u)) for u in (15, 16, 31, 32, 47, 48, 63)})
MUTANTS.update({f"hidden layer {k + 1}: bias[199] dropped": dict(params=_bias(k)) for k in range(4)})
MUTANTS.update({
    "output layer: bias[obs_dim - 1] dropped": dict(params=_bias(-1)),
    "state kept in bf16": dict(state_q=MC.bf16),
    "residual dropped": dict(residual=False),
    "second hidden layer skipped": dict(skip_layer=1),
    "last hidden layer skipped": dict(skip_layer=-2),
    "relu and swish exchanged": dict(swap_act=True),
    "action of step t + 1": dict(action_shift=1),
    "action of step t - 1": dict(action_shift=-1),
})


def mutant_states(case, params=None, swap_act=False, skip_layer=-1, rows=ROWS, **kw):
    """The kernel stand-in of mlp_cases.py with one thing wrong (None: the case has nothing of the kind)."""
    P = MC.params(case)
    if params is not None:
        P = params(P, case)
        if P is None:
            return None
    if skip_layer != -1:
        skip_layer = case.L - 1 if skip_layer == -2 else skip_layer
        if not 1 <= skip_layer < case.L:
            return None
    if kw.get("action_shift") and case.h < 2:
        return None
    if swap_act:
        kw["act"] = "swish" if case.act == "relu" else "relu"
    return MC.kernel_standin(case, rows=rows, P=P, skip_layer=skip_layer, **kw)


_want = {}


def small_want(case):
    if case.name not in _want:
        _want[case.name] = MC.want(case, rows=ROWS)
    return _want[case.name]


@pytest.mark.parametrize("name", MUTANTS, ids=lambda s: s.replace(" ", "_"))
def test_every_mutant_fails_some_case_tenfold(name):
    """Both robust parts of the criterion -- the median, and the share part counted as the factor by which ROW_BOUND can grow with
    more than SHARE_CAP of the rows still above it -- each by a factor of at least 10, on one and the same case."""
    best = (0.0, None)
    for case in MC.CASES:
        got = mutant_states(case, **MUTANTS[name])
        if got is None:
            continue
        s = MC.errors(got, small_want(case))
        f = min(s["median"] / MC.MEDIAN_BOUND, s["quantile"] / MC.ROW_BOUND)
        if f > best[0]:
            best = (f, case.name)
        if f >= 10:
            return
    pytest.fail(f"{name}: best case {best[1]} misses by {best[0]:.3g} only")


# ---- (c) the costs --------------------------------------------------------------------------------------------------------------
MODES = ("sum", "best", "final")
_cost_ref = {}


def cost_ref(env, mode):
    """(cost_term_cases case, states, actions) of an environment and mode, the reference on the emulation's f32-rounded states."""
    key = (env.name, mode)
    if key not in _cost_ref:
        states = MC.cost_states(env).astype(np.float32).astype(np.float64)   # what a kernel would hand out: f32
        acts = MC.cost_actions(env)
        _cost_ref[key] = (MC.cost_case(f"mlp-cpu-{env.name}-{mode}", env.spec, mode, states, acts), states, acts)
    return _cost_ref[key]


@pytest.mark.parametrize("env", [e for e in MC.COST_ENVS if e.name not in MC.LOPSIDED], ids=lambda e: e.name)
def test_cost_envs_fire_every_comparison(env):
    """Every comparison of the spec comes out both ways (true on 5-95 % of the (row, step) pairs), and at most 5 % of the rows are
    near a threshold: the near-threshold exclusion leaves 95 % of every case under the row bound.  (cost_term_cases.py asks 1 % of
    its synthetic linear models; here the compared columns of Relocate and FetchPickAndPlace move by a few 1e-3 per step beside
    state entries of order 1 that set the row's scale, so more rows pass within NEAR x that scale of a threshold.)"""
    states = MC.cost_states(env)
    rates = MC.comparison_rates(env.spec, states)
    for name, r in rates.items():
        assert 0.05 <= r <= 0.95, (name, rates)
    case, _, _ = cost_ref(env, "sum")
    assert CT.near(case).mean() <= 0.05, CT.near(case).mean()
    assert np.abs(states).max() < 20


def test_the_cost_table_names_the_environments_of_the_issue():
    assert {e.name.split("-")[0] for e in MC.COST_ENVS} == {"halfcheetah", "hopper", "reacher", "fetchreach", "fpp", "door", "relocate"}
    shapes = {e.name: (e.o, e.d) for e in MC.COST_ENVS}
    assert shapes["halfcheetah"] == (17, 6) and shapes["hopper"] == (12, 3) and shapes["reacher"] == (11, 2)
    assert shapes["fetchreach-sparse"] == (13, 4) and shapes["fpp-sparse"] == (28, 4) and shapes["door"] == (39, 28) and shapes["relocate"] == (39, 30)


def test_lopsided_best_cases_favour_the_first_and_the_last_step():
    for name, step in MC.LOPSIDED.items():
        env = MC.COST_ENV_BY_NAME[name]
        c = MC.step_costs(env.spec, MC.cost_states(env), MC.cost_actions(env))
        hist = np.bincount(c.argmin(1), minlength=2) / len(c)
        assert env.h == 2 and 0.6 <= hist[step] <= 0.85, (name, hist)


@pytest.mark.parametrize("env", MC.COST_ENVS, ids=lambda e: e.name)
@pytest.mark.parametrize("mode", MODES)
def test_the_f32_cost_arithmetic_passes_the_cost_criterion(env, mode):
    case, states, acts = cost_ref(env, mode)
    got = MC.costs_f32(env.spec, mode, states, acts)
    assert CT.agree(got, case), (CT.violations(got, case), CT.errors(got, case))


def _spec_mutants(spec):
    """{name: a spec with one thing wrong} -- every part of the cost that weighs at least 1e-3 (Door's 30-entry velocity term at
    weight 1e-5 is below what any table can see: cost_term_cases.py says so of its own)."""
    rep = dataclasses.replace
    out = {}
    if spec.ctrl_weight:
        out["ctrl_weight x 1.5"] = rep(spec, ctrl_weight=1.5 * spec.ctrl_weight)
    if spec.lin_weight:
        out["lin_weight x 1.5"] = rep(spec, lin_weight=1.5 * spec.lin_weight)
        out["lin_idx + 1"] = rep(spec, lin_idx=spec.lin_idx + 1)
    if spec.flip_idx >= 0:
        out["flip_thresh x 0.7"] = rep(spec, flip_thresh=0.7 * spec.flip_thresh)
        out["flip_penalty x 0.5"] = rep(spec, flip_penalty=0.5 * spec.flip_penalty)
        out["flip: the negative side dropped"] = ("flip_pos_only", spec)
    if spec.diff_idx >= 0:
        out["diff_weight x 1.1"] = rep(spec, diff_weight=1.1 * spec.diff_weight)
        out["diff_idx + 1"] = rep(spec, diff_idx=spec.diff_idx + 1)
        out["difference term dropped"] = rep(spec, diff_idx=-1)
    if spec.health_idx >= 0:
        out["health_penalty x 0.5"] = rep(spec, health_penalty=0.5 * spec.health_penalty)
        out["health_lo + 0.1"] = rep(spec, health_lo=spec.health_lo + 0.1)
        out["health_idx + 1"] = rep(spec, health_idx=spec.health_idx + 1)
        if spec.box_from >= 0:
            out["box x 0.8"] = rep(spec, box_lo=0.8 * spec.box_lo, box_hi=0.8 * spec.box_hi)
            out["box dropped"] = rep(spec, box_from=-1)
            out["box_from + 9"] = rep(spec, box_from=spec.box_from + 9)
    for j, tm in enumerate(spec.terms):
        if abs(tm.weight) < 1e-3:
            continue

        def with_term(**kw):
            return rep(spec, terms=spec.terms[:j] + (rep(tm, **kw),) + spec.terms[j + 1:])
        out[f"term {j}: weight x 1.5"] = with_term(weight=1.5 * tm.weight)
        out[f"term {j}: dropped"] = rep(spec, terms=spec.terms[:j] + spec.terms[j + 1:])
        out[f"term {j}: a + 1"] = with_term(a=tm.a + 1) if tm.a + tm.len < 39 and (tm.b < 0 or tm.b + tm.len < 39) else None
        if tm.len > 1:
            out[f"term {j}: len - 1"] = with_term(len=tm.len - 1)
        if tm.b >= 0:
            out[f"term {j}: second slice dropped"] = with_term(b=-1)
        if tm.kind in (O.TERM_NORM_GT, O.TERM_NORM_LT, O.TERM_STEP_GT, O.TERM_SQ_OFFSET) and tm.thresh:
            out[f"term {j}: thresh x 0.7"] = with_term(thresh=0.7 * tm.thresh)
        if tm.gate_idx >= 0:
            out[f"term {j}: gate dropped"] = with_term(gate_idx=-1)
            out[f"term {j}: gate_thresh x 0.5"] = with_term(gate_thresh=0.5 * tm.gate_thresh)
    return {k: v for k, v in out.items() if v is not None}


def _mutant_costs(m, env, mode, states, acts):
    if isinstance(m, tuple):   # the flip penalty on the positive side only
        full = MC.costs_f32(m[1], mode, states, acts)
        if mode != "sum":
            return None
        neg = (states[:, :-1, m[1].flip_idx] < -m[1].flip_thresh).sum(1)
        return full - m[1].flip_penalty * neg
    if m.lin_idx >= env.o or m.diff_idx >= env.o or m.health_idx >= env.o or m.box_from >= env.o:
        return None
    if any(t.a + t.len > env.o for t in m.terms):
        return None
    return MC.costs_f32(m, mode, states, acts)


def _rejected(got, case) -> bool:
    factor, count = CT.rejection(got, case)
    return factor >= 10 or count >= 10


@pytest.mark.parametrize("env", [e for e in MC.COST_ENVS if e.name not in MC.LOPSIDED], ids=lambda e: e.name)
def test_single_faults_of_the_cost_are_rejected(env):
    """cost_term_cases.py's convention: a wrong evaluation misses the row or the median bound by a factor >= 10 or leaves >= 10 rows
    that are not near a threshold out of bound, under some reduction."""
    survivors = []
    for name, m in _spec_mutants(env.spec).items():
        seen = False
        for mode in MODES:
            case, states, acts = cost_ref(env, mode)
            got = _mutant_costs(m, env, mode, states, acts)
            if got is None:
                continue
            seen = True
            if _rejected(got, case):
                break
        else:
            if seen:
                survivors.append(name)
    assert not survivors, survivors


def _reduced(spec, mode, states, acts, steps):
    """The f32 costs reduced over a slice of the steps only."""
    s32, a32 = np.asarray(states, np.float32), np.asarray(acts, np.float32)
    return O.spec_trajectory_costs(spec, s32[:, :-1][:, steps], a32[:, steps], s32[:, 1:][:, steps] if spec.needs_next_obs else None,
                                   mode=mode, dtype=np.float32).astype(np.float64)


@pytest.mark.parametrize("what,steps", [("steps 1 .. h-1", slice(1, None)), ("steps 0 .. h-2", slice(0, -1))])
def test_a_reduction_that_leaves_out_a_step_is_rejected(what, steps):
    """'best' at h = 2 with most minima on the step that is left out; 'sum' and 'final' on the h = 12 HalfCheetah case."""
    lop = MC.COST_ENV_BY_NAME["halfcheetah-best-first" if steps.start else "halfcheetah-best-last"]
    case, states, acts = cost_ref(lop, "best")
    assert _rejected(_reduced(lop.spec, "best", states, acts, steps), case), what
    env = MC.COST_ENV_BY_NAME["halfcheetah"]
    for mode in ("sum",) if steps.start else ("sum", "final"):
        case, states, acts = cost_ref(env, mode)
        assert _rejected(_reduced(env.spec, mode, states, acts, steps), case), (what, mode)


@pytest.mark.parametrize("shift", [1, -1])
def test_the_control_cost_of_a_neighbouring_steps_action_is_rejected(shift):
    env = MC.COST_ENV_BY_NAME["halfcheetah"]
    case, states, acts = cost_ref(env, "sum")
    idx = np.clip(np.arange(env.h) + shift, 0, env.h - 1)
    assert _rejected(MC.costs_f32(env.spec, "final", states, acts[:, idx]), cost_ref(env, "final")[0]) or \
        _rejected(MC.costs_f32(env.spec, "best", states, acts[:, idx]), cost_ref(env, "best")[0])
    assert case is not None


def test_the_control_cost_on_bf16_actions_is_rejected():
    """The control cost is taken on the f32 actions, not on the bf16 operands the input layer sees."""
    env = MC.COST_ENV_BY_NAME["reacher"]   # (no control cost there: nothing to see) -- and HalfCheetah, where there is
    env = MC.COST_ENV_BY_NAME["halfcheetah"]
    case, states, acts = cost_ref(env, "sum")
    got = MC.costs_f32(dataclasses.replace(env.spec, lin_weight=0.0, flip_idx=-1), "sum", states, MC.bf16(acts)) \
        - MC.costs_f32(dataclasses.replace(env.spec, lin_weight=0.0, flip_idx=-1), "sum", states, acts) + MC.costs_f32(env.spec, "sum", states, acts)
    assert _rejected(got, case), CT.rejection(got, case)
