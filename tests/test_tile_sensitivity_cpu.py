"""The test of the tile probes (no GPU): with a float32 CPU evaluation standing in for the tile kernels, the per-row criterion
passes the reference pair on every case of tile_cases.py, the table keeps the properties that make it discriminating (rows near
a threshold are rare, both signs of every flip case fire, every entry the entry group claims lies on a path into a scored
unit), every deliberately wrong model step is rejected on some case by a factor of ten -- and the criterion the tile kernels
were held to before (dense model, HalfCheetah's cost, 1e-5 of the sum's magnitude with a share allowance) accepts a list of them.

The reference pair, worst over the table (two seeds; per group in the output of test_reference_pair_agrees):
    row error 1.77e-6 (h30d6o17-unit0-k0-final)      median 7.75e-7 (h30d6o17-scale-obs30-unit0)
    state error 4.02e-6 of the row's largest |state entry| (h30d6o18-scale-obs30-unit0)
    by group, row / median / state:  unit 1.77e-6 / 5.83e-7 / 2.41e-6   flip 1.34e-6 / 1.22e-7 / 3.07e-6   scale 1.27e-6 / 7.75e-7 / 4.02e-6
                                     entry 9.35e-7 / 2.48e-7 / 1.05e-6   action 1.32e-7 / 4.5e-8 / 2.49e-7   control 1.17e-7 / 3.0e-8 / 0
The median and the state error leave cost_term_cases.MEASURED_MEDIAN / _STATE (3.5e-7 / 3.4e-6): tile_cases.py carries
constants of its own, these values x 4 (ROW_BOUND 7.2e-6 <= 1e-5, MEDIAN_BOUND 3.1e-6, NEAR 1.64e-5).

The mutants (285 single faults of the float64 oracle, test_mutants_are_rejected prints each with its factor and case): two start
observation entries swapped; one model entry -- tile -> tile, tile -> extra, extra -> tile, extra -> extra (o = 18), action ->
tile, action -> extra, the last action of the partial group, the second tile of O = 24 -- zeroed, x 1.01, rounded to 11 bits,
moved to the neighbouring row / column; a padded column read as non-zero (obs_dim 19); action 0 read as action 1; the action of
the step in front of a chunk boundary read as the next step's; the control cost without the last action entry / the last step /
with state entry 16 counted in; extra column 16 one step stale / not through tanh / doubled under the scale cases; final at
h - 2, best without the first step, sum without the last; the flip read from column 0; one sign only; the last row of the ragged
tile scored with its neighbour's actions.  Every one is rejected.  Weakest: an entry's low plane dropped (rounded to 11 bits) --
x 7.6 .. x 27 on the low-plane shift cases, every row out of bound (A[16][15] at o = 17: x 7.57); an entry x 1.01: x 19.6 and
more; everything else by x 26 and more.
What the table cannot see: a low plane dropped from an OFF-DIAGONAL entry of the dense model alone (0.012: 2^-12 of it moves a
state entry by 3e-6 of another per step -- x 0.6 .. x 1.4 of the bound on the unit readouts); the low-plane shift cases of the
entry group exist for that reason, and reject the same fault in every class of entry.  The chunk-boundary fault has no case at
(12,6,17) and (13,4,17): their actions are staged as a single chunk.  What it does not ask: accuracy relative to a state that stays
orders of magnitude below max(|obs0|, action bound) for the whole horizon -- the planes promise 2^-25 absolute at that scale
(fused_dev.h), the 22-bit stand-in does not model it, and the B = 0 scale cases keep the bound at the observation's scale
(EXPERIMENTS.md R11.1 has the figure of the case that did not).

What the criterion in force accepted (test_the_criterion_in_force_accepted_these: dense model, HalfCheetah's cost --
HumanoidStandup's at o = 24 --, 257 rows, every row within 1e-5 of the sum's magnitude, max(2, N // 50) rows near a threshold
excused; in all of sum / best / final it was run in): a dropped low plane in EVERY class of entry but action -> tile -- A[3][4],
A[15][16], A[16][15], A[16][17], A[17][16], A[19][20], B[5][16], B[4][16], B[5][17], B[9][16], B[16][23] -- and A[16][17] x 1.01 at
o = 18 (ACCEPTED_BEFORE below).  It rejects the zeroed and moved entries, the swapped start entries and the stale column: on a
dense model they reach the scored column within two steps.  What it could not do is NAME anything: every failure is one number
on a cost that mixes every column.
"""
import dataclasses

import numpy as np
import pytest

import cost_term_cases as CC
import tile_cases as TC
from oracle import icem_oracle as O

_measured = {}


# ---- (a) the reference pair ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", TC.GROUPS)
def test_reference_pair_agrees(group):
    """kernel_standin (f32, model entries and per-step states rounded to 22 bits; two seeds) against the float64 oracle: what
    the bounds were measured on passes them, with the factor of 4 tile_cases.py states."""
    worst = dict(row=0.0, median=0.0, state=0.0, row_case="", median_case="", state_case="")
    cases = TC.by_group(group)
    for case in cases:
        for seed in (0, 1):
            got, state_err = CC.kernel_standin(case, seed)
            state = float(np.nanmax(state_err)) if np.isfinite(state_err).any() else 0.0   # (control: the state is zero throughout)
            s = CC.errors(got, case, TC.BOUNDS)
            assert CC.agree(got, case, TC.BOUNDS), (case.name, seed, CC.violations(got, case, TC.BOUNDS))
            assert state <= TC.BOUNDS.near, (case.name, state)
            for key, v in (("row", s["worst"]), ("median", s["median"]), ("state", state)):
                if v > worst[key]:
                    worst[key], worst[key + "_case"] = v, case.name
    TC.forget(cases)
    _measured[group] = worst
    print(f"reference pair, {group}: worst row error {worst['row']:.3g} ({worst['row_case']}), median {worst['median']:.3g} "
          f"({worst['median_case']}), state error {worst['state']:.3g} ({worst['state_case']})")
    # what was measured stays what the docstring says: the bounds ARE 4 x those numbers
    assert worst["row"] <= TC.MEASURED_ROW and worst["median"] <= TC.MEASURED_MEDIAN and worst["state"] <= TC.MEASURED_STATE


def test_bounds_are_what_the_docstring_says():
    """The table's own constants: the reference pair leaves cost_term_cases.MEASURED_MEDIAN / _STATE (the docstring of
    tile_cases.py says where), so they are the newly measured values x 4; the row bound stays under 1e-5."""
    assert TC.BOUNDS == CC.Bounds(4 * TC.MEASURED_ROW, 4 * TC.MEASURED_MEDIAN, 4 * TC.MEASURED_STATE)
    assert TC.BOUNDS.row <= 1e-5
    assert TC.MEASURED_MEDIAN > CC.MEASURED_MEDIAN and TC.MEASURED_STATE > CC.MEASURED_STATE   # (else: that module's bounds as they are)
    assert (CC.MEASURED_ROW, CC.MEASURED_MEDIAN, CC.MEASURED_STATE) == (1.8e-6, 3.5e-7, 3.4e-6)   # untouched
    for key in ("MEASURED_ROW", "MEASURED_MEDIAN", "MEASURED_STATE"):
        assert f"{getattr(TC, key):.2g}".replace("e-0", "e-") in TC.__doc__, key


# ---- (b) the input conditions, from the oracle alone ---------------------------------------------------------------------
def test_table_shape():
    """Every compiled shape, every group; every launch <= 1100 rows with a ragged last tile, more than one tile but for the
    1-row cases; every cost is one the tile serves."""
    assert {TC.shape_of(c) for c in TC.CASES} == set(TC.SHAPES)
    assert {(30, 6, 17), (30, 6, 18), (12, 6, 17), (13, 4, 17), (30, 17, 24), (30, 17, 19)} == set(TC.SHAPES)
    for sh in TC.SHAPES:
        groups = {c.group for c in TC.CASES if TC.shape_of(c) == sh}
        assert groups == {f"{g}-{TC.tag(sh)}" for g in ("unit", "flip", "action", "control", "entry", "scale")}, sh
        assert sum(1 for c in TC.CASES if TC.shape_of(c) == sh and c.n == 1) == 1
    for c in TC.CASES:
        assert c.n <= 1100 and c.n % 16 and (c.n > 16 or c.n == 1), c.name
        assert not c.spec.terms and c.spec.lin_weight != 0 and not c.spec.extended, c.name
    neg = [c for c in TC.CASES if c.spec.flip_idx >= 0 and c.spec.flip_thresh < 0]
    assert len(neg) == len(TC.SHAPES)


def test_near_threshold_rows_are_rare_and_both_flip_signs_fire():
    for case in TC.CASES:
        if case.spec.flip_idx < 0:
            continue   # (no comparison: no row is near a threshold)
        share = CC.near(case, TC.BOUNDS).mean()
        assert share <= 0.01, (case.name, share)
        shares = O.observation_comparison_shares(case.spec, CC.reference(case)["obs"])
        assert set(shares) == {"flip>", "flip<"} and all(0.1 <= v <= 0.9 for v in shares.values()), (case.name, shares)
        TC.forget([case])
    readout = next(c for c in TC.CASES if c.group.startswith("unit"))
    assert not CC.near(readout, TC.BOUNDS).any()
    TC.forget([readout])


@pytest.mark.parametrize("shape", TC.SHAPES, ids=TC.tag)
def test_every_entry_lies_on_a_path_into_a_scored_unit(shape):
    """The coverage condition of the entry group, from the sparsity pattern alone: every entry a case claims is non-zero in
    its model and reaches the unit the case scores inside the horizon; together the cases claim every position of [A ; B]."""
    h, d, o = shape
    seen = set()
    for case in TC.by_group(f"entry-{TC.tag(shape)}"):
        assert case.claims and not TC.uncovered_claims(case), (case.name, TC.uncovered_claims(case))
        if case.model[2] == 0:
            A, B = case.matrices()
            w = np.concatenate([A[A != 0], B[B != 0]])
            assert len(set(np.abs(w))) == len(w) and np.all((np.abs(w) >= 0.9) & (np.abs(w) <= 1.0)), case.name
            assert np.array_equal(w.astype(np.float16).astype(np.float64), w) and (w > 0).any() and (w < 0).any(), case.name
            seen |= set(case.claims)
    assert seen == {("A", i, j) for i in range(o) for j in range(o)} | {("B", j, c) for j in range(d) for c in range(o)}
    # ... and the check is not vacuous: one step less and the longest cycle's first entry is out of reach
    long = TC.BY_NAME[f"{TC.tag(shape)}-shiftA1-unit0"]
    short = dataclasses.replace(long, h=min(h, len(long.claims)))
    assert TC.uncovered_claims(short)


# ---- (c) the mutants ------------------------------------------------------------------------------------------------------
def q11(x):
    """x rounded to 11 significant bits: what is left of an operand whose low fp16 plane is dropped."""
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    return np.ldexp(np.round(m * 2.0 ** 11) / 2.0 ** 11, e)


def evaluate(om, spec, ob, acts, mode, *, ctrl_acts=None, steps=slice(None), one_sign=False, pre_fault=None, post_fault=None,
             ctrl_state=None):
    """The float64 oracle with a fault switched on.  pre_fault(t, x, prev, pre) -> the pre-activation of step t (x, prev: the
    state of this and of the step before), post_fault(t, pre, nxt) -> the new state; ctrl_acts: what the control cost sees;
    ctrl_state: a state entry the control cost counts as well; steps: what the reduction runs over."""
    n, h, _ = acts.shape
    ca = acts if ctrl_acts is None else ctrl_acts
    sp = dataclasses.replace(spec, flip_idx=-1) if one_sign else spec
    x = np.broadcast_to(ob, (n, len(ob))).copy()
    prev = x
    C = np.empty((n, h))
    for t in range(h):
        pre = x @ om.A + acts[:, t] @ om.B
        if pre_fault is not None:
            pre = pre_fault(t, x, prev, pre)
        nxt = np.tanh(pre) if om.kind == O.MODEL_TANH else pre
        if post_fault is not None:
            nxt = post_fault(t, pre, nxt)
        c = O._step_cost(sp, x, ca[:, t], None, np.float64)
        if one_sign:
            c = c + (x[:, spec.flip_idx] > spec.flip_thresh) * spec.flip_penalty
        if ctrl_state is not None:
            c = c + spec.ctrl_weight * x[:, ctrl_state] ** 2
        C[:, t] = c
        prev, x = x, nxt
    C = C[:, steps]
    return C.sum(1) if mode == "sum" else C.min(1) if mode == "best" else C[:, -1]


def _model_with(om, fn):
    A, B = om.A.copy(), om.B.copy()
    fn(A, B)
    return O.SyntheticModel(A, B, om.kind)


def _entry_fault(which, M, i, j):
    """One entry of A or B (``M``): zeroed, x 1.01, its low plane dropped, swapped with the neighbouring row's / column's."""
    def fn(A, B):
        X = A if M == "A" else B
        i2, j2 = (i + 1) % X.shape[0], (j + 1) % X.shape[1]
        if which == "zeroed":
            X[i, j] = 0.0
        elif which == "x 1.01":
            X[i, j] *= 1.01
        elif which == "rounded to 11 bits":
            X[i, j] = q11(X[i, j])
        elif which == "moved to the neighbouring row":
            X[i, j], X[i2, j] = X[i2, j], X[i, j]
        else:
            X[i, j], X[i, j2] = X[i, j2], X[i, j]
    return fn


ENTRY_FAULTS = ("zeroed", "x 1.01", "rounded to 11 bits", "moved to the neighbouring row", "moved to the neighbouring column")


def _named(names):
    return [TC.BY_NAME[n] for n in names if n in TC.BY_NAME]


def _units(sh, ks, kinds=(0,), modes=("sum",)):
    return _named(f"{TC.tag(sh)}-unit{k}-k{kind}-{mode}" for k in ks for kind in kinds for mode in modes)


def _claiming(sh, entry):
    """The entry cases of the shape (scale repeats excluded) that claim ``entry``, and the dense unit case that reads its column."""
    return [c for c in TC.by_group(f"entry-{TC.tag(sh)}") if entry in c.claims] + _units(sh, (entry[2],), (0, 1), ("sum", "final"))


def entry_classes(sh):
    """(class, entry): one representative per kind of path through the tile, in natural units (reading unit k moves it to column 0
    and the units below it one column up: which entries sit in the extra columns changes from case to case, the classes name
    where they sit in the k = 0 cases)."""
    h, d, o = sh
    s = o - d
    out = [("tile -> tile", ("A", 3, 4)), ("tile -> extra", ("A", 15, 16)), ("extra -> tile", ("A", 16, 15)),
           ("action -> tile", ("B", 2, 2)), ("action -> extra", ("B", 16 - s, 16)), ("the last action of the partial group", ("B", d - 1, o - 1))]
    if o == 18:
        out += [("extra -> extra", ("A", 16, 17)), ("extra -> extra", ("A", 17, 16))]
    if o > 20:
        out += [("the second tile of O = 24", ("A", 19, 20))]
    return out


def all_mutants():
    """[(label, [cases it may be rejected on], case -> evaluate-kwargs (``om`` / ``ob`` / ``acts`` / ``spec`` replace the case's))]"""
    out = []
    for sh in TC.SHAPES:
        h, d, o = sh
        tg = TC.tag(sh)
        flips = TC.by_group(f"flip-{tg}")
        ctrl = TC.by_group(f"control-{tg}")
        actions = [c for c in TC.by_group(f"action-{tg}") if c.mode == "sum"]
        dense = _units(sh, (0, 1, 3, 16), (0, 1), ("sum", "final"))

        def swap(a, b):
            def kw(case):
                x = CC.inputs(case)[1].copy()
                x[[a, b]] = x[[b, a]]
                return dict(ob=x)
            return kw
        out.append((f"{tg}: start observation entries 0 and 1 swapped (tile / tile)", dense, swap(0, 1)))
        out.append((f"{tg}: start observation entries 3 and 16 swapped (tile / extra column)", dense, swap(3, 16)))
        for cls, entry in entry_classes(sh):
            for which in ENTRY_FAULTS:
                out.append((f"{tg}: {entry[0]}[{entry[1]}][{entry[2]}] ({cls}) {which}", _claiming(sh, entry),
                            lambda case, f=_entry_fault(which, *entry): dict(om=_model_with(CC.inputs(case)[0], f))))
        if o == 19:   # the padding of the second output tile: entry 19 of the staged observation and row 19 of the packed model are zero
            def padded(case):
                om, ob, _ = CC.inputs(case)
                return dict(pre_fault=lambda t, x, prev, pre: pre + (ob[0] * om.A[18] if t == 0 else 0.0))
            out.append((f"{tg}: a padded column read as non-zero (slot 19 starts from obs0[0] and feeds the model through row 18's weights)",
                        dense + _units(sh, (18,), (0, 1), ("sum", "final")), padded))

        def shifted_action(case):
            a = CC.inputs(case)[2].copy()
            a[..., 0] = a[..., 1]
            return dict(acts=a, ctrl_acts=a)
        out.append((f"{tg}: action 0 read as action 1", [c for c in actions if "-act0-" in c.name] + ctrl, shifted_action))
        tc = TC.chunk_steps(h, d)
        if tc < h:
            def next_chunk(case, tc=tc):
                a = CC.inputs(case)[2].copy()
                a[:, tc - 1] = a[:, tc]
                return dict(acts=a, ctrl_acts=a)
            out.append((f"{tg}: the action of step {tc - 1} read as step {tc}'s (the chunk boundary only)", ctrl + actions, next_chunk))
        for label, sel in (("action entry", lambda a: a[..., -1]), ("step", lambda a: a[:, -1])):
            def without(case, sel=sel):
                a = CC.inputs(case)[2].copy()
                sel(a)[...] = 0
                return dict(ctrl_acts=a)
            out.append((f"{tg}: control cost without the last {label}", ctrl, without))
        out.append((f"{tg}: control cost that also counts state entry 16", flips, lambda case: dict(ctrl_state=16)))
        reads16 = dense + _named(f"{tg}-shiftA1-unit{k}" for k in range(o)) + _named(f"{tg}-shiftA1-lo-unit{k}" for k in range(o))

        def stale(case):
            A = CC.inputs(case)[0].A
            return dict(pre_fault=lambda t, x, prev, pre: pre + (prev[:, 16:17] - x[:, 16:17]) * A[16])
        out.append((f"{tg}: extra column 16 carried one step stale", reads16, stale))
        out.append((f"{tg}: extra column 16 not passed through tanh", _units(sh, (0, 1, 3, 16), (1,), ("sum", "final")),
                    lambda case: dict(post_fault=lambda t, pre, nxt: np.concatenate([nxt[:, :16], pre[:, 16:17], nxt[:, 17:]], axis=1))))

        def doubled(case):
            A = CC.inputs(case)[0].A
            return dict(pre_fault=lambda t, x, prev, pre: pre + x[:, 16:17] * A[16])
        out.append((f"{tg}: extra column 16 off by a factor 2 (the scale cases only)", TC.by_group(f"scale-{tg}"), doubled))
        out.append((f"{tg}: final taken at step h - 2", _units(sh, (0, 16), (0, 1), ("final",)), lambda case: dict(steps=slice(0, case.h - 1))))
        out.append((f"{tg}: best without the first step", [c for c in TC.by_group(f"unit-{tg}") + flips if c.mode == "best"],
                    lambda case: dict(steps=slice(1, None))))
        out.append((f"{tg}: sum without the last step", _units(sh, (0, 16), (0, 1)), lambda case: dict(steps=slice(0, case.h - 1))))
        out.append((f"{tg}: flip read from column 0 where flip_idx != lin_idx", [c for c in flips if c.spec.flip_idx != c.spec.lin_idx],
                    lambda case: dict(spec=dataclasses.replace(case.spec, flip_idx=case.spec.lin_idx))))
        out.append((f"{tg}: flip firing on one sign only", flips, lambda case: dict(one_sign=True)))

        def neighbour(case):
            a = CC.inputs(case)[2].copy()
            a[-1] = a[-2]
            return dict(acts=a, ctrl_acts=a)
        out.append((f"{tg}: the last row of the ragged tile scored with its neighbour's actions", dense, neighbour))
    return out


MUTANTS = all_mutants()
# mutants the table cannot reject, by label (the module docstring says what it cannot see and why): none of the list above
UNSEEN = set()


def _rejection(label, cases, make_kw):
    best = (0.0, 0, None)
    for case in cases:
        om, ob, acts = CC.inputs(case)
        kw = dict(make_kw(case))
        got = evaluate(kw.pop("om", om), kw.pop("spec", case.spec), kw.pop("ob", ob), kw.pop("acts", acts), case.mode, **kw)
        factor, count = CC.rejection(got, case, TC.BOUNDS)
        if (factor >= 10, factor) > (best[0] >= 10, best[0]) or (best[0] < 10 and count > best[1]):
            best = (factor, count, case.name)
        if factor >= 10:
            break
    return best


@pytest.mark.parametrize("shape", TC.SHAPES, ids=TC.tag)
def test_mutants_are_rejected(shape):
    """Every wrong model step misses the row or the median bound by a factor >= 10 on some case (or leaves >= 10 rows that are
    not near a threshold out of bound); each line of the output names the mutant, its factor and the case."""
    failed = []
    mine = [m for m in MUTANTS if m[0].startswith(TC.tag(shape) + ":")]
    assert len(mine) >= 45
    for label, cases, make_kw in mine:
        assert cases, label
        factor, count, where = _rejection(label, cases, make_kw)
        line = f"mutant [{label}]: bound missed x {factor:.3g}, {count} rows out of bound, on {where}"
        print(line)
        if not (factor >= 10 or count >= 10) and label not in UNSEEN:
            failed.append(line)
    TC.forget([c for c in TC.CASES if TC.shape_of(c) == shape])
    assert not failed, "\n".join(failed)


def test_the_unmutated_oracle_passes_with_factor_zero():
    for case in [TC.by_group(g)[i] for g in TC.GROUPS for i in (0, -1)]:
        om, ob, acts = CC.inputs(case)
        factor, count = CC.rejection(evaluate(om, case.spec, ob, acts, case.mode), case, TC.BOUNDS)
        assert factor < 1e-6 and count == 0, (case.name, factor)
        TC.forget([case])


# ---- (d) what the criterion in force accepted -------------------------------------------------------------------------------
_old = {}
OLD_ROWS = 257   # test_gpu_shape_edges.py's N_ROWS: 16 whole tiles and one row


def _old_inputs(o, d, kind):
    """The inputs the tile kernels were tested on: the dense benchmark model, HalfCheetah's cost (HumanoidStandup's at o = 24),
    a start observation of 0.2 N(0, 1), actions uniform in [-1, 1], h = 30."""
    if (o, d, kind) not in _old:
        om = O.SyntheticModel.make(o, d, kind)
        spec = O.CostSpec.halfcheetah(o) if o <= 18 else O.CostSpec.humanoid_standup()
        rs = np.random.RandomState(30 * 1000 + d * 10 + o)
        f = lambda x: np.asarray(x).astype(np.float32).astype(np.float64)  # noqa: E731
        ob, acts = f(0.2 * rs.randn(o)), f(rs.uniform(-1, 1, (OLD_ROWS, 30, d)))
        obs = O.rollout_observations(om, ob, acts)
        _old[o, d, kind] = (om, spec, ob, acts, O.rollout_cost_magnitudes(om, spec, ob, acts), O.observation_margins(spec, obs))
    return _old[o, d, kind]


def old_criterion_accepts(o, d, kind, mode, fault):
    """1e-5 of the sum-mode magnitude on every row away from a threshold (within 1e-4 of the state's scale counts as near: more
    than the tests allowed), at most max(2, N // 50) rows near one off the bar."""
    om, spec, ob, acts, mag, margin = _old_inputs(o, d, kind)
    want = evaluate(om, spec, ob, acts, mode)
    kw = fault(om, ob, acts)
    got = evaluate(kw.pop("om", om), spec, kw.pop("ob", ob), kw.pop("acts", acts), mode, **kw)
    bad = np.abs(got - want) > 1e-5 * mag
    return not (bad & (margin > 1e-4)).any() and bad.sum() <= max(2, OLD_ROWS // 50)


def old_faults(o, d):
    """(label, (om, ob, acts) -> evaluate-kwargs): the model-step faults of the list above that have a meaning on the old inputs."""
    for cls, entry in entry_classes((30, d, o)):
        for which in ENTRY_FAULTS:
            yield (f"{entry[0]}[{entry[1]}][{entry[2]}] ({cls}) {which}",
                   lambda om, ob, acts, f=_entry_fault(which, *entry): dict(om=_model_with(om, f)))

    def swapped(om, ob, acts):
        x = ob.copy()
        x[[3, 16]] = x[[16, 3]]
        return dict(ob=x)
    yield "start observation entries 3 and 16 swapped", swapped
    yield ("extra column 16 carried one step stale",
           lambda om, ob, acts: dict(pre_fault=lambda t, x, prev, pre: pre + (prev[:, 16:17] - x[:, 16:17]) * om.A[16]))
    yield ("extra column 16 not passed through tanh (the tanh cases)",
           lambda om, ob, acts: dict(post_fault=lambda t, pre, nxt: np.concatenate([nxt[:, :16], pre[:, 16:17], nxt[:, 17:]], axis=1)))

    def shifted(om, ob, acts):
        a = acts.copy()
        a[..., 0] = a[..., 1]
        return dict(acts=a, ctrl_acts=a)
    yield "action 0 read as action 1", shifted

    def neighbour(om, ob, acts):
        a = acts.copy()
        a[-1] = a[-2]
        return dict(acts=a, ctrl_acts=a)
    yield "the last row scored with its neighbour's actions", neighbour


ACCEPTED_BEFORE = (
    'o = 17: A[3][4] (tile -> tile) rounded to 11 bits',
    'o = 17: A[15][16] (tile -> extra) rounded to 11 bits',
    'o = 17: A[16][15] (extra -> tile) rounded to 11 bits',
    'o = 17: B[5][16] (action -> extra) rounded to 11 bits',
    'o = 17: B[5][16] (the last action of the partial group) rounded to 11 bits',
    'o = 18: A[3][4] (tile -> tile) rounded to 11 bits',
    'o = 18: A[15][16] (tile -> extra) rounded to 11 bits',
    'o = 18: A[16][15] (extra -> tile) rounded to 11 bits',
    'o = 18: B[4][16] (action -> extra) rounded to 11 bits',
    'o = 18: B[5][17] (the last action of the partial group) rounded to 11 bits',
    'o = 18: A[16][17] (extra -> extra) x 1.01',
    'o = 18: A[16][17] (extra -> extra) rounded to 11 bits',
    'o = 18: A[17][16] (extra -> extra) rounded to 11 bits',
    'o = 24: A[3][4] (tile -> tile) rounded to 11 bits',
    'o = 24: A[15][16] (tile -> extra) rounded to 11 bits',
    'o = 24: A[16][15] (extra -> tile) rounded to 11 bits',
    'o = 24: B[9][16] (action -> extra) rounded to 11 bits',
    'o = 24: B[16][23] (the last action of the partial group) rounded to 11 bits',
    'o = 24: A[19][20] (the second tile of O = 24) rounded to 11 bits',
)


def test_the_criterion_in_force_accepted_these():
    """Why the table exists: the dense model under HalfCheetah's cost, 1e-5 of the sum's magnitude, accepts these wrong model
    steps of the float64 oracle in EVERY arithmetic the tile is tested in (the list is in the module docstring)."""
    accepted, rejected = [], []
    for (o, d) in ((17, 6), (18, 6), (24, 17)):
        for label, fault in old_faults(o, d):
            ok = all(old_criterion_accepts(o, d, kind, mode, fault) for kind, mode in ((0, "sum"), (1, "sum"), (1, "best"), (0, "final")))
            (accepted if ok else rejected).append(f"o = {o}: {label}")
    print("accepted by the criterion in force:\n  " + "\n  ".join(accepted))
    print("rejected by it:\n  " + "\n  ".join(rejected))
    assert accepted and rejected   # ... and it is not that it accepts everything
    assert tuple(accepted) == ACCEPTED_BEFORE
