"""The test of the wide probes (no GPU): with a float32 CPU evaluation standing in for the wide GEMM kernels, the per-row
criterion passes the reference pair on every case of wide_cases.py, the table keeps the properties that make it discriminating
(the shapes sit on the tiling functions' thresholds, both parities of the plane kernel's block count and both instantiations are
met, rows near a threshold are rare, both signs of every flip case fire, every class of the two index decompositions is claimed by
an entry on a path into a scored unit, the scale models separate every pair of neighbouring indices), every deliberately wrong
model step is rejected on some case by a factor of ten -- and the criterion the wide kernels were held to before
(test_wide_observation_rollout_matches_oracle: dense benchmark model, cost on unit 2, 1e-5 |want| + 2e-5, two rows excused)
accepts a named list of them, every csc mutant and every ksc mutant inside the observation rows among them.

The reference pair, worst over the table (per group in the output of test_reference_pair_agrees): see wide_cases.py.

The mutants (test_mutants_are_rejected prints each with its factor and case), per shape: one entry of [A ; B] per class of the
two index decompositions (wide_cases.plane_classes / exact_classes: first / middle / seam / last contraction block, every lane
group and slot, every wave, column tile and quad, the last live column) zeroed, x 1.01, moved to the neighbouring contraction
row / column, by 8 and by 32 rows and by 16 columns, rounded to 11 and to 16 bits; a whole 32-block zeroed (first, seam, last); a
column tile taken from the next tile and from the next wave's; a padded contraction row and a padded column read as non-zero;
action 0 read as action 1; the action rows shifted by one contraction slot; the actions of step t read as step t + 1's (d = 64
included); ksc[k] taken from k +- 1, 8, 32 and csc[c] from c +- 1, 4, 16, 16 NCT (observation and action rows); the model's
global scale off by 2; a row's S taken from the neighbouring row and from the same row of the neighbouring tile; the last row
scored with its neighbour's actions; the second batch of a workgroup started from the first batch's final state; a state column
one step stale / not through tanh; final at h - 2, best without the first step, sum without the last; the flip read from the
linear term's unit; one flip sign only.
Weakest (the factor on the first case that rejects; 1 449 mutants over the twelve shapes, 104 of them unseen): csc[c] and ksc[k] taken from a
neighbour, x 10 and more on the dense scale models (ksc of an action row x 11); the first padded column read as non-zero, x 10.8
at (378, 17); the third bf16 plane dropped from EVERY entry, x 11 .. x 19 on the lo3 shift cases (every row out of bound); a state
column not through tanh x 12, one step stale x 13.6; one entry x 1.01, x 19 and more; one entry moved by 1 / 8 / 32 rows x 24 and
more; one entry's low fp16 plane dropped (rounded to 11 bits) x 25 .. x 64 on the lo cases; everything else by x 150 and more.
What the table cannot see (unseen() below, each printed with its factor, and asserted to stay below x 10): ONE entry rounded to 16
bits -- the bf16 form's third plane dropped from a single entry: x 0.73 .. x 1.71.  The residue of the lo3 cases is 3 x 2^-19 of
a weight near 1: 5.7e-6 of ONE factor of the readout's product, against a row bound of 6.8e-6 of a magnitude that is twice the
readout (the state term).  No reshaping brings one entry to x 10: f32 leaves 8 bits below bf16's 16, so a single factor moves
by at most 2^-17.  What the table does not ask: accuracy relative to a state that stays orders of magnitude below the row's
largest contribution (2^-13 of it and less: the planes promise an absolute error there, k_rollout_wide_split.hip).

What the criterion in force accepted (test_the_criterion_in_force_accepted_these, ACCEPTED_BEFORE below; that test's assertions
in full -- the two excused rows must differ by a whole flip penalty -- at its own seven parametrisations and row counts, a fault
counting as accepted at a width when every case of that width accepts it: 148 of 294 faults over its six widths): all 68 csc
mutants and all 28 ksc mutants inside the observation rows -- on the benchmark model those scales are uniform, the mutant IS the
unmutated kernel --; a plane dropped from one entry in 34 of 36 places and the third bf16 plane dropped from every entry at four
widths of six; one entry x 1.01 in 10 places of 18; an entry moved by 16 columns (o = 33, 100), by 8 rows (o = 200) and B[16][383]
moved by one column (o = 384).  It rejects every zeroed entry, an action row's ksc taken from an observation row (the one scale
mutant that is not the identity there), a stale column, a shifted action, the last row scored with its neighbour's actions (the
row that misses is no whole-penalty difference) and the low fp16 plane dropped from every entry: on a dense model they reach the
scored column within two steps.  What it could not do is NAME anything.
"""
import dataclasses

import numpy as np
import pytest

import cost_term_cases as CC
import wide_cases as W
from oracle import icem_oracle as O

_measured = {}


# ---- (a) the reference pair ---------------------------------------------------------------------------------------------
def seeds_of(case):
    """The stand-in's seed perturbs the square roots of the NORM terms and nothing else: a cost without one (every cost of this
    table) gives the same numbers under every seed, and a second pass would measure nothing."""
    return (0, 1) if any(t.kind in (CC.NORM, CC.NORM_GT, CC.NORM_LT) for t in case.spec.terms) else (0,)


@pytest.mark.parametrize("group", W.GROUPS)
def test_reference_pair_agrees(group):
    """kernel_standin (f32, model entries and per-step states rounded to 22 bits; seeds_of: one seed suffices) against the float64 oracle: what
    the bounds were measured on passes them, with the factor of 4 wide_cases.py states."""
    worst = dict(row=0.0, median=0.0, state=0.0, row_case="", median_case="", state_case="")
    cases = W.by_group(group)
    for case in cases:
        for seed in seeds_of(case):
            got, state_err = CC.kernel_standin(case, seed)
            state = float(np.nanmax(state_err)) if np.isfinite(state_err).any() else 0.0   # (control: the state is zero throughout)
            s = CC.errors(got, case, W.BOUNDS)
            assert CC.agree(got, case, W.BOUNDS), (case.name, seed, CC.violations(got, case, W.BOUNDS))
            assert state <= W.BOUNDS.near, (case.name, state)
            for key, v in (("row", s["worst"]), ("median", s["median"]), ("state", state)):
                if v > worst[key]:
                    worst[key], worst[key + "_case"] = v, case.name
    W.forget(cases)
    _measured[group] = worst
    print(f"reference pair, {group}: worst row error {worst['row']:.3g} ({worst['row_case']}), median {worst['median']:.3g} "
          f"({worst['median_case']}), state error {worst['state']:.3g} ({worst['state_case']})")
    # what was measured stays what the docstring says: the bounds ARE 4 x those numbers
    assert worst["row"] <= W.MEASURED_ROW and worst["median"] <= W.MEASURED_MEDIAN and worst["state"] <= W.MEASURED_STATE


def test_bounds_are_what_the_docstring_says():
    """The table's own constants: the reference pair leaves cost_term_cases.MEASURED_MEDIAN / _STATE (the docstring of wide_cases.py
    says where), so they are the newly measured values x 4; the row bound stays at or under the 1e-5 the wide kernels' tests claim."""
    assert W.BOUNDS == CC.Bounds(4 * W.MEASURED_ROW, 4 * W.MEASURED_MEDIAN, 4 * W.MEASURED_STATE)
    assert W.BOUNDS.row <= 1e-5
    assert W.MEASURED_MEDIAN > CC.MEASURED_MEDIAN and W.MEASURED_STATE > CC.MEASURED_STATE   # (else: that module's bounds as they are)
    assert (CC.MEASURED_ROW, CC.MEASURED_MEDIAN, CC.MEASURED_STATE) == (1.8e-6, 3.5e-7, 3.4e-6)   # untouched
    for key in ("MEASURED_ROW", "MEASURED_MEDIAN", "MEASURED_STATE"):
        assert f"{getattr(W, key):.2g}".replace("e-0", "e-") in W.__doc__, key


# ---- (b) the table's properties -------------------------------------------------------------------------------------------
def test_shapes_sit_on_the_tiling_thresholds():
    """The shapes of the issue, each side of every threshold of the tiling functions, both parities of the plane kernel's block
    count (the m0 / m1 operand sets end swapped when it is odd), d on both sides of the held-ahead rule."""
    assert set(W.SHAPES) >= {(33, 4), (64, 6), (65, 3), (128, 8), (129, 3), (200, 64), (256, 17), (257, 6), (378, 17), (384, 32), (384, 64)}
    assert {W.shape_of(c) for c in W.CASES} == set(W.SHAPES)
    nt = {sh: W.exact_nt(sh[0]) for sh in W.SHAPES}
    nct = {sh: W.split_nct(sh[0]) for sh in W.SHAPES}
    assert (nt[33, 4], nt[64, 6], nt[65, 3], nt[128, 8], nt[129, 3], nt[256, 17], nt[257, 6], nt[378, 17]) == (4, 4, 8, 8, 16, 16, 24, 24)
    assert (nct[128, 8], nct[129, 3], nct[256, 17], nct[257, 6], nct[378, 17], nct[384, 32]) == (1, 2, 2, 3, 3, 3)
    kb = {sh: (sh[0] + sh[1] + 31) // 32 for sh in W.SHAPES}   # wide_split_kb's formula
    assert all(kb[sh] == W.split_kb(*sh) for sh in W.SHAPES)
    fits = [sh for sh in W.SHAPES if W.split_fits(*sh)]
    assert {kb[sh] % 2 for sh in fits} == {0, 1} and {kb[sh] % 2 for sh in fits if nct[sh] > 1} == {0, 1}
    assert kb[33, 4] == 2 and kb[378, 17] == 13 and kb[200, 64] % 2 == 1 and (180 + 12) % 32 == 0
    assert 32 * kb[384, 32] == W.SPLIT_KMAX and W.split_fits(384, 32) and not W.split_fits(384, 64) and fits == [sh for sh in W.SHAPES if sh != (384, 64)]
    assert W.exact_kb(384, 64) * 4 >= 448 and W.exact_kb(378, 17) == 99
    # the step's actions: held ahead in a four-tile batch at every d but 64, in a five-tile batch not at d = 32 either
    assert all(W.held_ahead(4, d) == (d != 64) for _, d in W.SHAPES) and not W.held_ahead(5, 32) and W.held_ahead(5, 17)
    assert 378 % 16 != 0 and 384 % 16 == 0   # the ragged last column tile, every column live


def test_row_counts_meet_both_instantiations():
    """FIVE from launch_rollout_wide_split's rule restated (wide_cases.is_five): 67 and 531 rows run the FIVE instantiation, 1,
    35 and 83 the regular one; every shape meets both in its unit, entry and scale groups, and has one 1-row case."""
    assert [W.is_five(n) for n in (1, 35, 67, 83, 531)] == [False, False, True, False, True]
    assert W.is_five(80) and not W.is_five(64) and not W.is_five(96) and W.is_five(129) and W.is_five(300) and W.is_five(4097)
    for sh in W.SHAPES:
        mine = [c for c in W.CASES if W.shape_of(c) == sh]
        assert sum(1 for c in mine if c.n == 1) == 1
        for g in ("unit", "entry", "scale"):
            assert {W.is_five(c.n) for c in mine if c.group.startswith(g)} == {False, True}, (sh, g)
        assert any(c.n == W.ROWS_TWO for c in mine if c.group.startswith("unit")) and any(c.n == W.ROWS_TWO for c in mine if c.group.startswith("scale"))
        assert {g.rsplit("-", 1)[0] for g in W.groups_of(sh)} >= {"unit-make", "unit-dense", "flip", "action", "control", "entry", "scale"}, sh
    for c in W.CASES:
        assert c.n <= 1100 and c.what, c.name
        assert not c.spec.terms and c.spec.lin_weight != 0 and not c.spec.extended, c.name
    assert any(c.h == 30 for c in W.by_group("long-o378d17"))


def test_near_threshold_rows_are_rare_and_both_flip_signs_fire():
    for case in W.CASES:
        if case.spec.flip_idx < 0:
            continue   # (no comparison: no row is near a threshold)
        share = CC.near(case, W.BOUNDS).mean()
        assert share <= 0.01, (case.name, share)
        shares = O.observation_comparison_shares(case.spec, CC.reference(case)["obs"])
        assert set(shares) == {"flip>", "flip<"} and all(0.1 <= v <= 0.9 for v in shares.values()), (case.name, shares)
        W.forget([case])
    readout = next(c for c in W.CASES if c.group.startswith("unit"))
    assert not CC.near(readout, W.BOUNDS).any()
    W.forget([readout])


@pytest.mark.parametrize("shape", W.SHAPES, ids=W.tag)
def test_every_class_is_claimed(shape):
    """The coverage condition of the entry group, from the sparsity pattern alone: every entry a case claims is non-zero in its
    model and reaches the unit the case scores inside the horizon; together the claimed entries meet every class of the plane
    kernel's and of the exact kernel's index decomposition -- in the plain cases and again in the low-plane ones."""
    o, d = shape
    need = W.all_classes(o, d)
    assert {"p:kb-first", "p:kb-seam", "p:kb-last", "p:last-live-column", "x:kb-first", "x:kb-seam", "x:kb-last"} <= need
    assert {f"p:v{v}" for v in range(8)} | {f"p:g{g}" for g in range(4)} | {f"x:g{g}" for g in range(4)} | {f"x:v{v}" for v in range(min(4, (o + 15) // 16))} <= need
    assert {f"p:ct{c}" for c in range(W.split_nct(o))} | {f"x:q{q}" for q in range(((o + 15) // 16 + 3) // 4)} <= need
    assert {f"p:wave{w}" for w in range(min(8, ((o + 15) // 16 + W.split_nct(o) - 1) // W.split_nct(o)))} <= need
    met = {0: set(), 1: set(), 2: set()}
    for case in W.by_group(f"entry-{W.tag(shape)}"):
        assert case.claims and not W.uncovered_claims(case), (case.name, W.uncovered_claims(case))
        A, B = case.matrices()
        for M in (A, B):
            w = M[M != 0]
            if not len(w):
                continue   # (shiftA: B = 0)
            assert len(set(w)) == len(w) and np.all((np.abs(w) >= 0.9) & (np.abs(w) < 1.0)) and (w > 0).any() and (w < 0).any(), case.name
            if case.model[2] == 0:
                assert np.array_equal(w.astype(np.float16).astype(np.float64), w), case.name
        for e in case.claims:
            met[case.model[2]] |= W.classes_of(e, o, d)
    for lo, seen in met.items():
        assert seen == need, (lo, sorted(need - seen))
    # ... and the check is not vacuous: a horizon one step short of the cycle's stride leaves the first entry out of reach
    long = W.BY_NAME[f"{W.tag(shape)}-shiftA1-unit0"]
    assert W.uncovered_claims(dataclasses.replace(long, h=len(long.claims)))


@pytest.mark.parametrize("shape", W.SHAPES, ids=W.tag)
def test_the_scale_patterns_separate_the_neighbours(shape):
    """From pack_wide_model_split's rule restated in numpy (wide_cases.pack_scales), on the dense scale models: any two
    contraction entries that differ by 1, 8 or 32 have different e_k (ksc), any two columns that differ by 1, 4, 16, 16 NCT or
    128 different f_j (csc) -- and on the benchmark model, which every earlier test ran on, they are all the same."""
    o, d = shape
    nct = W.split_nct(o)
    for units in ("pow2", "odd"):
        case = next(c for c in W.by_group(f"scale-{W.tag(shape)}") if c.units == units and c.model[0] == "dense")
        e, f = W.pack_scales(*case.matrices())
        for dk in (1, 8, 32):   # (the pairs across the obs | action seam included: wide_cases.seam_shift)
            assert (e[dk:] != e[:-dk]).all(), (units, dk, np.flatnonzero(e[dk:] == e[:-dk]))
        for dc in (1, 4, 16, 16 * nct, 128):
            if dc < o:
                assert (f[dc:] != f[:-dc]).all(), (units, dc, np.flatnonzero(f[dc:] == f[:-dc]))
        assert len(set(e)) >= 5 and len(set(f)) >= 5
    bench = O.SyntheticModel.make(o, d, 0)
    e, f = W.pack_scales(bench.A, bench.B)
    assert set(e[:o]) == {0} and set(e[o:]) <= {-1, -2} and set(f) == {0}   # (0.1 N(0, 1): the largest of o draws is 0.25 .. 0.5)
    # the graded cases: the plane scale S (from the row's largest contribution) differs between neighbouring rows and tiles
    graded = next(c for c in W.by_group(f"scale-{W.tag(shape)}") if "graded" in c.name and c.n == W.ROWS_TWO)
    assert graded.kind == O.MODEL_LINEAR   # (the state is scanned at every step: under tanh the rows would share sbound from step 1 on)
    for t in range(graded.h):
        sx = _plane_scale_exponents(graded, t)
        assert (sx[1:16] != sx[:15]).mean() >= 0.5 and (sx[16:32] != sx[:16]).mean() >= 0.5, (t, sx[:32])
    W.forget([graded])


# ---- (c) the mutants ------------------------------------------------------------------------------------------------------
def qbits(x, bits):
    """x rounded to ``bits`` significant bits: 11 = what is left of an operand whose low fp16 plane is dropped, 16 = of one whose
    third bf16 plane is."""
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    return np.ldexp(np.round(m * 2.0 ** bits) / 2.0 ** bits, e)


def evaluate(om, spec, ob, acts, mode, *, ctrl_acts=None, steps=slice(None), one_sign=False, pre_fault=None, post_fault=None):
    """The float64 oracle with a fault switched on.  ob: [o] or one start state per row [n, o]; pre_fault(t, x, prev, pre) -> the
    pre-activation of step t (x, prev: the state of this and of the step before), post_fault(t, pre, nxt) -> the new state;
    ctrl_acts: what the control cost sees; steps: what the reduction runs over."""
    n, h, _ = acts.shape
    ca = acts if ctrl_acts is None else ctrl_acts
    sp = dataclasses.replace(spec, flip_idx=-1) if one_sign else spec
    x = np.broadcast_to(ob, (n, ob.shape[-1])).copy()
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
        C[:, t] = c
        prev, x = x, nxt
    C = C[:, steps]
    return C.sum(1) if mode == "sum" else C.min(1) if mode == "best" else C[:, -1]


def _model_with(om, fn):
    """The model with fn(M) applied to M = [A ; B] ([o + d, o])."""
    M = np.concatenate([om.A, om.B])
    fn(M)
    o = om.A.shape[0]
    return O.SyntheticModel(M[:o].copy(), M[o:].copy(), om.kind)


def _entry_fault(which, k, c):
    """One entry M[k][c] of [A ; B]: zeroed, x 1.01, a plane dropped, swapped with the entry 1 / 8 / 32 contraction rows or 1 /
    16 columns on."""
    def fn(M):
        K, C = M.shape
        if which == "zeroed":
            M[k, c] = 0.0
        elif which == "x 1.01":
            M[k, c] *= 1.01
        elif which.startswith("rounded to"):
            M[k, c] = qbits(M[k, c], int(which.split()[2]))
        elif which.endswith("rows"):
            k2 = (k + int(which.split()[2])) % K
            M[k, c], M[k2, c] = M[k2, c], M[k, c]
        else:
            c2 = (c + int(which.split()[2])) % C
            M[k, c], M[k, c2] = M[k, c2], M[k, c]
    return fn


ENTRY_FAULTS = ("zeroed", "x 1.01", "moved by 1 rows", "moved by 1 columns", "moved by 8 rows", "moved by 32 rows", "moved by 16 columns",
                "rounded to 11 bits", "rounded to 16 bits")


def _named(names):
    return [W.BY_NAME[n] for n in names if n in W.BY_NAME]


def _units(sh, ks, modes=("sum", "final")):
    tg = W.tag(sh)
    return _named(n for k in ks for mode in modes for n in (f"{tg}-unit{k}-k0-{mode}", f"{tg}-unit{k}-k1-{mode}", f"{tg}-unit-dense{k}-k1-{mode}"))


_claim_index = {}


def _claiming(sh, entry, lo=None):
    """The entry cases of the shape (the scale group's included) that claim ``entry`` -- ``lo``: of that low-plane form only --
    and the dense unit cases that read its column."""
    if sh not in _claim_index:
        idx = {}
        for g in (f"entry-{W.tag(sh)}", f"scale-{W.tag(sh)}"):
            for c in W.by_group(g):
                for e in c.claims:
                    idx.setdefault(e, []).append(c)
        _claim_index[sh] = idx
    mine = [c for c in _claim_index[sh].get(entry, []) if lo is None or c.model[2] == lo]
    return mine + ([] if lo else _units(sh, (entry[2],)))


def representatives(sh):
    """Entries of [A ; B], chosen greedily among those the low-plane shifts claim (so that each has a plain, a lo and a lo3 case),
    until every class of both index decompositions is represented."""
    o, d = sh
    need, out = W.all_classes(o, d), []
    pool = [("A", i, (i + 1) % o) for i in range(o)] + [("B", j, (j + o - d) % o) for j in range(d)]
    while need:
        best = max(pool, key=lambda e: len(W.classes_of(e, o, d) & need))
        gain = W.classes_of(best, o, d) & need
        assert gain, sorted(need)
        out.append((best, sorted(gain)))
        need -= gain
    return out


def _plane_scale_exponents(case, t):
    """The exponent of the fp16 form's per-row plane scale at step t, split_first's rule restated: that of the row's largest
    contribution |x_k| 2^e_k over the observation and action entries (S is taken so that this stays below 2^15) -- under the tanh
    model from step 1 on the state is not scanned: its bound, the largest 2^e_k of a live observation row (sbound), stands in."""
    om, ob, acts = CC.inputs(case)
    e, _ = W.pack_scales(om.A, om.B)
    o = case.o
    act = np.abs(acts[:, t] * np.ldexp(1.0, e[o:])).max(axis=1)
    if om.kind == O.MODEL_TANH and t > 0:
        live = (om.A != 0).any(axis=1)
        state = np.full(case.n, np.ldexp(1.0, e[:o][live]).max() if live.any() else 0.0)
    else:
        state = np.abs(CC.reference(case)["obs"][:, t] * np.ldexp(1.0, e[:o])).max(axis=1)
    return np.frexp(np.maximum(state, act))[1]


def scale_fault_model(om, axis, at, delta):
    """The model with ksc[at] (axis 0) / csc[at] (axis 1) taken from at + delta: row / column ``at`` of [A ; B] off by the ratio of
    the two powers of two (pack_wide_model_split's rule: wide_cases.pack_scales)."""
    e, f = W.pack_scales(om.A, om.B)
    x = e if axis == 0 else f
    ratio = 2.0 ** float(x[at + delta] - x[at])

    def fn(M):
        if axis == 0:
            M[at] *= ratio
        else:
            M[:, at] *= ratio
    return _model_with(om, fn)


def scale_column(o):
    """A column of the largest column scale (c % 5 == 4) in the second wave's first tile (the first tile's at o = 33)."""
    return next((c for c in range(16 * W.split_nct(o) + 1, min(o, 16 * W.split_nct(o) + 16)) if c % 5 == 4), 19)


def all_mutants(sh):
    """[(label, [cases it may be rejected on], case -> evaluate-kwargs (``om`` / ``ob`` / ``acts`` / ``spec`` replace the case's))]"""
    o, d = sh
    tg, nct, out = W.tag(sh), W.split_nct(o), []
    flips = W.by_group(f"flip-{tg}")
    ctrl = W.by_group(f"control-{tg}")
    actions = W.by_group(f"action-{tg}")
    scale = W.by_group(f"scale-{tg}")
    edges = W.edge_units(o)
    dense = _units(sh, edges)

    def model(fn):
        return lambda case: dict(om=_model_with(CC.inputs(case)[0], fn))
    for entry, classes in representatives(sh):
        k, c = W.entry_index(entry, o)
        for which in ENTRY_FAULTS:
            lo = {"rounded to 11 bits": 1, "rounded to 16 bits": 2}.get(which)
            out.append((f"{tg}: {entry[0]}[{entry[1]}][{entry[2]}] ({', '.join(classes)}) {which}", _claiming(sh, entry, lo), model(_entry_fault(which, k, c))))
    lo3 = [c for c in W.by_group(f"entry-{tg}") if c.model[2] == 2]
    out.append((f"{tg}: the third bf16 plane dropped from every entry", lo3, model(lambda M: M.__setitem__(slice(None), qbits(M, 16)))))
    out.append((f"{tg}: the low fp16 plane dropped from every entry", [c for c in W.by_group(f"entry-{tg}") if c.model[2] == 1],
                model(lambda M: M.__setitem__(slice(None), qbits(M, 11)))))
    for name, kb in (("first", 0), ("seam", o // 32), ("last", (o + d - 1) // 32)):
        out.append((f"{tg}: contraction block {kb} (the {name} one) zeroed", dense, model(lambda M, kb=kb: M.__setitem__(slice(32 * kb, 32 * kb + 32), 0.0))))
    for name, step in (("ct -> ct + 1", 1), ("wave -> wave + 1", nct)):
        def tile(M, step=step):
            src = M[:, 16 * step:16 * step + 16].copy()
            M[:, :16] = 0.0
            M[:, :src.shape[1]] = src
        out.append((f"{tg}: column tile 0 computed from tile {step}'s operands ({name})", _units(sh, (0, 15)), model(tile)))

    def padded_column(case):
        om, ob, _ = CC.inputs(case)   # slot o of the staged row starts from obs0[0] and feeds the model through row o - 1's weights
        return dict(pre_fault=lambda t, x, prev, pre: pre + (ob[0] * om.A[o - 1] if t == 0 else 0.0))
    out.append((f"{tg}: the first padded column read as non-zero", dense, padded_column))

    def padded_row(case):
        om, ob, _ = CC.inputs(case)   # contraction slot o + d holds obs0[0] and meets the last action row's weights
        return dict(pre_fault=lambda t, x, prev, pre: pre + ob[0] * om.B[d - 1])
    out.append((f"{tg}: the first padded contraction row read as non-zero", dense, padded_row))

    def action_as_next(case):
        a = CC.inputs(case)[2].copy()
        a[..., 0] = a[..., 1]
        return dict(acts=a, ctrl_acts=a)
    out.append((f"{tg}: action 0 read as action 1", [c for c in actions if "-act0-" in c.name] + ctrl, action_as_next))

    def slot_shift(case):
        a = CC.inputs(case)[2]
        return dict(acts=np.roll(a, 1, axis=-1), ctrl_acts=a)
    out.append((f"{tg}: the action rows shifted by one contraction slot", actions + dense, slot_shift))

    def step_ahead(case):
        a = CC.inputs(case)[2]
        return dict(acts=np.concatenate([a[:, 1:], a[:, -1:]], axis=1), ctrl_acts=a)
    out.append((f"{tg}: the actions of step t read as step t + 1's (held {'ahead' if W.held_ahead(4, d) else 'in LDS: not ahead'} in a four-tile batch)",
                [c for c in actions if c.mode == "sum"] + dense, step_ahead))

    def scale_fault(axis, at, delta):
        return lambda case: dict(om=scale_fault_model(CC.inputs(case)[0], axis, at, delta))
    for k in (30, o + 1):   # an observation row (30 % 5 == 0: the largest row scale) and an action row
        for delta in (1, -1, 8, -8, 32, -32):
            if 0 <= k + delta < o + d:
                out.append((f"{tg}: ksc[{k}] taken from {k + delta} ({'observation' if k < o else 'action'} row)", scale, scale_fault(0, k, delta)))
    c0 = scale_column(o)
    for delta in sorted({1, -1, 4, -4, 16, -16, 16 * nct, -16 * nct}):
        if 0 <= c0 + delta < o:
            out.append((f"{tg}: csc[{c0}] taken from {c0 + delta}", scale, scale_fault(1, c0, delta)))
    out.append((f"{tg}: the model's global scale off by 2", dense, model(lambda M: M.__imul__(2.0))))
    graded = [c for c in scale if "graded" in c.name]

    def s_from(step):
        def kw(case):
            sx = [_plane_scale_exponents(case, t) for t in range(case.h)]
            src = np.clip(np.arange(case.n) + step, 0, case.n - 1) if step > 1 else np.arange(case.n) ^ 1
            src = np.minimum(src, case.n - 1)
            return dict(pre_fault=lambda t, x, prev, pre: pre * np.ldexp(1.0, sx[t][src] - sx[t])[:, None])
        return kw
    out.append((f"{tg}: a row's S taken from the neighbouring row", graded, s_from(1)))
    out.append((f"{tg}: a row's S taken from the same row of the neighbouring tile", graded, s_from(16)))

    def neighbour(case):
        a = CC.inputs(case)[2].copy()
        a[-1] = a[-2]
        return dict(acts=a, ctrl_acts=a)
    out.append((f"{tg}: the last row of the ragged tile scored with its neighbour's actions", dense, neighbour))

    def second_batch(case):
        om, ob, acts = CC.inputs(case)
        last = CC.reference(case)["obs"][:, -1]
        start = np.broadcast_to(ob, (case.n, o)).copy()
        start[64:] = om.predict(last, acts[:, -1])[:case.n - 64]
        return dict(ob=start)
    out.append((f"{tg}: the second batch of a workgroup started from the first batch's final state", [c for c in dense if c.n == W.ROWS_TWO], second_batch))
    for col in (16, o - 1):
        def stale(case, col=col):
            A = CC.inputs(case)[0].A
            return dict(pre_fault=lambda t, x, prev, pre: pre + (prev[:, col:col + 1] - x[:, col:col + 1]) * A[col])
        out.append((f"{tg}: state column {col} carried one step stale", dense + _named(f"{tg}-shiftA1-unit{k}" for k in range(o)), stale))
        out.append((f"{tg}: state column {col} not passed through tanh", [c for c in dense + _units(sh, (col,)) if c.kind == 1],
                    lambda case, col=col: dict(post_fault=lambda t, pre, nxt: np.concatenate([nxt[:, :col], pre[:, col:col + 1], nxt[:, col + 1:]], axis=1))))
    out.append((f"{tg}: final taken at step h - 2", [c for c in dense if c.mode == "final"], lambda case: dict(steps=slice(0, case.h - 1))))
    out.append((f"{tg}: best without the first step", [c for c in W.by_group(f"unit-make-{tg}") + flips if c.mode == "best"],
                lambda case: dict(steps=slice(1, None))))
    out.append((f"{tg}: sum without the last step", [c for c in dense if c.mode == "sum"], lambda case: dict(steps=slice(0, case.h - 1))))
    out.append((f"{tg}: flip read from the linear term's unit", [c for c in flips if c.spec.flip_idx != c.spec.lin_idx],
                lambda case: dict(spec=dataclasses.replace(case.spec, flip_idx=case.spec.lin_idx))))
    out.append((f"{tg}: flip firing on one sign only", flips, lambda case: dict(one_sign=True)))
    return out


def unseen(label):
    """Mutants the table cannot bring to x 10 (the module docstring says why): the bf16 form's third plane."""
    return "rounded to 16 bits" in label


def _rejection(label, cases, make_kw):
    best = (0.0, 0, None)
    for case in cases:
        om, ob, acts = CC.inputs(case)
        kw = dict(make_kw(case))
        got = evaluate(kw.pop("om", om), kw.pop("spec", case.spec), kw.pop("ob", ob), kw.pop("acts", acts), case.mode, **kw)
        factor, count = CC.rejection(got, case, W.BOUNDS)
        if (factor >= 10, factor) > (best[0] >= 10, best[0]) or (best[0] < 10 and count > best[1]):
            best = (factor, count, case.name)
        if factor >= 10:
            break
    return best


@pytest.mark.parametrize("shape", W.SHAPES, ids=W.tag)
def test_mutants_are_rejected(shape):
    """Every wrong model step misses the row or the median bound by a factor >= 10 on some case (or leaves >= 10 rows that are
    not near a threshold out of bound); each line of the output names the mutant, its factor and the case.  The unseen ones are
    printed with their factor too, and must stay unseen: a table that starts to see them has a docstring to correct."""
    failed = []
    mine = all_mutants(shape)
    assert len(mine) >= 60
    for label, cases, make_kw in mine:
        assert cases, label
        factor, count, where = _rejection(label, cases, make_kw)
        line = f"mutant [{label}]: bound missed x {factor:.3g}, {count} rows out of bound, on {where}"
        if unseen(label):
            print("UNSEEN " + line)
            assert factor < 10, line
        else:
            print(line)
            if not (factor >= 10 or count >= 10):
                failed.append(line)
    W.forget([c for c in W.CASES if W.shape_of(c) == shape])
    assert not failed, "\n".join(failed)


def test_the_unmutated_oracle_passes_with_factor_zero():
    for case in [W.by_group(g)[i] for sh in ((33, 4), (200, 64), W.LONG_SHAPE) for g in W.groups_of(sh) for i in (0, -1)]:
        om, ob, acts = CC.inputs(case)
        factor, count = CC.rejection(evaluate(om, case.spec, ob, acts, case.mode), case, W.BOUNDS)
        assert factor < 1e-6 and count == 0, (case.name, factor)
        W.forget([case])


# ---- (d) what the criterion in force accepted -------------------------------------------------------------------------------
OLD_CASES = [(378, 17, 30, 0, "sum", 300), (378, 17, 30, 1, "sum", 100), (100, 6, 12, 1, "best", 1000), (33, 4, 13, 0, "final", 77),
             (64, 6, 30, 1, "sum", 129), (384, 17, 30, 0, "sum", 40), (200, 3, 10, 1, "sum", 4097)]   # its own parametrisation
_old = {}


def _old_inputs(o, d, h, kind, mode, n):
    """test_wide_observation_rollout_matches_oracle's inputs, every row of them: the dense benchmark model, cost on unit 2 (flip on
    unit 1 at 0.05 under the linear model), obs 0.1 N(0, 1), actions uniform in [-0.4, 0.4] rounded to f32."""
    key = (o, d, h, kind, mode, n)
    if key not in _old:
        om = O.SyntheticModel.make(o, d, kind)
        flip_idx = 1 if kind == 0 else -1
        spec = O.CostSpec(0.1, 2, -1.0, flip_idx, 10.0, 0.05)
        rs = np.random.RandomState(o + n)
        ob = 0.1 * rs.randn(o)
        acts = rs.uniform(-0.4, 0.4, (n, h, d)).astype(np.float32).astype(np.float64)
        _old[key] = (om, spec, ob, acts, evaluate(om, spec, ob, acts, mode))
    return _old[key]


def old_criterion_accepts(key, fault):
    """That test's assertions, all of them: |got - want| <= 1e-5 |want| + 2e-5 on every row but two where the flip is on (none
    elsewhere), and every row that misses differs by a whole flip penalty (|diff| % 10 within 1e-3 of 0 or of 10)."""
    om, spec, ob, acts, want = _old_inputs(*key)
    kw = fault(om, ob, acts)
    got = evaluate(kw.pop("om", om), spec, kw.pop("ob", ob), kw.pop("acts", acts), key[4], **kw)
    diff = np.abs(got - want)
    bad = diff > 1e-5 * np.abs(want) + 2e-5
    if bad.sum() > (2 if spec.flip_idx >= 0 else 0):
        return False
    if bad.any():
        return bool(np.allclose(diff[bad] % 10.0, 0.0, atol=1e-3) or np.allclose(diff[bad] % 10.0, 10.0, atol=1e-3))
    return True


def old_faults(o, d):
    """(label, (om, ob, acts) -> evaluate-kwargs): the model-step faults of the list above that have a meaning on the old inputs."""
    nct = W.split_nct(o)
    for entry, _ in (((("A", 40 % o, 41 % o)), 0), (("A", 3, 2), 0), (("B", d - 1, o - 1), 0)):
        k, c = W.entry_index(entry, o)
        for which in ENTRY_FAULTS:
            yield f"{entry[0]}[{entry[1]}][{entry[2]}] {which}", lambda om, ob, acts, fn=_entry_fault(which, k, c): dict(om=_model_with(om, fn))
    yield "the low fp16 plane dropped from every entry", lambda om, ob, acts: dict(om=_model_with(om, lambda M: M.__setitem__(slice(None), qbits(M, 11))))
    yield "the third bf16 plane dropped from every entry", lambda om, ob, acts: dict(om=_model_with(om, lambda M: M.__setitem__(slice(None), qbits(M, 16))))

    def scale_fault(axis, at, delta):
        return lambda om, ob, acts: dict(om=scale_fault_model(om, axis, at, delta))
    for delta in (1, -1, 8, -8, 32, -32):
        if 0 <= 30 + delta < o:
            yield f"ksc[30] taken from {30 + delta} (observation row)", scale_fault(0, 30, delta)
    yield f"ksc[{o}] taken from {o - 1} (action row from an observation row)", scale_fault(0, o, -1)
    for c0 in (2, scale_column(o)):
        for delta in sorted({1, -1, 4, -4, 16, -16, 16 * nct, -16 * nct}):
            if 0 <= c0 + delta < o:
                yield f"csc[{c0}] taken from {c0 + delta}", scale_fault(1, c0, delta)
    yield "state column 16 carried one step stale", lambda om, ob, acts: dict(pre_fault=lambda t, x, prev, pre: pre + (prev[:, 16:17] - x[:, 16:17]) * om.A[16])

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
    'o = 33: A[7][8] x 1.01',
    'o = 33: A[7][8] moved by 16 columns',
    'o = 33: A[7][8] rounded to 11 bits',
    'o = 33: A[7][8] rounded to 16 bits',
    'o = 33: A[3][2] rounded to 11 bits',
    'o = 33: A[3][2] rounded to 16 bits',
    'o = 33: B[3][32] x 1.01',
    'o = 33: B[3][32] rounded to 11 bits',
    'o = 33: B[3][32] rounded to 16 bits',
    'o = 33: the third bf16 plane dropped from every entry',
    'o = 33: ksc[30] taken from 31 (observation row)',
    'o = 33: ksc[30] taken from 29 (observation row)',
    'o = 33: ksc[30] taken from 22 (observation row)',
    'o = 33: csc[2] taken from 1',
    'o = 33: csc[2] taken from 3',
    'o = 33: csc[2] taken from 6',
    'o = 33: csc[2] taken from 18',
    'o = 33: csc[19] taken from 3',
    'o = 33: csc[19] taken from 15',
    'o = 33: csc[19] taken from 18',
    'o = 33: csc[19] taken from 20',
    'o = 33: csc[19] taken from 23',
    'o = 64: A[40][41] x 1.01',
    'o = 64: A[40][41] rounded to 11 bits',
    'o = 64: A[40][41] rounded to 16 bits',
    'o = 64: A[3][2] rounded to 16 bits',
    'o = 64: B[5][63] rounded to 16 bits',
    'o = 64: ksc[30] taken from 31 (observation row)',
    'o = 64: ksc[30] taken from 29 (observation row)',
    'o = 64: ksc[30] taken from 38 (observation row)',
    'o = 64: ksc[30] taken from 22 (observation row)',
    'o = 64: ksc[30] taken from 62 (observation row)',
    'o = 64: csc[2] taken from 1',
    'o = 64: csc[2] taken from 3',
    'o = 64: csc[2] taken from 6',
    'o = 64: csc[2] taken from 18',
    'o = 64: csc[19] taken from 3',
    'o = 64: csc[19] taken from 15',
    'o = 64: csc[19] taken from 18',
    'o = 64: csc[19] taken from 20',
    'o = 64: csc[19] taken from 23',
    'o = 64: csc[19] taken from 35',
    'o = 100: A[40][41] x 1.01',
    'o = 100: A[40][41] moved by 16 columns',
    'o = 100: A[40][41] rounded to 11 bits',
    'o = 100: A[40][41] rounded to 16 bits',
    'o = 100: A[3][2] x 1.01',
    'o = 100: A[3][2] rounded to 11 bits',
    'o = 100: A[3][2] rounded to 16 bits',
    'o = 100: B[5][99] rounded to 11 bits',
    'o = 100: B[5][99] rounded to 16 bits',
    'o = 100: the third bf16 plane dropped from every entry',
    'o = 100: ksc[30] taken from 31 (observation row)',
    'o = 100: ksc[30] taken from 29 (observation row)',
    'o = 100: ksc[30] taken from 38 (observation row)',
    'o = 100: ksc[30] taken from 22 (observation row)',
    'o = 100: ksc[30] taken from 62 (observation row)',
    'o = 100: csc[2] taken from 1',
    'o = 100: csc[2] taken from 3',
    'o = 100: csc[2] taken from 6',
    'o = 100: csc[2] taken from 18',
    'o = 100: csc[19] taken from 3',
    'o = 100: csc[19] taken from 15',
    'o = 100: csc[19] taken from 18',
    'o = 100: csc[19] taken from 20',
    'o = 100: csc[19] taken from 23',
    'o = 100: csc[19] taken from 35',
    'o = 200: A[40][41] x 1.01',
    'o = 200: A[40][41] moved by 8 rows',
    'o = 200: A[40][41] rounded to 11 bits',
    'o = 200: A[40][41] rounded to 16 bits',
    'o = 200: A[3][2] rounded to 11 bits',
    'o = 200: A[3][2] rounded to 16 bits',
    'o = 200: B[2][199] rounded to 11 bits',
    'o = 200: B[2][199] rounded to 16 bits',
    'o = 200: the third bf16 plane dropped from every entry',
    'o = 200: ksc[30] taken from 31 (observation row)',
    'o = 200: ksc[30] taken from 29 (observation row)',
    'o = 200: ksc[30] taken from 38 (observation row)',
    'o = 200: ksc[30] taken from 22 (observation row)',
    'o = 200: ksc[30] taken from 62 (observation row)',
    'o = 200: csc[2] taken from 1',
    'o = 200: csc[2] taken from 3',
    'o = 200: csc[2] taken from 6',
    'o = 200: csc[2] taken from 18',
    'o = 200: csc[2] taken from 34',
    'o = 200: csc[34] taken from 2',
    'o = 200: csc[34] taken from 18',
    'o = 200: csc[34] taken from 30',
    'o = 200: csc[34] taken from 33',
    'o = 200: csc[34] taken from 35',
    'o = 200: csc[34] taken from 38',
    'o = 200: csc[34] taken from 50',
    'o = 200: csc[34] taken from 66',
    'o = 378: A[40][41] x 1.01',
    'o = 378: A[40][41] rounded to 11 bits',
    'o = 378: A[40][41] rounded to 16 bits',
    'o = 378: A[3][2] rounded to 11 bits',
    'o = 378: A[3][2] rounded to 16 bits',
    'o = 378: B[16][377] rounded to 11 bits',
    'o = 378: B[16][377] rounded to 16 bits',
    'o = 378: ksc[30] taken from 31 (observation row)',
    'o = 378: ksc[30] taken from 29 (observation row)',
    'o = 378: ksc[30] taken from 38 (observation row)',
    'o = 378: ksc[30] taken from 22 (observation row)',
    'o = 378: ksc[30] taken from 62 (observation row)',
    'o = 378: csc[2] taken from 1',
    'o = 378: csc[2] taken from 3',
    'o = 378: csc[2] taken from 6',
    'o = 378: csc[2] taken from 18',
    'o = 378: csc[2] taken from 50',
    'o = 378: csc[49] taken from 1',
    'o = 378: csc[49] taken from 33',
    'o = 378: csc[49] taken from 45',
    'o = 378: csc[49] taken from 48',
    'o = 378: csc[49] taken from 50',
    'o = 378: csc[49] taken from 53',
    'o = 378: csc[49] taken from 65',
    'o = 378: csc[49] taken from 97',
    'o = 384: A[40][41] x 1.01',
    'o = 384: A[40][41] rounded to 11 bits',
    'o = 384: A[40][41] rounded to 16 bits',
    'o = 384: A[3][2] x 1.01',
    'o = 384: A[3][2] rounded to 11 bits',
    'o = 384: A[3][2] rounded to 16 bits',
    'o = 384: B[16][383] x 1.01',
    'o = 384: B[16][383] moved by 1 columns',
    'o = 384: B[16][383] rounded to 11 bits',
    'o = 384: B[16][383] rounded to 16 bits',
    'o = 384: the third bf16 plane dropped from every entry',
    'o = 384: ksc[30] taken from 31 (observation row)',
    'o = 384: ksc[30] taken from 29 (observation row)',
    'o = 384: ksc[30] taken from 38 (observation row)',
    'o = 384: ksc[30] taken from 22 (observation row)',
    'o = 384: ksc[30] taken from 62 (observation row)',
    'o = 384: csc[2] taken from 1',
    'o = 384: csc[2] taken from 3',
    'o = 384: csc[2] taken from 6',
    'o = 384: csc[2] taken from 18',
    'o = 384: csc[2] taken from 50',
    'o = 384: csc[49] taken from 1',
    'o = 384: csc[49] taken from 33',
    'o = 384: csc[49] taken from 45',
    'o = 384: csc[49] taken from 48',
    'o = 384: csc[49] taken from 50',
    'o = 384: csc[49] taken from 53',
    'o = 384: csc[49] taken from 65',
    'o = 384: csc[49] taken from 97',
)


def test_the_criterion_in_force_accepted_these():
    """Why the table exists: test_wide_observation_rollout_matches_oracle's own criterion, at its own shapes and on its own
    inputs, accepts these wrong model steps of the float64 oracle -- at EVERY case of a width (the list is in ACCEPTED_BEFORE)."""
    accepted, rejected = [], []
    widths = sorted({(k[0], k[1]) for k in OLD_CASES})
    for (o, d) in widths:
        keys = [k for k in OLD_CASES if (k[0], k[1]) == (o, d)]
        for label, fault in old_faults(o, d):
            ok = all(old_criterion_accepts(key, fault) for key in keys)
            (accepted if ok else rejected).append(f"o = {o}: {label}")
    print("accepted by the criterion in force:\n  " + "\n  ".join(accepted))
    print("rejected by it:\n  " + "\n  ".join(rejected))
    assert accepted and rejected   # ... and it is not that it accepts everything
    # every csc mutant and every ksc mutant inside the observation rows: those scales are uniform on the benchmark model
    scale = [a for a in accepted if ("csc[" in a or "(observation row)" in a)]
    assert len(scale) == sum(1 for (o, d) in widths for label, _ in old_faults(o, d) if "csc[" in label or "(observation row)" in label)
    assert any("rounded to 11 bits" in a for a in accepted) and any("third bf16 plane dropped from every" in a for a in accepted)
    assert tuple(accepted) == ACCEPTED_BEFORE
