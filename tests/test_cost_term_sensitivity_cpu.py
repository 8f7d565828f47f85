"""The test of the cost-term tests (no GPU): with a float32 CPU evaluation standing in for the kernels, the per-row
criterion of cost_term_cases.py passes the reference pair on every case, the case table keeps the properties that make it
discriminating (near-threshold rows are rare, every comparison comes out both ways), every deliberately wrong evaluation
of the cost is rejected on some case by a factor of ten -- and the share criterion the rollout tests had before
(> 99 % of the rows within 1e-5 of the sum-mode magnitude) accepts a list of them."""
import dataclasses

import numpy as np
import pytest

import cost_term_cases as CC
from oracle import icem_oracle as O

GROUPS = sorted({c.group for c in CC.CASES})
_measured = {}


# ---- (a) the reference pair ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_reference_pair_agrees(group):
    """rollout_costs in float32 with 22-bit model entries and states and square roots off by an ulp (two seeds) against
    the float64 oracle: what the bounds were measured on passes them, with the factor of 4 cost_term_cases.py states."""
    worst = dict(row=0.0, median=0.0, state=0.0, row_case="", median_case="", state_case="")
    for case in [c for c in CC.CASES if c.group == group]:
        for seed in (0, 1):
            got, state_err = CC.kernel_standin(case, seed)
            s = CC.errors(got, case)
            assert CC.agree(got, case), (case.name, seed, CC.violations(got, case))
            assert state_err.max() <= CC.NEAR, (case.name, state_err.max())
            for key, v in (("row", s["worst"]), ("median", s["median"]), ("state", float(state_err.max()))):
                if v > worst[key]:
                    worst[key], worst[key + "_case"] = v, case.name
    _measured[group] = worst
    print(f"reference pair, {group}: worst row error {worst['row']:.3g} ({worst['row_case']}), median {worst['median']:.3g} "
          f"({worst['median_case']}), state error {worst['state']:.3g} ({worst['state_case']})")
    # within 4 x of the numbers in the docstring: the bounds ARE 4 x those numbers
    assert worst["row"] <= 4 * CC.MEASURED_ROW and worst["median"] <= 4 * CC.MEASURED_MEDIAN and worst["state"] <= 4 * CC.MEASURED_STATE


def test_bounds_are_what_the_docstring_says():
    assert CC.ROW_BOUND == 4 * CC.MEASURED_ROW <= 1e-5   # never looser than what the rollout tests claimed before
    assert CC.MEDIAN_BOUND == 4 * CC.MEASURED_MEDIAN and CC.NEAR == 4 * CC.MEASURED_STATE
    for key in ("MEASURED_ROW", "MEASURED_MEDIAN", "MEASURED_STATE"):
        assert f"{getattr(CC, key):.2g}".replace("e-0", "e-") in CC.__doc__, key


# ---- (b) the input conditions, from the oracle alone ---------------------------------------------------------------------
def test_near_threshold_rows_are_rare_in_every_case():
    for case in CC.CASES:
        share = CC.near(case).mean()
        assert share <= 0.01, (case.name, share)


def test_every_comparison_comes_out_both_ways():
    """On 10-90 % of the rows of the cases made for it: every comparison of the three shipped specs (Door's 1.0 and 1.35 in
    both model kinds -- at 0.5 and 0.7 under tanh --, Relocate's 0.1 and 0.05), both signs of every flip case; and every
    KIND of comparison on some case of the table."""
    kinds = {}
    for case in CC.CASES:
        shares = O.observation_comparison_shares(case.spec, CC.reference(case)["obs"])
        for name, v in shares.items():
            kind = name.split(":")[-1]
            kinds[kind] = kinds.get(kind, False) or 0.1 <= v <= 0.9
        if case.fires or case.group == "flip":
            assert shares and all(0.1 <= v <= 0.9 for v in shares.values()), (case.name, shares)
    assert set(kinds) == {"flip>", "flip<", "health_lo", "health_hi", "box", "step_gt", "norm_gt", "norm_lt", "gate"}
    assert all(kinds.values()), kinds
    fired = {c.name.rsplit("-", 2)[0] for c in CC.CASES if c.fires}
    assert fired == {f"{n}-k{k}" for n in ("door", "relocate", "fpp-sparse") for k in (0, 1)}


def test_magnitudes_and_margins_of_the_oracle():
    case = CC.BY_NAME["relocate-k0-best-533x30"]
    om, ob, acts = CC.inputs(case)
    obs = O.rollout_observations(om, ob, acts)
    step = np.stack([O._step_cost(case.spec, obs[:, t], acts[:, t], None, np.float64) for t in range(case.h)], 1)
    mags = np.stack([sum(O._magnitude_addends(case.spec, obs[:, t], acts[:, t], None)) for t in range(case.h)], 1)
    np.testing.assert_allclose(O.rollout_cost_magnitudes(om, case.spec, ob, acts, "final"), mags[:, -1], rtol=1e-12)
    np.testing.assert_allclose(O.rollout_cost_magnitudes(om, case.spec, ob, acts, "best"), mags[np.arange(case.n), step.argmin(1)], rtol=1e-12)
    np.testing.assert_allclose(O.rollout_cost_magnitudes(om, case.spec, ob, acts), mags.sum(1), rtol=1e-12)
    assert np.array_equal(O.rollout_cost_magnitudes(om, case.spec, ob, acts), O.rollout_cost_magnitudes(om, case.spec, ob, acts, "sum"))
    # the margin of a row: by hand for Relocate's lift threshold alone
    lift = dataclasses.replace(case.spec, terms=case.spec.terms[1:2])
    want = np.abs(obs[:, :, 38] - 0.04).min(1) / np.abs(obs).max((1, 2))
    np.testing.assert_allclose(O.threshold_margins(om, lift, ob, acts), want, rtol=1e-12)
    assert np.all(O.threshold_margins(om, case.spec, ob, acts) <= want)
    assert np.all(np.isinf(O.threshold_margins(om, CC._spec(lin_weight=1.0), ob, acts)))


# ---- (c) the mutants ------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class _NoSqrt(O.CostSpec):
    def term_value(self, tm, obs):   # NORM, NORM_GT, NORM_LT on the sum of squares itself
        if tm.kind not in (CC.NORM, CC.NORM_GT, CC.NORM_LT):
            return super().term_value(tm, obs)
        ss = super().term_value(dataclasses.replace(tm, kind=CC.SUMSQ, weight=1.0, gate_idx=-1), obs)
        f = ss if tm.kind == CC.NORM else (ss > tm.thresh if tm.kind == CC.NORM_GT else ss < tm.thresh).astype(np.float64)
        if tm.gate_idx >= 0:
            f = f * (obs[..., tm.gate_idx] > tm.gate_thresh)
        return tm.weight * f


def _fields(spec):
    return {f.name: getattr(spec, f.name) for f in dataclasses.fields(spec)}


def evaluate(om, spec, ob, acts, mode, *, steps=slice(None), ctrl_acts=None, no_sqrt=False, one_sign=False, tail=None, obs=None):
    """The float64 oracle with a fault switched on: per-step costs (control cost from ``ctrl_acts``), reduced over ``steps``.
    ``obs``: the rollout's observations where the caller has them already."""
    obs = O.rollout_observations(om, ob, acts) if obs is None else obs
    h = acts.shape[1]
    ca = acts if ctrl_acts is None else ctrl_acts
    sp = _NoSqrt(**_fields(spec)) if no_sqrt else spec
    if one_sign:
        sp = dataclasses.replace(sp, flip_idx=-1)
    C = np.empty(acts.shape[:2])
    for t in range(h):
        nxt = obs[:, t + 1] if t + 1 < h else om.predict(obs[:, t], acts[:, t])
        C[:, t] = O._step_cost(sp, obs[:, t], ca[:, t], nxt, np.float64)
        if one_sign:
            C[:, t] += (obs[:, t, spec.flip_idx] > spec.flip_thresh) * spec.flip_penalty
    C = C[:, steps]
    out = C.sum(1) if mode == "sum" else C.min(1) if mode == "best" else C[:, -1]
    if tail is not None:
        out = out.copy()
        out[-5:] *= tail
    return out


def _with_term(spec, j, **kw):
    tm = list(spec.terms)
    tm[j] = dataclasses.replace(tm[j], **kw)
    return dataclasses.replace(spec, terms=tuple(tm))


def term_mutants(spec, o):
    """(label, evaluate-kwargs) of every single-term fault of a spec's term list."""
    slices = (CC.NORM, CC.NORM_GT, CC.NORM_LT, CC.SUMSQ)
    for j, tm in enumerate(spec.terms):
        yield f"term {j} dropped", dict(spec=dataclasses.replace(spec, terms=spec.terms[:j] + spec.terms[j + 1:]))
        yield f"term {j} weight x 1.01", dict(spec=_with_term(spec, j, weight=tm.weight * 1.01))
        if tm.kind in slices:
            if tm.len > 1:
                yield f"term {j} len - 1", dict(spec=_with_term(spec, j, len=tm.len - 1))
            fits = tm.a + 1 + tm.len <= o
            yield f"term {j} a + 1", dict(spec=_with_term(spec, j, a=tm.a + 1, len=tm.len if fits else tm.len - 1))
            if tm.b >= 0:
                yield f"term {j} b dropped", dict(spec=_with_term(spec, j, b=-1))
        if tm.kind not in (CC.NORM, CC.SUMSQ):
            yield f"term {j} threshold x 1.1", dict(spec=_with_term(spec, j, thresh=tm.thresh * 1.1))
        if tm.kind in (CC.NORM_GT, CC.NORM_LT):
            yield f"term {j} NORM_GT <-> NORM_LT", dict(spec=_with_term(spec, j, kind=CC.NORM_GT + CC.NORM_LT - tm.kind))
        if tm.gate_idx >= 0:
            yield f"term {j} gate dropped", dict(spec=_with_term(spec, j, gate_idx=-1))
            yield f"term {j} gate index + 1", dict(spec=_with_term(spec, j, gate_idx=(tm.gate_idx + 1) % o))
            if tm.gate_thresh:
                yield f"term {j} gate threshold x 1.1", dict(spec=_with_term(spec, j, gate_thresh=tm.gate_thresh * 1.1))
    if any(tm.kind in (CC.NORM, CC.NORM_GT, CC.NORM_LT) for tm in spec.terms):
        yield "NORM without the square root", dict(no_sqrt=True)


def _model_with(om, fn):
    A, B = om.A.copy(), om.B.copy()
    fn(A, B)
    return O.SyntheticModel(A, B, om.kind)


# what the table cannot see (cost_term_cases.py names them): under tanh every velocity is below 1, and 1 % of Door's
# 1e-5 x sum of 30 squares is 3e-6 of a step's cost; the same fault under the linear model is rejected on door-fast
UNSEEN = {("door-k1", "term 2 weight x 1.01")}


def all_mutants():
    """[(label, [cases it may be rejected on], evaluate-kwargs given the case)]"""
    out = []
    shipped = {}
    for c in CC.SHIPPED_CASES:
        shipped.setdefault(c.name.split("-k")[0] + f"-k{c.kind}", []).append(c)
    for key, cases in shipped.items():
        if key.startswith("door-fast"):
            continue
        if key.startswith("door-k0"):
            cases = cases + [c for c in CC.SHIPPED_CASES if c.name.startswith("door-fast")]
        for label, kw in term_mutants(cases[0].spec, cases[0].o):
            if (key, label) not in UNSEEN:
                out.append((f"{key}: {label}", cases, lambda case, kw=kw: kw))
    for c in CC.PROGRAM_CASES:   # (Relocate's lists are Door's, at the same o: their mutants would say the same twice)
        if "-fwd-" in c.name and c.mode == "sum" and not c.name.startswith("relocate"):
            twin = CC.BY_NAME[[n for n in CC.BY_NAME if n.startswith(c.name.split("-fwd-")[0] + "-rev-")][0]]
            for label, kw in term_mutants(c.spec, c.o):
                # (the reversed list's terms are the same objects in the other order: the fault goes into the same term)
                def for_case(case, kw=kw, fwd=c):
                    if case is fwd or "spec" not in kw:
                        return kw
                    return dict(spec=dataclasses.replace(kw["spec"], terms=kw["spec"].terms[::-1]))
                out.append((f"{c.name.split('-fwd-')[0]}: {label}", [c, twin], for_case))
    for label, sel in (("last action entry", lambda a: a[..., -1]), ("last step", lambda a: a[:, -1])):
        def ctrl(case, sel=sel):
            a = CC.inputs(case)[2].copy()
            sel(a)[...] = 0
            return dict(ctrl_acts=a)
        out.append((f"control cost without the {label}", CC.CONTROL_CASES, ctrl))
    out.append(("flip with one sign only", CC.FLIP_CASES, lambda case: dict(one_sign=True)))
    big = [c for c in CC.SHIPPED_CASES if c.n == 533]
    for mode in CC.MODES:
        cases = [c for c in big if c.mode == mode] + [c for c in CC.READOUT_CASES if c.mode == mode and "unit0-" in c.name]
        out.append((f"{mode} over steps 0 .. h-2", cases, lambda case: dict(steps=slice(0, case.h - 1))))
        if mode != "final":   # (the last step of 1 .. h-1 is the last step: not a fault of 'final')
            out.append((f"{mode} over steps 1 .. h-1", cases, lambda case: dict(steps=slice(1, None))))
    door = [c for c in big if c.name.startswith("door")]
    out.append(("model entry A[3, 3] zeroed (a column no Door term reads)", door,
                lambda case: dict(om=_model_with(CC.inputs(case)[0], lambda A, B: A.__setitem__((3, 3), 0.0)))))
    out.append(("model entry B[5, 2] zeroed (a column no Door term reads)", door,
                lambda case: dict(om=_model_with(CC.inputs(case)[0], lambda A, B: B.__setitem__((5, 2), 0.0)))))
    out.append(("A[28, 28] x (1 + 2^-11) (Door's hinge column)", door,
                lambda case: dict(om=_model_with(CC.inputs(case)[0], lambda A, B: A.__setitem__((28, 28), A[28, 28] * (1 + 2.0 ** -11))))))
    out.append(("the last 5 rows x 1.5", big, lambda case: dict(tail=1.5)))
    return out


MUTANTS = all_mutants()
_report = []


def _rejection(label, cases, make_kw):
    best = (0.0, 0, None)
    for case in cases:
        om, ob, acts = CC.inputs(case)
        kw = dict(make_kw(case))
        if "om" not in kw:
            kw["obs"] = CC.reference(case)["obs"]
        got = evaluate(kw.pop("om", om), kw.pop("spec", case.spec), ob, acts, case.mode, **kw)
        factor, count = CC.rejection(got, case)
        if (factor >= 10, factor) > (best[0] >= 10, best[0]) or (best[0] < 10 and count > best[1]):
            best = (factor, count, case.name)
        if factor >= 10:
            break
    return best


@pytest.mark.parametrize("index", range(0, len(MUTANTS), 40))
def test_mutants_are_rejected(index):
    """Every wrong evaluation misses the row or the median bound by a factor >= 10 on some case (or leaves >= 10 rows that
    are not near a threshold out of bound); each line of the output names the mutant, its factor and the case."""
    failed = []
    for label, cases, make_kw in MUTANTS[index:index + 40]:
        factor, count, where = _rejection(label, cases, make_kw)
        line = f"mutant [{label}]: bound missed x {factor:.3g}, {count} rows out of bound, on {where}"
        print(line)
        if not (factor >= 10 or count >= 10):
            failed.append(line)
    assert not failed, "\n".join(failed)


def test_the_unmutated_oracle_passes_with_factor_zero():
    for case in CC.SHIPPED_CASES[:6] + CC.PROGRAM_CASES[:4]:
        om, ob, acts = CC.inputs(case)
        factor, count = CC.rejection(evaluate(om, case.spec, ob, acts, case.mode), case)
        assert factor < 1e-6 and count == 0, (case.name, factor)


# ---- (d) what the share criterion let through ------------------------------------------------------------------------------
_old = {}


def _old_inputs(name, kind):
    """The inputs of test_gpu_hn_shapes.py::test_rollout_on_tilehn_matches_the_float64_oracle, their rollout and magnitudes."""
    if (name, kind) not in _old:
        (o, d), spec = {"door": (CC.HN_SHAPES["door"], O.CostSpec.door()), "relocate": (CC.HN_SHAPES["relocate"], O.CostSpec.relocate()),
                        "fpp": (CC.HN_SHAPES["fpp"], O.CostSpec.fetch_pick_and_place())}[name]
        rs = np.random.RandomState(3 + kind)
        obs0 = 0.2 * rs.randn(o)
        om, acts = O.SyntheticModel.make(o, d, kind), rs.uniform(-1, 1, (16 * 33 + 5, 30, d))
        _old[name, kind] = (om, spec, obs0, acts, O.rollout_observations(om, obs0, acts), O.rollout_cost_magnitudes(om, spec, obs0, acts))
    return _old[name, kind]


def _old_criterion_accepts(name, kind, mode, **fault):
    om, spec, obs0, acts, obs, mag = _old_inputs(name, kind)
    want = evaluate(om, spec, obs0, acts, mode, obs=obs)
    got = evaluate(om, fault.pop("spec", spec), obs0, acts, mode, obs=obs, **fault)
    ok = np.abs(got - want) <= 1e-5 * mag
    return ok.mean() > 0.99 and (mode != "sum" or np.median(np.abs(got - want) / mag) < 2e-6)


OLD_CASES = [(0, "sum"), (1, "sum"), (1, "best"), (0, "final")]


def test_the_share_criterion_accepted_these():
    """Why the per-row criterion exists: > 99 % of 533 rows within 1e-5 of the sum-mode magnitude, on the inputs of
    test_gpu_hn_shapes.py, accepts each of these wrong evaluations of the float64 oracle."""
    rel, door = O.CostSpec.relocate(), O.CostSpec.door()
    drop = lambda s, j: dataclasses.replace(s, terms=s.terms[:j] + s.terms[j + 1:])  # noqa: E731
    for kind, mode in OLD_CASES:
        assert _old_criterion_accepts("relocate", kind, mode, spec=drop(rel, 4)), ("-20 bonus dropped", kind, mode)
        for name in ("door", "relocate", "fpp"):
            assert _old_criterion_accepts(name, kind, mode, tail=1.5), ("last 5 rows x 1.5", name, kind, mode)
    assert _old_criterion_accepts("relocate", 0, "sum", spec=drop(rel, 3))                          # -10 bonus dropped
    assert _old_criterion_accepts("relocate", 0, "sum", spec=_with_term(rel, 3, thresh=0.11))
    for j in (3, 4):
        assert _old_criterion_accepts("relocate", 0, "final", spec=drop(rel, j))
        assert _old_criterion_accepts("relocate", 0, "final", spec=_with_term(rel, j, len=2))
    assert _old_criterion_accepts("relocate", 0, "final", spec=_with_term(rel, 1, thresh=0.044))
    for mode in ("sum", "best"):   # Door under tanh: the hinge entry never exceeds 1
        for j in (4, 5):
            assert _old_criterion_accepts("door", 1, mode, spec=drop(door, j))
            assert _old_criterion_accepts("door", 1, mode, spec=_with_term(door, j, thresh=door.terms[j].thresh * 1.1))
    assert _old_criterion_accepts("door", 1, "sum", spec=_with_term(door, 2, len=29))
    assert _old_criterion_accepts("door", 1, "best", spec=drop(door, 2))
    # ... and it is not that it accepts everything
    assert not _old_criterion_accepts("door", 0, "sum", spec=drop(door, 0))
