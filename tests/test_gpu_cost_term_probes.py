"""The device evaluations of the env cost terms -- TileHN in its three wave arrangements (k_rollout_hn.hip), the wide GEMM
kernels (k_rollout_wide.hip exact f32, k_rollout_wide_split.hip on the fp16 planes), the exact-f32 GEMM kernel at o <= 32 and
the general rollout kernel in f32 and f64 (generic_kernels.hip) -- through icem_rollout_cost on the case table of
cost_term_cases.py, against the float64 oracle under that module's per-row criterion: every row that is not near a threshold
(oracle.threshold_margins) within ROW_BOUND of its per-mode magnitude, no share allowance; bounds measured between two CPU
evaluations, none taken from a kernel; test_cost_term_sensitivity_cpu.py shows what the criterion rejects.  The readout
cases name the state unit, the action entry or the term list a failure belongs to.

Every (case, implementation) prints its figures (errors()) before it asserts: run with -s to read them.
"""
import dataclasses

import numpy as np
import pytest
import torch

import cost_term_cases as CC

pytestmark = pytest.mark.gpu

HN_VARIANTS = {"hn-split": {}, "hn-pair": {"hn_split": 0}, "hn-single": {"hn_pair": 0}}
_planners = {}


def np_(t):
    return t.detach().cpu().numpy().astype(np.float64)


def device_spec(spec):
    from icem_amd.envs import CostSpec, CostTerm
    d = {f.name: getattr(spec, f.name) for f in dataclasses.fields(spec)}
    d["terms"] = tuple(CostTerm(**dataclasses.asdict(t)) for t in spec.terms)
    return CostSpec(**d)


def planner(case, dtype="f32"):
    """One planner per (shape, horizon, mode, bound, dtype); model, cost and arithmetic are set per case."""
    from icem_amd import IcemConfig, IcemPlanner
    key = (case.o, case.d, case.h, case.mode, case.high, dtype)
    if key not in _planners:
        _planners[key] = IcemPlanner(IcemConfig(horizon=case.h, act_dim=case.d, num_traj=1100, opt_iters=1, dtype=dtype, seed=7,
                                                cost_mode=case.mode), -case.high * np.ones(case.d), case.high * np.ones(case.d))
    return _planners[key]


def implementations(case):
    """The implementations that serve the case's shape and spec."""
    out = list(HN_VARIANTS) if case.tilehn else []
    if case.o > 32:
        out += ["wide-planes", "wide-f32"]
    else:
        out += ["gemm-f32", "general-f32", "general-f64"]
    return out


def kernel_costs(case, impl):
    from icem_amd import _lib as L
    om, ob, acts = CC.inputs(case)
    pl = planner(case, "f64" if impl == "general-f64" else "f32")
    L.reset_options()
    try:
        for k, v in HN_VARIANTS.get(impl, {}).items():
            L.set_option(k, v)
        pl.set_model(om.kind, om.A, om.B)
        pl.set_cost_spec(device_spec(case.spec))
        if pl.dt == torch.float32:
            if case.o > 32:
                pl.set_wide_arith("f32" if impl == "wide-f32" else "auto")
            pl.set_tile_arith("auto" if impl in HN_VARIANTS else "f32")
            assert pl.tile_arith == (1 if impl in HN_VARIANTS else 0), (case.name, impl, pl.tile_growth)
            if impl == "wide-f32":
                assert pl.wide_arith == "f32"
        pl.reset()
        a = torch.as_tensor(acts, dtype=pl.dt, device=pl.device)
        if impl.startswith("general"):   # (asking for the observations takes the call to the general kernel)
            got = pl.rollout_cost(ob, a, return_observations=True)[0]
        else:
            got = pl.rollout_cost(ob, a)
        return np_(got)
    finally:
        L.reset_options()


def check(case, impl):
    """[] or the violations of one (case, implementation), each naming what the case reads out."""
    got = kernel_costs(case, impl)
    if impl == "general-f64":
        w = CC.want(case)
        ok = np.abs(got - w) <= CC.F64_ATOL + CC.F64_RTOL * np.abs(w)
        return [] if got.shape == w.shape and ok.all() else [f"{case.name} [{impl}] {case.what}: f64 costs off by {np.abs(got - w).max():.3g}"]
    s = CC.errors(got, case) if got.shape == CC.want(case).shape else None
    print(case.name, impl, s)
    return [f"{case.name} [{impl}] {case.what}: {v}" for v in CC.violations(got, case)]


def _assert_all(cases):
    bad = [v for case in cases for impl in implementations(case) for v in check(case, impl)]
    assert not bad, f"{len(bad)} violations:\n" + "\n".join(bad[:40])


@pytest.mark.parametrize("case", CC.SHIPPED_CASES + CC.ENV_CASES + CC.FLIP_CASES + CC.PROGRAM_CASES, ids=lambda c: c.name)
def test_cost_terms_on_the_case_table(case):
    _assert_all([case])


@pytest.mark.parametrize("group", sorted({c.group for c in CC.READOUT_CASES}) + ["control"])
def test_readouts(group):
    """State-unit, action-entry and control-cost readouts of one shape: the loop over the units / entries runs in here."""
    _assert_all([c for c in CC.READOUT_CASES + CC.CONTROL_CASES if c.group == group])


@pytest.mark.parametrize("shape", list(CC.HN_SHAPES))
def test_last_pool_of_whole_mpc_steps(shape):
    """icem_plan_step on TileHN, two MPC steps at N = 533: the last pool -- sampled rows of a decayed population with a ragged
    last tile, shifted-elite rows -- re-scored under the per-row criterion instead of a share."""
    from icem_amd import IcemConfig, IcemPlanner
    src = CC.BY_NAME[{"door": "door-k0-sum-533x30", "relocate": "relocate-k1-sum-533x30", "fpp": "fpp-sparse-k1-sum-533x30"}[shape]]
    om, ob, _ = CC.inputs(src)
    pl = IcemPlanner(IcemConfig(horizon=30, act_dim=src.d, num_traj=533, opt_iters=3, dtype="f32", seed=7), -np.ones(src.d), np.ones(src.d))
    pl.set_model(om.kind, om.A, om.B)
    pl.set_cost_spec(device_spec(src.spec))
    pl.reset()
    assert pl.tile_arith == 1
    for s in range(2):
        obs = ob if s == 0 else CC.q22(0.9 * ob).astype(np.float32).astype(np.float64)
        pl.plan_step(obs)
        n_last = pl.population_sizes[-1]
        pool = np_(pl.actions[:n_last])
        case = dataclasses.replace(src, name=f"{src.name}-pool{s}", n=n_last, fires=False)
        CC.give_inputs(case, om, obs, pool)
        got = np_(pl.costs[:n_last])
        print(case.name, CC.errors(got, case))
        assert CC.agree(got, case), (case.name, CC.violations(got, case))
