"""The wide GEMM rollout kernels' model step -- rollout_wide_split_kernel on the fp16 planes ("f16x2") and on the bf16 planes
("bf16x3"), rollout_wide_kernel in exact f32 ("f32"), rollout_rows_wide_kernel behind it in whole MPC steps -- on the case table
of wide_cases.py, against the float64 oracle under cost_term_cases.py's per-row criterion with that table's bounds: every row
that is not near a threshold within ROW_BOUND of its per-mode magnitude, no share allowance; bounds measured between two CPU
evaluations, none taken from a kernel; test_wide_sensitivity_cpu.py shows what the criterion rejects.  A violation names the
state unit, the action entry, the model entries or the scale model its case reads out.

Every case runs in all three arithmetics through IcemPlanner.rollout_cost, the arithmetic named via set_wide_arith and
``wide_arith`` asserted to be what was asked -- but at (384, 64), which the plane kernel's LDS does not hold: there the handle
reports "f32" whatever is asked.

Every (case, implementation) prints its figures (errors()) before it asserts, every test the worst row error per
implementation: run with -s to read them.
"""
import dataclasses
import time

import numpy as np
import pytest
import torch

import cost_term_cases as CC
import wide_cases as W

pytestmark = pytest.mark.gpu

ARITHS = ("f16x2", "bf16x3", "f32")
_planners = {}


def np_(t):
    return t.detach().cpu().numpy().astype(np.float64)


def device_spec(spec):
    from icem_amd.envs import CostSpec, CostTerm
    d = {f.name: getattr(spec, f.name) for f in dataclasses.fields(spec)}
    d["terms"] = tuple(CostTerm(**dataclasses.asdict(t)) for t in spec.terms)
    return CostSpec(**d)


def planner(case):
    """One planner per (shape, horizon, mode, bound); model, cost and arithmetic are set per case."""
    from icem_amd import IcemConfig, IcemPlanner
    key = (case.o, case.d, case.h, case.mode, case.high)
    if key not in _planners:
        _planners[key] = IcemPlanner(IcemConfig(horizon=case.h, act_dim=case.d, num_traj=1100, opt_iters=1, dtype="f32", seed=7,
                                                cost_mode=case.mode), -case.high * np.ones(case.d), case.high * np.ones(case.d))
    return _planners[key]


def expected_arith(case, arith):
    return arith if W.split_fits(case.o, case.d) else "f32"


def configure(pl, case, arith):
    """Model, cost and arithmetic of the case on the planner; the arithmetic in effect is the one asked for."""
    om = CC.inputs(case)[0]
    pl.set_model(om.kind, om.A, om.B)
    pl.set_cost_spec(device_spec(case.spec))
    got = pl.set_wide_arith(arith)
    assert got == pl.wide_arith == expected_arith(case, arith), (case.name, arith, got, pl.wide_imbalance_log2)
    pl.reset()


def run_cases(cases):
    """Every case in every arithmetic.  Cases that share their inputs (the readouts of one model) share the model upload and the
    action tensor; returns (violations, worst row error per arithmetic)."""
    worst, bad = {}, []
    by_input = {}
    for case in cases:
        by_input.setdefault((CC.input_key(case), case.h, case.mode, case.high), []).append(case)
    for group in by_input.values():
        first = group[0]
        _, ob, acts = CC.inputs(first)
        pl = planner(first)
        a = torch.as_tensor(acts, dtype=pl.dt, device=pl.device)
        for arith in ARITHS:
            configure(pl, first, arith)
            for case in group:
                pl.set_cost_spec(device_spec(case.spec))
                assert pl.wide_arith == expected_arith(case, arith), (case.name, arith, pl.wide_arith)
                got = np_(pl.rollout_cost(ob, a))
                s = CC.errors(got, case, W.BOUNDS) if got.shape == CC.want(case).shape else None
                print(case.name, arith, s)
                if s is not None and s["worst"] > worst.get(arith, (-1.0, ""))[0]:
                    worst[arith] = (s["worst"], case.name)
                bad += [f"{case.name} [{arith}] {case.what}: {v}" for v in CC.violations(got, case, W.BOUNDS)]
    return bad, worst


@pytest.mark.parametrize("group", W.GROUPS)
def test_wide_readouts(group):
    """One (group, shape) of the table through rollout_cost: the loop over the units / entries / scale models runs in here."""
    cases = W.by_group(group)
    t0 = time.perf_counter()
    bad, worst = run_cases(cases)
    W.forget(cases)
    for arith, (e, name) in sorted(worst.items()):
        print(f"[worst] {group} {arith}: row error {e:.3g} ({name}), bound {W.BOUNDS.row:.3g}")
    print(f"[time] {group}: {len(cases)} cases x {len(ARITHS)} arithmetics in {time.perf_counter() - t0:.2f} s")
    assert not bad, f"{len(bad)} violations:\n" + "\n".join(bad[:40])


@pytest.mark.parametrize("shape", [(129, 3), (378, 17), (384, 64)], ids=W.tag)
def test_a_row_costs_the_same_wherever_it_sits(shape):
    """The same action rows at rows 0 .., 16 tt + 3 .. of every tile, in the ragged last tile and in the fifth tile of a FIVE
    launch, under a scale-group model: the same bits per arithmetic (the kernel's header: a row's result depends on that row and
    the model only, wherever the row sits in a launch)."""
    o, d = shape
    src = W.BY_NAME[f"{W.tag(shape)}-scale-pow2-unit{o - 1}"]
    _, ob, base = CC.inputs(src)
    h = src.h
    rows = np.random.RandomState(5).uniform(-1, 1, (3, h, d)).astype(np.float32).astype(np.float64)
    pl = planner(src)
    for arith in ARITHS:
        configure(pl, src, arith)
        alone = pl.rollout_cost(ob, torch.as_tensor(rows, dtype=pl.dt, device=pl.device))
        for n in (W.ROWS, W.ROWS_FIVE, W.ROWS_TWO):   # regular, FIVE (the fifth tile: rows 64 ..), two batches
            assert W.is_five(n) == (n == W.ROWS_FIVE)
            for pos in sorted({0, 16 + 3, 16 * ((n - 1) // 16), n - 3} | ({16 * tt + 3 for tt in range(n // 16)})):
                acts = np.resize(base, (n, h, d)).copy()
                acts[pos:pos + 3] = rows
                got = pl.rollout_cost(ob, torch.as_tensor(acts, dtype=pl.dt, device=pl.device))
                assert torch.equal(got[pos:pos + 3], alone), (arith, n, pos, got[pos:pos + 3].tolist(), alone.tolist())
                assert torch.isfinite(got).all()
    W.forget([src])


@pytest.mark.parametrize("N", [64, 300])
@pytest.mark.parametrize("arith", ARITHS)
def test_last_pool_of_whole_mpc_steps_on_the_gemm_kernels(arith, N):
    """icem_plan_step at (378, 17) under a scale-group model, two MPC steps of one iteration each: the last pool -- the sampled
    rows and, from step 1, the shifted elites behind them (N = 64: they open the fifth tile of the plane kernel's only workgroup,
    and in "f32" they are rolled out by rollout_rows_wide_kernel) -- re-scored under the per-row criterion."""
    from icem_amd import IcemConfig, IcemPlanner
    o, d = W.LONG_SHAPE
    src = W.BY_NAME[f"{W.tag(W.LONG_SHAPE)}-scale-pow2-unit374"]   # (374 % 5 == 4: a unit of the largest scale, so that the row's magnitude is its own)
    om, ob, _ = CC.inputs(src)
    pl = IcemPlanner(IcemConfig(horizon=src.h, act_dim=d, num_traj=N, opt_iters=1, dtype="f32", seed=7, cost_mode=src.mode), -np.ones(d), np.ones(d))
    configure(pl, src, arith)
    assert pl.n_reuse > 0
    made = []
    for s in range(2):
        obs = ob if s == 0 else CC.q22(0.9 * ob).astype(np.float32).astype(np.float64)
        pl.plan_step(obs)
        n_pool = pl.population_sizes[-1] + (pl.n_reuse if s > 0 else 0)
        assert pl.actions.shape[0] >= n_pool and pl.wide_arith == arith
        if N == 64 and s > 0:
            assert W.is_five(n_pool) and (n_pool - pl.n_reuse) % 16 == 0   # the fifth tile / the row-wise tail
        pool = np_(pl.actions[:n_pool])
        case = dataclasses.replace(src, name=f"{src.name}-{arith}-pool{s}-{N}", n=n_pool, claims=())
        CC.give_inputs(case, om, obs, pool)
        made.append(case)
        got = np_(pl.costs[:n_pool])
        print(case.name, CC.errors(got, case, W.BOUNDS))
        assert CC.agree(got, case, W.BOUNDS), (case.name, src.what, CC.violations(got, case, W.BOUNDS))
    W.forget(made + [src])
    for case in made:
        CC._given.pop(case.name, None)
