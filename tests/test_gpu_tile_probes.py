"""The narrow tile kernels' model step -- Tile16H (fp16 planes, the default), Tile16 and Tile4 (exact f32) of fused_dev.h, in
rollout16_kernel, sample_rollout_kernel (Tile16H::step_lone included) and iter_ahead_kernel -- on the case table of
tile_cases.py, against the float64 oracle under cost_term_cases.py's per-row criterion with that table's bounds: every row
that is not near a threshold within ROW_BOUND of its per-mode magnitude, no share allowance; bounds measured between two CPU
evaluations, none taken from a kernel; test_tile_sensitivity_cpu.py shows what the criterion rejects.  A violation names the
state unit, the action entry or the model entries its case reads out.

Implementations: tile-planes (set_tile_arith("auto"), tile_arith == 1; one-tile widths only) and tile-f32 (tile_arith == 0).
The route witness of test_gpu_shape_edges.py -- icem_wide_arith == 0 (the tile route; 1 would be the exact-f32 GEMM kernel) on
every case, ``rollout_cost`` among profile_read()'s categories once per shape and implementation -- fails a case that is
silently served by another kernel.

Every (case, implementation) prints its figures (errors()) before it asserts, every test the worst row error per
implementation: run with -s to read them.
"""
import dataclasses

import numpy as np
import pytest
import torch

import cost_term_cases as CC
import tile_cases as TC

pytestmark = pytest.mark.gpu

ARITH = {"tile-planes": ("auto", 1), "tile-f32": ("f32", 0)}
_planners, _witnessed = {}, set()


def np_(t):
    return t.detach().cpu().numpy().astype(np.float64)


def device_spec(spec):
    from icem_amd.envs import CostSpec, CostTerm
    d = {f.name: getattr(spec, f.name) for f in dataclasses.fields(spec)}
    d["terms"] = tuple(CostTerm(**dataclasses.asdict(t)) for t in spec.terms)
    return CostSpec(**d)


def planner(case):
    """One planner per (shape, mode, bound); model, cost and arithmetic are set per case."""
    from icem_amd import IcemConfig, IcemPlanner
    key = (case.o, case.d, case.h, case.mode, case.high)
    if key not in _planners:
        _planners[key] = IcemPlanner(IcemConfig(horizon=case.h, act_dim=case.d, num_traj=1100, opt_iters=1, dtype="f32", seed=7,
                                                cost_mode=case.mode), -case.high * np.ones(case.d), case.high * np.ones(case.d))
    return _planners[key]


def implementations(case):
    planes = TC.planes_served(case.o) and not (case.spec.flip_idx >= 0 and case.spec.flip_thresh < 0)
    return (["tile-planes"] if planes else []) + ["tile-f32"]


def configure(pl, case, impl):
    """Model, cost and arithmetic of the case on the planner; the route is the tile's, in the arithmetic asked for."""
    om = CC.inputs(case)[0]
    pl.set_model(om.kind, om.A, om.B)
    pl.set_cost_spec(device_spec(case.spec))
    mode, want = ARITH[impl]
    assert pl.set_tile_arith(mode) == want, (case.name, impl, pl.tile_growth)
    assert int(pl.lib.icem_wide_arith(pl._h)) == 0, (case.name, impl, "not on the tile route")
    pl.reset()


def kernel_costs(case, impl):
    _, ob, acts = CC.inputs(case)
    pl = planner(case)
    configure(pl, case, impl)
    a = torch.as_tensor(acts, dtype=pl.dt, device=pl.device)
    witness = (TC.shape_of(case), impl)
    if witness not in _witnessed:   # once per shape and implementation: the launch is the tile rollout's
        pl.profile_enable(True)
        pl.profile_read()
        got = pl.rollout_cost(ob, a)
        prof = sorted(pl.profile_read())
        pl.profile_enable(False)
        assert prof == ["rollout_cost"], (case.name, impl, prof)
        _witnessed.add(witness)
        return np_(got)
    return np_(pl.rollout_cost(ob, a))


def check(case, impl, worst):
    """[] or the violations of one (case, implementation), each naming what the case reads out."""
    got = kernel_costs(case, impl)
    s = CC.errors(got, case, TC.BOUNDS) if got.shape == CC.want(case).shape else None
    print(case.name, impl, s)
    if s is not None and s["worst"] > worst.get(impl, (-1.0, ""))[0]:
        worst[impl] = (s["worst"], case.name)
    return [f"{case.name} [{impl}] {case.what}: {v}" for v in CC.violations(got, case, TC.BOUNDS)]


@pytest.mark.parametrize("group", TC.GROUPS)
def test_tile_readouts(group):
    """One (shape, group) of the table through rollout_cost (rollout16_kernel): the loop over the units / entries runs in here."""
    cases = TC.by_group(group)
    worst, bad = {}, []
    for case in cases:
        if case.spec.flip_idx >= 0 and case.spec.flip_thresh < 0 and TC.planes_served(case.o):
            pl = planner(case)   # a negative flip threshold: the handle keeps the exact tile whatever is asked
            om = CC.inputs(case)[0]
            pl.set_model(om.kind, om.A, om.B)
            pl.set_cost_spec(device_spec(case.spec))
            assert pl.set_tile_arith("auto") == 0 and pl.set_tile_arith("f16x2") == 0, case.name
        for impl in implementations(case):
            bad += check(case, impl, worst)
    TC.forget(cases)
    for impl, (e, name) in sorted(worst.items()):
        print(f"[worst] {group} {impl}: row error {e:.3g} ({name}), bound {TC.BOUNDS.row:.3g}")
    assert not bad, f"{len(bad)} violations:\n" + "\n".join(bad[:40])


@pytest.mark.parametrize("shape", [(30, 6, 17), (30, 17, 24)], ids=TC.tag)
def test_a_row_costs_the_same_wherever_it_sits(shape):
    """One action row at rows 0, 15, 16, in the ragged last tile and alone: its cost has the same bits, in both arithmetics
    (a lane, a tile or a launch size that changed a trajectory's arithmetic would show here)."""
    h, d, o = shape
    src = TC.BY_NAME[f"{TC.tag(shape)}-flip16-lin{o - 1}-k1-sum"]
    _, ob, base = CC.inputs(src)
    n = TC.ROWS
    base = base[:n]
    row = np.random.RandomState(5).uniform(-1, 1, (h, d)).astype(np.float32).astype(np.float64)
    pl = planner(src)
    for impl in implementations(src):
        configure(pl, src, impl)
        alone = pl.rollout_cost(ob, torch.as_tensor(row[None], dtype=pl.dt, device=pl.device))[0]
        for pos in (0, 15, 16, n - 1):
            acts = base.copy()
            acts[pos] = row
            got = pl.rollout_cost(ob, torch.as_tensor(acts, dtype=pl.dt, device=pl.device))
            assert torch.equal(got[pos], alone), (impl, pos, float(got[pos]), float(alone))
            others = np.delete(np.arange(n), pos)
            assert torch.isfinite(got[others]).all()
    TC.forget([src])


SINGLE = ({"sample_rollout"}, {"rollout_cost"})        # (categories profile_read() must show, categories it must not)
PAIR = ({"sample_clip", "rollout_cost"}, {"sample_rollout"})
AHEAD = ({"sample_rollout", "sample_clip"}, {"rollout_cost"})   # (sample_clip: the pipeline's own launch of raw noise rows, see below)
# (shape, arithmetic, population, iterations, kernel categories, launch form[, development options the steps run under])
POOLS = [
    ((30, 6, 17), "tile-planes", 533, 3, SINGLE, "single launch, Tile16H::step_lone"),
    ((30, 6, 17), "tile-f32", 533, 3, SINGLE, "single launch, Tile4"),
    ((30, 6, 18), "tile-planes", 533, 3, SINGLE, "single launch, Tile16H::step (REM = 2)"),
    ((30, 6, 18), "tile-f32", 533, 3, SINGLE, "single launch, Tile4"),
    ((13, 4, 17), "tile-planes", 533, 3, SINGLE, "single launch, Tile16H"),
    ((13, 4, 17), "tile-f32", 533, 3, SINGLE, "single launch, Tile4"),
    ((30, 17, 24), "tile-f32", 533, 3, SINGLE, "single launch, two output tiles"),
    # (what populations beyond the single-launch kernel's slabs take at two output tiles: here at 535 rows, by switching that kernel off)
    ((30, 17, 24), "tile-f32", 535, 3, PAIR, "sampler + rollout16 pair, two output tiles", {"fuse_max_rw": 0}),
    # the smallest population whose every iteration stays above 8192 rows (512 tiles), with ragged last tiles: 10 243, 8 194
    ((30, 6, 17), "tile-planes", 10243, 2, AHEAD, "noise-ahead launches, Stream16::run_xf"),
]
POOL_COSTS = ("unit16", "shiftB")


@pytest.mark.parametrize("cost", POOL_COSTS)
@pytest.mark.parametrize("pool", POOLS, ids=[f"{TC.tag(p[0])}-{p[1]}-{p[2]}" for p in POOLS])
def test_last_pool_of_whole_mpc_steps_on_the_tile(pool, cost):
    """icem_plan_step on the tile kernels, two MPC steps: the last pool -- sampled rows of a decayed population with a ragged
    last tile, shifted-elite rows -- re-scored under the per-row criterion; the launches are of the class the case names."""
    from icem_amd import IcemConfig, IcemPlanner, _lib as L
    shape, impl, N, iters, classes, form = pool[:6]
    options = pool[6] if len(pool) > 6 else {}
    h, d, o = shape
    name = f"{TC.tag(shape)}-unit16-k1-sum" if cost == "unit16" else f"{TC.tag(shape)}-shiftB{o - d}-act{d - 1}"
    src = TC.BY_NAME[name]
    om, ob, _ = CC.inputs(src)

    def make(n_traj):
        pl = IcemPlanner(IcemConfig(horizon=h, act_dim=d, num_traj=n_traj, opt_iters=iters, dtype="f32", seed=7), -np.ones(d), np.ones(d))
        configure(pl, src, impl)
        pl.profile_enable(True)
        return pl
    L.reset_options()
    made = []
    try:
        for k, v in options.items():
            L.set_option(k, v)
        pl = make(N)
        assert all(n % 16 for n in pl.population_sizes), pl.population_sizes
        if N > 8192:
            assert min(pl.population_sizes) > 8192
        for s in range(2):
            obs = ob if s == 0 else CC.q22(0.9 * ob).astype(np.float32).astype(np.float64)
            pl.plan_step(obs)
            n_last = pl.population_sizes[-1]
            pool = np_(pl.actions[:n_last])
            case = dataclasses.replace(src, name=f"{src.name}-{impl}-pool{s}-{N}", n=n_last, claims=())
            CC.give_inputs(case, om, obs, pool)
            made.append(case)
            got = np_(pl.costs[:n_last])
            print(case.name, form, CC.errors(got, case, TC.BOUNDS))
            assert CC.agree(got, case, TC.BOUNDS), (case.name, form, src.what, CC.violations(got, case, TC.BOUNDS))
        prof = pl.profile_read()
        print(src.name, impl, form, {k: v[1:] for k, v in prof.items()})
        assert classes[0] <= set(prof) and not classes[1] & set(prof), (form, prof)
    finally:
        L.reset_options()
    if N > 8192:
        # sample_rollout is the noise-ahead launch here, not the single-launch kernel: only that pipeline draws a step nobody
        # predicted -- the first -- as ONE launch of raw noise rows (pop[0] x h units); with it switched off there is no such launch
        assert prof["sample_clip"][1:] == (1, pl.population_sizes[0] * h), prof
        try:
            L.set_option("noise_ahead", 0)
            twin = make(N)
            twin.plan_step(ob)
            torch.cuda.synchronize()
            assert "sample_clip" not in twin.profile_read()
        finally:
            L.reset_options()
    TC.forget(made + [src])
    for case in made:
        CC._given.pop(case.name, None)
