"""K1, the colored-noise sampler, on the case table of noise_cases.py against its float64 reference under its per-draw,
per-sample criterion (test_noise_sensitivity_cpu.py shows what that criterion rejects): the normals (icem_philox_normals) on the
table's keys and on every planted coordinate; the operator (icem_sample_clip: the folded kernel at its horizons, the generic
thread and quad forms elsewhere and in f64); a row's bits wherever it sits in a call; and the fused carriers of whole MPC steps
-- the single-launch kernel's quad phase, the sampler + rollout pair, the noise-ahead launches, the merge-prologue sampler -- whose
last pool is clip(mean + std y) of a distribution read off the planner, held per row to the criterion and, where the carrier
promises sample_row's bits, to icem_sample_clip bit for bit.

Every test prints its figures before it asserts ([worst] lines: run with -s); nothing is asserted against a number taken from
the device."""
import dataclasses

import numpy as np
import pytest
import torch

import cost_term_cases as CC
import noise_cases as NC
import tile_cases as TC

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
_planners, _refs = {}, {}


def np_(t):
    return t.detach().cpu().numpy().astype(np.float64)


def planner(case, name):
    """One planner per (shape, dtype, generator, beta, box, seed): the operators are stateless."""
    from icem_amd import IcemConfig, IcemPlanner
    key = (case.h, case.d, name, case.rounds, case.beta, case.dist, case.seed)
    if key not in _planners:
        low, high = NC.box(case.d, case.dist, NC.DTYPES[name])
        _planners[key] = IcemPlanner(IcemConfig(horizon=case.h, act_dim=case.d, num_traj=64, dtype=name, seed=case.seed,
                                                rng_rounds=case.rounds, noise_beta=case.beta), low, high)
    return _planners[key]


def ref(case, name):
    if (case.name, name) not in _refs:
        _refs[case.name, name] = NC.reference(case, NC.DTYPES[name])
    return _refs[case.name, name]


def draw_order(z_r, z_i, h):
    F = h // 2 + 1
    return np.concatenate([np_(z_r), np_(z_i)[..., 1:1 + h - F]], axis=-1)


def sample(pl, case, r, **over):
    kw = dict(offset=case.offset, first_index=case.first, row0_mean=case.row0, t_begin=case.t_begin)
    kw.update(over)
    n = kw.pop("n", case.n)
    return pl.sample_clip(n, r["mean"], r["std"], **kw)


# ---- the normals -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f32", "f64"])
def test_normals_on_the_tables_keys(name):
    dtype, worst, bad = NC.DTYPES[name], (0.0, None), []
    for case in NC.CASES:
        pl, r = planner(case, name), ref(case, name)
        z_r, z_i = pl.philox_normals(case.n, offset=case.offset, first_index=case.first)
        g = draw_order(z_r, z_i, case.h)
        assert (np_(z_i)[..., 0] == 0).all() and (np_(z_i)[..., 1 + case.h - (case.h // 2 + 1):] == 0).all(), case.name
        m = NC.normals_miss(g, r["g"], dtype)
        err = float(np.abs(g - r["g"]).max()) if np.isfinite(g).all() else np.inf
        print(case.name, name, f"worst |dg| {err:.3g}  miss {m:.3g}")
        worst = max(worst, (err, case.name))
        bad += [(case.name, err, m)] if not m <= 1.0 else []
    print(f"[worst] normals {name} table: |dg| {worst[0]:.3g} ({worst[1]}), bound {NC.E_G_F64 if dtype is F64 else NC.E_G_F32:.3g}")
    assert not bad, bad


@pytest.mark.parametrize("name", ["f32", "f64"])
def test_normals_on_the_planted_coordinates(name):
    """Every planted pair, and the rows around it, under the table's one bound."""
    dtype, worst, bad = NC.DTYPES[name], {}, []
    for cls, (row, dim, pair, word), case in NC.planted_cases():
        pl, r = planner(case, name), ref(case, name)
        z_r, z_i = pl.philox_normals(case.n, offset=case.offset, first_index=case.first)
        g = draw_order(z_r, z_i, case.h)
        at = slice(2 * pair, 2 * pair + 2)
        pair_dev, pair_ref = g[1, dim, at], r["g"][1, dim, at]
        err = float(np.abs(pair_dev - pair_ref).max()) if np.isfinite(pair_dev).all() else np.inf
        m = NC.normals_miss(g, r["g"], dtype)
        print(f"{cls} row {row} dim {dim} pair {pair} word {word:#x} {name}: device {pair_dev}, reference {pair_ref}, "
              f"|dg| {err:.3g}, case miss {m:.3g}")
        if err >= worst.get(cls, (-1.0, None))[0]:
            worst[cls] = (err, (row, dim, pair))
        bad += [(cls, row, dim, pair, err, m)] if not m <= 1.0 else []
        if cls == "u1_one" and dtype is F32:
            assert (pair_dev == 0).all(), (cls, row, pair_dev)           # sqrt(-2 ln 1): the normal is +-0
    for cls, (e, where) in sorted(worst.items()):
        print(f"[worst] normals {name} planted {cls}: |dg| {e:.3g} {where}, bound {NC.E_G_F64 if dtype is F64 else NC.E_G_F32:.3g}")
    assert not bad, bad


# ---- the operators -----------------------------------------------------------------------------------------------------------
def check_samples(case, name, got, r, tag, worst, bad):
    dtype, tb = NC.DTYPES[name], case.t_begin
    a_dev, a_ref = NC.time_slice(np_(got), tb), NC.time_slice(r["a"], tb)
    m = NC.samples_miss(a_dev, a_ref, r["std"][tb:], dtype)
    rows = slice(1, None) if case.row0 and case.first == 0 else slice(None)
    err = NC.samples_error(a_dev[rows], a_ref[rows], r["std"][tb:], NC.EPS32 if dtype is F32 else 0.0) if np.isfinite(a_dev).all() else np.inf
    print(case.name, name, tag, f"worst sample error / std {err:.3g}  miss {m:.3g}")
    if err > worst.get(tag, (-1.0, None))[0]:
        worst[tag] = (err, case.name)
    if not m <= 1.0:
        w = np.unravel_index(np.argmax(np.abs(a_dev - a_ref)), a_ref.shape)
        bad.append((case.name, name, tag, m, "worst at (row, t, j)", w, a_dev[w], a_ref[w]))


def report(worst, bad, what, name):
    for tag, (e, where) in sorted(worst.items()):
        print(f"[worst] {what} {name} {tag}: sample error / std {e:.3g} ({where}), bound {NC.E_Y_F64 if name == 'f64' else NC.E_Y_F32:.3g}")
    assert not bad, f"{len(bad)} violations:\n" + "\n".join(map(str, bad[:40]))


def test_the_folded_sampler_on_the_table():
    """icem_sample_clip on device noise at the folded sampler's horizons, f32: sample_folded_kernel, every case of the table and
    every planted row."""
    worst, bad, seen = {}, [], set()
    for case in NC.FOLDED_CASES + [c for _, _, c in NC.planted_cases()]:
        pl, r = planner(case, "f32"), ref(case, "f32")
        assert NC.form_of(case) == "folded"
        if (case.h, case.d) not in seen:   # once per shape: the launch is a sampler's
            pl.profile_enable(True)
            pl.profile_read()
            got = sample(pl, case, r)
            prof = pl.profile_read()
            pl.profile_enable(False)
            assert sorted(prof) == ["sample_clip"] and prof["sample_clip"][1:] == (1, case.n * case.h), (case.name, prof)
            seen.add((case.h, case.d))
        else:
            got = sample(pl, case, r)
        tag = "folded" if case.seed == NC.SEED else "folded planted"
        check_samples(case, "f32", got, r, tag, worst, bad)
        if case.row0:
            assert (np_(got)[0] == NC.w64(r["mean"])).all() == (case.first == 0), case.name
    report(worst, bad, "operator", "f32")


@pytest.mark.parametrize("name", ["f32", "f64"])
@pytest.mark.parametrize("quad", [0, 1], ids=["thread", "quad"])
def test_the_generic_sampler_on_the_table(quad, name):
    """The generic sampler (option gk_sample 0: one thread per row; 1: a quad per row) at the other horizons -- and, in f64, at the
    folded sampler's: the strict-parity sampler on device noise, one case per HMAX and more."""
    from icem_amd import _lib as L
    worst, bad = {}, []
    cases = NC.GENERIC_CASES + (NC.F64_FOLDED_H_CASES if name == "f64" else [])
    L.reset_options()
    try:
        L.set_option("gk_sample", quad)
        for case in cases:
            pl, r = planner(case, name), ref(case, name)
            if case.t_begin:
                out = torch.full((case.n, case.h, case.d), 9.0, dtype=pl.dt, device=pl.device)
                got = sample(pl, case, r, out=out)
                assert (np_(got)[:, :case.t_begin] == 9.0).all(), case.name     # icem.py:102: only the last steps are written
            else:
                got = sample(pl, case, r)
            check_samples(case, name, got, r, "quad" if quad else "thread", worst, bad)
            if case.row0:
                assert (np_(got)[0] == NC.w64(r["mean"])).all() == (case.first == 0), case.name
    finally:
        L.reset_options()
    report(worst, bad, "operator", name)


POSITIONS = [   # (case, option gk_sample or None for the folded kernel, rows per workgroup)
    ("12x6x45-b0.25-open", None, NC.SWG // 6),
    ("30x18x15-b0.25-tight-row0-first0", None, NC.SWG // 18),
    ("5x3x90-b0.25-open", 0, NC.WG // 3),
    ("5x3x90-b0.25-open", 1, (NC.WG // 4) // 3),
    ("32x4x70-b0.25-tight", 0, NC.WG // 4),
    ("32x4x70-b0.25-tight", 1, (NC.WG // 4) // 4),
]


@pytest.mark.parametrize("which", POSITIONS, ids=lambda w: f"{w[0]}-{'folded' if w[1] is None else ('thread', 'quad')[w[1]]}")
def test_a_row_draws_the_same_wherever_it_sits(which):
    """Global row R drawn alone (first_index = R, n = 1) has the bits of row R inside the longer call: at position 0, the last of
    a workgroup, the first of the next, and the last of the ragged last workgroup."""
    from icem_amd import _lib as L
    name, opt, tpw = which
    case = NC.BY_NAME[name]
    pl, r = planner(case, "f32"), ref(case, "f32")
    assert tpw < case.n and case.n % tpw, (tpw, case.n)
    L.reset_options()
    try:
        if opt is not None:
            L.set_option("gk_sample", opt)
        whole = sample(pl, case, r, row0_mean=False)
        for pos in (0, tpw - 1, tpw, case.n - 1):
            alone = sample(pl, case, r, n=1, first_index=case.first + pos, row0_mean=False)
            assert torch.equal(alone[0], whole[pos]), (name, pos, float((alone[0] - whole[pos]).abs().max()))
            pair = sample(pl, case, r, n=2, first_index=case.first + pos - 1, row0_mean=False) if case.first + pos else None
            assert pair is None or torch.equal(pair[1], whole[pos]), (name, pos)
    finally:
        L.reset_options()


# ---- the fused carriers ------------------------------------------------------------------------------------------------------
ARITH = {"tile-planes": ("auto", 1), "tile-f32": ("f32", 0)}
SINGLE = ({"sample_rollout"}, {"rollout_cost"})        # (categories profile_read() must show, categories it must not)
PAIR = ({"sample_clip", "rollout_cost"}, {"sample_rollout"})
AHEAD = ({"sample_rollout", "sample_clip"}, {"rollout_cost"})
# (shape, arithmetic, population, kernel categories, launch form, development options): test_gpu_tile_probes.POOLS' populations
CARRIERS = [
    ((30, 6, 17), "tile-planes", 533, SINGLE, "single launch, quad sampling phase", {}),
    ((13, 4, 17), "tile-planes", 533, SINGLE, "single launch, quad sampling phase, odd H", {}),
    ((30, 6, 17), "tile-planes", 535, PAIR, "sampler + rollout pair", {"fuse_max_rw": 0}),
    # (the noise-ahead launches need opt_iters >= 2 -- below --: a one-iteration step of 10 243 rows is one sample_rollout launch)
    ((30, 6, 17), "tile-planes", 10243, SINGLE, "one launch, 10 243 rows", {}),
]
SEED_STEP = 7


def device_spec(spec):
    from icem_amd.envs import CostSpec, CostTerm
    d = {f.name: getattr(spec, f.name) for f in dataclasses.fields(spec)}
    d["terms"] = tuple(CostTerm(**dataclasses.asdict(t)) for t in spec.terms)
    return CostSpec(**d)


def step_planner(shape, impl, N, iters):
    from icem_amd import IcemConfig, IcemPlanner
    h, d, o = shape
    src = TC.BY_NAME[f"{TC.tag(shape)}-unit16-k1-sum"]
    om, ob, _ = CC.inputs(src)
    pl = IcemPlanner(IcemConfig(horizon=h, act_dim=d, num_traj=N, opt_iters=iters, dtype="f32", seed=SEED_STEP), -np.ones(d), np.ones(d))
    pl.set_model(om.kind, om.A, om.B)
    pl.set_cost_spec(device_spec(src.spec))
    mode, want = ARITH[impl]
    assert pl.set_tile_arith(mode) == want and int(pl.lib.icem_wide_arith(pl._h)) == 0
    pl.reset()
    return pl, ob, src


def pool_reference(pl, n, call, mean, std, first=0, row0=True):
    """The float64 reference of rows first .. first + n of sampling call ``call`` under the distribution (mean, std) as the
    device held it."""
    case = NC._case(pl.h, pl.d, n, beta=pl.cfg.noise_beta, first=first, seed=SEED_STEP, offset=pl.noise_offset(call), row0=row0)
    tables = (pl.low.cpu().numpy(), pl.high.cpu().numpy(), mean, std)
    return case, NC.reference(case, F32, tables)


def hold_rows(pl, op, call, lo, hi, mean, std, row0, tag, worst, bad):
    """pl.actions[lo:hi] -- rows lo .. hi of sampling call ``call`` -- against the reference and against the operator's bits
    (``op``: a planner of the same shape and seed that is never stepped)."""
    case, r = pool_reference(pl, hi - lo, call, mean, std, first=lo, row0=row0)
    rows = pl.actions[lo:hi].clone()
    check_samples(case, "f32", rows, r, tag, worst, bad)
    if row0 and lo == 0 and not (np_(rows[0]) == NC.w64(mean)).all():
        bad.append((tag, "row 0 is not the mean"))
    want = op.sample_clip(hi - lo, mean, std, offset=pl.noise_offset(call), first_index=lo, row0_mean=row0)
    if not torch.equal(rows, want):
        diff = (rows - want).abs()
        bad.append((tag, "not the operator's bits", int((diff > 0).sum()), float(diff.max())))


def hold_shifted(pl, op, call, base, elites, mean, std, tag, bad):
    """The shifted-elite rows behind ``base`` sampled rows: the kept actions exact copies of the previous elites' (icem.py:97-100),
    the last action freshly drawn at the step's shift offset (icem.py:102) -- criterion and the operator's bits."""
    n_reuse = pl.n_reuse
    rows = pl.actions[base:base + n_reuse].clone()
    if not torch.equal(rows[:, :-1], elites[:n_reuse, 1:]):
        bad.append((tag, "kept actions of the shifted elites"))
    _, r = pool_reference(pl, n_reuse, call, mean, std, row0=False)
    m = NC.samples_miss(np_(rows)[:, -1:], r["a"][:, -1:], r["std"][-1:], F32)
    print(tag, f"shifted elites' last action: miss {m:.3g}")
    bad += [(tag, "shifted elites' last action", m)] if not m <= 1.0 else []
    want = op.sample_clip(n_reuse, mean, std, offset=pl.noise_offset(call))
    if not torch.equal(rows[:, -1], want[:, -1]):
        bad.append((tag, "shifted elites' last action: not the operator's bits"))


def second_obs(ob):
    return CC.q22(0.9 * ob).astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("carrier", CARRIERS, ids=[f"{TC.tag(c[0])}-{c[2]}" for c in CARRIERS])
def test_the_pool_of_one_iteration_steps(carrier):
    """Two MPC steps with opt_iters = 1: the pool is clip(mean + std y) of the distribution read from pl.mean / pl.std BEFORE the
    step -- the mean row, the sampled rows, and from the second step on the shifted elites."""
    from icem_amd import _lib as L
    shape, impl, N, classes, form, options = carrier
    worst, bad, made = {}, [], []
    L.reset_options()
    try:
        op, ob, src = step_planner(shape, impl, N, 1)          # the operator's planner: default options, never stepped
        made.append(src)
        for k, v in options.items():
            L.set_option(k, v)
        pl, _, _ = step_planner(shape, impl, N, 1)
        pl.profile_enable(True)
        for s in range(2):
            mean, std = pl.mean.cpu().numpy().copy(), pl.std.cpu().numpy().copy()
            elites = pl.current_elites()[0].clone() if s else None
            pl.plan_step(ob if s == 0 else second_obs(ob))
            torch.cuda.synchronize()
            tag = f"{form}, step {s}"
            hold_rows(pl, op, 2 * s, 0, N, mean, std, True, tag, worst, bad)
            if s and pl.n_reuse:
                hold_shifted(pl, op, 2 * s + 1, N, elites, mean, std, tag, bad)
        prof = pl.profile_read()
        print(form, {k: v[1:] for k, v in prof.items()})
        assert classes[0] <= set(prof) and not classes[1] & set(prof), (form, prof)
    finally:
        L.reset_options()
        TC.forget(made)
    report(worst, bad, "carrier", "f32")


# (shape, arithmetic, population, iterations, kernel categories or None, launch form, development options)
ITERATED = [
    ((30, 6, 17), "tile-planes", 533, 3, SINGLE, "single launch with a merge prologue", {}),
    ((30, 6, 17), "tile-planes", 535, 3, PAIR, "sample_folded_merge_kernel + rollout", {"fuse_max_rw": 0}),
    # 10 243 -> 8 194 rows: every iteration above the noise-ahead launches' 8 192 (noise_rows_kernel for the first step,
    # merge_noise_kernel for the second, the iter_ahead noise role for iteration 1, Stream16::run_xf's affine map)
    ((30, 6, 17), "tile-planes", 10243, 2, AHEAD, "noise-ahead launches", {}),
    # 10 243 -> 8 194 -> 6 555: the last iteration is below them and the pipeline stays off: six sample_rollout launches
    ((30, 6, 17), "tile-planes", 10243, 3, SINGLE, "single launches with merge prologues, 10 243 rows", {}),
    # 12 805 -> 10 244 -> 8 195 (none a multiple of 16): three iterations of noise-ahead launches, the iter_ahead noise role twice
    ((30, 6, 17), "tile-planes", 12805, 3, AHEAD, "noise-ahead launches, three iterations", {}),
]


@pytest.mark.parametrize("carrier", ITERATED, ids=[f"{TC.tag(c[0])}-{c[2]}-{c[3]}it" for c in ITERATED])
def test_the_pools_of_iterated_steps(carrier):
    """opt_iters = 3 (2), two MPC steps.  The distribution in front of every iteration comes from a split-API twin (held bit-equal
    to the one-call step by the suite, and here through the executed action).  The one-call step's last pool is held to it whole.
    Consecutive iterations alternate between pl.actions and the handle's second pool, so of iteration 0 of a three-iteration step
    the rows the last, smaller pool has not overwritten are held too -- pl.actions[pop[2] : pop[0]] -- and in the second step the
    shifted elites behind them.  Not under the noise-ahead launches: they keep every pool but the last in buffers of the handle's
    own (those rows of pl.actions stay zero), so what noise_rows_kernel and merge_noise_kernel draw for iteration 0 is seen here
    through its elites: the K rows the first merge of a two-iteration step leaves in the elite pair's other half are held to the
    operator's rows bit for bit, and the twin's distribution in front of the last iteration, under which the last pool has the
    operator's bits, is their refit."""
    from icem_amd import _lib as L
    shape, impl, N, iters, classes, form, options = carrier
    worst, bad, made = {}, [], []
    L.reset_options()
    try:
        op, ob, src = step_planner(shape, impl, N, iters)      # the operator's planner: default options, never stepped
        made.append(src)
        for k, v in options.items():
            L.set_option(k, v)
        pl, _, _ = step_planner(shape, impl, N, iters)
        twin, _, _ = step_planner(shape, impl, N, iters)
        pl.profile_enable(True)
        pop = pl.population_sizes
        assert all(a > b for a, b in zip(pop, pop[1:])), pop
        for s in range(2):
            obs = ob if s == 0 else second_obs(ob)
            dist = [(twin.mean.cpu().numpy().copy(), twin.std.cpu().numpy().copy())]
            elites = twin.current_elites()[0].clone() if s else None

            def on_iteration(it):
                dist.append((twin.mean.cpu().numpy().copy(), twin.std.cpu().numpy().copy()))
            a_twin = twin.plan_step(obs, on_iteration=on_iteration).clone()
            a = pl.plan_step(obs).clone()
            torch.cuda.synchronize()
            assert torch.equal(a, a_twin), (form, s, "the split-API twin is not the one-call step's twin")
            for it in range(iters - 1, -1 if classes is not AHEAD else iters - 2, -2):     # (the iterations whose pool is pl.actions)
                last = it == iters - 1
                lo = 0 if last else pop[it + 2]
                tag = f"{form}, step {s}" + ("" if last else f", iteration {it} rows {lo}..{pop[it]}")
                hold_rows(pl, op, (iters + 1) * s + it, lo, pop[it], *dist[it], last, tag, worst, bad)
            if s and pl.n_reuse and iters % 2 and classes is not AHEAD:
                hold_shifted(pl, op, (iters + 1) * s + iters, pop[0], elites, *dist[0], f"{form}, step {s}", bad)
            if iters == 2:
                # iteration 0's elites are still in the elite pair's other half: K whole rows of iteration 0's pool, each the
                # operator's row bit for bit (or, in the second step, a shifted elite) -- the per-sample view of what the
                # noise-ahead launches draw for iteration 0 (noise_rows_kernel, then merge_noise_kernel)
                held = pl.elites_actions[(s * iters + 1) & 1].clone()
                cand = op.sample_clip(pop[0], *dist[0], offset=pl.noise_offset((iters + 1) * s))
                if s and pl.n_reuse:
                    last = op.sample_clip(pl.n_reuse, *dist[0], offset=pl.noise_offset((iters + 1) * s + iters))[:, -1:]
                    cand = torch.cat([cand, torch.cat([elites[:pl.n_reuse, 1:], last], dim=1)])
                found = [bool((cand == e).flatten(1).all(dim=1).any()) for e in held]
                print(f"{form}, step {s}: iteration 0's elites found among the operator's rows: {found}")
                if not all(found):
                    bad.append((f"{form}, step {s}", "an elite of iteration 0 is not a row of the operator's pool", found))
        prof = pl.profile_read()
        print(form, {k: v[1:] for k, v in prof.items()})
        assert classes is None or (classes[0] <= set(prof) and not classes[1] & set(prof)), (form, prof)
        if classes is AHEAD:   # the pipeline's own launch of raw noise rows: the first step's, which nobody predicted
            assert prof["sample_clip"][1:] == (1, pop[0] * pl.h), prof
    finally:
        L.reset_options()
        TC.forget(made)
    report(worst, bad, "carrier", "f32")
