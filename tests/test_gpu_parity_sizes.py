"""Parity of the f32 THROUGHPUT kernels at the benchmark's own sizes (BASELINE.json configs[1..3]), held to
north_star's bar: elite index sets bit-exact, costs / mean / std / executed action within 1e-5 relative.

The only part of the device loop the float64 oracle cannot restate bit for bit is the Box-Muller transform on the
hardware log2 / sqrt / sin / cos (<= 4e-6 absolute on a normal).  These tests take it out of the comparison: the
oracle is driven by the DEVICE's own f32 normals (``icem_philox_normals`` -- same stream, same transform as the
fused samplers), so everything downstream -- inverse DFT, affine + clip, rollout, cost, top-K, refit, elite
shifting / keeping, the executed action -- is compared at 1e-5 with exact elite index sets, at N = 4096 x 5 and
N = 65536 x 5 iterations (h=30, d=6, o=17, beta=0.25) and on the d=17 / beta=2 shape.

Two planners run every case: one through the split API (``icem_plan_iter_local`` / ``_merge``; per-iteration
state is visible between the calls and is what the oracle is compared with), one through ``icem_plan_step`` (the
launches ``bench.py`` times: merges folded into the next launch's prologue, ping-pong buffers), which must
reproduce the split run bit for bit.  References: icem/controllers/icem.py:106-211.
"""
import numpy as np
import pytest
import torch

from oracle import icem_oracle as O
from oracle_loop import ATOL, RTOL, DeviceNormals, full_loop, np_

pytestmark = pytest.mark.gpu

# (RTOL, ATOL = 1e-5, 2e-6: north_star: 1e-5 relative; the floor covers entries near zero (actions live in [-1, 1]))
# Trajectory costs are sums of h step costs whose positive (control, penalty) and negative (velocity / height) terms
# cancel: "1e-5 relative" is taken relative to the MAGNITUDE of that sum -- sum_t sum |addend|, the scale rounding errors
# have (oracle.rollout_cost_magnitudes) -- with no absolute floor on top: a cost is never granted more than 1e-5 of what
# was added up to make it.


def _make(N, iters, h, d, o, kind, beta, seed, env_kind, cost_mode="sum", arith=None, model_ab=None):
    from icem_amd import DeviceSyntheticModel, IcemConfig, IcemPlanner, halfcheetah_env, humanoid_standup_env
    from icem_amd import envs as E
    shipped = {"door": (E.door_env, O.CostSpec.door), "relocate": (E.relocate_env, O.CostSpec.relocate),
               "fpp": (E.fetch_pick_and_place_env, O.CostSpec.fetch_pick_and_place)}
    if env_kind in shipped:
        env = shipped[env_kind][0]()
        assert (env.obs_dim, env.action_space.shape[0]) == (o, d)
    else:
        env = halfcheetah_env(o) if env_kind == "halfcheetah" else humanoid_standup_env(o)
    model = DeviceSyntheticModel.make(o, d, kind=kind) if model_ab is None else DeviceSyntheticModel(model_ab[0], model_ab[1], kind)

    def mk():
        pl = IcemPlanner(IcemConfig(horizon=h, act_dim=d, num_traj=N, opt_iters=iters, dtype="f32", seed=seed,
                                    noise_beta=beta, cost_mode=cost_mode), env.action_space.low, env.action_space.high)
        pl.set_model(model.kind, model.A, model.B)
        pl.set_cost_spec(env.cost_spec)
        if arith is not None:   # icem_set_tile_arith: 0 = the exact f32 tile, 1 = fp16 planes (None: by the configuration)
            assert pl.set_tile_arith(arith) == arith
        pl.reset()
        return pl
    if env_kind in shipped:
        oc = shipped[env_kind][1]()
    else:
        oc = O.CostSpec.halfcheetah(o) if env_kind == "halfcheetah" else O.CostSpec.humanoid_standup()
    return env, model, oc, mk


CASES = [
    # BASELINE configs[1]: the benchmark's headline workload
    pytest.param(4096, 5, 30, 6, 17, 0, 0.25, "halfcheetah", 1234, id="c2_N4096x5"),
    pytest.param(4096, 5, 30, 6, 17, 1, 0.25, "halfcheetah", 7, id="c2_tanh_N4096x5"),
    # BASELINE configs[3] on one GPU: north_star's roofline target size
    pytest.param(65536, 5, 30, 6, 17, 0, 0.25, "halfcheetah", 1234, id="c4_N65536x5"),
    # BASELINE configs[2] (latent o=24): 17 action dims, beta = 2
    pytest.param(16384, 3, 30, 17, 24, 1, 2.0, "humanoid", 1234, id="c3_N16384x3_d17_beta2"),
    # HumanoidStandup at its REAL observation width (icem/environments/mujoco.py:241-252): the GEMM rollout kernel
    pytest.param(2048, 2, 30, 17, 378, 1, 2.0, "humanoid", 5, id="c3wide_o378_N2048x2"),
    # ... and at the size `bench.py --workload c3` / `also_c3` times it: 16 384 rows x 3 iterations; from the second MPC
    # step on rows 16 384..16 386 (the shifted elites) are the fifth tile of the launch's first workgroup
    pytest.param(16384, 3, 30, 17, 378, 1, 2.0, "humanoid", 1234, id="c3wide_o378_N16384x3"),
]


@pytest.mark.parametrize("N,iters,h,d,o,kind,beta,env_kind,seed", CASES)
def test_full_loop_at_benchmark_size_against_oracle_on_device_normals(N, iters, h, d, o, kind, beta, env_kind, seed):
    _full_loop(N, iters, h, d, o, kind, beta, env_kind, seed, "sum")


# The tile arithmetic (icem_set_tile_arith) at the same bar.  c2 and c4 above run on the fp16 planes by default (AUTO: wherever
# the tile serves them); here: c2 and c4 on the exact tile, the tanh model and the o = 18 shape on the planes at that size, and
# the headline population forced onto the planes (its single-launch kernel then rolls out on Tile16H).
@pytest.mark.parametrize("N,iters,o,kind,arith,mode,seed", [
    pytest.param(65536, 5, 17, 0, 0, "sum", 1234, id="c4_exact_tile"),
    pytest.param(65536, 3, 17, 1, 1, "sum", 11, id="c4_tanh_fp16_planes"),
    pytest.param(40000, 3, 18, 0, 1, "best", 12, id="o18_fp16_planes_best"),
    pytest.param(4096, 5, 17, 0, 1, "sum", 1234, id="c2_fp16_planes"),
    pytest.param(4096, 5, 17, 0, 0, "sum", 1234, id="c2_exact_tile"),
    pytest.param(4096, 3, 17, 1, 1, "final", 13, id="c2_tanh_fp16_planes_final"),
])
def test_full_loop_in_each_tile_arithmetic(N, iters, o, kind, arith, mode, seed):
    _full_loop(N, iters, 30, 6, o, kind, 0.25, "halfcheetah", seed, mode, arith=arith)


@pytest.mark.parametrize("cost_mode", ["best", "final"])
def test_full_loop_at_benchmark_size_best_and_final(cost_mode):
    """cost_along_trajectory = "best" / "final" (abstract_controller.py:82-87) through the WHOLE loop at the headline
    population (N = 4096 x 5 iterations), held to the same bar as "sum": elite index sets identical to the float64
    oracle's in every iteration, costs to 1e-5 of their magnitude."""
    _full_loop(4096, 5, 30, 6, 17, 1, 0.25, "halfcheetah", 21, cost_mode)


# The reference's other shipped settings (settings/{door,relocate,fpp}: icem/environments/mjenvs.py:57-78, 155-174,
# robotics.py:150-164; beta from README.md:21-29) at the headline population, on the TileHN kernel (k_rollout_hn.hip: the model
# step on the 16-bit matrix cores, the term list across the four lanes of a trajectory): the same bar -- every cost within
# 1e-5 of its magnitude, the float64 oracle's elite sets -- with the indicator terms (opening / closeness bonuses) in play.
@pytest.mark.parametrize("env_kind,d,o,beta,kind,seed", [
    pytest.param("door", 28, 39, 2.5, 1, 31, id="door_N4096x3"),
    pytest.param("relocate", 30, 39, 3.5, 1, 32, id="relocate_N4096x3"),
    pytest.param("fpp", 4, 28, 3.0, 0, 33, id="fpp_N4096x3"),
])
def test_full_loop_on_the_shipped_door_relocate_fpp_shapes(env_kind, d, o, beta, kind, seed):
    _full_loop(4096, 3, 30, d, o, kind, beta, env_kind, seed, "sum", expect_arith=1)


# The literal bound, for the record.  A trajectory cost is a sum of h x (d + 2) addends of both signs; an
# f32 sum carries rounding of ~1e-6 of what was ADDED UP (the magnitude), so |err| / |cost| is that times the cancellation
# factor magnitude / |cost|.  The tests hold every cost to 1e-5 of its magnitude; LITERALLY 1e-5 of |cost| is asserted for the
# trajectories whose sum does not cancel below half of its magnitude, and the whole distribution -- max |err| / |cost| per
# cancellation bucket -- is written to gpurun_out/literal_bounds.jsonl (copied to profiles/ per round) and printed (`pytest -s`).
LITERAL_BUCKETS = (0.5, 0.1, 0.01, 0.0)   # |cost| / magnitude at least ...


def _literal_record(tag, case, err, cost, mag):
    import json
    import os
    ratio = np.abs(cost) / mag
    lit = err / np.maximum(np.abs(cost), 1e-300)
    row = {"case": case, "where": tag, "n": int(err.size), "max_err_over_magnitude": float((err / mag).max()), "buckets": []}
    hi = np.inf
    for lo in LITERAL_BUCKETS:
        pick = (ratio >= lo) & (ratio < hi)
        row["buckets"].append({"cost_over_magnitude": f">= {lo}" if hi == np.inf else f"[{lo}, {hi})", "share": float(pick.mean()),
                               "max_err_over_cost": float(lit[pick].max()) if pick.any() else None})
        hi = lo
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    if os.path.isdir(out):
        with open(os.path.join(out, "literal_bounds.jsonl"), "a") as f:
            f.write(json.dumps(row) + "\n")
    print("[literal bound]", json.dumps(row))
    return row


def _growing_model(o, d, rate, seed=2):
    """x' = x A + a B with A = rate I (+ a weak coupling into the scored entry, which itself decays): states of 1e4-1e5 at the
    end of the horizon, costs of 1e3-1e5 -- finite and ordered in the reference's float64 (icem.py:147-159, 199)."""
    A = rate * np.eye(o)
    A[:, 8] += 0.01
    A[8, 8] = 0.5
    B = 0.05 * np.random.RandomState(seed).randn(d, o)
    return A, B


@pytest.mark.parametrize("env_kind,d,o,rate,beta,seed", [
    pytest.param("halfcheetah", 6, 17, 1.5, 0.25, 41, id="halfcheetah_A1.5I_N4096x3"),
    pytest.param("door", 28, 39, 1.4, 2.5, 42, id="door_A1.4I_N4096x3"),
])
def test_full_loop_with_a_model_that_outgrows_fp16_range(env_kind, d, o, rate, beta, seed):
    """the DEFAULT arithmetic on a model whose states leave fp16's range inside the horizon (1.5^30 = 1.9e5 >
    2^11).  Round 5 rolled such a model out on the fp16 planes: every cost NaN, the elites chosen by index.  Now the handle
    sees the reachable growth at icem_set_model (icem_tile_growth > 2^10), keeps the exact tile / the exact-f32 GEMM kernel,
    and the whole loop holds north_star's bar against the float64 oracle: elite sets identical, every cost finite, 1e-5."""
    # (an EXPANDING system amplifies every rounding with the state: 30 steps of an f32 chain at a growth of 1e5 carry 2-3e-5 of
    #  the magnitude whatever computes them in f32 -- the bar here is 5e-5 and, as everywhere, identical elite sets; strict
    #  parity on such a model is dtype f64)
    _full_loop(4096, 3, 30, d, o, 0, beta, env_kind, seed, "sum", expect_arith=0, model_ab=_growing_model(o, d, rate), rtol=5e-5)


def _full_loop(N, iters, h, d, o, kind, beta, env_kind, seed, cost_mode, arith=None, expect_arith=None, model_ab=None, rtol=None):
    """The whole-loop comparison (tests/oracle_loop.py: full_loop) on the env factories above, plus the literal bound."""
    RTOL_C = rtol if rtol is not None else RTOL
    env, model, oc, mk = _make(N, iters, h, d, o, kind, beta, seed, env_kind, cost_mode, arith, model_ab)
    om = O.SyntheticModel(model.A, model.B, model.kind)

    def literal(tag, err, cost, mag, split):
        # ... and LITERALLY 1e-5 of |cost| wherever the sum does not cancel below half of what was added up
        case = f"{env_kind} N={N}x{iters} d={d} o={o} kind={kind} {cost_mode} arith={split.tile_arith if o <= 48 else split.wide_arith}" + (" growing-model" if model_ab is not None else "")
        row = _literal_record(tag, case, err, cost, mag)
        if row["buckets"][0]["max_err_over_cost"] is not None:
            assert row["buckets"][0]["max_err_over_cost"] <= 2 * RTOL_C, (tag, row)
    full_loop(mk, om, oc, N=N, iters=iters, h=h, o=o, beta=beta, cost_mode=cost_mode, low=env.action_space.low,
              high=env.action_space.high, rtol=rtol, expect_arith=expect_arith, on_iter_record=literal)


@pytest.mark.parametrize("exact", [0, 1, 2])   # icem_set_wide_exact: fp16 planes (default) / exact f32 / bf16 planes
@pytest.mark.parametrize("kind,mode", [(1, "sum"), (0, "best")])
def test_wide_shifted_elite_rows_equal_the_tile_kernel_bit_for_bit(kind, mode, exact):
    """o = 378: the shifted elites of iteration 0 (icem.py:131-137) would open a tile of their own behind a population
    that fills whole tiles.  Exact-f32 path: they are rolled out row by row instead (rollout_rows_wide_kernel: one fmaf
    chain per observation column in the matrix pipe's order) and reach the merge through the cost array.  bf16-split path
    (default): the launch's first workgroup takes them as a fifth tile of its batch.  Either way their costs are the
    bits the tile kernel produces for the same rows wherever they sit in a launch, and the step's result is the one the
    all-tiles path gives."""
    from icem_amd import DeviceSyntheticModel, IcemConfig, IcemPlanner, humanoid_standup_env
    o, d, h = 378, 17, 30
    env = humanoid_standup_env(o)
    model = DeviceSyntheticModel.make(o, d, kind=kind)

    def mk(N):
        pl = IcemPlanner(IcemConfig(horizon=h, act_dim=d, num_traj=N, opt_iters=2, dtype="f32", seed=3, noise_beta=2.0,
                                    cost_mode=mode), env.action_space.low, env.action_space.high)
        pl.set_wide_exact(exact)
        pl.set_model(model.kind, model.A, model.B)
        pl.set_cost_spec(env.cost_spec)
        pl.reset()
        return pl
    pl = mk(64)
    n_reuse = pl.n_reuse
    assert n_reuse > 0
    seen = {}

    def on_iteration(it):
        if it == 0:
            seen["costs"] = pl.costs[:64 + n_reuse].clone()
            seen["actions"] = pl.actions[:64 + n_reuse].clone()
    for s in range(2):
        obs = 0.1 * np.random.RandomState(s).randn(o)
        pl.plan_step(obs, on_iteration=on_iteration)
    tile = pl.rollout_cost(obs, seen["actions"])          # every row through rollout_wide_kernel's tiles
    assert torch.equal(tile, seen["costs"])
    # the elites of iteration 0 come out of pool costs either way: same selection as a host top-k of those costs
    idx = O.topk_sorted(seen["costs"].cpu().numpy(), pl.K)
    assert idx.max() < 64 + n_reuse


def test_box_muller_residual_is_the_only_f32_term_the_oracle_cannot_restate():
    """The looser bounds of the Philox-mode tests in test_gpu_parity.py (rtol 2e-4 / 5e-4) are the RNG-only residual:
    the device's normals differ from the oracle's float32 Box-Muller by the hardware transcendentals (measured here,
    bound 4e-6 absolute), while the integer side of the generator is bit-exact (a normal never lands in another
    stream position)."""
    from icem_amd import IcemConfig, IcemPlanner
    h, d, n = 30, 6, 4096
    pl = IcemPlanner(IcemConfig(horizon=h, act_dim=d, num_traj=n, dtype="f32", seed=99), -np.ones(d), np.ones(d))
    z_r, z_i = pl.philox_normals(n, offset=3)
    w_r, w_i = O.philox_white_noise(99, 3, n, d, h, dtype=np.float32)
    err = max(np.abs(np_(z_r) - w_r).max(), np.abs(np_(z_i) - w_i).max())
    assert err <= 4e-6, err
    assert err > 0  # if this ever becomes bit-exact the loose Philox-mode tolerances can go


def test_fast_sampler_consumes_exactly_the_philox_normals():
    """The fused f32 sampler (icem_sample_clip's fast path = the code of every fused kernel's sampling phase) on
    mean 0 / std 1 / wide bounds equals the oracle's synthesis of ``icem_philox_normals``'s output to 1e-5: same stream,
    same Box-Muller -- which is what lets the tests above feed the oracle the device's normals."""
    from icem_amd import IcemConfig, IcemPlanner
    for h, d, beta in ((30, 6, 0.25), (30, 17, 2.0), (12, 6, 0.25), (13, 4, 1.0)):
        n = 5000
        pl = IcemPlanner(IcemConfig(horizon=h, act_dim=d, num_traj=n, dtype="f32", seed=5, noise_beta=beta),
                         -100 * np.ones(d), 100 * np.ones(d))
        mean, std = np.zeros((h, d)), np.ones((h, d))
        got = np_(pl.sample_clip(n, mean, std, offset=11))
        z_r, z_i = pl.philox_normals(n, offset=11)
        want = O.sample_action_sequences(mean, std, -100 * np.ones(d), 100 * np.ones(d), beta, np_(z_r), np_(z_i))
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)


def test_humanoid_standup_cost_at_real_observation_width():
    """HumanoidStandup's cost_fn on its real o=378 observations (icem/environments/mujoco.py:259-277): the vector
    recorded from the reference (tests/golden/cost_fn_vectors.npz:hs) through ``icem_trajectory_cost``."""
    import os
    from golden_util import GOLDEN
    from icem_amd import IcemConfig, IcemPlanner, humanoid_standup_env
    z = np.load(os.path.join(GOLDEN, "cost_fn_vectors.npz"))
    obs, act, want = z["o378"], z["a17"], z["hs"]  # [4, 10, 378], [4, 10, 17], [4, 10]
    n, h, o = obs.shape
    env = humanoid_standup_env()
    for dtype, t in (("f64", dict(rtol=1e-12, atol=1e-12)), ("f32", dict(rtol=1e-5, atol=1e-5))):
        for mode in ("sum", "best", "final"):
            pl = IcemPlanner(IcemConfig(horizon=h, act_dim=17, num_traj=n, elites_size=2, opt_iters=1, cost_mode=mode, dtype=dtype),
                             env.action_space.low, env.action_space.high)
            pl.set_cost_spec(env.cost_spec)
            got = np_(pl.trajectory_cost(torch.as_tensor(obs, dtype=pl.dt, device=pl.device),
                                         torch.as_tensor(act, dtype=pl.dt, device=pl.device)))
            ref = {"sum": want.sum(1), "best": want.min(1), "final": want[:, -1]}[mode]
            np.testing.assert_allclose(got, ref, **t)


@pytest.mark.parametrize("o,d,h,kind,mode,n", [(378, 17, 30, 0, "sum", 300), (378, 17, 30, 1, "sum", 100), (100, 6, 12, 1, "best", 1000),
                                              (33, 4, 13, 0, "final", 77), (64, 6, 30, 1, "sum", 129), (384, 17, 30, 0, "sum", 40),
                                              (200, 3, 10, 1, "sum", 4097)])
@pytest.mark.parametrize("exact", [0, 1, 2])   # icem_set_wide_exact: fp16 planes (default) / exact f32 / bf16 planes
def test_wide_observation_rollout_matches_oracle(o, d, h, kind, mode, n, exact):
    """The model step at observation widths 33..384 as a GEMM on the matrix cores -- rollout_wide_split_kernel (default:
    every f32 operand as three bf16 planes, six products per multiply-add; k_rollout_wide_split.hip) and
    rollout_wide_kernel (icem_set_wide_exact: exact f32; k_rollout_wide.hip) -- against the float64 oracle rollout
    (predict_n_steps + trajectory_cost_fn, icem/models/abstract_models.py:17-53,
    icem/controllers/abstract_controller.py:74-91) at the SAME 1e-5; o = 378, d = 17 is HumanoidStandup's real shape
    (icem/environments/mujoco.py:241-277).  n = 300 / 129 / 4097 leave a fifth tile to a workgroup's batch."""
    from icem_amd import DeviceSyntheticModel, IcemConfig, IcemPlanner
    model = DeviceSyntheticModel.make(o, d, kind=kind)
    lo, hi = -0.4 * np.ones(d), 0.4 * np.ones(d)
    pl = IcemPlanner(IcemConfig(horizon=h, act_dim=d, num_traj=max(n, 4), elites_size=2, opt_iters=1, cost_mode=mode, dtype="f32"), lo, hi)
    pl.set_wide_exact(exact)
    pl.set_model(model.kind, model.A, model.B)
    flip_idx = 1 if kind == 0 else -1
    pl.set_cost(0.1, 2, -1.0, flip_idx, 10.0, 0.05)
    oc = O.CostSpec(0.1, 2, -1.0, flip_idx, 10.0, 0.05)
    rs = np.random.RandomState(o + n)
    obs = 0.1 * rs.randn(o)
    act = rs.uniform(-0.4, 0.4, (n, h, d)).astype(np.float32)
    got = np_(pl.rollout_cost(obs, torch.as_tensor(act, device=pl.device)))
    want = O.rollout_costs(O.SyntheticModel(model.A, model.B, model.kind), oc, obs, act.astype(np.float64), mode=mode)
    bad = np.abs(got - want) > 1e-5 * np.abs(want) + 2e-5
    # a flip indicator may land on the other side of its threshold in f32: allow a handful of whole-penalty differences
    assert bad.sum() <= (2 if flip_idx >= 0 else 0), (bad.sum(), np.abs(got - want).max())
    if bad.any():
        assert np.allclose(np.abs(got - want)[bad] % 10.0, 0.0, atol=1e-3) or np.allclose(np.abs(got - want)[bad] % 10.0, 10.0, atol=1e-3)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("scale", [1e-30, 1e-6, 1.0, 7e4, 1e9])
def test_wide_fp16_planes_follow_the_magnitudes(scale, kind):
    """The fp16 planes of rollout_wide_split_kernel hold x 2^k with k chosen per trajectory row and per step from the row's
    largest entry (and once for the model): observations far outside fp16's range (65 504) or far below its normal
    numbers cost no accuracy -- the costs stay within 1e-5 of the float64 oracle's like the exact-f32 kernel's, for the
    linear model (whose state keeps the observation's magnitude) and the tanh one, actions of ordinary size beside
    observations 10^9 times larger included.  A NaN observation entry poisons every trajectory (they all start from it),
    like the exact kernel; a model with a NaN weight likewise."""
    from icem_amd import DeviceSyntheticModel, IcemConfig, IcemPlanner
    o, d, h, n = 200, 6, 10, 129
    model = DeviceSyntheticModel.make(o, d, kind=kind)
    lo, hi = -0.4 * np.ones(d), 0.4 * np.ones(d)
    rs = np.random.RandomState(11)
    obs = scale * rs.randn(o)
    act = rs.uniform(-0.4, 0.4, (n, h, d)).astype(np.float32)
    oc = O.CostSpec(0.1, 2, -1.0, -1, 0.0, 0.0)
    want = O.rollout_costs(O.SyntheticModel(model.A, model.B, model.kind), oc, obs.astype(np.float32).astype(np.float64), act.astype(np.float64))
    got = {}
    for m in (0, 1):
        pl = IcemPlanner(IcemConfig(horizon=h, act_dim=d, num_traj=n, elites_size=2, opt_iters=1, dtype="f32"), lo, hi)
        pl.set_wide_exact(m)
        pl.set_model(model.kind, model.A, model.B)
        pl.set_cost(0.1, 2, -1.0, -1, 0.0, 0.0)
        got[m] = np_(pl.rollout_cost(obs, torch.as_tensor(act, device=pl.device))).astype(np.float64)
        assert np.all(np.isfinite(got[m])), m
        # the linear term reads one state entry: the bar is relative to the state's magnitude, not to a cancelling sum
        tol = 1e-5 * np.abs(want) + 2e-5 * max(1.0, float(np.abs(obs).max()) if kind == 0 else 1.0)
        assert np.all(np.abs(got[m] - want) <= tol), (m, np.abs(got[m] - want).max(), np.abs(want).max())
    bad_obs = obs.copy()
    bad_obs[5] = np.nan
    assert np.all(np.isnan(np_(pl.rollout_cost(bad_obs, torch.as_tensor(act, device=pl.device)))))   # (exact kernel)
    pl.set_wide_exact(0)
    assert np.all(np.isnan(np_(pl.rollout_cost(bad_obs, torch.as_tensor(act, device=pl.device)))))


@pytest.mark.parametrize("mode", [0, 2])   # fp16 planes / bf16 planes
def test_wide_split_planes_in_mixed_units(mode):
    """The same linear dynamics in other units: x' = x D with D = diag(10^-4 .. 10^6) turns (A, B) into (D^-1 A D, B D) --
    observation entries a million times larger than their neighbours, multiplied by weights a million times smaller.  The
    fp16 planes carry entry k as x_k 2^e_k and the model's row k as M[k][:] 2^-e_k (pack_wide_model_split: the rows
    equilibrated), so a trajectory row's scale follows its largest CONTRIBUTION and the small entries keep their bits: costs
    within 1e-5 of the float64 oracle on the transformed problem, like the bf16 planes (exact operands) and the exact-f32
    kernel.  Three observation entries the model ignores (zero rows of A) hold 1e9: they take no part."""
    from icem_amd import IcemConfig, IcemPlanner, DeviceSyntheticModel
    o, d, h, n = 120, 5, 12, 96
    base = DeviceSyntheticModel.make(o, d, kind=0)
    rs = np.random.RandomState(5)
    D = 10.0 ** rs.uniform(-4, 6, o)
    D[2] = 1.0   # (the cost's linear term reads entry 2: keep its unit)
    A = np.asarray(base.A, np.float64).reshape(o, o) / D[:, None] * D[None, :]
    B = np.asarray(base.B, np.float64).reshape(d, o) * D[None, :]
    ignored = [7, 50, 99]
    A[ignored, :] = 0.0
    obs = 0.3 * rs.randn(o) * D
    obs[ignored] = 1e9
    act = rs.uniform(-0.4, 0.4, (n, h, d)).astype(np.float32)
    oc = O.CostSpec(0.1, 2, -1.0, -1, 0.0, 0.0)
    want = O.rollout_costs(O.SyntheticModel(A, B, 0), oc, obs.astype(np.float32).astype(np.float64), act.astype(np.float64))
    lo, hi = -0.4 * np.ones(d), 0.4 * np.ones(d)
    pl = IcemPlanner(IcemConfig(horizon=h, act_dim=d, num_traj=n, elites_size=2, opt_iters=1, dtype="f32"), lo, hi)
    pl.set_wide_exact(mode)
    pl.set_model(0, A, B)
    pl.set_cost(0.1, 2, -1.0, -1, 0.0, 0.0)
    got = np_(pl.rollout_cost(obs, torch.as_tensor(act, device=pl.device))).astype(np.float64)
    assert np.all(np.isfinite(got))
    assert np.all(np.abs(got - want) <= 1e-5 * np.abs(want) + 2e-5), (np.abs(got - want).max(), np.abs(want).max())


def test_wide_auto_picks_the_arithmetic_from_the_balanced_model():
    """icem_set_wide_arith's default (ICEM_WIDE_AUTO): the fp16 planes for a model one sweep of balancing brings within
    2^13 of its largest weight -- the benchmark's 0.95 I + 0.05 N / sqrt(o), a dense Gaussian model -- and the bf16
    planes (exact operands) for one it does not: a 10 x 10 block of A whose rows are 2^20 weaker outside the block, which no
    diagonal scaling takes out.  The named modes override it; the ABI <= 3 spelling still works; costs stay within 1e-5 of the
    float64 oracle in whatever AUTO picked, on a state that exercises the small weights."""
    from icem_amd import IcemConfig, IcemPlanner, DeviceSyntheticModel
    o, d, h, n = 120, 5, 12, 96
    base = DeviceSyntheticModel.make(o, d, kind=0)
    A0 = np.asarray(base.A, np.float64).reshape(o, o)
    B0 = np.asarray(base.B, np.float64).reshape(d, o)
    rs = np.random.RandomState(9)
    lo, hi = -0.4 * np.ones(d), 0.4 * np.ones(d)

    def planner(A, B):
        pl = IcemPlanner(IcemConfig(horizon=h, act_dim=d, num_traj=n, elites_size=2, opt_iters=1, dtype="f32"), lo, hi)
        pl.set_model(0, A, B)
        pl.set_cost(0.1, 2, -1.0, -1, 0.0, 0.0)
        return pl
    pl = planner(A0, B0)
    assert pl.wide_arith == "f16x2" and pl.wide_imbalance_log2 <= 13, (pl.wide_arith, pl.wide_imbalance_log2)
    pl = planner(rs.randn(o, o) / np.sqrt(o), B0)   # a dense Gaussian model: incidental small entries do not count
    assert pl.wide_arith == "f16x2" and pl.wide_imbalance_log2 <= 13, (pl.wide_arith, pl.wide_imbalance_log2)
    # (the same dynamics in units ten decades apart measure 14-16 after the ONE sweep the pack does: AUTO is conservative
    #  there and takes the bf16 planes; test_wide_split_planes_in_mixed_units holds both plane forms to 1e-5 on that model)
    A = A0.copy()
    A[10:20, :10] *= 2.0 ** -20    # ten state entries whose weights outside their own block sit 2^20 below those inside it
    A[10:20, 20:] *= 2.0 ** -20
    pl = planner(A, B0)
    assert pl.wide_imbalance_log2 > 13 and pl.wide_arith == "bf16x3", (pl.wide_arith, pl.wide_imbalance_log2)
    obs = 0.3 * rs.randn(o)
    obs[10:20] *= 2.0 ** 10    # ... and carry large values: the small weights' contributions are of ordinary size
    act = rs.uniform(-0.4, 0.4, (n, h, d)).astype(np.float32)
    oc = O.CostSpec(0.1, 2, -1.0, -1, 0.0, 0.0)
    want = O.rollout_costs(O.SyntheticModel(A, B0, 0), oc, obs.astype(np.float32).astype(np.float64), act.astype(np.float64))
    got = np_(pl.rollout_cost(obs, torch.as_tensor(act, device=pl.device))).astype(np.float64)
    assert np.all(np.isfinite(got))
    assert np.all(np.abs(got - want) <= 1e-5 * np.abs(want) + 2e-5), (np.abs(got - want).max(), np.abs(want).max())
    for name in ("f16x2", "f32", "bf16x3"):
        assert pl.set_wide_arith(name) == name
    pl.set_wide_exact(0)
    assert pl.wide_arith == "f16x2"
    assert pl.set_wide_arith("auto") == "bf16x3"
    with pytest.raises(Exception, match="INVALID|wide arithmetic"):
        pl.set_wide_arith(3)


@pytest.mark.soak
@pytest.mark.parametrize("N", [4096, 16384])
def test_soak_elite_sets_against_float64_oracle(N):
    """Randomised soak (was tools/dbg/soak_oracle.py at N=1000): over many seeds, how often does the f32 device loop
    pick a different elite set than the float64 oracle fed the same (device) normals?  Must be never."""
    import os
    seeds = int(os.environ.get("ICEM_SOAK_SEEDS", "12"))
    h, d, o, iters = 30, 6, 17, 3
    bad = []
    for seed in range(seeds):
        env, model, oc, mk = _make(N, iters, h, d, o, 1, 0.25, 1000 + seed, "halfcheetah")
        om = O.SyntheticModel(model.A, model.B, model.kind)
        pl, rng = mk(), mk()
        noise = DeviceNormals(rng, iters)
        orc = O.IcemOracle(O.IcemParams(horizon=h, num_simulated_trajectories=N, opt_iterations=iters),
                           env.action_space.low.astype(np.float64), env.action_space.high.astype(np.float64),
                           lambda ob, ac: O.rollout_costs(om, oc, ob, ac), noise)
        orc.beginning_of_rollout()
        for s in range(2):
            ob = 0.1 * np.random.RandomState(1000 + seed * 7 + s).randn(o)
            if s:
                noise.begin_step()
            a = np_(pl.plan_step(ob))
            w = orc.get_action(ob)
            if not (np.allclose(a, w, rtol=RTOL, atol=ATOL) and np.allclose(np_(pl.mean), orc.mean, rtol=RTOL, atol=ATOL)):
                bad.append((seed, s))
                break
    assert not bad, f"{len(bad)} of {seeds} seeds leave 1e-5: {bad}"
