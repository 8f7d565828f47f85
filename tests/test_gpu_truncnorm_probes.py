"""The truncated-normal sampler of the CEM baseline on the GPU against truncnorm_cases.py: ``sample_truncnorm`` (sample_truncnorm_kernel)
on planted uniforms and on its own stream, ``cem_bounds`` (cem_bounds_kernel), and the samplers of the fused steps --
cem_sample_kernel (``plan_step_cem``), cem_sample_batch_kernel (``plan_step_cem_batch``) and cem_sample_gather_batch_kernel
(``plan_step_cem_learned_batch``) -- each held to the two-sided float64 quantile on the device's own inputs, per entry, at the
criterion of the case file (f64: 1e-10 in z; f32: 2e-6 in z), and to the operator bit for bit where two kernels share the text.

With the one-sided quantile of the commit before this file (z = Phi^-1(pa + u pd) alone) 57 of these 233 failed on the MI355X
(35 planted, 16 device-stream, 4 fused, 2 batched: the f32 upper-tail cases, and in f64 the planted 1 - 2^-53); EXPERIMENTS R17.1."""
import numpy as np
import pytest
import torch

import truncnorm_cases as TC
from oracle import icem_oracle as O   # checker only

pytestmark = pytest.mark.gpu

WG, LDS_MAX = 256, 64 * 1024
_planners = {}


def np_(t):
    return t.detach().cpu().numpy()


def planner(h, d, n, name, rounds=10, seed=TC.SEED, model=None, K=2, cached=True):
    """A planner on the case file's action box; ``model``: (o, kind) of a built-in model, for the fused step."""
    from icem_amd import DeviceSyntheticModel, IcemConfig, IcemPlanner
    key = (h, d, n, name, rounds, seed, model, K)
    if cached and key in _planners:
        return _planners[key]
    low, high = TC.box(d, np.float64)
    cfg = IcemConfig(horizon=h, act_dim=d, num_traj=n, elites_size=K, opt_iters=1, cost_mode="sum", use_mean_actions=False,
                     keep_previous_elites=False, shift_elites=False, factor_decrease=1.0, alpha=0.1, init_std=0.5, dtype=name,
                     rng_rounds=rounds, seed=seed)
    pl = IcemPlanner(cfg, low, high)
    if model is not None:
        o, kind = model
        m = DeviceSyntheticModel.make(o, d, kind=kind, seed_a=11, seed_b=12)
        pl.set_model(m.kind, m.A, m.B)
        pl.set_cost(0.1, o - 1, -1.0, min(1, o - 1), 10.0, 0.3)
    pl.new_episode()
    if cached:
        _planners[key] = pl
    return pl


def dev(pl, x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=pl.dt, device=pl.device)


def device_inputs(pl, case, dtype, check_bounds=True):
    """The case's distribution on the device, its bounds made by ``cem_bounds`` (and held to their own criterion) unless the
    case gives them -> tensors (mean, std, lower, upper) and the same as arrays of the planner dtype."""
    low, high, mean, std = TC.distribution(case, dtype)
    assert np.array_equal(np_(pl.low), low) and np.array_equal(np_(pl.high), high)
    mean_t, std_t = dev(pl, mean), dev(pl, std)
    if case.bounds == "direct":
        lower, upper = TC.direct_bounds(case, dtype)
        lower_t, upper_t = dev(pl, lower), dev(pl, upper)
    else:
        lev = case.bounds == "levine"
        lower_t, upper_t = pl.cem_bounds(mean_t, std_t, lev)
        if check_bounds:
            f = TC.bounds_miss(np_(std_t), np_(lower_t), np_(upper_t), mean, std, low, high, lev, dtype)
            print(f"{case.name} {dtype.__name__}: bounds miss {f:.3g}")
            assert f <= 1.0, f
    return (mean_t, std_t, lower_t, upper_t), tuple(np_(t) for t in (mean_t, std_t, lower_t, upper_t))


def held(tag, a_dev, arrays, u, dtype):
    f, dz = TC.miss(a_dev, *arrays, u, dtype), TC.accuracy(a_dev, *arrays, u, dtype)
    print(f"{tag} {dtype.__name__}: miss {f:.4g}  worst (|a - a_ref| - eps |a_ref|) / std {dz:.4g}")
    assert f <= 1.0, (tag, f, dz)


# ---- 1. the operators ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TC.DTYPES)
@pytest.mark.parametrize("case", TC.CASES, ids=lambda c: c.name)
def test_planted_uniforms_and_bounds(case, name):
    """cem_bounds within its bound, then sample_truncnorm(u = planted) within the criterion, on the bounds the device made."""
    dtype = TC.DTYPES[name]
    pl = planner(case.h, case.d, case.n, name)
    tensors, arrays = device_inputs(pl, case, dtype)
    u = TC.uniforms(case, dtype)
    a = pl.sample_truncnorm(case.n, *tensors, dev(pl, u))
    held(f"{case.name} planted", np_(a), arrays, u, dtype)
    zero = arrays[1] == 0
    assert np.array_equal(np_(a)[:, zero], np.broadcast_to(arrays[0][zero], (case.n, zero.sum())))   # std == 0: the mean


@pytest.mark.parametrize("name", TC.DTYPES)
@pytest.mark.parametrize("case", TC.CASES, ids=lambda c: c.name)
def test_the_device_stream_is_the_oracles_and_meets_the_criterion(case, name):
    """sample_truncnorm(u = None) is sample_truncnorm(u = oracle.philox_uniforms) bit for bit at rng_rounds 7 and 10 and a
    stream offset with both words set -- the oracle's uniforms ARE the device's --, and is within the criterion on them."""
    dtype = TC.DTYPES[name]
    offset = (3 << 32) + 5
    for rounds in (7, 10):
        pl = planner(case.h, case.d, case.n, name, rounds)
        tensors, arrays = device_inputs(pl, case, dtype, check_bounds=False)
        u = TC.stream(case, dtype, rounds, offset)
        own = np_(pl.sample_truncnorm(case.n, *tensors, None, offset=offset))
        given = np_(pl.sample_truncnorm(case.n, *tensors, dev(pl, u)))
        assert np.array_equal(own, given), rounds
        held(f"{case.name} stream r{rounds}", own, arrays, u, dtype)


# ---- 2. the fused samplers ----------------------------------------------------------------------------------------------------
def tpw(h, d, dtype):
    """cem_sample_tpw (k_cem.hip): rows per workgroup, -> (tpw, the LDS bound sets it)."""
    row = h * d * np.dtype(dtype).itemsize
    by_lds = LDS_MAX // row - 3
    return min(WG // d, by_lds), by_lds < WG // d


# (h, d, o, kind) of the fused steps: the case table's shapes that the built-in rollouts take
FUSED = [(13, 3, 24, 1), (30, 6, 17, 0), (12, 17, 8, 1), (40, 6, 16, 0)]


def fused_case(h, d, dist, dtype):
    rows, _ = tpw(h, d, dtype)
    n = 2 * rows + 3   # three workgroups, the last with three rows
    return TC.Case(f"{h}x{d}x{n}-{dist}-plain", h, d, n, dist, "plain")


def solo_step(pl, case, dtype):
    """plan_step_cem (one iteration) on copies of the case's tensors -> (the step's pool, the operator's draw at the step's
    offset, the arrays the draw read)."""
    assert pl.cem_step_ok()
    tensors, arrays = device_inputs(pl, case, dtype, check_bounds=False)
    want = np_(pl.sample_truncnorm(case.n, *tensors, None, offset=pl.noise_offset(pl.mpc_step * pl.cfg.opt_iters)))
    mine = [t.clone() for t in tensors]
    obs = 0.1 * np.random.RandomState(100).randn(pl.obs_dim)
    pl.plan_step_cem(obs, *mine, like_levine=False, shift_means=True, execute_best_elite=True)
    torch.cuda.synchronize()
    assert pl.cem_step_launches == 3
    return np_(pl.cem_actions).copy(), want, arrays


@pytest.mark.parametrize("name", TC.DTYPES)
@pytest.mark.parametrize("h,d,o,kind", FUSED)
def test_the_fused_sampler_on_the_edge_distributions(h, d, o, kind, name):
    """cem_sample_kernel: the pool of a one-iteration plan_step_cem is the operator's draw at noise_offset bit for bit and meets
    the criterion; N = 2 tpw + 3, and in f64 at 40 x 6 it is the LDS bound that sets tpw."""
    dtype = TC.DTYPES[name]
    rows, by_lds = tpw(h, d, dtype)
    assert by_lds == ((h, d, name) == (40, 6, "f64"))
    for dist in TC.EDGE_DISTS:
        case = fused_case(h, d, dist, dtype)
        assert case.n % rows != 0
        pl = planner(h, d, case.n, name, model=(o, kind), cached=False)
        got, want, arrays = solo_step(pl, case, dtype)
        assert np.array_equal(got, want), dist
        held(f"{case.name} fused", got, arrays, TC.stream(case, dtype), dtype)


@pytest.mark.parametrize("name", TC.DTYPES)
@pytest.mark.parametrize("h,d,o,kind,dists", [(30, 6, 17, 0, ("bound", "zero", "wide")), (13, 3, 24, 1, ("ulp", "bound", "zero"))])
def test_a_batch_of_three_edge_distributions_equals_its_solo_twins(h, d, o, kind, dists, name):
    """cem_sample_batch_kernel: B = 3, a different edge distribution and seed per problem; every problem's pool is its solo
    twin's bit for bit, and within the criterion."""
    from icem_amd import IcemPlanner
    dtype = TC.DTYPES[name]
    cases = [fused_case(h, d, dist, dtype) for dist in dists]
    n = cases[0].n
    batch = [planner(h, d, n, name, seed=TC.SEED + i, model=(o, kind), cached=False) for i in range(3)]
    twins = [planner(h, d, n, name, seed=TC.SEED + i, model=(o, kind), cached=False) for i in range(3)]
    ins = [device_inputs(pl, case, dtype, check_bounds=False) for pl, case in zip(batch, cases)]
    obs = [0.1 * np.random.RandomState(100).randn(o) for _ in range(3)]
    IcemPlanner.plan_step_cem_batch(batch, obs, [tuple(t.clone() for t in tensors) for tensors, _ in ins], like_levine=False,
                                    shift_means=True, execute_best_elite=True)
    torch.cuda.synchronize()
    for i, (pb, pt, case) in enumerate(zip(batch, twins, cases)):
        got, want, arrays = solo_step(pt, case, dtype)
        assert np.array_equal(np_(pb.cem_actions), got) and np.array_equal(got, want), (i, case.name)
        held(f"{case.name} batch problem {i}", np_(pb.cem_actions), arrays, TC.stream(case, dtype, seed=TC.SEED + i), dtype)


def test_the_gathering_sampler_of_the_learned_batch():
    """cem_sample_gather_batch_kernel: plan_step_cem_learned_batch at the smallest population it admits (N = 16, h = 12, K = 2,
    one iteration), B = 2 on two edge distributions.  The batch's pool is scratch; the elite set is not: it equals the solo
    twin's bit for bit, and row k of it -- row elite_idx[k] of the draw -- meets the criterion."""
    from icem_amd import DeviceRSSMModel, IcemPlanner
    dtype, h, d, n = np.float32, 12, 6, 16
    model = DeviceRSSMModel(seed=3)
    cases = [TC.Case(f"{h}x{d}x{n}-{dist}-plain", h, d, n, dist, "plain") for dist in ("bound", "ulp")]
    batch = [planner(h, d, n, "f32", seed=TC.SEED + i, cached=False) for i in range(2)]
    twins = [planner(h, d, n, "f32", seed=TC.SEED + i, cached=False) for i in range(2)]
    assert all(pl.cem_learned_step_ok() for pl in batch)
    ins = [device_inputs(pl, case, dtype, check_bounds=False) for pl, case in zip(batch, cases)]
    obs = np.stack([(0.3 * np.random.RandomState(1000 * i).randn(230)).astype(np.float32) for i in range(2)])
    flags = dict(like_levine=False, shift_means=True, execute_best_elite=True)
    IcemPlanner.plan_step_cem_learned_batch(batch, model, obs, [tuple(t.clone() for t in tensors) for tensors, _ in ins], **flags)
    torch.cuda.synchronize()
    for i, (pb, pt, case) in enumerate(zip(batch, twins, cases)):
        tensors, arrays = device_inputs(pt, case, dtype, check_bounds=False)
        pt.plan_step_cem_learned(model, obs[i], *[t.clone() for t in tensors], **flags)
        torch.cuda.synchronize()
        idx, elites = np_(pb.cem_elite_idx), np_(pb.cem_elites)
        assert np.array_equal(idx, np_(pt.cem_elite_idx)) and np.array_equal(elites, np_(pt.cem_elites)), i
        assert np.array_equal(elites, np_(pt.cem_actions)[idx])
        u = TC.stream(case, dtype, seed=TC.SEED + i)
        held(f"{case.name} learned batch problem {i}", elites, arrays, u[idx], dtype)
        held(f"{case.name} learned solo problem {i}", np_(pt.cem_actions), arrays, u, dtype)
