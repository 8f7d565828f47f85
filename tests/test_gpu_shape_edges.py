"""Oracle parity at every shape edge the C ABI accepts (horizon 2..64, act_dim 1..64, num_elites 1..64, obs_dim 1..384),
on both sides of every internal threshold that switches a kernel, a table size or a code path.

Each row of CASES names the threshold it sits on and where it lives.  Every case does two things:

(a) ``rollout_cost`` against ``oracle.rollout_costs`` on 257 random action rows (a ragged last tile): f64 within 1e-10 of
    each cost's magnitude, f32 within 1e-5 of it (trajectories whose float64 state sits within the f32 error of a
    threshold may differ by whole penalties, and are counted: tests/oracle_loop.py);
(b) two MPC steps of two iterations through the whole planner: f32 against the float64 oracle fed the device's normals
    (tests/oracle_loop.py: full_loop), f64 against the oracle restating the device's Philox stream at 1e-9.

The route witness: ``icem_wide_arith`` (0 on the tile route, 1 on the exact-f32 GEMM route -- narrow models -- or the
arithmetic in effect at o > 32), ``icem_tile_arith``, and the kernel categories ``profile_read`` saw.
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from oracle import icem_oracle as O
from oracle_loop import ATOL, RTOL, DeviceNormals, check_costs, full_loop, near_threshold, np_, penalty_quanta, record, strict_loop

pytestmark = pytest.mark.gpu

N_ROWS = 257   # (a): 16 whole tiles and one row


def _case(cid, h, d, o, *, K=10, N=300, dtype="f32", kind=0, mode="sum", ks=True, cost=None, wide=None, expect=None,
          beta=0.25, iters=2):
    """cost: None (a flip and a linear term on separate entries), or a dict of CostSpec fields.  wide: the wide arithmetic
    asked for (icem_set_wide_arith name).  expect: the raw icem_wide_arith the route must report (None: not checked)."""
    return pytest.param(dict(h=h, d=d, o=o, K=K, N=N, dtype=dtype, kind=kind, mode=mode, ks=ks, cost=cost, wide=wide,
                             expect=expect, beta=beta, iters=iters), id=cid)


GEMM, TILE = 1, 0   # icem_wide_arith on a narrow model: the exact-f32 GEMM kernel / the tile kernels (abi.hip:385-393)
CASES = []
# ---- horizon: the ABI's limits h = 2 / 64 (abi.hip:206), the synthesis table's HMAX = 32 / 64 switch at h = 32 / 33
#      (abi.hip:221), h = 10: a fast-sampler horizon with no compiled rollout (fused_dev.h:26) -> fast sampler + GEMM
for _h in (2, 3, 10, 31, 32, 33, 63, 64):
    for _dt in ("f32", "f64"):
        CASES.append(_case(f"h{_h}_{_dt}", _h, 3, 8, dtype=_dt, kind=_h % 2, mode=("sum", "best", "final")[_h % 3],
                           ks=_h % 4 != 3, expect=GEMM if _dt == "f32" else None))
# ---- act_dim: the ABI's limits d = 1 / 64 (abi.hip:207); 8 / 9, 16 / 17, 32 / 33: the GEMM kernel's 4-row contraction
#      blocks of [obs | act] (k_rollout_wide.hip:282) and the f64 rollout's action registers; narrow GEMM route and the f64
#      generic route
for _d in (1, 8, 9, 16, 17, 32, 33, 64):
    for _dt in ("f32", "f64"):
        CASES.append(_case(f"d{_d}_{_dt}", 12, _d, 12, dtype=_dt, kind=_d % 2, mode=("sum", "final", "best")[_d % 3],
                           ks=_d % 3 != 2, N=200, expect=GEMM if _dt == "f32" else None))
# ---- o = 384 at the split kernel's LDS fit o + d <= 416 (k_rollout_wide_split.hip:555, abi.hip:390): d = 32 on the fp16
#      planes, d = 33 and 64 fall back to exact f32 whatever is asked
CASES += [
    _case("o384_d32_split", 8, 32, 384, N=64, kind=1, wide="auto", expect=0),
    _case("o384_d33_exact_fallback", 8, 33, 384, N=64, kind=0, wide="auto", expect=1, mode="best"),
    _case("o384_d64_exact_fallback", 8, 64, 384, N=64, kind=1, wide="bf16x3", expect=1, ks=False),
]
# ---- obs_dim
CASES += [
    # o = 1: the one entry is both the linear and the flip entry (lin_idx == flip_idx)
    _case("o1_f32", 12, 2, 1, cost=dict(lin_idx=0, flip_idx=0), expect=GEMM),
    _case("o1_f64", 12, 2, 1, dtype="f64", cost=dict(lin_idx=0, flip_idx=0), kind=1),
]
for _o in (7, 8, 9):   # pick_O's first padded width 8 (abi.hip:127): 7 pads, 8 does not, 9 pads to 16
    for _dt in ("f32", "f64"):
        CASES.append(_case(f"o{_o}_{_dt}", 12, 3, _o, dtype=_dt, kind=_o % 2, expect=GEMM if _dt == "f32" else None))
# (30, 17, O = 24): o = 19..23 pad to the two-tile Tile16 (plan.hip::ensure_fast_model) -- the tile route, padding columns included
for _o in (19, 20, 21, 22, 23, 24):
    CASES.append(_case(f"o{_o}_d17_tile", 30, 17, _o, N=256, kind=1, beta=2.0, expect=TILE,
                       cost=dict(lin_idx=_o - 1, flip_idx=2, flip_thresh=0.5)))
for _o in (31, 32):   # the widest narrow model (O = 32) ...
    for _dt in ("f32", "f64"):
        CASES.append(_case(f"o{_o}_{_dt}", 12, 4, _o, dtype=_dt, kind=1, expect=GEMM if _dt == "f32" else None))
CASES.append(_case("o33_wide", 12, 4, 33, kind=1, expect=0))   # ... and the narrowest wide one (abi.hip:459)
# the GEMM tile-count buckets wide_nt = 4 / 8 / 16 / 24 column tiles at o = 64/65, 128/129, 256/257, 383/384
# (k_rollout_wide.hip:284, wide_split_nct k_rollout_wide_split.hip:556), in each wide arithmetic
for _o in (64, 65, 128, 129, 256, 257, 383, 384):
    for _w, _e in (("f16x2", 0), ("bf16x3", 2), ("f32", 1)):
        CASES.append(_case(f"o{_o}_{_w}", 8, 4, _o, N=64, kind=_o % 2, wide=_w, expect=_e,
                           mode=("sum", "best", "final")[_o % 3], ks=_o % 2 == 0))
# ---- num_elites: K = 1 clamps to 2 (planner.py:48), K + 1 <= 12 the folded merge (k_sample.hip:305), 16 / 17 the
#      register-gathered elites, 32 / 33 the GEMM and tile kernels' candidate lists (k_rollout.hip:47, k_rollout_wide.hip:276:
#      beyond them the generic f32 kernels), 64 the ABI's limit (abi.hip:208); N = 2K and 2K + 1 (icem.py:127's floor)
for _K in (1, 11, 12, 16, 17, 31, 32, 33, 64):
    for _dt in ("f32", "f64"):
        CASES.append(_case(f"K{_K}_{_dt}", 12, 3, 8, K=_K, N=max(4, 2 * _K) + (_K % 2), dtype=_dt, kind=_K % 2,
                           expect=(GEMM if _K <= 32 else None) if _dt == "f32" else None))
CASES += [_case("K16_N33_f32", 12, 3, 8, K=16, N=33, expect=GEMM), _case("K17_N34_f32", 12, 3, 8, K=17, N=34, expect=GEMM),
          _case("K33_N67_f32", 12, 3, 8, K=33, N=67, mode="best"), _case("K64_N129_f64", 12, 3, 8, K=64, N=129, dtype="f64")]
for _K in (11, 12, 16, 17, 32, 33):   # ... and on the compiled tile shape (30, 6, 17)
    CASES.append(_case(f"K{_K}_tile_30_6_17", 30, 6, 17, K=_K, N=4 * _K + 1, kind=1, expect=TILE if _K <= 32 else None,
                       cost=dict(flip_thresh=1.2)))
# ---- cost spec on a compiled shape (30, 6, 17): the tile's static cost columns (plan.hip::ensure_fast_model)
CASES += [
    _case("cost_flip_eq_lin_tile", 30, 6, 17, N=512, expect=TILE, cost=dict(lin_idx=3, flip_idx=3, flip_thresh=0.4)),
    _case("cost_flip_eq_lin_tile_f64", 30, 6, 17, N=300, dtype="f64", cost=dict(lin_idx=3, flip_idx=3, flip_thresh=0.4)),
    _case("cost_no_flip_tile", 30, 6, 17, N=512, kind=1, mode="best", expect=TILE, cost=dict(flip_idx=-1)),
    _case("cost_negative_thresh_tile", 30, 6, 17, N=512, mode="final", ks=False, expect=TILE, cost=dict(flip_thresh=-0.3)),
    _case("cost_lin_weight0_gemm", 30, 6, 17, N=512, kind=1, expect=GEMM, cost=dict(lin_weight=0.0)),   # abi.hip:305
    _case("cost_lin_weight0_gemm_12_6_17", 12, 6, 17, N=300, mode="best", expect=GEMM, cost=dict(lin_weight=0.0, flip_idx=-1)),
]


def _spec(o, cost):
    base = dict(ctrl_weight=0.1, lin_idx=o - 1, lin_weight=-1.0, flip_idx=min(1, o - 1), flip_penalty=10.0, flip_thresh=0.6)
    base.update(cost or {})
    return O.CostSpec(**base)


def _planner(c, om, spec, N, iters, low, high, seed=5):
    from icem_amd import IcemConfig, IcemPlanner
    pl = IcemPlanner(IcemConfig(horizon=c["h"], act_dim=c["d"], num_traj=N, elites_size=c["K"], opt_iters=iters,
                                dtype=c["dtype"], seed=seed, noise_beta=c["beta"], cost_mode=c["mode"],
                                keep_previous_elites=c["ks"], shift_elites=c["ks"]), low, high)
    if c["wide"] is not None:
        pl.set_wide_arith(c["wide"])
    pl.set_model(om.kind, om.A, om.B)
    pl.set_cost(spec.ctrl_weight, spec.lin_idx, spec.lin_weight, spec.flip_idx, spec.flip_penalty, spec.flip_thresh)
    pl.reset()
    return pl


def _route(pl):
    return int(pl.lib.icem_wide_arith(pl._h)), pl.tile_arith


@pytest.mark.parametrize("c", CASES)
def test_shape_edge_against_the_oracle(c, request):
    h, d, o, dtype = c["h"], c["d"], c["o"], c["dtype"]
    t0 = time.monotonic_ns()
    om = O.SyntheticModel.make(o, d, c["kind"])
    spec = _spec(o, c["cost"])
    low, high = -0.7 * np.ones(d), 0.9 * np.ones(d)
    if o > 32:
        low, high = -0.4 * np.ones(d), 0.4 * np.ones(d)
    # (a) rollout_cost on N_ROWS rows
    pa = _planner(c, om, spec, N_ROWS, 1, low, high)
    if c["expect"] is not None:
        assert _route(pa)[0] == c["expect"], (_route(pa), c)
    if c["expect"] == TILE:
        assert pa.set_tile_arith("f32") == 0   # (the exact tile: f32 operands, the oracle's bar at any population)
    rs = np.random.RandomState(h * 1000 + d * 10 + o)
    obs0 = (0.2 * rs.randn(o)).astype(np.float32).astype(np.float64)
    act = rs.uniform(low, high, (N_ROWS, h, d))
    npdt = np.float64 if dtype == "f64" else np.float32
    act = act.astype(npdt).astype(np.float64)
    pa.profile_enable(True)
    got = np_(pa.rollout_cost(obs0, torch.as_tensor(act, dtype=pa.dt, device=pa.device)))
    prof_a = sorted(pa.profile_read())
    want = O.rollout_costs(om, spec, obs0, act, mode=c["mode"])
    mag = O.rollout_cost_magnitudes(om, spec, obs0, act)
    if dtype == "f64":
        err = np.abs(got - want)
        assert np.all(err <= 1e-10 * mag), (err.max(), int(np.argmax(err / mag)))
        moved = 0
    else:
        near = near_threshold(om, spec, obs0, act)
        moved = check_costs(got, want, mag, RTOL, near, penalty_quanta(spec), "rollout_cost")
        assert moved <= max(2, N_ROWS // 50), (moved, int(near.sum()))
    # (b) two MPC steps x two iterations through the whole planner
    N, iters = c["N"], c["iters"]
    if dtype == "f64":
        pl = _planner(c, om, spec, N, iters, low, high, seed=17)
        pl.profile_enable(True)
        strict_loop(pl, om, spec, seed=17, N=N, iters=iters, h=h, o=o, beta=c["beta"], cost_mode=c["mode"], low=low,
                    high=high, elites_size=c["K"], keep=c["ks"], shift=c["ks"])
        prof_b = sorted(pl.profile_read())
        assert "sample_rollout" not in prof_b and "rollout_cost" in prof_b, prof_b   # the generic f64 kernels
        near_b = 0
    else:
        made = []

        def mk():
            pl = _planner(c, om, spec, N, iters, low, high, seed=17)
            pl.profile_enable(True)
            made.append(pl)
            return pl
        near_b = full_loop(mk, om, spec, N=N, iters=iters, h=h, o=o, beta=c["beta"], cost_mode=c["mode"], low=low, high=high,
                           elites_size=c["K"], keep=c["ks"], shift=c["ks"], obs_scale=0.2, allow_near=True,
                           max_near=max(2, N // 50))
        prof_b = sorted(made[1].profile_read())
        if c["expect"] is not None:
            assert _route(made[0])[0] == c["expect"], (_route(made[0]), c)
    torch.cuda.synchronize()
    # (the monotonic-clock window of the case: a kernel trace of the module lines up with it)
    record(dict(case=request.node.callspec.id, shape=f"h{h} d{d} o{o} K{c['K']} N{N} {dtype}", route=_route(pa),
                rollout_kernels=prof_a, plan_kernels=prof_b, near_threshold_differing=[moved, near_b],
                window_ns=[t0, time.monotonic_ns()]))


# ---------------------------------------------------------------------------------------------- samplers
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("h,d,n", [
    (2, 3, 500), (33, 3, 500), (64, 3, 500),     # four lanes per row: N d <= 262144 (generic_kernels.hip:1278); HMAX 32 / 64
    (33, 1, 300000), (64, 1, 300000),            # one lane per row: N d > 262144, d = 1
    (33, 64, 4200), (64, 64, 4200), (2, 64, 4200),   # one lane per row at the largest d
    (64, 64, 4096),                              # four lanes at N d = 262144 exactly
])
def test_generic_sampler_consumes_exactly_the_philox_normals(h, d, n, dtype):
    """The generic sampler (icem_sample_clip off the fast horizons) on mean 0 / std 1 / wide bounds equals the oracle's
    synthesis of ``icem_philox_normals``'s output: same stream, same transform, in both of its forms -- which is what lets the
    loops above feed the oracle the device's normals at these horizons.  f64 to 1e-12, f32 to 1e-5."""
    from icem_amd import IcemConfig, IcemPlanner
    beta = 1.0
    pl = IcemPlanner(IcemConfig(horizon=h, act_dim=d, num_traj=n, dtype=dtype, seed=5, noise_beta=beta),
                     -100 * np.ones(d), 100 * np.ones(d))
    mean, std = np.zeros((h, d)), np.ones((h, d))
    got = np_(pl.sample_clip(n, mean, std, offset=11))
    z_r, z_i = pl.philox_normals(n, offset=11)
    want = O.sample_action_sequences(mean, std, -100 * np.ones(d), 100 * np.ones(d), beta, np_(z_r), np_(z_i))
    tol = dict(rtol=1e-12, atol=1e-13) if dtype == "f64" else dict(rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got, want, **tol)
    if dtype == "f64":   # ... and the normals are the oracle's Philox restatement
        w_r, w_i = O.philox_white_noise(5, 11, n, d, h, dtype=np.float64)
        np.testing.assert_allclose(np_(z_r), w_r, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(np_(z_i), w_i, rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------------------------------------- refusals
def _c_config(**kw):
    from icem_amd import IcemConfig
    base = dict(horizon=12, act_dim=3, num_traj=64, dtype="f32", seed=3)
    cfg = IcemConfig(**base).to_c()
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


@pytest.mark.parametrize("field,value", [("horizon", 1), ("horizon", 65), ("act_dim", 0), ("act_dim", 65),
                                         ("num_elites", 0), ("num_elites", 65)])
def test_create_refuses_one_step_past_each_edge(field, value):
    """icem_create one step past the ABI's limits (abi.hip:206-208): ICEM_E_UNSUPPORTED, no handle."""
    from icem_amd import _lib as L
    lib = L.load_library()
    h = C.c_void_p()
    assert lib.icem_create(C.byref(_c_config(**{field: value})), C.byref(h)) == L.ICEM_E_UNSUPPORTED
    assert not h.value
    ok = C.c_void_p()   # ... and at the edge itself it is accepted
    edge = {("horizon", 1): 2, ("horizon", 65): 64, ("act_dim", 0): 1, ("act_dim", 65): 64, ("num_elites", 0): 1,
            ("num_elites", 65): 64}[(field, value)]
    assert lib.icem_create(C.byref(_c_config(**{field: edge})), C.byref(ok)) == 0 and ok.value
    lib.icem_destroy(ok)


def _plan_twice(pl, o, seed=1):
    out = []
    for s in range(2):
        obs = 0.2 * np.random.RandomState(seed + s).randn(o)
        out.append(np_(pl.plan_step(obs)).copy())
    return out + [np_(pl.mean), np_(pl.std)]


REFUSALS = [(dt, K, bad, good) for dt, K, bad in (("f32", 10, 0), ("f32", 10, 385), ("f64", 10, 33), ("f32", 33, 33),
                                                   ("f32", 33, 378))
            for good in (17, 12, 378) if not (good > 32 and (dt == "f64" or K > 32))]


@pytest.mark.parametrize("dtype,K,o_bad,o_good", REFUSALS, ids=[f"{dt}_K{K}_o{b}_after_o{g}" for dt, K, b, g in REFUSALS])
def test_set_model_refusals_leave_the_handle_planning(dtype, K, o_bad, o_good):
    """icem_set_model one step past the widths a configuration serves -- o = 0 and 385 (abi.hip:461, :481), f64 with o = 33,
    o > 32 with K = 33 (abi.hip:461-463) -- returns ICEM_E_UNSUPPORTED with nothing launched, and the handle plans afterwards
    exactly like one that never saw the call (bit for bit), whatever model it held: the tile shape, a narrow GEMM one, or a
    wide one."""
    from icem_amd import IcemConfig, IcemPlanner, _lib as L
    h, d = (30, 6) if o_good == 17 else (12, 6)
    om = O.SyntheticModel.make(o_good, d, 1)
    spec = _spec(o_good, None)

    def mk():
        pl = IcemPlanner(IcemConfig(horizon=h, act_dim=d, num_traj=256, elites_size=K, opt_iters=2, dtype=dtype, seed=4),
                         -np.ones(d), np.ones(d))
        pl.set_model(om.kind, om.A, om.B)
        pl.set_cost(spec.ctrl_weight, spec.lin_idx, spec.lin_weight, spec.flip_idx, spec.flip_penalty, spec.flip_thresh)
        return pl
    pl, fresh = mk(), mk()
    route = _route(pl)
    pl.profile_enable(True)
    bad = max(o_bad, 1)
    A, B = np.eye(bad), np.zeros((d, bad))
    rc = pl.lib.icem_set_model(pl._h, 0, o_bad, A.ctypes.data_as(C.POINTER(C.c_double)), B.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == L.ICEM_E_UNSUPPORTED
    assert pl.profile_read() == {}                            # nothing launched
    pl.set_cost(spec.ctrl_weight, spec.lin_idx, spec.lin_weight, spec.flip_idx, spec.flip_penalty, spec.flip_thresh)
    assert _route(pl) == route                                # the route the handle's own model had
    pl.reset()
    fresh.reset()
    rs = np.random.RandomState(0)
    obs0 = 0.2 * rs.randn(o_good)
    act = torch.as_tensor(rs.uniform(-1, 1, (N_ROWS, h, d)), dtype=pl.dt, device=pl.device)
    assert torch.equal(pl.rollout_cost(obs0, act), fresh.rollout_cost(obs0, act))
    for x, y in zip(_plan_twice(pl, o_good), _plan_twice(fresh, o_good)):
        assert np.array_equal(x, y)


# ---------------------------------------------------------------------------------------------- reconfiguration
def test_reconfigured_handle_equals_a_fresh_one():
    """The packed model is cached and invalidated by hand (plan.hip::ensure_fast_model; abi.hip:308, 382, 394, 537): one
    handle taken through a sequence of route switches computes, after each, what a freshly built handle with the same final
    configuration computes -- rollout costs and one MPC step, bit for bit."""
    from icem_amd import IcemConfig, IcemPlanner, halfcheetah_env
    from icem_amd import envs as E
    h, d = 30, 6
    narrow = O.SyntheticModel.make(17, d, 1)
    wide = O.SyntheticModel.make(378, d, 1)
    terms_spec = E.hopper_env(healthy_z_range=(-0.05, float("inf")), healthy_state_range=(-0.45, 0.45)).cost_spec
    cheetah = halfcheetah_env(17).cost_spec
    base = dict(ctrl_weight=0.1, lin_idx=8, lin_weight=-1.0, flip_idx=1, flip_penalty=10.0, flip_thresh=0.6)

    def new_handle():
        return IcemPlanner(IcemConfig(horizon=h, act_dim=d, num_traj=512, opt_iters=2, dtype="f32", seed=8), -np.ones(d), np.ones(d))

    # each step: (what changes, the full configuration after it)
    steps = [
        ("start: tile", dict(model=narrow, cost=base, terms=None, wide="auto", tile="auto")),
        ("lin_weight = 0: GEMM", dict(model=narrow, cost=dict(base, lin_weight=0.0), terms=None, wide="auto", tile="auto")),
        ("back to the tile", dict(model=narrow, cost=base, terms=None, wide="auto", tile="auto")),
        ("cost columns moved: re-permuted packing", dict(model=narrow, cost=dict(base, lin_idx=4, flip_idx=4), terms=None,
                                                          wide="auto", tile="auto")),
        ("exact tile", dict(model=narrow, cost=dict(base, lin_idx=4, flip_idx=4), terms=None, wide="auto", tile="f32")),
        ("wide model", dict(model=wide, cost=base, terms=None, wide="auto", tile="f32")),
        ("wide exact", dict(model=wide, cost=base, terms=None, wide="f32", tile="f32")),
        ("wide bf16x3", dict(model=wide, cost=base, terms=None, wide="bf16x3", tile="f32")),
        ("narrow again", dict(model=narrow, cost=base, terms=None, wide="bf16x3", tile="auto")),
        ("terms on", dict(model=narrow, cost=base, terms=terms_spec, wide="bf16x3", tile="auto")),
        ("terms off", dict(model=narrow, cost=base, terms=None, wide="bf16x3", tile="auto")),
        ("halfcheetah cost columns", dict(model=narrow, cost=dict(base, flip_thresh=cheetah.flip_thresh), terms=None,
                                          wide="auto", tile="f16x2")),
    ]

    def apply(pl, cfg, prev):
        if prev is None or cfg["wide"] != prev["wide"]:
            pl.set_wide_arith(cfg["wide"])
        if prev is None or cfg["tile"] != prev["tile"]:
            pl.set_tile_arith(cfg["tile"])
        if prev is None or cfg["model"] is not prev["model"]:
            m = cfg["model"]
            pl.set_model(m.kind, m.A, m.B)
        c = cfg["cost"]
        pl.set_cost(c["ctrl_weight"], c["lin_idx"], c["lin_weight"], c["flip_idx"], c["flip_penalty"], c["flip_thresh"])
        if cfg["terms"] is not None:
            pl.set_cost_spec(cfg["terms"])
        elif prev is not None and prev["terms"] is not None:
            pl.lib.icem_set_cost_terms(pl._h, None)

    pl = new_handle()
    prev = None
    for what, cfg in steps:
        apply(pl, cfg, prev)
        prev = cfg
        fresh = new_handle()
        apply(fresh, cfg, None)
        assert _route(pl) == _route(fresh), what
        o = cfg["model"].A.shape[0]
        rs = np.random.RandomState(len(what))
        obs0 = 0.2 * rs.randn(o)
        act = torch.as_tensor(rs.uniform(-1, 1, (N_ROWS, h, d)), dtype=pl.dt, device=pl.device)
        assert torch.equal(pl.rollout_cost(obs0, act), fresh.rollout_cost(obs0, act)), what
        pl.reset()
        fresh.reset()
        a, b = np_(pl.plan_step(obs0)), np_(fresh.plan_step(obs0))
        assert np.array_equal(a, b), what
        assert np.array_equal(np_(pl.mean), np_(fresh.mean)) and np.array_equal(np_(pl.std), np_(fresh.std)), what
