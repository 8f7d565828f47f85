"""Cases, emulation and acceptance criteria shared by test_mlp_cpu.py, test_mlp_sensitivity_cpu.py, test_gpu_mlp_probes.py and
test_gpu_mlp_controllers.py (a plain module, no fixtures): what icem_mlp_rollout_cost is run on, and when its states count as
equal to the float64 emulation of its rounding points (``emulated_states`` with q = bf16).

The rounding points (icem_amd/csrc/k_mlp_rollout.hip): every weight is bf16 (pack time); the state, the action and every
hidden activation are rounded to bf16 as matrix operands only; accumulation (bias first), biases, activations, the residual
add and the state itself are the working type -- f32 in the kernel, float64 in the reference.

The criterion for the states (rssm_cases.py's convention).  Row error e = max over (t, k) |got - want| / max|want| per case
(no ``1 +``).  Two evaluations of the same rounding points agree to f32 accumulation noise on most rows and differ by one bf16
rounding flip (2^-9 of one operand, then carried through the recurrence) on a few:
    median(e) <= MEDIAN_BOUND,   share of rows with e > ROW_BOUND <= SHARE_CAP,   max(e) <= MAX_BOUND.
ROW_BOUND = 2e-5 sits between the two populations.

Where the bounds come from: the reference pair, on the CPU, never the kernel.  ``want`` (float64) against ``kernel_standin``
(float32, K blocked by 32, sigmoid outputs off by up to +-2 f32 ulp, two perturbation seeds), worst value over the whole table
(test_mlp_sensitivity_cpu.py::test_reference_pair_agrees re-measures it):
    median   2.7e-7   (2.62e-7 o32d32-L4-swish-333x30: four swish layers over 30 steps; the relu cases stay below 1e-7)
    share    0.067    (22 of 333 rows, o64d6-L4-relu-333x12; every other case <= 0.047)
    maximum  1.6e-3   (1.51e-3 o17d6-L2-relu-1007x12)
Bounds: median x 4 = 1.08e-6, share x 2 = 0.134 (a condition, <= 0.32: the table holds only cases on which the pair stays at or
under 0.16), maximum x 4 = 6.4e-3 -- the factors cover the matrix instruction's own accumulation order, which no CPU blocking
reproduces.  (Flips never decay in a residual state, so the share grows with the horizon and the output gain: the table keeps
h = 30 at output gain 0.15 and below, where the pair measures 0.03; at 0.3 the state itself runs away to |s| = 34.)

The criterion for the costs is cost_term_cases.py's, unchanged (row bound on every row that is not near a threshold, median
bound): the kernel's costs against the float64 oracle cost evaluated on the kernel's OWN states (``observations``) and the f32
actions -- ``cost_case`` builds that reference and hands it to cost_term_cases.

The table.  Observation widths 1, 3, 16, 17, 32, 33, 39, 64 (every 16-block and 32-block edge of the layout), action widths
1, 6, 32, hidden layers 1, 2, 4, both activations, populations 1, 13, 16, 17 (pooled launches), 333, 1007, horizons 1, 2, 12,
30.  Hidden weights at gain 2.5 .. 3 (relu) with obs0 = 0.5 .. 1 N(0, 1): across the relu cases every hidden unit of every
layer position is positive on some row (test_mlp_sensitivity_cpu.py asserts it).  The output gain keeps |s| below 10 over the
horizon; long horizons and deep networks take a smaller one.
"""
from collections import namedtuple

import numpy as np

from oracle import icem_oracle as O
from oracle.rssm_oracle import bf16

HID = 200
MODES = {"sum": 0, "best": 1, "final": 2}

# gain: on every hidden weight matrix; out_gain: on Wout; obs: scale of obs0 = scale * N(0, 1)
# launches: the rows of the case come from that many launches of n rows each, every launch with an observation and actions of
# its own -- one launch of 1 or 13 rows says nothing about a median.
Case = namedtuple("Case", "name o d L act h n wseed gain out_gain obs launches")


def _case(name, o, d, L, act, h, n, wseed=0, gain=1.5, out_gain=0.5, obs=0.5, launches=1):
    return Case(name, o, d, L, act, h, n, wseed, gain, out_gain, obs, launches)


CASES = [
    _case("o17d6-L2-relu-1007x12", 17, 6, 2, "relu", 12, 1007, gain=2.5, out_gain=0.4),
    _case("o17d6-L2-relu-333x30", 17, 6, 2, "relu", 30, 333, wseed=1, gain=2.5, out_gain=0.15),
    _case("o32d32-L4-swish-333x30", 32, 32, 4, "swish", 30, 333, wseed=2, gain=1.0, out_gain=0.1),
    _case("o3d1-L1-relu-1007x12", 3, 1, 1, "relu", 12, 1007, wseed=3, gain=2.5),
    _case("o1d1-L1-swish-17x2", 1, 1, 1, "swish", 2, 17, wseed=4, gain=2.0, launches=8),
    _case("o16d6-L2-swish-16x12", 16, 6, 2, "swish", 12, 16, wseed=5, launches=8),
    _case("o33d6-L2-relu-333x12", 33, 6, 2, "relu", 12, 333, wseed=6, gain=2.5, out_gain=0.3),
    _case("o39d32-L2-relu-333x12", 39, 32, 2, "relu", 12, 333, wseed=7, gain=2.5, out_gain=0.3),
    _case("o64d6-L4-relu-333x12", 64, 6, 4, "relu", 12, 333, wseed=16, gain=2.5, out_gain=0.1),
    _case("o64d1-L1-swish-333x2", 64, 1, 1, "swish", 2, 333, wseed=9),
    _case("o17d6-L2-relu-1x1", 17, 6, 2, "relu", 1, 1, wseed=10, gain=2.5, launches=96),
    _case("o17d6-L1-swish-13x2", 17, 6, 1, "swish", 2, 13, wseed=11, launches=10),
    _case("o32d1-L1-relu-17x12", 32, 1, 1, "relu", 12, 17, wseed=12, gain=2.5, out_gain=0.2, launches=8),
    _case("o39d6-L4-swish-333x12", 39, 6, 4, "swish", 12, 333, wseed=13, gain=1.0, out_gain=0.3),
    _case("o17d32-L4-relu-1007x12", 17, 32, 4, "relu", 12, 1007, wseed=14, gain=3.0, out_gain=0.1, obs=1.0),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

_modules = {}


def module(case):
    """The f32 torch module of the case (CPU): declared_mlp(wseed) with the hidden weights times gain, Wout times out_gain."""
    import torch
    from icem_amd.models import declared_mlp
    key = (case.o, case.d, case.L, case.act, case.wseed, case.gain, case.out_gain)
    if key not in _modules:
        net = declared_mlp(case.o, case.d, layers=case.L, activation=case.act, seed=case.wseed, device="cpu").module
        with torch.no_grad():
            for lin in net.hidden:
                lin.weight.mul_(case.gain)
            net.out.weight.mul_(case.out_gain)
        _modules[key] = net
    return _modules[key]


def params_of(net) -> dict:
    """{"W": [hidden weights], "b": [hidden biases], "Wout", "bout", "act"} as float64 arrays of the module's f32 values."""
    f = lambda t: t.detach().cpu().numpy().astype(np.float64)  # noqa: E731
    return dict(W=[f(lin.weight) for lin in net.hidden], b=[f(lin.bias) for lin in net.hidden], Wout=f(net.out.weight),
                bout=f(net.out.bias), act=net.activation)


def params(case) -> dict:
    return params_of(module(case))


def launches(case, rows=None):
    """[(obs [o], actions [n, h, d])] of the case (float64 arrays holding f32 values); ``rows`` caps the rows of a launch."""
    n = case.n if rows is None else min(case.n, rows)
    f = lambda x: np.asarray(x).astype(np.float32).astype(np.float64)  # noqa: E731
    out = []
    for i in range(case.launches):
        ob = case.obs * np.random.RandomState(100 + case.wseed + 1000 * i).randn(case.o)
        acts = np.random.RandomState(600 + case.wseed + 1000 * i).uniform(-1, 1, (n, case.h, case.d))
        out.append((f(ob), f(acts)))
    return out


def over_launches(case, fn, rows=None) -> np.ndarray:
    """fn(obs, actions) -> [n, ...] for every launch of the case, stacked along the rows."""
    return np.concatenate([fn(ob, acts) for ob, acts in launches(case, rows)], 0)


# ---- the emulation ------------------------------------------------------------------------------------------------------
def emulated_states(P: dict, obs0, actions, q=None, dtype=np.float64, act_ulp: float = 0.0, rng=None, kblock: int = 0, state_q=None,
                    residual: bool = True, skip_layer: int = -1, act: str = None, action_shift: int = 0, active: dict = None) -> np.ndarray:
    """States ``[n, h + 1, o]`` (s_0 .. s_h) of ``actions [n, h, d]`` from ``obs0 [o]``.

    ``q``        rounding applied to the weights and to every matrix operand (``bf16``: the kernel's rounding points; ``None``:
                 none -- in float64 that is the network itself);
    ``dtype``    the type of accumulators, biases, activations, the residual add and the state;
    ``kblock``   > 0: contractions accumulate block by block of that many inputs, bias first (the matrix instruction's K = 32;
                 the input layer's state and action columns are blocks of their own, as in the packed layout);
    ``act_ulp``  > 0: every sigmoid output is multiplied by ``1 + e``, ``e`` uniform in ``+-act_ulp * 2^-23`` (``rng``);
    the rest are single faults for the sensitivity test: ``state_q`` rounds the stored state, ``residual=False`` drops the
    ``s +``, ``skip_layer`` leaves out hidden layer k >= 1, ``act`` overrides the activation, ``action_shift`` feeds the action of
    step t + shift (clamped to the horizon); ``active`` receives, per hidden layer, which units were positive somewhere."""
    q = q or (lambda x: x)
    ft = np.dtype(dtype).type
    W = [q(w).astype(ft) for w in P["W"]]
    b = [x.astype(ft) for x in P["b"]]
    Wout, bout = q(P["Wout"]).astype(ft), P["bout"].astype(ft)
    act = act or P["act"]
    actions = np.asarray(actions)
    n, h, d = actions.shape
    s = np.broadcast_to(np.asarray(obs0, dtype=np.float32).astype(ft), (n, len(obs0))).copy()   # the kernel reads obs0 as f32
    o = s.shape[1]
    one, eps = ft(1), ft(act_ulp * 2.0 ** -23)

    def dense(x, w, bias, splits=None):
        if kblock <= 0:
            return x @ w.T + bias
        acc = np.broadcast_to(bias, (x.shape[0], w.shape[0])).astype(ft)
        for c0, c1 in (splits or [(0, w.shape[1])]):
            for k0 in range(c0, c1, kblock):
                k1 = min(k0 + kblock, c1)
                acc = acc + x[:, k0:k1] @ w[:, k0:k1].T
        return acc

    def activation(y, layer):
        if active is not None:
            active[layer] = active.get(layer, False) | (y > 0).any(0)
        if act == "relu":
            return np.maximum(y, 0)
        sig = one / (one + np.exp(-y))
        if act_ulp > 0:
            sig = sig * (one + eps * rng.uniform(-1, 1, y.shape).astype(ft))
        return y * sig

    states = [s]
    for t in range(h):
        a = actions[:, min(max(t + action_shift, 0), h - 1)].astype(ft)
        x = np.concatenate([q(s), q(a)], -1)
        x = q(activation(dense(x, W[0], b[0], [(0, o), (o, o + d)]), 0))
        for k in range(1, len(W)):
            if k == skip_layer:
                continue
            x = q(activation(dense(x, W[k], b[k]), k))
        delta = dense(x, Wout, bout)
        s = (s + delta if residual else delta).astype(ft)
        if state_q is not None:
            s = state_q(s)
        states.append(s)
    return np.stack(states, 1)


def want(case, rows=None, **kw) -> np.ndarray:
    """The float64 emulation of the kernel's rounding points: the reference of the tests."""
    P = params(case)
    return over_launches(case, lambda ob, a: emulated_states(P, ob, a, q=bf16, **kw), rows)


def kernel_standin(case, rows=None, P=None, seed=0, **kw) -> np.ndarray:
    """What stands for the kernel on the CPU: the same emulation in float32, contractions accumulated in blocks of 32, every
    sigmoid output off by a random relative error within +-2 ulp of f32 (v_exp_f32 and v_rcp_f32 are documented to 1 ulp each)."""
    P = params(case) if P is None else P
    rng = np.random.RandomState(seed)
    kw = dict(dict(q=bf16, dtype=np.float32, kblock=32, act_ulp=2.0, rng=rng), **kw)
    return over_launches(case, lambda ob, a: emulated_states(P, ob, a, **kw), rows).astype(np.float64)


# ---- acceptance of the states ---------------------------------------------------------------------------------------------
# the reference pair's worst values over the table, two seeds (measured on the CPU: test_reference_pair_agrees re-measures them)
PAIR_MEDIAN = 2.7e-7   # 2.62e-7 o32d32-L4-swish-333x30 (four swish layers, 30 steps; next 1.28e-7 o39d6-L4-swish, relu cases <= 1e-7)
PAIR_SHARE = 0.067     # o64d6-L4-relu-333x12; then 0.047 (o16d6-L2-swish-16x12, o17d32-L4-relu-1007x12); <= 0.16: the condition on the table
PAIR_MAX = 1.6e-3      # 1.51e-3 o17d6-L2-relu-1007x12; 1.37e-3 o33d6-L2-relu-333x12
MEDIAN_BOUND = 4 * PAIR_MEDIAN
ROW_BOUND = 2e-5
SHARE_CAP = 2 * PAIR_SHARE
MAX_BOUND = 4 * PAIR_MAX
assert SHARE_CAP <= 0.32


def row_errors(got, want_) -> np.ndarray:
    got, want_ = np.asarray(got, np.float64), np.asarray(want_, np.float64)
    e = np.abs(got - want_).reshape(len(want_), -1).max(1) / np.abs(want_).max()
    return np.where(np.isfinite(e), e, np.inf)


def errors(got, want_) -> dict:
    """Row errors normalised by max|want|: their median, the share above ROW_BOUND, the maximum, and the (1 - SHARE_CAP)
    quantile (the share part is missed by the factor this quantile has over ROW_BOUND)."""
    e = row_errors(got, want_)
    return dict(median=float(np.median(e)), share=float((e > ROW_BOUND).mean()), max=float(e.max()),
                quantile=float(np.quantile(e, 1 - SHARE_CAP)), worst_row=int(e.argmax()), rows=len(e))


def violations(got, want_) -> list:
    got = np.asarray(got)
    if got.shape != np.asarray(want_).shape:
        return [f"shape {got.shape} instead of {np.asarray(want_).shape}"]
    s = errors(got, want_)
    out = []
    if not s["median"] <= MEDIAN_BOUND:
        out.append(f"median row error {s['median']:.3g} > {MEDIAN_BOUND:.3g}")
    if not s["share"] <= SHARE_CAP:
        out.append(f"{s['share']:.3f} of the rows above {ROW_BOUND:.3g} > {SHARE_CAP:.3g}")
    if not s["max"] <= MAX_BOUND:
        out.append(f"largest row error {s['max']:.3g} (row {s['worst_row']}) > {MAX_BOUND:.3g}")
    return out


def agree(got, want_) -> bool:
    return not violations(got, want_)


# ---- the packed layout, restated entry by entry (icem_amd/csrc/icem_mlp.h) -------------------------------------------------
def param_elems(o, d, L) -> int:
    sk, ob = (o + 31) // 32, (o + 15) // 16
    return 13 * (sk + 1) * 512 + 416 + (L - 1) * (13 * 7 * 512 + 416) + ob * 7 * 512 + 32 * ob


def unpack(buf, o, d, L) -> list:
    """[(weight [rows, cols] float32 of the bf16 entries, bias [rows] float32)] per layer of a packed buffer (int16 tensor),
    by the layout's index formula: block (ob, kb), lane 16 g + i, entry v holds W[16 ob + i][32 kb + 8 g + v]."""
    import torch
    raw = buf.detach().cpu().contiguous()
    sk, ob_n = (o + 31) // 32, (o + 15) // 16
    shapes = [(13, sk + 1)] + [(13, 7)] * (L - 1) + [(ob_n, 7)]
    out, at = [], 0
    for nob, nkb in shapes:
        cnt = nob * nkb * 512
        blocks = (raw[at:at + cnt].to(torch.int32) << 16).view(torch.float32).reshape(nob, nkb, 4, 16, 8).numpy()
        at += cnt
        w = np.zeros((16 * nob, 32 * nkb), np.float32)
        for ob in range(nob):
            for kb in range(nkb):
                for g in range(4):
                    w[16 * ob:16 * ob + 16, 32 * kb + 8 * g:32 * kb + 8 * g + 8] = blocks[ob, kb, g]
        bias = raw[at:at + 32 * nob].contiguous().view(torch.float32).numpy().copy()
        at += 32 * nob
        out.append((w, bias))
    assert at == raw.numel()
    return out


# ---- the costs: cost_term_cases.py's criterion on the kernel's own states ---------------------------------------------------
def cost_case(name, spec, mode, states, acts):
    """A cost_term_cases.Case whose reference is the float64 oracle cost of ``spec`` on ``states [n, h + 1, o]`` (the kernel's own
    ``observations``, or the emulation's) and ``acts [n, h, d]``: want, the per-row magnitude (oracle.trajectory_cost_magnitudes +
    the state term), the threshold margins -- everything cost_term_cases' ``violations`` / ``rejection`` read."""
    import cost_term_cases as CT
    states, acts = np.asarray(states, np.float64), np.asarray(acts, np.float64)
    n, h, d = acts.shape
    obs, nxt = states[:, :-1], states[:, 1:]
    nx = nxt if spec.needs_next_obs else None
    smax = np.abs(obs).max(axis=(1, 2))
    mag = O.trajectory_cost_magnitudes(spec, obs, acts, nx, mode=mode) + CT.state_weight(spec) * smax * (h if mode == "sum" else 1)
    case = CT.Case(name, "mlp", states.shape[2], d, h, 0, mode, n, spec)
    CT._ref[name] = dict(want=O.spec_trajectory_costs(spec, obs, acts, nx, mode=mode, dtype=np.float64), mag=mag,
                         margin=O.observation_margins(spec, obs), smax=smax, obs=obs)
    return case


def costs_f32(spec, mode, states, acts) -> np.ndarray:
    """The kernel's cost arithmetic on the CPU: oracle.spec_trajectory_costs in float32 on the f32 states."""
    s32 = np.asarray(states, np.float32)
    nx = s32[:, 1:] if spec.needs_next_obs else None
    return O.spec_trajectory_costs(spec, s32[:, :-1], np.asarray(acts, np.float32), nx, mode=mode, dtype=np.float32).astype(np.float64)


# ---- the cost table: the environments' cost programs at their widths -------------------------------------------------------
# A two-layer relu network per environment (hidden gain 2.5, the input layer's action columns times act_gain so that the rows
# of a launch spread); col_gain ((column, gain)): Wout's row and bout's entry of that state column times gain (how far the
# column moves per step); obs_sets: one launch per entry, ((column, value), ..) put into obs0 after obs_scale * N(0, 1);
# bias_set ((column, value)): bout entries put in at the end.  Chosen by search over the float64 emulation (never a kernel) so
# that every comparison of the spec comes out both ways: true on 10-90 % of the (row, step) pairs of the case
# (test_mlp_sensitivity_cpu.py::test_cost_envs_fire_every_comparison), with at most 1 % of the rows near a threshold.
CostEnv = namedtuple("CostEnv", "name o d spec wseed out_gain act_gain col_gain obs_scale obs_sets bias_set n h")


def _env(name, o, d, spec, wseed, out_gain=0.3, act_gain=3.0, col_gain=(), obs_scale=0.3, obs_sets=((),), bias_set=(), n=333, h=12):
    return CostEnv(name, o, d, spec, wseed, out_gain, act_gain, tuple(col_gain), obs_scale, tuple(obs_sets), tuple(bias_set), n, h)


def _cost_envs():
    hopper = O.CostSpec.hopper(healthy_z_range=(-0.05, float("inf")), healthy_state_range=(-0.45, 0.45))   # cost_term_cases' ranges
    fpp_cols = (0, 1, 2, 3, 4, 5, 25, 26, 27)
    return [
        _env("halfcheetah", 17, 6, O.CostSpec.halfcheetah(17), 20, obs_sets=(((1, 1.45),), ((1, -2.6),))),
        _env("hopper", 12, 3, hopper, 21, out_gain=0.1, obs_scale=0.1, obs_sets=(((1, 1.0),), ((1, 0.3),))),
        _env("reacher", 11, 2, O.CostSpec.reacher(11), 22),
        _env("fetchreach-sparse", 13, 4, O.CostSpec.fetch_reach(10, True, 0.4), 23, out_gain=0.1, obs_scale=0.15),
        _env("fpp-sparse", 28, 4, O.CostSpec.fetch_pick_and_place(sparse=True), 24, out_gain=0.1, col_gain=tuple((c, 0.1) for c in fpp_cols),
             obs_sets=(tuple((c, 0.0 if 3 <= c <= 5 else 0.02 if c < 3 else -0.03) for c in fpp_cols),)),
        _env("fpp-dense", 28, 4, O.CostSpec.fetch_pick_and_place(), 24),
        _env("door", 39, 28, O.CostSpec.door(), 25, obs_sets=(((28, 0.1),), ((28, 0.9),), ((28, 1.25),)), n=111),
        _env("relocate", 39, 30, O.CostSpec.relocate(), 26, out_gain=0.1, col_gain=((36, 0.25), (37, 0.25), (38, 0.25)),
             obs_sets=(((36, 0.06), (37, -0.03), (38, 0.045)), ((36, 0.025), (37, -0.02), (38, 0.033)))),
        # 'best' at h = 2 where one step holds most of the minima: a reduction over steps 1 .. h-1 or 0 .. h-2 moves most rows
        _env("halfcheetah-best-first", 17, 6, O.CostSpec.halfcheetah(17), 27, bias_set=((8, -0.1),), h=2),
        _env("halfcheetah-best-last", 17, 6, O.CostSpec.halfcheetah(17), 28, bias_set=((8, 0.1),), h=2),
    ]


COST_ENVS = _cost_envs()
COST_ENV_BY_NAME = {e.name: e for e in COST_ENVS}
LOPSIDED = {"halfcheetah-best-first": 0, "halfcheetah-best-last": 1}   # env -> the step that holds most minima


def cost_module(env):
    """The f32 torch module of a cost environment (CPU)."""
    import torch
    from icem_amd.models import declared_mlp
    key = ("cost", env.name)
    if key not in _modules:
        net = declared_mlp(env.o, env.d, layers=2, activation="relu", seed=env.wseed, device="cpu").module
        with torch.no_grad():
            for lin in net.hidden:
                lin.weight.mul_(2.5)
            net.hidden[0].weight[:, env.o:].mul_(env.act_gain)
            net.out.weight.mul_(env.out_gain)
            for c, g in env.col_gain:
                net.out.weight[c].mul_(g)
                net.out.bias[c].mul_(g)
            for c, v in env.bias_set:
                net.out.bias[c] = v
        _modules[key] = net
    return _modules[key]


def cost_launches(env):
    """[(obs0 [o], actions [n, h, d])] of a cost environment, one per entry of obs_sets: float64 arrays holding f32 values."""
    f = lambda x: np.asarray(x).astype(np.float32).astype(np.float64)  # noqa: E731
    out = []
    for i, obs_set in enumerate(env.obs_sets):
        rs = np.random.RandomState(300 + env.wseed + 1000 * i)
        ob = env.obs_scale * rs.randn(env.o)
        for c, v in obs_set:
            ob[c] = v
        out.append((f(ob), f(rs.uniform(-1, 1, (env.n, env.h, env.d)))))
    return out


def cost_actions(env) -> np.ndarray:
    return np.concatenate([a for _, a in cost_launches(env)], 0)


def cost_states(env) -> np.ndarray:
    """The float64 emulation's states of a cost environment's launches: what the CPU tests score in the kernel's place."""
    P = params_of(cost_module(env))
    return np.concatenate([emulated_states(P, ob, acts, q=bf16) for ob, acts in cost_launches(env)], 0)


def comparison_rates(spec, states) -> dict:
    """{comparison: the share of the (row, step) pairs on which it is true} over the pre-action states of ``states [n, h + 1, o]``."""
    obs = np.asarray(states, np.float64)[:, :-1]
    hits = {}
    for t in range(obs.shape[1]):
        for name, dist in O._comparisons(spec, obs[:, t]):
            hits.setdefault(name, []).append(dist > 0)
    return {k: float(np.mean(v)) for k, v in hits.items()}


def step_costs(spec, states, acts) -> np.ndarray:
    """Float64 per-step costs [n, h] of the spec on states [n, h + 1, o]."""
    states, acts = np.asarray(states, np.float64), np.asarray(acts, np.float64)
    return np.stack([O.spec_trajectory_costs(spec, states[:, t:t + 1], acts[:, t:t + 1], states[:, t + 1:t + 2], mode="final", dtype=np.float64)
                     for t in range(acts.shape[1])], 1)
