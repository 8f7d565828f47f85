"""Cases and acceptance criterion shared by test_cost_term_sensitivity_cpu.py and test_gpu_cost_term_probes.py (a plain
module, no fixtures): what the device evaluations of the env cost terms (icem_cost_terms + icem_cost_spec in TileHN, the
wide GEMM kernels and the general rollout kernel) are run on, and when their costs count as equal to the float64 oracle.

The criterion.  Row error e = |got - want| / m; want = the float64 oracle on the inputs the kernels see (model, observation
and actions rounded to f32), m = the row's per-mode magnitude: oracle.rollout_cost_magnitudes(mode=) -- sum |addend| over
all steps ('sum'), of the last scored step ('final'), of the step the float64 minimum is taken at ('best') -- plus a state
term, (|lin_weight| + sum |w| over the NORM terms) x the row's largest |state entry| (x h in 'sum'): the parts of the cost
that are linear in the state carry the state's ABSOLUTE error whatever their own value (a state unit read out near zero, the
norm of a small difference), and the reference pair shows it (without the term the readout of a unit that passes through zero
has no bound at all).  Both from the float64 oracle alone.
    every row that is NOT near a threshold:  e <= ROW_BOUND        (no share allowance)
    median of e over the case:                 <= MEDIAN_BOUND
A row is near a threshold when oracle.threshold_margins <= NEAR: some compared quantity of some step -- flip (both signs),
STEP_GT, NORM_GT / NORM_LT, a gate, the health range, the box -- is within NEAR x (the row's largest |state entry|) of its
threshold.  Such a row may miss the bound (an indicator may come out the other way: a whole bonus).  At most 1 % of the rows
of any case are near a threshold: a condition on the INPUTS, asserted from the oracle alone.

Where the bounds come from: the reference pair, on the CPU, never a kernel.  want against kernel_standin: the same costs in
float32 (oracle.spec_trajectory_costs(dtype=float32), the kernels' order of additions) with the model entries and every step's
state rounded to 22 significant bits (two fp16 planes) and every square root off by -1 / 0 / +1 ulp, two perturbation seeds.
Worst values over the whole table (test_cost_term_sensitivity_cpu.py::test_reference_pair_agrees re-measures them):
    row error     1.8e-6   (1.72e-6 relocate-unit14-k0-final; shipped specs 1.69e-6 door-fast-k0-final, term programs 1.48e-6)
    median        3.5e-7   (3.41e-7 door-unit14-k0-final; 3.34e-7 door-fast-k0-final-273x30)
    state error   3.4e-6   of the row's largest |state entry| (3.32e-6 door-k0-sum-273x30; tanh cases <= 2e-6)
Bounds: each x 4 -- ROW_BOUND 7.2e-6 (below the 1e-5 the rollout tests claimed against the larger sum-mode magnitude),
MEDIAN_BOUND 1.4e-6, NEAR 1.36e-5 -- the factor covers the matrix instruction's accumulation order, which no CPU loop
reproduces (the factor and the reason of rssm_cases.py).  The general kernel in f64: rtol 1e-10, as elsewhere in the suite.

What the bounds reject (test_cost_term_sensitivity_cpu.py, 339 single faults of the float64 oracle): every one misses the row
or the median bound by a factor >= 10 on some case or leaves >= 10 rows that are not near a threshold out of bound.  Weakest:
Door's 30-entry velocity term (weight 1e-5) under tanh with a + 1 / len - 1 (x 2.2 / x 2.4, 49 / 67 rows), its weight x 1.01
under the linear model (x 5.9, 101 rows on door-fast), len - 1 / a + 1 there (x 10 / x 14); every other fault by x 33 and more.
What the table CANNOT see: that term's weight x 1.01 under tanh (every velocity below 1: 3e-6 of a step's cost); a low fp16
plane dropped, or a model entry wrong, in a column that no term of ANY case reads and that feeds none (the unit readouts read
every column, so there is none at o = 39 / 28 -- the narrow tile kernels, Tile16H / Tile16 / Tile4 at o = 17 .. 24, which no case
of THIS table reaches, have the same readouts and an entry-by-entry model table in tile_cases.py, test_gpu_tile_probes.py; the
wide GEMM kernels are reached here at o = 39 only -- one column tile per wave, NT = 4, uniform ksc / csc --, which is NOT their
entry coverage: NCT > 1, NT > 4, the FIVE instantiation and the per-entry scales are wide_cases.py, test_gpu_wide_probes.py);
'final' over steps 1 .. h-1 (the same step); a zero threshold x 1.1.

The table (all cases <= 1100 rows, one launch each; h = 30 where TileHN serves the shape, h = 12 for the other kernels):
  shipped    Door, Relocate, FetchPickAndPlace dense and sparse x model kind 0 / 1 x sum / best / final at 533 rows (33 tiles
             + 5), 273 (17 tiles + 1), 1 row, and h = 12; inputs under which every comparison of the spec is true at some
             step and false at another on 10-90 % of the rows (SHIPPED below; Door under tanh with the bonuses at 0.2 / 0.5 /
             0.7: the hinge entry stays inside (-1, 1)); door-fast: velocities of +-3, where the 1e-5 term weighs something
  envs       Ant, Hopper, Humanoid, Reacher, FetchReach-sparse at h = 12 (wide GEMM kernels, general kernel)
  unit-*     program 0, cost = state unit k: every k, both kinds, final and sum, 64 rows
  action-*   A = 0, B one-hot: cost = 0.75 x action entry j, every j (the partial group 28, 29 at d = 30; 27 at d = 28; 3 at d = 4)
  control    A = B = 0, ctrl_weight 0.1, row r has the single action entry (t, j) = divmod(r, d): 0.1 a^2; bare and before a term list
  flip       flip and linear parts on units 0, 15, 16, 31, 32, o - 1, both signs firing on 10-90 % of the rows
  programs   lists filling every slot of {0,2,0}, {0,4,1}, {1,1,4}; each also reversed (the host sorts terms into slots: the
             result may differ by f32 addition order only, and is held to the same bound against the oracle of the order given)
"""
import dataclasses
import typing

import numpy as np

from oracle import icem_oracle as O

MODES = ("sum", "best", "final")
T = O.CostTerm
NORM, NORM_GT, NORM_LT, SQ_OFFSET, SUMSQ, STEP_GT = (O.TERM_NORM, O.TERM_NORM_GT, O.TERM_NORM_LT, O.TERM_SQ_OFFSET,
                                                     O.TERM_SUMSQ, O.TERM_STEP_GT)
HN_SHAPES = {"door": (39, 28), "relocate": (39, 30), "fpp": (28, 4)}   # (o, d) of the TileHN kernels, h = 30


@dataclasses.dataclass(eq=False)
class Case:
    """One launch.  model: "make" = SyntheticModel.make(o, d, kind) with the columns of ``col_gain`` ((column, gain): B's
    column and A's off-diagonal entries of that column times gain), ("onehot", j, k, w) = A = 0 and B = w at [j, k] only,
    "zero" = A = B = 0 (a subclass with a ``matrices()`` method brings forms of its own: tile_cases.py); every entry rounded to
    f32 (the device keeps the model in f32).  obs: ``obs_scale`` * N(0, 1), entries
    of ``obs_set`` ((index, value)) put in afterwards.  acts: "uniform" = ``act_scale`` * U(-1, 1); "single" = row r has
    one non-zero entry, at (t, j) = divmod(r, d).  ``high``: the planner's action bound (low = -high)."""
    name: str
    group: str
    o: int
    d: int
    h: int
    kind: int
    mode: str
    n: int
    spec: O.CostSpec
    seed: int = 3
    obs_scale: float = 0.2
    act_scale: float = 1.0
    col_gain: tuple = ()
    obs_set: tuple = ()
    model: object = "make"
    acts: str = "uniform"
    high: float = 1.0
    fires: bool = False      # a shipped spec "made to fire": every comparison true at some step and false at another on 10-90 % of the rows
    what: str = ""           # readout cases: what a failure names

    @property
    def tilehn(self) -> bool:
        """Does TileHN serve the case (a compiled shape at h = 30, a term list that fits a compiled program)?"""
        if (self.o, self.d) not in HN_SHAPES.values() or self.h != 30:
            return False
        if self.spec.diff_idx >= 0 or self.spec.health_idx >= 0:
            return False
        n32 = sum(1 for t in self.spec.terms if t.kind not in (STEP_GT, SQ_OFFSET) and 4 < t.len <= 32)
        n4 = sum(1 for t in self.spec.terms if t.kind not in (STEP_GT, SQ_OFFSET) and t.len <= 4)
        npt = sum(1 for t in self.spec.terms if t.kind in (STEP_GT, SQ_OFFSET))
        long_ok = all(t.len <= 32 for t in self.spec.terms if t.kind not in (STEP_GT, SQ_OFFSET))
        return long_ok and any(n32 <= a and n4 <= b and npt <= c for a, b, c in ((0, 0, 0), (0, 2, 0), (0, 4, 1), (1, 1, 4)))


_given, _inputs, _rollouts, _ref = {}, {}, {}, {}


def input_key(case):
    """Cases that differ in the cost alone (the readouts of one shape, a list and its reversal) share inputs and rollouts."""
    if case.name in _given:
        return ("given", case.name)
    return (case.o, case.d, case.h, case.kind, case.n, case.seed, case.obs_scale, case.act_scale, case.col_gain, case.obs_set,
            case.model, case.acts)


def give_inputs(case, om, obs0, acts):
    """Inputs that come from elsewhere (the last pool of an MPC step) for a case made on the spot."""
    _given[case.name] = (om, obs0, acts)


def inputs(case):
    """(oracle model, obs0 [o], actions [n, h, d]): float64 arrays holding f32 values -- what the f32 kernels are handed."""
    key = input_key(case)
    if key[0] == "given":
        return _given[case.name]
    if key not in _inputs:
        o, d = case.o, case.d
        if hasattr(case, "matrices"):   # a subclass with model forms of its own (tile_cases.py)
            A, B = case.matrices()
        elif case.model == "make":
            m = O.SyntheticModel.make(o, d, case.kind)
            A, B = m.A.copy(), m.B.copy()
            for c, g in case.col_gain:
                diag = A[c, c]
                A[:, c] *= g
                A[c, c] = diag
                B[:, c] *= g
        else:
            A, B = np.zeros((o, o)), np.zeros((d, o))
            if case.model != "zero":
                _, j, k, w = case.model
                B[j, k] = w
        f = lambda x: np.asarray(x).astype(np.float32).astype(np.float64)  # noqa: E731
        rs = np.random.RandomState(case.seed)
        obs0 = case.obs_scale * rs.randn(o)
        for i, v in case.obs_set:
            obs0[i] = v
        if case.acts == "uniform":
            acts = case.act_scale * rs.uniform(-1, 1, (case.n, case.h, d))
        else:
            assert case.n == case.h * d
            acts = np.zeros((case.n, case.h * d))
            acts[np.arange(case.n), np.arange(case.n)] = rs.uniform(0.3, 1.0, case.n) * rs.choice([-1.0, 1.0], case.n) * case.act_scale
            acts = acts.reshape(case.n, case.h, d)
        _inputs[key] = (O.SyntheticModel(f(A), f(B), case.kind), f(obs0), f(acts))
    return _inputs[key]


def q22(x):
    """x rounded to 22 significant bits: what two fp16 planes (11 + 11) hold of an operand."""
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    return np.ldexp(np.round(m * 2.0 ** 22) / 2.0 ** 22, e)


class _PlaneModel(O.SyntheticModel):
    def predict(self, obs, act):
        return q22(super().predict(obs, act)).astype(obs.dtype)


def _with_next(model, obs, acts):
    return np.concatenate([obs[:, 1:], model.predict(obs[:, -1], acts[:, -1])[:, None]], axis=1)


def rollouts(case) -> dict:
    """The two rollouts of the case's inputs: float64 (obs, nxt [n, h, o], smax [n]) and the float32 stand-in's (obs32, nxt32:
    model entries and every step's state rounded to 22 significant bits; state_err [n]: its largest state error over the
    row's largest |state entry|)."""
    key = input_key(case)
    if key not in _rollouts:
        om, ob, acts = inputs(case)
        obs = O.rollout_observations(om, ob, acts)
        m32 = _PlaneModel(q22(om.A), q22(om.B), om.kind)
        a32 = acts.astype(np.float32)
        obs32 = O.rollout_observations(m32, q22(ob).astype(np.float32), a32)
        assert obs32.dtype == np.float32
        smax = np.abs(obs).max(axis=(1, 2))
        with np.errstate(invalid="ignore", divide="ignore"):   # (a state that is zero throughout: NaN, no error to speak of)
            state_err = np.abs(obs32 - obs).max(axis=(1, 2)) / smax
        _rollouts[key] = dict(obs=obs, nxt=_with_next(om, obs, acts), smax=smax, obs32=obs32, nxt32=_with_next(m32, obs32, a32),
                              state_err=state_err)
    return _rollouts[key]


def state_weight(spec) -> float:
    """Sum of |weight| over the parts of the cost that are LINEAR in the state: the linear term and the NORM terms."""
    w = abs(spec.lin_weight)
    return w + sum(abs(t.weight) for t in spec.terms if t.kind == NORM)


def reference(case) -> dict:
    """Everything the criterion needs, from the float64 oracle alone: want, magnitude, margin, smax, observations."""
    if case.name not in _ref:
        _, _, acts = inputs(case)
        r = rollouts(case)
        nxt = r["nxt"] if case.spec.needs_next_obs else None
        mag = O.trajectory_cost_magnitudes(case.spec, r["obs"], acts, nxt, mode=case.mode)
        mag = mag + state_weight(case.spec) * r["smax"] * (case.h if case.mode == "sum" else 1)
        _ref[case.name] = dict(want=O.spec_trajectory_costs(case.spec, r["obs"], acts, nxt, mode=case.mode, dtype=np.float64), mag=mag,
                               margin=O.observation_margins(case.spec, r["obs"]), smax=r["smax"], obs=r["obs"])
    return _ref[case.name]


def want(case) -> np.ndarray:
    return reference(case)["want"]


# ---- the float32 stand-in for the kernels (the reference pair's other half) ---------------------------------------------
@dataclasses.dataclass
class _UlpSpec(O.CostSpec):
    """The spec with every square root off by -1, 0 or +1 ulp of f32 (v_sqrt_f32 is documented to 1 ulp)."""
    rng: object = None

    def term_value(self, tm, obs):
        if tm.kind not in (NORM, NORM_GT, NORM_LT):
            return super().term_value(tm, obs)
        dt = obs.dtype.type
        acc = np.zeros(obs.shape[:-1], dtype=obs.dtype)
        for m in range(tm.len):
            v = obs[..., tm.a + m]
            if tm.b >= 0:
                v = v - obs[..., tm.b + m]
            acc = acc + v * v
        r = np.sqrt(acc)
        r = (r * (dt(1) + dt(2.0 ** -23) * self.rng.randint(-1, 2, r.shape).astype(obs.dtype))).astype(obs.dtype)
        f = r if tm.kind == NORM else (r > dt(tm.thresh) if tm.kind == NORM_GT else r < dt(tm.thresh)).astype(obs.dtype)
        if tm.gate_idx >= 0:
            f = f * (obs[..., tm.gate_idx] > dt(tm.gate_thresh)).astype(obs.dtype)
        return dt(tm.weight) * f


def kernel_standin(case, seed=0):
    """(costs [n] float64, largest state error of the row / the row's largest |state entry| [n]): rollout_costs in float32
    with the model entries and every step's state rounded to 22 significant bits and the square roots off by up to 1 ulp
    (``seed``: of those perturbations)."""
    _, _, acts = inputs(case)
    r = rollouts(case)
    spec = _UlpSpec(**{f.name: getattr(case.spec, f.name) for f in dataclasses.fields(case.spec)}, rng=np.random.RandomState(seed))
    got = O.spec_trajectory_costs(spec, r["obs32"], acts.astype(np.float32), r["nxt32"] if spec.needs_next_obs else None,
                                  mode=case.mode, dtype=np.float32)
    assert got.dtype == np.float32
    return got.astype(np.float64), r["state_err"]


# ---- acceptance ---------------------------------------------------------------------------------------------------------
MEASURED_ROW, MEASURED_MEDIAN, MEASURED_STATE = 1.8e-6, 3.5e-7, 3.4e-6   # the reference pair's worst values (docstring)
NEAR = 4 * MEASURED_STATE
ROW_BOUND = 4 * MEASURED_ROW
MEDIAN_BOUND = 4 * MEASURED_MEDIAN
F64_RTOL, F64_ATOL = 1e-10, 1e-12   # the general kernel in f64, as elsewhere in the suite


def row_errors(got, case) -> np.ndarray:
    ref = reference(case)
    diff = np.abs(np.asarray(got, np.float64) - ref["want"])
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.where(diff == 0, 0.0, diff / ref["mag"])
    return np.where(np.isfinite(e), e, np.inf)


class Bounds(typing.NamedTuple):
    """The criterion's three numbers; a table with a reference pair of its own (tile_cases.py) passes its own."""
    row: float
    median: float
    near: float


BOUNDS = Bounds(ROW_BOUND, MEDIAN_BOUND, NEAR)


def near(case, bounds=BOUNDS) -> np.ndarray:
    return reference(case)["margin"] <= bounds.near


def errors(got, case, bounds=BOUNDS) -> dict:
    """Row errors against the float64 oracle: the largest over the rows that are not near a threshold, how many of those
    rows are out of bound, the median over all rows, the share of near-threshold rows and how many of them miss."""
    e, nr = row_errors(got, case), near(case, bounds)
    far = np.where(nr, 0.0, e)
    return dict(worst=float(far.max()), worst_row=int(far.argmax()), out=int((far > bounds.row).sum()), median=float(np.median(e)),
                near_share=float(nr.mean()), near_out=int((nr & (e > bounds.row)).sum()), rows=len(e))


def violations(got, case, bounds=BOUNDS) -> list:
    got = np.asarray(got)
    if got.shape != want(case).shape:
        return [f"shape {got.shape} instead of {want(case).shape}"]
    s, out = errors(got, case, bounds), []
    if s["out"]:
        ref = reference(case)
        r = s["worst_row"]
        out.append(f"{s['out']} of {s['rows']} rows that are not near a threshold above {bounds.row:.3g}: worst {s['worst']:.3g} in row "
                   f"{r} (got {float(got[r]):.9g}, want {ref['want'][r]:.9g}, magnitude {ref['mag'][r]:.3g}, margin {ref['margin'][r]:.3g})")
    if not s["median"] <= bounds.median:
        out.append(f"median row error {s['median']:.3g} > {bounds.median:.3g}")
    return out


def agree(got, case, bounds=BOUNDS) -> bool:
    return not violations(got, case, bounds)


def rejection(got, case, bounds=BOUNDS) -> tuple:
    """(factor, count): by how much ``got`` misses the row or the median bound, and how many rows that are not near a
    threshold are out of bound -- a wrong evaluation counts as rejected at factor >= 10 or count >= 10."""
    s = errors(got, case, bounds)
    return max(s["worst"] / bounds.row, s["median"] / bounds.median), s["out"]


# ---- the table ----------------------------------------------------------------------------------------------------------
def _spec(terms=(), **kw):
    base = dict(ctrl_weight=0.0, lin_idx=0, lin_weight=0.0, flip_idx=-1, flip_penalty=0.0, flip_thresh=0.0)
    base.update(kw)
    return O.CostSpec(terms=tuple(terms), **base)


def _thresholds(spec, idx, vals):
    tm = list(spec.terms)
    for i, v in zip(idx, vals):
        tm[i] = dataclasses.replace(tm[i], thresh=v)
    return dataclasses.replace(spec, terms=tuple(tm))


_FPP_COLS = (0, 1, 2, 3, 4, 5, 25, 26, 27)
_FPP_OBS = tuple((c, 0.03 * (-1) ** c) for c in _FPP_COLS)
# (spec, shape, {kind: inputs under which every comparison of the spec is true at some step and false at another on 10-90 %
#  of 533 rows}) -- found by search over the float64 oracle (comparison_shares), never on a kernel.  Door under the tanh
# model: the door entry stays inside (-1, 1), so the shipped structure with the bonuses' thresholds at 0.2 / 0.5 / 0.7.
SHIPPED = {
    "door": (HN_SHAPES["door"], {0: O.CostSpec.door(), 1: _thresholds(O.CostSpec.door(), (3, 4, 5), (0.2, 0.5, 0.7))},
             {0: dict(obs_set=((28, 0.0),)), 1: dict(obs_set=((28, -0.3),))}),
    "relocate": (HN_SHAPES["relocate"], {0: O.CostSpec.relocate(), 1: O.CostSpec.relocate()},
                 {0: dict(col_gain=((36, 0.1), (37, 0.1), (38, 0.1)), obs_set=((36, 0.09), (37, -0.045), (38, -0.03))),
                  1: dict(col_gain=((36, 0.1), (37, 0.1), (38, 0.1)), obs_set=((36, 0.09), (37, -0.045), (38, 0.0)))}),
    "fpp-sparse": (HN_SHAPES["fpp"], {k: O.CostSpec.fetch_pick_and_place(sparse=True) for k in (0, 1)},
                   {0: dict(col_gain=tuple((c, 0.08) for c in _FPP_COLS), obs_set=_FPP_OBS, act_scale=0.5),
                    1: dict(col_gain=tuple((c, 0.05) for c in _FPP_COLS), obs_set=_FPP_OBS)}),
    "fpp-dense": (HN_SHAPES["fpp"], {k: O.CostSpec.fetch_pick_and_place() for k in (0, 1)}, {0: {}, 1: {}}),
}


def _shipped_cases():
    out = []
    for name, ((o, d), specs, kw) in SHIPPED.items():
        for kind in (0, 1):
            for mode in MODES:   # 33 tiles + 5 rows
                out.append(Case(f"{name}-k{kind}-{mode}-533x30", "shipped", o, d, 30, kind, mode, 533, specs[kind],
                                fires=name != "fpp-dense", **kw[kind]))
        # one row past a whole number of tiles, exactly one row (a launch with one live lane in sixteen), and the GEMM and
        # general kernels' step loops at a second horizon
        out.append(Case(f"{name}-k0-sum-273x30", "shipped", o, d, 30, 0, "sum", 16 * 17 + 1, specs[0], **dict(kw[0], seed=3 if name == "relocate" else 5)))
        out.append(Case(f"{name}-k1-best-1x30", "shipped", o, d, 30, 1, "best", 1, specs[1], **kw[1]))
        out.append(Case(f"{name}-k1-sum-257x12", "shipped", o, d, 12, 1, "sum", 257, specs[1], **kw[1]))
        out.append(Case(f"{name}-k0-final-257x12", "shipped", o, d, 12, 0, "final", 257, specs[0], **kw[0]))
    # Door's 30-entry velocity term (weight 1e-5) where it weighs something: velocities of +-3
    vel = tuple((i, 3.0 * (-1) ** i) for i in range(9, 39) if i not in (28, 29, 30, 31, 32, 33, 34))
    for mode in ("sum", "final"):
        out.append(Case(f"door-fast-k0-{mode}-273x30", "shipped", 39, 28, 30, 0, mode, 273, O.CostSpec.door(), obs_set=vel + ((28, 0.0),)))
    return out


def _other_env_cases():
    """Ant, Hopper, Humanoid, Reacher, FetchReach-sparse on the kernels that serve them (health ranges moved to where the
    synthetic latent lives, as test_gpu_parity.py does, and both ends of a range inside it; FetchReach's threshold at 0.4,
    where the norm crosses it on a third to two thirds of the rows), h = 12."""
    envs = [("ant", 113, 8, 1.0, O.CostSpec.ant(healthy_z_range=(-0.05, 0.3))),
            ("hopper", 12, 3, 1.0, O.CostSpec.hopper(healthy_z_range=(-0.05, float("inf")), healthy_state_range=(-0.45, 0.45))),
            ("humanoid", 376, 17, 0.4, O.CostSpec.humanoid(healthy_z_range=(-0.05, 0.4))),
            ("reacher", 11, 2, 1.0, O.CostSpec.reacher(11)),
            ("fetchreach-sparse", 13, 4, 1.0, O.CostSpec.fetch_reach(10, True, 0.4))]
    out = []
    for name, o, d, high, spec in envs:
        for kind, mode in ((1, "sum"), (0, "best"), (1, "final")):
            if name == "humanoid" and kind == 0:
                continue   # (one linear-model case at o = 376 costs the CPU test seconds and the kernels nothing new)
            out.append(Case(f"{name}-k{kind}-{mode}-257x12", "envs", o, d, 12, kind, mode, 257, spec, act_scale=high, high=high))
    return out


def _readout_cases():
    """Program 0 of TileHN (no terms, no flip, no control cost): the cost IS state unit k (mode final: at the last scored
    step; sum: summed over the steps), or -- A = 0, B one-hot -- ONE action entry times one weight."""
    out = []
    for shape, (o, d) in HN_SHAPES.items():
        for mode in ("final", "sum"):
            for kind in (0, 1):
                for k in range(o):
                    out.append(Case(f"{shape}-unit{k}-k{kind}-{mode}", f"unit-{shape}", o, d, 30, kind, mode, 64,
                                    _spec(lin_idx=k, lin_weight=1.0), seed=7, what=f"state unit {k}, model kind {kind}, {mode}"))
            for j in range(d):
                k = (7 * j + 3) % o
                out.append(Case(f"{shape}-act{j}-{mode}", f"action-{shape}", o, d, 30, 0, mode, 64, _spec(lin_idx=k, lin_weight=1.0),
                                seed=8, model=("onehot", j, k, 0.75), what=f"action entry {j} (through state unit {k}), {mode}"))
    return out


def _control_cases():
    """A = B = 0, ctrl_weight 0.1, h d rows with ONE non-zero action entry each, at (t, j) = divmod(row, d): every (t, j)
    -- the last step's action, which only the control cost ever sees, and the partial action group -- is 0.1 a^2 of its own
    row; alone and in front of a term list."""
    out = []
    for shape, (o, d) in HN_SHAPES.items():
        lists = {"bare": (), "terms": O.CostSpec.fetch_pick_and_place().terms if shape == "fpp" else O.CostSpec.door().terms}
        for tag, terms in lists.items():
            for mode in ("sum", "final"):
                out.append(Case(f"{shape}-ctrl-{tag}-{mode}", "control", o, d, 30, 0, mode, 30 * d, _spec(terms, ctrl_weight=0.1),
                                seed=9, model="zero", acts="single", what="row r: action entry (t, j) = divmod(r, d)"))
    return out


FLIP_THRESH = {}   # case name -> threshold, filled by _flip_cases from the float64 rollout


def _flip_cases():
    """icem_cost_spec's flip and linear parts (base_cost) on the TileHN shapes, on units at every 16-block edge; the flip
    threshold is the median over the rows of max_t |x_u| of the float64 rollout (to three digits), so that each sign fires
    on some rows and not on others."""
    out = []
    for shape, (o, d) in HN_SHAPES.items():
        units = [u for u in (0, 15, 16, 31, 32, o - 1) if u < o]
        for i, u in enumerate(units):
            kind, lin = i % 2, units[(i + 1) % len(units)]
            probe = Case(f"{shape}-flip{u}-probe", "flip", o, d, 30, kind, "sum", 273, _spec(), seed=12 + i, obs_set=((u, 0.0),))
            x = reference(probe)["obs"][:, :, u]
            th = float(f"{np.median(np.abs(x).max(axis=1)):.3g}")
            for mode in ("sum", "best") if i == 0 else ("sum",):
                out.append(Case(f"{shape}-flip{u}-lin{lin}-k{kind}-{mode}", "flip", o, d, 30, kind, mode, 273,
                                O.CostSpec(0.1, lin, -1.0, u, 10.0, th), seed=12 + i, obs_set=((u, 0.0),),
                                what=f"flip on unit {u} at +-{th}, linear term on unit {lin}"))
    return out


def _program_cases():
    """Term lists that fill every slot of TileHN's compiled programs {0,2,0}, {0,4,1}, {1,1,4}: slice lengths 1, 3, 4, 5
    and 32 (28 at o = 28), starts at 0, 15, 16, 31 and o - len, difference slices across 16-blocks, a gate on a unit of
    another block, a negative threshold, a negative weight on a NORM; each list also in reversed order."""
    out = []
    for shape, (o, d) in HN_SHAPES.items():
        far = 31 if o > 32 else 27
        L = min(32, o)
        lists = {
            "p020": (T(NORM, 0, -1, 1, 0.7), T(NORM_LT, 15, o - 4, 4, -3.0, 0.5, gate_idx=far, gate_thresh=-0.05)),
            "p041": (T(NORM, 16, -1, 3, -0.2), T(SUMSQ, far, -1, 1, 0.5), T(NORM_GT, o - 4, 0, 4, 2.0, 0.55),
                     T(NORM, 15, o - 3, 3, 0.3, gate_idx=0, gate_thresh=0.1), T(STEP_GT, far, -1, 1, -1.5, -0.1)),
            "p114-len5": (T(NORM, 15, o - 5, 5, 0.4), T(NORM_GT, 0, 16, 3, 1.0, 0.4), T(STEP_GT, 16, -1, 1, 2.0, -0.15),
                          T(SQ_OFFSET, o - 1, -1, 1, 0.3, -0.4), T(STEP_GT, 15, -1, 1, -1.0, 0.1, gate_idx=far, gate_thresh=0.0),
                          T(SQ_OFFSET, 0, -1, 1, -0.2, 0.25)),
            "p114-len32": (T(SUMSQ, o - L, -1, L, 0.05), T(NORM, o - 1, -1, 1, 0.5, gate_idx=15, gate_thresh=0.0),
                           T(STEP_GT, 0, -1, 1, 1.0, 0.2), T(SQ_OFFSET, 16, -1, 1, 0.5, 0.3), T(STEP_GT, o - 1, -1, 1, -2.0, -0.2),
                           T(SQ_OFFSET, far, -1, 1, 0.1, -1.0)),
        }
        # every list in 'sum' in both orders, and the given order under a second reduction
        second = {"p020": "final", "p041": "best", "p114-len5": "final", "p114-len32": "best"}
        for i, (tag, terms) in enumerate(lists.items()):
            for order, tl, mode in (("fwd", terms, "sum"), ("rev", terms[::-1], "sum"), ("fwd", terms, second[tag])):
                kind = (i + (order == "rev")) % 2
                out.append(Case(f"{shape}-{tag}-{order}-k{kind}-{mode}", "programs", o, d, 30, kind, mode, 273, _spec(tl), seed=41 + i,
                                what=f"term list {tag} in {'the given' if order == 'fwd' else 'reversed'} order"))
    return out


SHIPPED_CASES = _shipped_cases()
ENV_CASES = _other_env_cases()
READOUT_CASES = _readout_cases()
CONTROL_CASES = _control_cases()
FLIP_CASES = _flip_cases()
PROGRAM_CASES = _program_cases()
CASES = SHIPPED_CASES + ENV_CASES + READOUT_CASES + CONTROL_CASES + FLIP_CASES + PROGRAM_CASES
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
