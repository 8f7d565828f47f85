"""Shapes, problem layouts, the comparison and a NumPy stand-in shared by test_gpu_mlp_models.py and
test_mlp_models_sensitivity_cpu.py (a plain module, no fixtures): what icem_mlp_rollout_cost_models / _ensemble are run on, and
when a launch counts as right.

The contract is bit for bit: a tile holds 16 rows of ONE problem in the problem's own order and an MFMA column depends only on
its own trajectory, so every cost and every state of every problem is what the solo launch gives that problem alone.  The
comparison (``launch_mismatches`` / ``ensemble_mismatches``) therefore takes no tolerance: ``np.array_equal`` per problem against
the problem's own solo result -- on the GPU ``DeviceMLPModel.rollout_cost(..., return_observations=True)``, on the CPU the
stand-in run on one problem.

The stand-in (``Standin.launch``) walks the launch as the kernel does -- problem by problem, tile by tile, 16 rows with the
padding rows of a problem's last tile repeating its last row, costs and states stored at the problem's cost base -- on
mlp_cases.kernel_standin's arithmetic (float32, bf16 operands, K blocked by 32; no activation noise: a row is computed alone,
so its bits do not depend on its neighbours, as an MFMA column's do not) and mlp_cases.costs_f32.  ``fault=`` plants one single
fault; test_mlp_models_sensitivity_cpu.py shows that the comparison accepts the faithful stand-in and rejects every fault on the
layouts below.
"""
from collections import namedtuple

import numpy as np

import mlp_cases as MC
from oracle import icem_oracle as O
from oracle.rssm_oracle import bf16

MODE_NAMES = ["sum", "best", "final"]   # cost_mode 0, 1, 2

# ---- shapes: mlp_cases' table entries (their gains), at the widths, depths and activations the kernel instantiates --------------
# o = 17 (one state K block) and 33 (two), d = 1 and 6, L = 1, 2 and 4, relu and swish, h = 2 and 12
Shape = namedtuple("Shape", "name case h")


def _shape(name, base, h, **over):
    return Shape(name, MC.BY_NAME[base]._replace(name=name, h=h, **over), h)


SHAPES = [
    _shape("o17d6-L2-relu-h12", "o17d6-L2-relu-1007x12", 12),
    _shape("o33d6-L2-relu-h12", "o33d6-L2-relu-333x12", 12),
    _shape("o17d6-L1-swish-h2", "o17d6-L1-swish-13x2", 2),
    _shape("o33d1-L4-swish-h12", "o39d6-L4-swish-333x12", 12, o=33, d=1),
    _shape("o17d1-L4-relu-h2", "o64d6-L4-relu-333x12", 2, o=17, d=1),
]
SHAPE_BY_NAME = {s.name: s for s in SHAPES}
HOPPER = MC.COST_ENV_BY_NAME["hopper"]   # o = 12, d = 3: the difference term (reads s_h), the health term and its box


def plain_spec(o):
    """A HalfCheetah-shaped cost at any width >= 9: control, forward velocity, flip penalty (no term list)."""
    return O.CostSpec(0.1, 8, -1.0, 1, 10.0, 0.7)


def shape_module(shape, k):
    """Model k of a shape: the table entry's module from another weight seed (f32 torch module, CPU)."""
    return MC.module(shape.case._replace(wseed=shape.case.wseed + 40 * k))


def hopper_module(k):
    return MC.cost_module(HOPPER._replace(name=f"hopper-model{k}", wseed=HOPPER.wseed + 40 * k))


# ---- layouts: the problems of a launch ------------------------------------------------------------------------------------------
# problem = (model, obs_row, action_row0, rows); the costs (and states) of problem p start at sum(rows[:p])
Layout = namedtuple("Layout", "name problems n_models n_obs n_action_rows")


def _back_to_back(rows):
    return [int(sum(rows[:p])) for p in range(len(rows))]


def _layout(name, rows, models=None, obs_rows=None, action_row0=None, n_obs=None, n_action_rows=None):
    B = len(rows)
    models = list(range(B)) if models is None else models
    obs_rows = list(range(B)) if obs_rows is None else obs_rows
    action_row0 = _back_to_back(rows) if action_row0 is None else action_row0
    n_action_rows = max(a + r for a, r in zip(action_row0, rows)) if n_action_rows is None else n_action_rows
    return Layout(name, [tuple(int(v) for v in q) for q in zip(models, obs_rows, action_row0, rows)], max(models) + 1,
                  max(obs_rows) + 1 if n_obs is None else n_obs, n_action_rows)


LAYOUTS = [
    # every row count around a tile edge in one launch; the start observations a permutation that is not the identity, n_obs > B
    _layout("mixed-1-15-16-17-33", [1, 15, 16, 17, 33], obs_rows=[3, 0, 6, 1, 4], n_obs=7),
    _layout("one-17", [17]),
    # a problem behind a 17-row neighbour (its cost base is 17, not 32), one row of action slack behind the last problem
    _layout("two-17-5", [17, 5], obs_rows=[1, 0], n_action_rows=23),
    # overlapping action rows: problem 1 sits inside problem 0's, problem 2 straddles its end
    _layout("three-overlap", [16, 1, 33], action_row0=[0, 7, 10], obs_rows=[2, 0, 1], n_obs=4),
    # all coinciding (an ensemble's layout), one model serving two problems beside a different one
    _layout("three-coincide", [17, 17, 17], models=[0, 1, 0], action_row0=[0, 0, 0], obs_rows=[0, 0, 1]),
    # a full table: 32 problems of 1 .. 17 rows, four models, eight observations
    _layout("thirty-two", [1 + (5 * p) % 17 for p in range(32)], models=[p % 4 for p in range(32)],
            obs_rows=[(3 * p + 1) % 8 for p in range(32)]),
]
LAYOUT_BY_NAME = {l.name: l for l in LAYOUTS}


def inputs(o, d, h, layout, seed=0):
    """(obs table [n_obs, o], actions [n_action_rows, h, d]) of a launch: float32 arrays."""
    rs = np.random.RandomState(1000 + seed)
    return (0.5 * rs.randn(layout.n_obs, o)).astype(np.float32), rs.uniform(-1, 1, (layout.n_action_rows, h, d)).astype(np.float32)


# ---- the comparison ---------------------------------------------------------------------------------------------------------------
def launch_mismatches(costs, states, problems, solo) -> list:
    """What is wrong with a launch's ``costs [sum rows]`` and ``states [sum rows, h + 1, o]`` (None: not asked for):
    problem p's slice must be ``solo(p) -> (costs [rows], states [rows, h + 1, o])`` bit for bit.  [] when nothing is."""
    total = sum(q[3] for q in problems)
    costs = np.asarray(costs)
    if costs.shape != (total,):
        return [f"costs {costs.shape} instead of ({total},)"]
    out, at = [], 0
    for p, q in enumerate(problems):
        want_c, want_s = solo(p)
        want_c = np.asarray(want_c)
        assert want_c.shape == (q[3],) and np.isfinite(want_c).all(), (p, want_c.shape)
        if not np.array_equal(costs[at:at + q[3]], want_c):
            out.append(f"problem {p} {q}: costs differ in rows {np.flatnonzero(costs[at:at + q[3]] != want_c)[:4].tolist()}")
        if states is not None:
            got_s, want_s = np.asarray(states)[at:at + q[3]], np.asarray(want_s)
            if got_s.shape != want_s.shape:
                out.append(f"problem {p} {q}: states {got_s.shape} instead of {want_s.shape}")
            elif not np.array_equal(got_s, want_s):
                out.append(f"problem {p} {q}: states differ in rows {np.flatnonzero((got_s != want_s).any(axis=(1, 2)))[:4].tolist()}")
        at += q[3]
    return out


def reduce_restatement(member_costs, reduce) -> np.ndarray:
    """icem_rssm_ensemble_reduce in float32 NumPy: the members in the order 0, 1, ..; mean: ((c0 + c1) + ..) * float32(1 / E);
    max: the worst member, a NaN member makes the row NaN."""
    mc = np.asarray(member_costs, np.float32)
    acc = mc[0].copy()
    for c in mc[1:]:
        acc = acc + c if reduce == "mean" else np.where((c > acc) | np.isnan(c), c, acc)
    return (acc * np.float32(1.0 / len(mc))).astype(np.float32) if reduce == "mean" else acc


def ensemble_mismatches(member_costs, costs, solo_member_costs, reduce) -> list:
    """``member_costs [E, n]`` must be the members' own solo costs, ``costs [n]`` the restated reduction of them -- bit for bit,
    NaN rows included."""
    mc, want = np.asarray(member_costs), np.asarray(solo_member_costs)
    if mc.shape != want.shape:
        return [f"member_costs {mc.shape} instead of {want.shape}"]
    out = [f"member {e} differs from its solo costs" for e in range(len(want)) if not np.array_equal(mc[e], want[e], equal_nan=True)]
    if not np.array_equal(np.asarray(costs), reduce_restatement(want, reduce), equal_nan=True):
        out.append(f"costs are not the restated {reduce} of the members")
    return out


# ---- the stand-in -------------------------------------------------------------------------------------------------------------------
SENTINEL = np.float32(-12345.0)   # what a buffer holds where nothing was stored


class Standin:
    """A launch on the CPU.  ``params``: the models' float64 parameter dicts (mlp_cases.params_of); ``spec``: the cost."""

    def __init__(self, params, spec, obs, actions, mode="sum"):
        self.params, self.spec, self.obs, self.actions, self.mode = params, spec, np.asarray(obs), np.asarray(actions), mode
        self.h, self.o = self.actions.shape[1], self.obs.shape[1]
        self._rows = {}

    def row(self, model, obs_row, action_row):
        """(cost, states [h + 1, o]) of one trajectory, computed alone."""
        key = (model, obs_row, action_row)
        if key not in self._rows:
            a = self.actions[action_row:action_row + 1].astype(np.float64)
            s = MC.emulated_states(self.params[model], self.obs[obs_row].astype(np.float64), a, q=bf16, dtype=np.float32, kblock=32)
            c = MC.costs_f32(self.spec, self.mode, s, a).astype(np.float32)
            self._rows[key] = (c[0], s[0].astype(np.float32))
        return self._rows[key]

    def launch(self, problems, fault=None):
        """-> (costs [sum rows], states [sum rows, h + 1, o]) as the kernel lays them out; ``fault``: one of FAULTS."""
        total, per = sum(q[3] for q in problems), (self.h + 1) * self.o
        stride = self.h * self.o if fault == "states-stride-h" else per
        room = 16 * sum((q[3] + 15) // 16 for q in problems) + 16   # (a faulty launch stores past the end: the buffers have slack)
        costs = np.full(room, SENTINEL, np.float32)
        states = np.full(room * per, SENTINEL, np.float32)
        bases, at = [], 0
        for q in problems:
            bases.append(at)
            at += 16 * ((q[3] + 15) // 16) if fault == "cost-base-16" else q[3]
        order = range(len(problems))
        for p in (reversed(order) if fault == "padding-from-neighbour" else order):   # (the stray stores land last)
            model, obs_row, a0, rows = problems[p]
            model = problems[0][0] if fault == "params-of-problem-0" else model
            obs_row = p % len(self.obs) if fault == "obs-row-ignored" else obs_row
            a0 = 0 if fault == "action-row0-ignored" else a0
            for tile in range((rows + 15) // 16):
                if fault == "last-tile-dropped" and 16 * tile + 16 > rows:
                    continue
                for j in range(16):
                    r = 16 * tile + j
                    if r >= rows and fault != "padding-from-neighbour":
                        continue   # a padding row repeats the problem's last row and is never stored
                    c, s = self.row(model, obs_row, min(a0 + r, len(self.actions) - 1))
                    costs[bases[p] + r] = c
                    states[(bases[p] + r) * stride:(bases[p] + r) * stride + per] = s.ravel()
        return costs[:total], states[:total * per].reshape(total, self.h + 1, self.o)

    def solo(self, problems):
        """solo(p) for launch_mismatches: problem p as a launch of its own."""
        def run(p):
            model, obs_row, a0, rows = problems[p]
            return self.launch([(model, obs_row, a0, rows)])
        return run

    def batch(self, planner_rows, members, fault=None):
        """DeviceMLPEnsemble.rollout_cost_batch's launch: planners back to back in the actions, planner b from observation b,
        B x E problems in member-major order -> member_costs [E, sum rows]."""
        row0, B = _back_to_back(planner_rows), len(planner_rows)
        if fault == "problem-major":
            problems = [(e, b, row0[b], planner_rows[b]) for b in range(B) for e in range(members)]
        else:
            problems = [(e, b, row0[b], planner_rows[b]) for e in range(members) for b in range(B)]
        return self.launch(problems)[0].reshape(members, sum(planner_rows))


def standin_reduce(member_costs, reduce, fault=None) -> np.ndarray:
    """The reduction launch on the CPU, with its two single faults."""
    mc = np.asarray(member_costs, np.float32)
    if fault == "mean-divides-first":
        inv, acc = np.float32(1.0 / len(mc)), mc[0] * np.float32(1.0 / len(mc))
        for c in mc[1:]:
            acc = acc + c * inv
        return acc.astype(np.float32)
    if fault == "max-ignores-nan":
        acc = mc[0].copy()
        for c in mc[1:]:
            acc = np.fmax(acc, c)
        return acc
    return reduce_restatement(mc, reduce)


LAUNCH_FAULTS = ["params-of-problem-0", "obs-row-ignored", "action-row0-ignored", "cost-base-16", "padding-from-neighbour",
                 "last-tile-dropped", "states-stride-h"]
