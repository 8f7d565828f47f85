"""The learned-dynamics MPC step (declared RSSM, DeviceRSSMModel) against the float64 oracle, iteration by iteration.

The fused entries icem_plan_step_learned / _batch are held bit for bit to the stage-wise loop of the controller
(test_gpu_learned_step.py); this module holds the stage-wise loop itself to ``oracle.icem_oracle.IcemOracle``.  The form
oracle_loop.py::full_loop has does not carry over: the RSSM kernel's costs differ from any CPU evaluation by bf16 rounding
flips (rssm_cases.py), a free-running oracle would pick other elites and the two loops would part.  So the costs are
TEACHER-FORCED: the oracle's ``rollout_cost`` hands back the costs the device computed for that iteration, its noise is the
device's own normals (oracle_loop.DeviceNormals), and every other stage then sees what the device saw:

- the pool of every iteration (main rows, row 0 = mean, shifted rows, row count) to oracle_loop.RTOL / ATOL;
- the elite index set over [pool | kept]: the oracle's, identical and in order (same numbers, ties by index), the recorded
  elite costs bit-equal to the device costs at those indices, the recorded elite rows bit-equal to the recorded pool rows
  resp. the previous iteration's recorded elites;
- mean / std after every refit, the executed action, the shifted mean and the reset std to RTOL / ATOL;
- last_min_cost == the minimum over the last pool and its kept elites, bit for bit.

The costs themselves are checked on the planner's own pools: against ``rssm_oracle.emulated_costs(q = bf16)`` under the
criterion of rssm_cases.py, row errors normalised per rollout call by that call's max|want| and pooled over the case.

:class:`ControllerRecorder` and :func:`record_operator_step` produce the record, :func:`check` is pure NumPy over it (the
CPU sensitivity test feeds it a NumPy stand-in for the device).  A record:
    dict(params=O.IcemParams, low, high, mode, steps=[step]),
    step = dict(obs, iters=[it], executed, last_min_cost, mean_end, std_end),
    it   = dict(mean0, std0, pool [rows, h, d], costs [rows], elite_actions [K, h, d], elite_costs [K], mean, std)
-- f32 values of the device held as they are (costs, elites: bit comparisons) and compared in float64.

Helper module of the suite (imported by tests, collects nothing itself).
"""
import numpy as np

import rssm_cases as RC
from oracle import icem_oracle as O
from oracle import rssm_oracle as RO
from oracle_loop import ATOL, RTOL


# ------------------------------------------------------------------------------------------------ the cases
# Keyword arguments of test_gpu_learned_step.controller (horizon, n, cost, asp: overrides of ASP) per case, shared by the
# GPU test and the CPU sensitivity test.  N = 128, factor_decrease_num = 1.25, 3 iterations: rows 128 (+ n_reuse shifted
# ones from the second step on), 102, 81.  The first block restates test_gpu_learned_step.VARIANTS (the GPU test asserts
# that it does).  ``criterion``: False where the reference pair itself breaks rssm_cases' share cap (sum / final at
# h = 30, see rssm_cases.py) -- such a case keeps every other assertion.  ``low`` / ``high``: through IcemPlanner directly.
ASP = dict(alpha=0.1, elites_size=10, opt_iterations=3, init_std=0.5, use_mean_actions=True, keep_previous_elites=True,
           shift_elites_over_time=True, fraction_elites_reused=0.3, noise_beta=0.25)
VARIANT_CASES = {
    "h12": dict(),
    "h10": dict(horizon=10),
    "n126_full_last_workgroup": dict(n=126),
    "no_keep": dict(asp=dict(keep_previous_elites=False)),
    "no_shift": dict(asp=dict(shift_elites_over_time=False)),
    "no_mean_row": dict(asp=dict(use_mean_actions=False)),
    "best": dict(cost="best"),
    "final": dict(cost="final"),
    "white": dict(asp=dict(noise_beta=0)),
}
LOW, HIGH = [-1, -.5, -.25, 0, -2, -1], [1, .25, .75, .5, 3, 0.1]
CASES = dict(VARIANT_CASES, **{
    # 'best' from the state the float64 network settles into (rssm_cases' "settled"): the minima spread over the steps --
    # from 0.3 N(0, 1), as in "best" above, they sit on steps 0 and 1 alone (step 0: one cost for all rows, exact ties)
    "best_settled": dict(cost="best", obs="settled"),
    "h30_best": dict(horizon=30, cost="best", obs="settled"),
    "h30_sum": dict(horizon=30, criterion=False),
    "k2_nothing_reused": dict(asp=dict(elites_size=2)),                       # n_reuse = 0: the oracle asks for an empty shifted batch
    "k32_half_reused": dict(asp=dict(elites_size=32, fraction_elites_reused=0.5)),   # 16 kept / shifted rows
    "alpha0": dict(asp=dict(alpha=0.0)),
    "alpha0.9": dict(asp=dict(alpha=0.9)),
    "n24_floor": dict(n=24),                                                   # populations 24, 20, 20: the 2 K floor is active
    "bounds": dict(low=LOW, high=HIGH),
})
N_STEPS = 5


def case_settings(name):
    """-> (horizon, n, cost, asp, low, high, criterion) of a case, defaults filled in."""
    kw = CASES[name]
    return dict(horizon=kw.get("horizon", 12), n=kw.get("n", 128), cost=kw.get("cost", "sum"), asp=dict(ASP, **kw.get("asp", {})),
                low=np.asarray(kw.get("low", [-1.0] * 6), np.float64), high=np.asarray(kw.get("high", [1.0] * 6), np.float64),
                criterion=kw.get("criterion", True))


def observations(n, seed=9):
    rs = np.random.RandomState(seed)
    return [0.3 * rs.randn(230) for _ in range(n)]


def settled_observation(P, seed, k=8):
    """The state the float64 network (parameters ``P``) reaches from 0.3 N(0, 1) after ``k`` steps of uniform actions."""
    rs = np.random.RandomState(seed)
    ob = 0.3 * rs.randn(1, 230)
    for _ in range(k):
        ob = RO.step(P, ob, rs.uniform(-1, 1, (1, 6)))
    return ob[0]


def first_observations(name, P, count=1, seed=9):
    """The first observation of ``count`` controllers of a case; step k plans from it + 0.01 k (:func:`step_observations`)."""
    if CASES[name].get("obs") == "settled":
        return [settled_observation(P, 13 + 7 * i) for i in range(count)]
    return observations(count, seed)


def step_observations(ob0, n_steps=N_STEPS):
    return [ob0 + 0.01 * k for k in range(n_steps)]


# ------------------------------------------------------------------------------------------------ recording
def host(t):
    return t.detach().cpu().numpy().copy()


def oracle_params(*, horizon, n, cost="sum", elites_size=10, opt_iterations=3, factor_decrease_num=1.25, alpha=0.1,
                  init_std=0.5, use_mean_actions=True, keep_previous_elites=True, shift_elites_over_time=True,
                  fraction_elites_reused=0.3, noise_beta=0.25):
    return O.IcemParams(horizon=horizon, num_simulated_trajectories=n, factor_decrease_num=factor_decrease_num,
                        cost_along_trajectory=cost, alpha=alpha, elites_size=elites_size, opt_iterations=opt_iterations,
                        init_std=init_std, use_mean_actions=use_mean_actions, keep_previous_elites=keep_previous_elites,
                        shift_elites_over_time=shift_elites_over_time, fraction_elites_reused=fraction_elites_reused,
                        noise_beta=noise_beta)


def new_record(params, low, high):
    return dict(params=params, low=np.asarray(low, np.float64), high=np.asarray(high, np.float64),
                mode=params.cost_along_trajectory, steps=[])


class ControllerRecorder:
    """Wraps the stage methods of ONE ``MpcICemHip`` on ``DeviceRSSMModel`` (on the instance: no library or controller code
    changes) and records what its stage-wise loop did.  :meth:`step` runs ``get_action`` under ``learned_step = 0``, which
    sends the controller down ``_get_action_stagewise``."""

    def __init__(self, ctrl):
        c = self.c = ctrl
        sp = dict(alpha=c.alpha, elites_size=c.elites_size, opt_iterations=c.opt_iter, init_std=c.init_std,
                  use_mean_actions=bool(c.use_mean_actions), keep_previous_elites=bool(c.keep_previous_elites),
                  shift_elites_over_time=bool(c.shift_elites_over_time), fraction_elites_reused=c.fraction_elites_reused,
                  noise_beta=c.noise_beta)
        space = c.env.action_space
        self.record = new_record(oracle_params(horizon=c.horizon, n=c.num_sim_traj, cost=c.cost_along_trajectory,
                                               factor_decrease_num=c.factor_decrease_num, **sp), space.low, space.high)
        self._its = None
        sample, costs_of, update, finish = c._stage_sample, c._costs_of, c._stage_update, c._stage_finish

        def stage_sample(i, noise, actions):
            assert i == len(self._its)
            it = dict(mean0=host(c.planner.mean), std0=host(c.planner.std))
            sample(i, noise, actions)
            it["pool"] = host(actions)
            self._its.append(it)

        def stage_costs(obs, actions):
            costs = costs_of(obs, actions)
            self._its[-1]["costs"] = host(costs)
            return costs

        def stage_update(i, costs, actions):
            update(i, costs, actions)
            self._its[i].update(elite_actions=host(c._elite_actions), elite_costs=host(c._elite_costs),
                                mean=host(c.planner.mean), std=host(c.planner.std))

        def stage_finish():
            out = finish()
            self._end = dict(mean_end=host(c.planner.mean), std_end=host(c.planner.std))
            return out

        c._stage_sample, c._costs_of, c._stage_update, c._stage_finish = stage_sample, stage_costs, stage_update, stage_finish

    def step(self, obs):
        from icem_amd import _lib as L
        self._its, self._end = [], None
        L.set_option("learned_step", 0)
        try:
            assert not self.c.planner.learned_step_ok()
            executed = self.c.get_action(obs, None)
        finally:
            L.set_option("learned_step", 1)
        assert self._end is not None and len(self._its) == self.c.opt_iter and self.c.planner.learned_step_launches == 0, \
            "the step did not go through the stage-wise loop"
        self.record["steps"].append(dict(obs=np.asarray(obs, np.float64).copy(), iters=self._its, executed=np.asarray(executed).copy(),
                                         last_min_cost=self.c.last_min_cost, **self._end))
        return executed


def record_operator_step(record, p, m, ob, elites, *, use_mean=True, keep=True, shift=True, mode=0):
    """``MpcICemHip._get_action_stagewise``'s operators in its order on a bare planner ``p`` (as
    test_gpu_learned_step.py::operator_step), recorded into ``record``.  ``elites`` = (actions, costs) of the step before
    or None.  -> (executed | best cost [d + 1] on the host, elites of the last iteration, elites of the one before)."""
    import torch
    it_n = p.cfg.opt_iters
    base = p.noise_offset(p.mpc_step * (it_n + 1))
    before, its = None, []
    for i, n_i in enumerate(p.population_sizes):
        shifted = i == 0 and shift and elites is not None and p.n_reuse > 0
        it = dict(mean0=host(p.mean), std0=host(p.std))
        acts = torch.empty((n_i + (p.n_reuse if shifted else 0), p.h, p.d), dtype=p.dt, device=p.device)
        p.sample_clip(n_i, p.mean, p.std, offset=base + i, row0_mean=bool(use_mean and i == it_n - 1), out=acts[:n_i])
        if shifted:
            acts[n_i:, :-1] = elites[0][:p.n_reuse, 1:]
            p.sample_clip(p.n_reuse, p.mean, p.std, offset=base + it_n, t_begin=p.h - 1, out=acts[n_i:])
        costs = m.rollout_cost(ob, acts, mode)
        kept = i > 0 and keep and p.n_reuse > 0
        before = elites
        ec, _, ea = p.update_distribution(costs, acts, p.K, p.mean, p.std, elites[1][:p.n_reuse] if kept else None,
                                          elites[0][:p.n_reuse] if kept else None)
        elites = (ea, ec)
        it.update(pool=host(acts), costs=host(costs), elite_actions=host(ea), elite_costs=host(ec), mean=host(p.mean), std=host(p.std))
        its.append(it)
    p.shift(p.mean, p.std)
    p.mpc_step += 1
    out = host(torch.cat([elites[0][0, 0], elites[1][:1]]))
    record["steps"].append(dict(obs=np.asarray(ob, np.float64).copy(), iters=its, executed=out[:-1].astype(np.float64),
                                last_min_cost=float(out[-1]), mean_end=host(p.mean), std_end=host(p.std)))
    return out, elites, before


class EpisodeNormals:
    """What oracle_loop.DeviceNormals asks of a planner, with the planner's current episode folded into every offset."""

    def __init__(self, planner):
        self.pl, self.F, self.d, self.h = planner, planner.F, planner.d, planner.h

    def philox_normals(self, num, offset=0):
        return self.pl.philox_normals(num, offset=self.pl.noise_offset(offset))


# ------------------------------------------------------------------------------------------------ checking
class LoopMismatch(AssertionError):
    """``failures``: [(tag, what, factor)] -- factor None: an exact property (shape, index set, bits) does not hold;
    a number: a tolerance is missed by that factor.  ``factor``: None if any exact property fails, else the largest miss."""

    def __init__(self, failures):
        self.failures = failures
        self.exact = any(f is None for _, _, f in failures)
        self.factor = None if self.exact else max(f for _, _, f in failures)
        super().__init__("%d mismatches, the first: %r%s" % (len(failures), failures[:4], "" if self.exact else
                                                            "; worst tolerance miss x %.3g" % self.factor))


def _miss(got, want):
    """By what factor ``got`` misses ``|got - want| <= ATOL + RTOL |want|`` (<= 1: it holds)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return None
    r = np.abs(got - want) / (ATOL + RTOL * np.abs(want))
    r = np.where(np.isfinite(r), r, np.inf)
    return float(r.max()) if r.size else 0.0


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b)


def cost_rows(P, record, exact=False):
    """(got, want) of every simulated row of the record, each rollout call divided by that call's max|want|: the float64
    emulation of the kernel's rounding points on the RECORDED pool (``exact``: the float64 network itself, undivided)."""
    got, want = [], []
    for st in record["steps"]:
        for it in st["iters"]:
            w = RO.emulated_costs(P, st["obs"], it["pool"].astype(np.float64), record["mode"], **({} if exact else dict(q=RO.bf16)))
            scale = 1.0 if exact else np.abs(w).max()
            got.append(it["costs"].astype(np.float64) / scale)
            want.append(w / scale)
    return np.concatenate(got), np.concatenate(want)


def check(record, noise, P=None, cost_criterion=True):
    """The checks of the module docstring over ``record``.  ``noise``: the oracle's noise callback with ``begin_step()``
    (oracle_loop.DeviceNormals on the device's normals; PhiloxNoiseSchedule for a stand-in).  ``P``: the float64 parameters
    of the model (rssm_oracle.params_from_state_dict) -- given: the costs are compared with the emulation on the recorded
    pools, under rssm_cases' criterion where ``cost_criterion`` and the loose 5e-2 (1 + max|exact|) bound always.
    Raises :class:`LoopMismatch` naming every failure; -> dict of the worst deviations (and the pooled cost statistics)."""
    p, low, high = record["params"], record["low"], record["high"]
    K, iters = p.num_elites, p.opt_iterations
    fails, worst = [], dict(pool=0.0, mean=0.0, std=0.0, end=0.0)
    cursor = {}

    def recorded_costs(ob, actions):
        it = record["steps"][cursor["s"]]["iters"][cursor["i"]]
        cursor["i"] += 1
        if it["costs"].shape != (actions.shape[0],):
            raise LoopMismatch([(f"step {cursor['s']} iteration {cursor['i'] - 1}", "rows: recorded %d, oracle %d"
                                 % (len(it["costs"]), actions.shape[0]), None)])
        return it["costs"].astype(np.float64)

    def close(tag, what, got, want, key=None):
        f = _miss(got, want)
        if key is not None and f is not None:
            worst[key] = max(worst[key], float(np.abs(np.asarray(got, np.float64) - want).max()) if np.size(want) else 0.0)
        if f is None or not f <= 1:
            fails.append((tag, what, f))

    def exact(tag, what, ok):
        if not ok:
            fails.append((tag, what, None))

    orc = O.IcemOracle(p, low, high, recorded_costs, noise)
    orc.beginning_of_rollout()
    for s, st in enumerate(record["steps"]):
        if s:
            noise.begin_step()
        cursor.update(s=s, i=0)
        exact(f"step {s}", "iterations recorded", len(st["iters"]) == iters)
        mean_in, std_in = orc.mean.copy(), orc.std.copy()
        want = orc.get_action(st["obs"])
        prev = record["steps"][s - 1]["iters"][-1] if s else None
        for i, (dev, ref) in enumerate(zip(st["iters"], orc.trace[-1])):
            tag = f"step {s} iteration {i}"
            close(tag, "mean before the iteration", dev["mean0"], mean_in, "mean")
            close(tag, "std before the iteration", dev["std0"], std_in, "std")
            mean_in, std_in = ref.mean, ref.std
            # the pool: main rows, row 0 = mean on the last iteration, shifted rows behind them, the row count
            close(tag, "pool", dev["pool"], ref.actions, "pool")
            exact(tag, "pool inside the bounds (as f32 holds them)",
                  bool(np.all((dev["pool"] >= low.astype(np.float32)) & (dev["pool"] <= high.astype(np.float32)))))
            # elites: over the device costs of [pool | kept], the oracle's own index set, in order
            n_keep = len(ref.costs) - len(ref.actions)
            exact(tag, "kept elites without a previous set", n_keep == 0 or prev is not None)
            all_costs = dev["costs"] if not n_keep else np.concatenate([dev["costs"], prev["elite_costs"][:n_keep]])
            idx = O.topk_sorted(all_costs.astype(np.float64), K)
            exact(tag, "elite index set", _same(idx, ref.elite_idx))
            exact(tag, "elite costs are the device costs at the elite indices", _same(dev["elite_costs"], all_costs[idx]))
            rows = dev["pool"] if not n_keep else np.concatenate([dev["pool"], prev["elite_actions"][:n_keep]])
            exact(tag, "elite rows are the pool's / the kept elites' rows", _same(dev["elite_actions"], rows[idx]))
            close(tag, "mean after the refit", dev["mean"], ref.mean, "mean")
            close(tag, "std after the refit", dev["std"], ref.std, "std")
            prev = dev
        tag = f"step {s} end"
        close(tag, "executed action", st["executed"], want, "end")
        close(tag, "shifted mean", st["mean_end"], orc.mean, "end")
        close(tag, "reset std", st["std_end"], orc.std, "end")
        exact(tag, "last_min_cost", np.float32(st["last_min_cost"]) == all_costs.min() and float(all_costs.min()) == orc.last_min_cost)
    out = dict(worst)
    if P is not None and not fails:
        got, want = cost_rows(P, record)
        out.update(cost=RC.errors(got, want), rows=len(got))
        if cost_criterion:
            bad = RC.violations(got, want)
            if bad:
                fails.append(("costs", "; ".join(bad), None))
        got, ex = cost_rows(P, record, exact=True)
        if not np.abs(got - ex).max() <= 5e-2 * (1 + np.abs(ex).max()):
            fails.append(("costs", "bf16 accuracy against the network itself", float(np.abs(got - ex).max() / (5e-2 * (1 + np.abs(ex).max())))))
    if fails:
        raise LoopMismatch(fails)
    return out
