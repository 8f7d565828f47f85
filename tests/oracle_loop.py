"""The whole-loop comparison of the f32 planner with the float64 oracle, at any shape the C ABI accepts.

The one part of the device loop the float64 oracle cannot restate bit for bit is the Box-Muller transform on the hardware
transcendentals; :class:`DeviceNormals` takes it out of the comparison by handing the oracle the DEVICE's own f32 normals
(``icem_philox_normals``), call for call.  :func:`full_loop` then checks every iteration of every MPC step:

- the sampled pool to 1e-5;
- every trajectory cost to 1e-5 of its magnitude (``oracle.rollout_cost_magnitudes``);
- the elite index set, identical to the oracle's;
- the gathered elite rows, bit for bit;
- mean, std and the executed action to 1e-5;

and that the launches ``icem_plan_step`` makes (merges folded into the next launch) reproduce the split run bit for bit.

An f32 state may land on the other side of a flip / health / indicator threshold where the float64 state lies within the
f32 error of it: :func:`near_threshold` names those trajectories.  Only they may differ, only by whole penalties, and how
many there were is returned for the caller to bound and report.

Helper module of the suite (imported by tests, collects nothing itself).
"""
import json

import numpy as np
import torch

from oracle import icem_oracle as O

RTOL, ATOL = 1e-5, 2e-6  # north_star: 1e-5 relative; the floor covers entries near zero (actions live in [-1, 1])


def np_(t):
    return t.detach().cpu().numpy().astype(np.float64)


class DeviceNormals:
    """Noise callback for the oracle that hands it the device's own f32 normals, call for call (the offsets of
    :class:`oracle.icem_oracle.PhiloxNoiseSchedule`)."""

    def __init__(self, planner, iters, shift=True, white=False):
        self.pl, self.iters, self.shift, self.white = planner, iters, shift, white
        self.step = -1
        self.begin_step()

    def begin_step(self):
        self.step += 1
        self.it = 0
        self.shift_done = False

    def __call__(self, num):
        base = self.step * (self.iters + 1)
        if self.shift and self.step > 0 and self.it == 1 and not self.shift_done:
            self.shift_done = True
            off = base + self.iters
        else:
            off = base + self.it
            self.it += 1
        if num == 0:   # (no elite is reused at K = 2: the oracle still asks for the empty shifted batch)
            F = self.pl.F
            return np.zeros((0, self.pl.d, F)), np.zeros((0, self.pl.d, F))
        z_r, z_i = self.pl.philox_normals(num, offset=off)
        z_r, z_i = np_(z_r), np_(z_i)
        if self.white:
            F = self.pl.F
            g = np.concatenate([z_r, z_i[..., 1:1 + (self.pl.h - F)]], axis=-1)
            return np.ascontiguousarray(g.transpose([0, 2, 1])), None
        return z_r, z_i


# ------------------------------------------------------------------------------------------------ thresholds
def _indicator_values(oc, obs):
    """(value, threshold) pairs of every indicator the cost evaluates on a state [P, o]: the flip term (+-thresh), the health
    interval and box, and the thresholds and gates of the term list."""
    out = []
    if oc.flip_idx >= 0 and oc.flip_penalty != 0:
        v = obs[:, oc.flip_idx]
        out += [(v, oc.flip_thresh), (v, -oc.flip_thresh)]
    if oc.health_idx >= 0 and oc.health_penalty != 0:
        v = obs[:, oc.health_idx]
        out += [(v, oc.health_lo), (v, oc.health_hi)]
        if oc.box_from >= 0:
            for k in range(oc.box_from, obs.shape[1]):
                out += [(obs[:, k], oc.box_lo), (obs[:, k], oc.box_hi)]
    for tm in oc.terms:
        if tm.kind == O.TERM_STEP_GT:
            out.append((obs[:, tm.a], tm.thresh))
        elif tm.kind in (O.TERM_NORM_GT, O.TERM_NORM_LT):
            acc = np.zeros(obs.shape[0], dtype=obs.dtype)
            for m in range(tm.len):
                v = obs[:, tm.a + m] - (obs[:, tm.b + m] if tm.b >= 0 else 0)
                acc = acc + v * v
            out.append((np.sqrt(acc), tm.thresh))
        if tm.gate_idx >= 0:
            out.append((obs[:, tm.gate_idx], tm.gate_thresh))
    return out


def near_threshold(om, oc, obs0, actions, safety=16.0):
    """Boolean [P]: trajectories whose float64 state lies within the f32 error bound of one of the cost's thresholds at
    some step.  The bound is ``safety`` x the distance between the float64 rollout and its f32 restatement (the same
    operations in f32, another summation order than the device's) plus 2^-20 of the value's and the threshold's size."""
    actions = np.asarray(actions, dtype=np.float64)
    P, h, _ = actions.shape
    x64 = np.broadcast_to(np.asarray(obs0, np.float64), (P, len(obs0))).copy()
    x32 = x64.astype(np.float32)
    a32 = actions.astype(np.float32)
    near = np.zeros(P, bool)
    for t in range(h):
        for (v64, th), (v32, _) in zip(_indicator_values(oc, x64), _indicator_values(oc, x32)):
            with np.errstate(invalid="ignore"):
                bound = safety * np.abs(v64 - v32.astype(np.float64)) + 2.0 ** -20 * (np.abs(v64) + abs(th))
                near |= ~(np.abs(v64 - th) > bound)
        x64 = om.predict(x64, actions[:, t])
        x32 = om.predict(x32, a32[:, t])
    return near


def penalty_quanta(oc):
    """The whole penalties a threshold crossing can move a step's cost by."""
    q = [abs(oc.flip_penalty)] if oc.flip_idx >= 0 else []
    if oc.health_idx >= 0:
        q.append(abs(oc.health_penalty))
    q += [abs(tm.weight) for tm in oc.terms if tm.kind in (O.TERM_STEP_GT, O.TERM_NORM_GT, O.TERM_NORM_LT) or tm.gate_idx >= 0]
    return [x for x in q if x > 0]


def whole_penalties(diff, quanta, tol):
    """True where ``diff`` is a sum of whole penalties (each used up to 64 times) to within ``tol``."""
    diff = np.abs(np.asarray(diff, np.float64))
    ok = diff <= tol
    if not quanta:
        return ok
    quanta = sorted(set(quanta))[:3]   # (combinations of at most three distinct penalties)
    sums = {0.0}
    for q in quanta:
        sums = {s + k * q for s in sums for k in range(65)}
    sums = np.array(sorted(sums))
    dist = np.min(np.abs(diff[:, None] - sums[None, :]), axis=1)
    return ok | (dist <= tol)


def check_costs(got, want, mag, rtol, near, quanta, tag):
    """Every cost within ``rtol`` of its magnitude, except trajectories ``near`` a threshold, which may differ by whole
    penalties.  Returns the number of trajectories that did."""
    got = np.asarray(got, np.float64)
    assert np.all(np.isfinite(got)), tag
    err = np.abs(got - want)
    bad = err > rtol * mag
    stray = bad & ~near
    if stray.any():
        w = int(np.argmax(np.where(stray, err - rtol * mag, -np.inf)))
        raise AssertionError((tag, "cost off the bar away from any threshold", w, err[w], mag[w], want[w]))
    if bad.any():
        assert np.all(whole_penalties(err[bad], quanta, rtol * (mag[bad] + max(quanta)))), \
            (tag, "near-threshold cost off by other than whole penalties", err[bad])
    return int(bad.sum())


# ------------------------------------------------------------------------------------------------ the loop
def record(row):
    """One JSON line on stdout (``pytest -s``): what a case excluded, for the record."""
    print("[record]", json.dumps(row))


def full_loop(mk, om, oc, *, N, iters, h, o, beta, cost_mode, low, high, elites_size=10, keep=True, shift=True,
              use_mean=True, rtol=None, n_steps=2, obs_scale=0.1, obs_seed=100, expect_arith=None, on_iter_record=None,
              allow_near=False, max_near=None):
    """f32 planner vs the float64 oracle fed the device's normals (module docstring).  ``mk()`` returns a freshly reset
    planner of the configuration (three are made: split API, ``icem_plan_step``, and one that only draws the normals).
    ``on_iter_record(tag, err, cost, mag, planner)`` sees every iteration's costs.  ``allow_near``: trajectories near a
    threshold (:func:`near_threshold`) may differ by whole penalties -- returns how many did (``max_near`` bounds it per
    iteration); otherwise every cost is held to the bar."""
    RTOL_C = rtol if rtol is not None else RTOL   # (costs; mean / std / actions keep the module's RTOL)
    split, fused, rng = mk(), mk(), mk()
    if expect_arith is not None:
        assert split.tile_arith == expect_arith
    noise = DeviceNormals(rng, iters, shift=shift)
    low, high = np.asarray(low, np.float64), np.asarray(high, np.float64)
    orc = O.IcemOracle(O.IcemParams(horizon=h, num_simulated_trajectories=N, opt_iterations=iters, noise_beta=beta,
                                    elites_size=elites_size, keep_previous_elites=keep, shift_elites_over_time=shift,
                                    use_mean_actions=use_mean),
                       low, high, lambda ob, ac: O.rollout_costs(om, oc, ob, ac, mode=cost_mode), noise)
    orc.beginning_of_rollout()
    K, n_reuse = split.K, split.n_reuse
    assert K == orc.p.num_elites
    quanta = penalty_quanta(oc) if allow_near else []
    n_near = 0
    for s in range(n_steps):
        obs = obs_scale * np.random.RandomState(obs_seed + s).randn(o)
        if s:
            noise.begin_step()
        want = orc.get_action(obs)
        trace = orc.trace[-1]
        seen = []

        def on_iteration(it):
            n_it = split.population_sizes[it]
            n_extra = n_reuse if (it == 0 and s > 0 and shift) else 0
            n_keep = n_reuse if (it > 0 and keep) else 0
            g = (s * iters + it) & 1  # elite buffer the merge of this iteration read (the previous set) ...
            pool_costs = split.costs[:n_it + n_extra]
            if n_keep:
                pool_costs = torch.cat([pool_costs, split.elites_costs[g][:n_keep]])
            seen.append(dict(costs=pool_costs.cpu().numpy().copy(),
                             actions=np_(split.actions[:n_it + n_extra]),
                             elites=np_(split.elites_actions[g ^ 1]), elite_costs=np_(split.elites_costs[g ^ 1]),
                             mean=None if it == iters - 1 else np_(split.mean), std=None if it == iters - 1 else np_(split.std)))

        got_split = np_(split.plan_step(obs, on_iteration=on_iteration)).copy()
        got_fused = np_(fused.plan_step(obs)).copy()
        kept_mag = np.zeros(0)
        kept_near = np.zeros(0, bool)
        assert len(seen) == len(trace) == iters
        for it, (dev, ref) in enumerate(zip(seen, trace)):
            tag = f"step {s} iteration {it}"
            # the sampled pool (inverse DFT + affine + clip on the device's normals)
            np.testing.assert_allclose(dev["actions"], ref.actions, rtol=RTOL, atol=ATOL, err_msg=tag)
            # every trajectory cost, not only the elites': within 1e-5 of the magnitude of the sum it is (kept elites
            # behind the simulated rows carry cost and magnitude over from the iteration that simulated them)
            mag = np.concatenate([O.rollout_cost_magnitudes(om, oc, obs, ref.actions), kept_mag])
            assert mag.shape == ref.costs.shape, tag
            near = np.concatenate([near_threshold(om, oc, obs, ref.actions) if quanta else np.zeros(len(ref.actions), bool),
                                   kept_near])
            err = np.abs(dev["costs"].astype(np.float64) - ref.costs)
            if quanta:
                moved = check_costs(dev["costs"], ref.costs, mag, RTOL_C, near, quanta, tag)
                if max_near is not None:
                    assert moved <= max_near, (tag, moved, int(near.sum()))
                n_near += moved
            else:
                worst = int(np.argmax(err - RTOL_C * mag))
                assert err[worst] <= RTOL_C * mag[worst], (tag, worst, err[worst], mag[worst], ref.costs[worst])
                assert np.all(np.isfinite(dev["costs"])), tag
            if on_iter_record is not None:
                on_iter_record(tag, err, ref.costs, mag, split)
            if keep:   # (the next iteration's pool ends in the best n_reuse elites of this one: icem.py:143-145)
                kept_mag = mag[ref.elite_idx[:n_reuse]]
                kept_near = near[ref.elite_idx[:n_reuse]]
            # device top-K == sorted order of the device's own costs (ties by index), bit for bit ...
            idx_dev = O.topk_sorted(dev["costs"], K)
            assert np.array_equal(dev["elite_costs"], dev["costs"][idx_dev].astype(np.float64)), tag
            # ... and the SAME elite index set as the float64 oracle's (north_star: elite index sets bit-exact); inside the
            # set two elites may trade places only where their float64 costs agree to 1e-5
            assert set(idx_dev.tolist()) == set(ref.elite_idx.tolist()), (tag, idx_dev, ref.elite_idx)
            moved = idx_dev != ref.elite_idx
            assert np.all(np.abs(ref.costs[idx_dev[moved]] - ref.costs[ref.elite_idx[moved]]) <= RTOL_C * mag[idx_dev[moved]]), tag
            if it == iters - 1:
                assert idx_dev[0] == ref.elite_idx[0], tag  # the executed action comes from the same trajectory
            pool = dev["actions"]
            sim = idx_dev < pool.shape[0]
            assert np.array_equal(dev["elites"][sim], pool[idx_dev[sim]]), tag  # gathered rows, bit-exact
            if dev["mean"] is not None:
                np.testing.assert_allclose(dev["mean"], ref.mean, rtol=RTOL, atol=ATOL, err_msg=tag)
                np.testing.assert_allclose(dev["std"], ref.std, rtol=RTOL, atol=ATOL, err_msg=tag)
        np.testing.assert_allclose(got_split, want, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(np_(split.mean), orc.mean, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(np_(split.std), orc.std, rtol=RTOL, atol=ATOL)
        assert abs(np_(split.best_cost)[0] - orc.last_min_cost) <= RTOL_C * mag[idx_dev[0]]
        # the launches the benchmark times (merge prologues, ping-pong buffers) == the split run, bit for bit
        assert np.array_equal(got_fused, got_split)
        assert np.array_equal(np_(fused.mean), np_(split.mean)) and np.array_equal(np_(fused.std), np_(split.std))
        ea_f, ec_f = fused.current_elites()
        ea_s, ec_s = split.current_elites()
        assert np.array_equal(np_(ea_f), np_(ea_s)) and np.array_equal(np_(ec_f), np_(ec_s))
        n_last = split.population_sizes[-1]
        assert np.array_equal(np_(fused.costs[:n_last]), np_(split.costs[:n_last]))
        assert np.array_equal(np_(fused.actions[:n_last]), np_(split.actions[:n_last]))
    return n_near


def strict_loop(pl, om, oc, *, seed, N, iters, h, o, beta, cost_mode, low, high, elites_size=10, keep=True, shift=True,
                use_mean=True, n_steps=2, obs_scale=0.2, obs_seed=7, rtol=1e-9, atol=1e-11):
    """The f64 planner (reset, device Philox noise) against the oracle restating the same stream
    (``PhiloxNoiseSchedule``): executed action, mean and std to 1e-9 over ``n_steps`` MPC steps."""
    d = pl.d
    sched = O.PhiloxNoiseSchedule(seed, iters, d, h, shift=shift, dtype=np.float64, white=beta <= 0)
    orc = O.IcemOracle(O.IcemParams(horizon=h, num_simulated_trajectories=N, opt_iterations=iters, noise_beta=beta,
                                    elites_size=elites_size, keep_previous_elites=keep, shift_elites_over_time=shift,
                                    use_mean_actions=use_mean),
                       np.asarray(low, np.float64), np.asarray(high, np.float64),
                       lambda ob, ac: O.rollout_costs(om, oc, ob, ac, mode=cost_mode),
                       lambda num: tuple(None if z is None else z.astype(np.float64) for z in sched(num)))
    orc.beginning_of_rollout()
    rs = np.random.RandomState(obs_seed)
    for step in range(n_steps):
        obs = obs_scale * rs.randn(o)
        if step:
            sched.begin_step()
        got = np_(pl.plan_step(obs))
        want = orc.get_action(obs)
        np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=f"step {step}")
        np.testing.assert_allclose(np_(pl.mean), orc.mean, rtol=rtol, atol=atol, err_msg=f"step {step}")
        np.testing.assert_allclose(np_(pl.std), orc.std, rtol=rtol, atol=atol, err_msg=f"step {step}")
    return orc
