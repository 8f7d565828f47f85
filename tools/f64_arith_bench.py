"""The two float64 arithmetics of the rollout (icem_set_f64_arith): the fma chain of the generic kernels against the f64 matrix
cores (k_rollout_f64.hip), planners timed in turns in one process, in blocks of STEPS steps between two synchronisations
(plan_step_resident: no host work besides the launches), min / median / max of ROUNDS blocks; then a few profiled steps for the
rollout's time per launch (the ProfScope counters, icem_profile_read).  Workloads:

  c2-f64   N = 4096 x 5 iterations, h = 30, d = 6, o = 17 (bench.py's `also_f64`): chain and matrix cores
  door     N = 4096 x 3, h = 30, d = 28, o = 39 with Door's term list: matrix cores only (the chain ends at o = 32); at o = 32 with
           the same kind of list the chain runs its one-thread-per-trajectory form: both, as `door32`
  c3-f64   N = 16384 x 3, h = 12, d = 17, o = 378 (HumanoidStandup): matrix cores only -- there is no float64 predecessor

Prints a table and, last, ONE JSON line.   python tools/f64_arith_bench.py [c2 door door32 c3]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from icem_amd import DeviceSyntheticModel, IcemConfig, IcemPlanner  # noqa: E402
from icem_amd import envs as E  # noqa: E402
from icem_amd import _lib as L, build as B_  # noqa: E402

STEPS, ROUNDS, WARMUP = 10, 5, 6

WORKLOADS = {   # name: (env, N, iterations, horizon, arithmetics)
    "c2": (lambda: E.halfcheetah_env(17), 4096, 5, 30, ("chain", "mfma")),
    "door": (lambda: E.door_env(), 4096, 3, 30, ("mfma",)),
    "door32": (lambda: E.door_env(32, nq=24, nv=24), 4096, 3, 30, ("chain", "mfma")),
    "c3": (lambda: E.humanoid_standup_env(378), 16384, 3, 12, ("mfma",)),
}


def planner(env, N, iters, h, arith):
    o, d = env.obs_dim, env.action_space.shape[0]
    model = DeviceSyntheticModel.make(o, d, kind=1)
    pl = IcemPlanner(IcemConfig(horizon=h, act_dim=d, num_traj=N, opt_iters=iters, dtype="f64", seed=1234), env.action_space.low, env.action_space.high)
    pl.set_f64_arith(arith)
    pl.set_model(model.kind, model.A, model.B)
    pl.set_cost_spec(env.cost_spec)
    pl.reset()
    pl.obs0.copy_(torch.as_tensor(0.1 * np.random.RandomState(0).randn(o), dtype=pl.dt))
    return pl


def block(fn, steps=STEPS):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def stats(xs):
    xs = sorted(xs)
    return dict(min=round(xs[0], 5), median=round(xs[len(xs) // 2], 5), max=round(xs[-1], 5))


def rollout_us_per_launch(pl, steps=4):
    pl.profile_enable(True)
    pl.profile_read()
    for _ in range(steps):
        pl.plan_step_resident()
    torch.cuda.synchronize()
    ms, cnt, _units = pl.profile_read()["rollout_cost"]
    pl.profile_enable(False)
    return round(1e3 * ms / cnt, 3), cnt // steps


def main(names):
    res = dict(build=B_.embedded_hash(L.lib_path()), device=torch.cuda.get_device_name(0), dtype="f64", steps_per_block=STEPS, blocks=ROUNDS,
               workloads={})
    print("workload | arith | ms per MPC step (min, max) | rollout us per launch (launches per step)")
    for name in names:
        mk_env, N, iters, h, ariths = WORKLOADS[name]
        env = mk_env()
        pls = {a: planner(env, N, iters, h, a) for a in ariths}
        for _ in range(WARMUP):
            for pl in pls.values():
                pl.plan_step_resident()
        times = {a: [] for a in ariths}
        for _ in range(ROUNDS):   # in turns: a drift of the clocks hits both alike
            for a, pl in pls.items():
                times[a].append(block(pl.plan_step_resident))
        out = dict(N=N, iters=iters, h=h, d=env.action_space.shape[0], o=env.obs_dim)
        for a, pl in pls.items():
            s = stats(times[a])
            us, per_step = rollout_us_per_launch(pl)
            out[a] = dict(step_ms=s, rollout_us_per_launch=us, rollout_launches_per_step=per_step, checksum=float(pl.mean.sum()))
            print(f"  {name:7s}| {a:5s} | {s['median']:8.4f} ({s['min']:.4f}, {s['max']:.4f}) | {us:9.2f} ({per_step})", flush=True)
        res["workloads"][name] = out
        del pls
    print(json.dumps(res))


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("no GPU: this tool measures and has nothing to say without one")
    main([a for a in sys.argv[1:] if a in WORKLOADS] or list(WORKLOADS))
