"""icem_plan_step_batch_f64 against stepping alone, at the strict-parity headline configuration: dtype f64, N = 4096, h = 30, d = 6,
o = 17, 5 iterations (bench.py's `also_f64`), problems with models and seeds of their own, B = 2, 4, 8, 16 planners.  Per B: ms per
batched MPC step against one solo step and against B solo steps, timed in turns in one process in blocks of STEPS steps between two
synchronisations (plan_step_resident / plan_step_batch_f64 without observations: no host work besides the launches), min / median /
max of ROUNDS blocks.  Prints a table and, last, ONE JSON line.

  python tools/f64_batch_bench.py                 the table + the JSON line
  python tools/f64_batch_bench.py --solo          solo steps only, through nothing the batch added: the A/B against a library of the
                                                  commit before it (tools/experiments/ab_libs.sh "python tools/f64_batch_bench.py --solo"
                                                  0 P 0 P; the bindings want every symbol, so libicem_P.so is that commit's objects
                                                  linked with a two-function stub of icem_plan_step_batch_f64 / icem_batch_f64_launches)
  python tools/f64_batch_bench.py --trace 8       a few solo steps, then a few batched ones of B problems and nothing else, for
                                                  rocprofv3 --kernel-trace --stats -- python tools/f64_batch_bench.py --trace 8
  --batches 4,8                                   narrow the table
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from icem_amd import DeviceSyntheticModel, IcemConfig, IcemPlanner, halfcheetah_env  # noqa: E402
from icem_amd import _lib as L, build as B_  # noqa: E402

N, H, D, OBS, ITERS = 4096, 30, 6, 17, 5
STEPS, ROUNDS, WARMUP = 20, 7, 14


def planners(nb):
    env = halfcheetah_env(OBS)
    out = []
    for i in range(nb):
        model = DeviceSyntheticModel.make(OBS, D, seed_a=i, seed_b=100 + i)
        pl = IcemPlanner(IcemConfig(horizon=H, act_dim=D, num_traj=N, opt_iters=ITERS, dtype="f64", seed=1234 + i),
                         env.action_space.low, env.action_space.high)
        pl.set_model(model.kind, model.A, model.B)
        pl.set_cost_spec(env.cost_spec)
        pl.reset()
        pl.obs0.copy_(torch.as_tensor(0.1 * np.random.RandomState(i).randn(OBS), dtype=pl.dt))
        out.append(pl)
    return out


def block(fn, steps=STEPS):
    """ms per call of fn over `steps` calls between two synchronisations."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def stats(xs):
    xs = sorted(xs)
    return dict(min=round(xs[0], 5), median=round(xs[len(xs) // 2], 5), max=round(xs[-1], 5))


def head():
    return dict(build=B_.embedded_hash(L.lib_path()), device=torch.cuda.get_device_name(0), dtype="f64", N=N, h=H, d=D, o=OBS,
                iters=ITERS, steps_per_block=STEPS, blocks=ROUNDS)


def solo_only():
    pl = planners(1)[0]
    for _ in range(WARMUP):
        pl.plan_step_resident()
    s = stats([block(pl.plan_step_resident) for _ in range(ROUNDS)])
    print(f"solo icem_plan_step (f64, N={N}, {ITERS} iterations): {s['median']:.4f} ms per MPC step (min {s['min']:.4f}, max {s['max']:.4f})  "
          f"checksum {float(pl.mean.sum()):.12f}")
    print(json.dumps(dict(head(), solo_ms=s)))


def table(batches):
    res = dict(head(), batches={})
    print("   B | batched ms per step (min, max) | one solo step ms (min, max) | B solo steps ms | batched / B solo | launches per batched step")
    for nb in batches:
        together, alone = planners(nb), planners(nb)

        def batched():
            IcemPlanner.plan_step_batch_f64(together)

        def solos():
            for pl in alone:
                pl.plan_step_resident()

        for _ in range(WARMUP):   # (fourteen steps: the batch's argument arrays have stopped changing)
            batched()
            solos()
        up = together[0].batch_uploads
        tb, ts = [], []
        for _ in range(ROUNDS):
            tb.append(block(batched))
            ts.append(block(solos) / nb)
        assert together[0].batch_uploads == up, "the timed steps uploaded argument blocks"
        b, s = stats(tb), stats(ts)
        res["batches"][str(nb)] = dict(batched_ms=b, solo_ms=s, batched_over_B_solo=round(b["median"] / (nb * s["median"]), 4),
                                       launches=together[0].batch_f64_launches)
        print(f"  {nb:2d} | {b['median']:8.4f} ({b['min']:.4f}, {b['max']:.4f})     | {s['median']:8.4f} ({s['min']:.4f}, {s['max']:.4f})  | "
              f"{nb * s['median']:8.4f}        | {b['median'] / (nb * s['median']):8.3f}         | {together[0].batch_f64_launches}", flush=True)
        del together, alone
    print(json.dumps(res))


def trace(nb):
    alone, together = planners(1)[0], planners(nb)
    for _ in range(8):
        alone.plan_step_resident()
    torch.cuda.synchronize()
    for _ in range(8):
        IcemPlanner.plan_step_batch_f64(together)
    torch.cuda.synchronize()
    print(f"f64 N={N}: 8 solo steps, then 8 batched steps of {nb} problems")


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("no GPU: this tool measures and has nothing to say without one")
    if "--trace" in sys.argv:
        trace(int(sys.argv[sys.argv.index("--trace") + 1]))
    elif "--solo" in sys.argv:
        solo_only()
    else:
        table([int(x) for x in sys.argv[sys.argv.index("--batches") + 1].split(",")] if "--batches" in sys.argv else [2, 4, 8, 16])
