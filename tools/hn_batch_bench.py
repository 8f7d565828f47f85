"""icem_plan_step_batch on the TileHN shapes against stepping alone: Door, Relocate and FetchPickAndPlace as bench.py's workloads
of those names (h = 30, 5 iterations, their beta and model kind, problems with models and seeds of their own) at N = 4096 and
N = 1024, B = 1, 2, 4, 8, 16 planners.  Per (shape, N, B): ms per batched MPC step against B solo steps, timed in turns in one
process in blocks of STEPS steps between two synchronisations (plan_step_resident / plan_step_batch without observations: no host
work besides the launches), the median block with min and max of ROUNDS.

  python tools/hn_batch_bench.py                    the table
  python tools/hn_batch_bench.py --solo             solo steps only, through nothing the batch added: it also runs on a library from
                                                    before it (tools/experiments/ab_libs.sh "python tools/hn_batch_bench.py --solo" 0 P 0 P)
  python tools/hn_batch_bench.py --trace door 4096 8   a few solo steps, then a few batched ones of one case and nothing else, for
                                                    rocprofv3 --kernel-trace --stats -- python tools/hn_batch_bench.py --trace ...
  --shapes door,fpp  --sizes 4096  --batches 4,8    narrow the table
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from icem_amd import DeviceSyntheticModel, IcemConfig, IcemPlanner, envs as E  # noqa: E402
from icem_amd import _lib as L, build as B_  # noqa: E402

# bench.py's WORKLOADS["door" / "relocate" / "fpp"]
SHAPES = {"door": dict(env=E.door_env, beta=2.5, kind=1), "relocate": dict(env=E.relocate_env, beta=3.5, kind=1),
          "fpp": dict(env=E.fetch_pick_and_place_env, beta=3.0, kind=0)}
ITERS, STEPS, ROUNDS, WARMUP = 5, 30, 7, 12


def planners(name, N, nb):
    w = SHAPES[name]
    env = w["env"]()
    o, d = env.obs_dim, env.action_space.shape[0]
    out = []
    for i in range(nb):
        model = DeviceSyntheticModel.make(o, d, kind=w["kind"], seed_a=i, seed_b=100 + i)
        pl = IcemPlanner(IcemConfig(horizon=30, act_dim=d, num_traj=N, opt_iters=ITERS, noise_beta=w["beta"], dtype="f32", seed=1234 + i),
                         env.action_space.low, env.action_space.high)
        pl.set_model(model.kind, model.A, model.B)
        pl.set_cost_spec(env.cost_spec)
        pl.reset()
        pl.obs0.copy_(torch.as_tensor(0.1 * np.random.RandomState(i).randn(o), dtype=pl.dt))
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


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def solo_table(shapes, sizes):
    print(f"build {B_.embedded_hash(L.lib_path())}  device {torch.cuda.get_device_name(0)}  solo icem_plan_step, {ITERS} iterations, "
          f"median (min, max) of {ROUNDS} blocks of {STEPS} steps")
    for name in shapes:
        for N in sizes:
            pl = planners(name, N, 1)[0]
            for _ in range(WARMUP):
                pl.plan_step_resident()
            m, lo, hi = med([block(pl.plan_step_resident) for _ in range(ROUNDS)])
            print(f"  {name:8s} N={N:5d}: {1e3 * m:7.1f} us per MPC step ({1e3 * lo:.1f}, {1e3 * hi:.1f})  checksum {float(pl.mean.sum()):.6f}")


def table(shapes, sizes, batches):
    print(f"build {B_.embedded_hash(L.lib_path())}  device {torch.cuda.get_device_name(0)}  {ITERS} iterations, median (min, max) of "
          f"{ROUNDS} blocks of {STEPS} steps, batched and solo in turns")
    print("  shape       N   B | batched ms per step (min, max) | B solo steps ms (min, max)    | batched / solo | us per problem: batched, solo")
    for name in shapes:
        for N in sizes:
            for nb in batches:
                together, alone = planners(name, N, nb), planners(name, N, nb)

                def batched():
                    IcemPlanner.plan_step_batch(together)

                def solos():
                    for pl in alone:
                        pl.plan_step_resident()

                for _ in range(WARMUP):   # (twelve steps: the batch's argument arrays have stopped changing)
                    batched()
                    solos()
                up = together[0].batch_uploads
                tb, ts = [], []
                for _ in range(ROUNDS):
                    tb.append(block(batched))
                    ts.append(block(solos))
                assert nb == 1 or together[0].batch_uploads == up, "the timed steps uploaded argument blocks"
                (b, blo, bhi), (s, slo, shi) = med(tb), med(ts)
                print(f"  {name:8s} {N:5d}  {nb:2d} | {b:8.4f} ({blo:.4f}, {bhi:.4f})     | {s:8.4f} ({slo:.4f}, {shi:.4f})   | {b / s:14.3f} | "
                      f"{1e3 * b / nb:7.1f}, {1e3 * s / nb:7.1f}", flush=True)
                del together, alone


def trace(name, N, nb):
    alone, together = planners(name, N, 1)[0], planners(name, N, nb)
    for _ in range(8):
        alone.plan_step_resident()
    torch.cuda.synchronize()
    for _ in range(8):
        IcemPlanner.plan_step_batch(together)
    torch.cuda.synchronize()
    print(f"{name} N={N}: 8 solo steps, then 8 batched steps of {nb} problems")


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("no GPU: this tool measures and has nothing to say without one")

    def opt(flag, default):
        return sys.argv[sys.argv.index(flag) + 1].split(",") if flag in sys.argv else default
    shapes = opt("--shapes", list(SHAPES))
    sizes = [int(x) for x in opt("--sizes", [4096, 1024])]
    batches = [int(x) for x in opt("--batches", [1, 2, 4, 8, 16])]
    if "--trace" in sys.argv:
        at = sys.argv.index("--trace")
        trace(sys.argv[at + 1], int(sys.argv[at + 2]), int(sys.argv[at + 3]))
    elif "--solo" in sys.argv:
        solo_table(shapes, sizes)
    else:
        table(shapes, sizes, batches)
