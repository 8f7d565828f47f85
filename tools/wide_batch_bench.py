"""icem_plan_step_batch on the GEMM-kernel shapes against stepping alone: HumanoidStandup at its real width (o = 378, d = 17, the
fp16 planes: bench.py's c3 workload -- beta 2.0, 3 iterations, tanh model -- at smaller populations) at N = 256, 1024 and 4096, and
Hopper (o = 12, d = 3, the exact-f32 kernel's narrow form) at N = 256; B = 2, 4, 8, 16, 32 planners with models and seeds of their
own.  Per (shape, N, B): ms per batched MPC step against B solo steps of the SAME library, in turns in one process, each block of
STEPS steps between two device events (plan_step_resident / plan_step_batch without observations: no host work besides the
launches); min / median / max of ROUNDS blocks, ROUNDS x STEPS >= 100 warmed steps per side.

  python tools/wide_batch_bench.py                          the table (EXPERIMENTS R9.1)
  --shapes standup,hopper  --sizes 256  --batches 4,8       narrow the table (hopper is measured at the sizes <= 256 only)
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from icem_amd import DeviceSyntheticModel, IcemConfig, IcemPlanner, envs as E  # noqa: E402
from icem_amd import _lib as L, build as B_  # noqa: E402

SHAPES = {"standup": dict(env=lambda: E.humanoid_standup_env(378), beta=2.0, kind=1, iters=3, max_n=1 << 30),
          "hopper": dict(env=E.hopper_env, beta=2.0, kind=1, iters=3, max_n=256)}
STEPS, ROUNDS, WARMUP = 25, 5, 12


def planners(name, N, nb):
    w = SHAPES[name]
    env = w["env"]()
    o, d = env.obs_dim, env.action_space.shape[0]
    out = []
    for i in range(nb):
        model = DeviceSyntheticModel.make(o, d, kind=w["kind"], seed_a=i, seed_b=100 + i)
        pl = IcemPlanner(IcemConfig(horizon=30, act_dim=d, num_traj=N, opt_iters=w["iters"], noise_beta=w["beta"], dtype="f32", seed=1234 + i),
                         env.action_space.low, env.action_space.high)
        pl.set_model(model.kind, model.A, model.B)
        pl.set_cost_spec(env.cost_spec)
        pl.reset()
        pl.obs0.copy_(torch.as_tensor(0.1 * np.random.RandomState(i).randn(o), dtype=pl.dt))
        out.append(pl)
    return out


def block(fn, steps=STEPS):
    """ms per call of fn over `steps` calls between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def table(shapes, sizes, batches):
    print(f"build {B_.embedded_hash(L.lib_path())}  device {torch.cuda.get_device_name(0)}  median (min, max) of {ROUNDS} blocks of {STEPS} "
          f"steps between device events, batched and solo in turns")
    print("  shape       N   B | batched ms per step (min, max) | B solo steps ms (min, max)    | batched / solo | us per problem: batched, solo")
    for name in shapes:
        for N in sizes:
            if N > SHAPES[name]["max_n"]:
                continue
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


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("no GPU: this tool measures and has nothing to say without one")

    def opt(flag, default):
        return sys.argv[sys.argv.index(flag) + 1].split(",") if flag in sys.argv else default
    table(opt("--shapes", list(SHAPES)), [int(x) for x in opt("--sizes", [256, 1024, 4096])], [int(x) for x in opt("--batches", [2, 4, 8, 16, 32])])
