"""ms per ``MpcCemStdHip.get_action`` at the HalfCheetah shape (h = 30, d = 6, o = 17, 5 CEM iterations, 10 elites, f32),
N in {512, 4096}: the fused step (``icem_plan_step_cem``) against the stage-wise loop over the operators, same process, warm,
in alternating blocks -- a host clock around BLOCK calls, each of which ends in its device-to-host copy of the result; median
with min and max over BLOCKS blocks.

  python tools/cem_step_bench.py               fused and stage-wise, both sizes (+ the launch count and an equality check)
  python tools/cem_step_bench.py --stagewise   the stage-wise loop alone.  It binds only what the library exports, so it also
                                               runs on a library from before the entry -- the parent commit's loop, same box:
                                                   ICEM_HIP_LIB=<parent's libicem_hip.so> python tools/cem_step_bench.py --stagewise
                                               (tools/experiments/ab_libs.sh "python tools/cem_step_bench.py --stagewise" 0 P 0 P)
  python tools/cem_step_bench.py --trace       TRACE_STEPS steps of each variant and nothing else, for the kernels' own times --
                                               the step's sampler (cem_sample_kernel) against the operator's
                                               (sample_truncnorm_kernel) -- in a run of its own:
                                                   rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- \\
                                                       python tools/cem_step_bench.py --trace
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from icem_amd import _lib as L  # noqa: E402

H, D, O_, ITERS, SIZES = 30, 6, 17, 5, (512, 4096)
WARMUP, BLOCK, BLOCKS, TRACE_STEPS = 20, 200, 9, 50


def bind_what_the_library_has():
    """An older library lacks the newest entries: the stage-wise loop needs none of them."""
    have = C.CDLL(L.lib_path())
    L.SYMBOLS[:] = [s for s in L.SYMBOLS if hasattr(have, s[0])]


def controller(n, fused):
    from icem_amd import DeviceSyntheticModel, MpcCemStdHip, halfcheetah_env
    c = MpcCemStdHip(env=halfcheetah_env(O_), forward_model=DeviceSyntheticModel.make(O_, D, kind=0), horizon=H,
                     num_simulated_trajectories=n, cost_along_trajectory="sum", verbose=False, dtype="f32", seed=1,
                     **({"fused_step": fused} if fused is not None else {}),
                     action_sampler_params=dict(alpha=0.1, elites_size=10, opt_iterations=ITERS, init_std=0.5, shift_means=True,
                                                execute_best_elite=True, bounds_like_levine=False))
    c.beginning_of_rollout(observation=np.zeros(O_), state=None, mode="train")
    return c


def block_ms(c, obs, reps=BLOCK):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        c.get_action(obs, None)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def report(what, n, ms, extra=""):
    ms = sorted(ms)
    print(f"  {what:<28s} N = {n:5d}: median {ms[len(ms) // 2]:7.4f} ms per get_action (min {ms[0]:.4f}, max {ms[-1]:.4f}; "
          f"{len(ms)} blocks of {BLOCK}){extra}", flush=True)


def main():
    stagewise_only, trace = "--stagewise" in sys.argv, "--trace" in sys.argv
    if stagewise_only:
        bind_what_the_library_has()
    lib = L.load_library()
    print(f"build {lib.icem_build_hash().decode()}  device {torch.cuda.get_device_name(0)}  h = {H}, d = {D}, o = {O_}, "
          f"{ITERS} iterations, f32; warm-up {WARMUP} calls", flush=True)
    obs = 0.1 * np.random.RandomState(0).randn(O_)
    for n in SIZES:
        # (a library without the keyword's entry: the constructor of its own tree would not know `fused_step` either, but the
        #  tool runs THIS tree's Python on it, where False never asks the library)
        ctrls = {"stage-wise loop": controller(n, False)}
        if not stagewise_only:
            ctrls = {"fused step": controller(n, True), **ctrls}
        for c in ctrls.values():
            for _ in range(WARMUP):
                c.get_action(obs, None)
        if trace:
            for c in ctrls.values():
                block_ms(c, obs, TRACE_STEPS)
            continue
        if not stagewise_only:   # the same seed, the same steps so far: the two controllers agree bit for bit
            a, b = ctrls["fused step"], ctrls["stage-wise loop"]
            same = np.array_equal(a.get_action(obs, None), b.get_action(obs, None)) and np.array_equal(a.mean, b.mean)
            print(f"  N = {n}: fused == stage-wise: {same}; launches per fused step: {a.planner.cem_step_launches}", flush=True)
        t = {k: [] for k in ctrls}
        for _ in range(BLOCKS):
            for k, c in ctrls.items():
                t[k].append(block_ms(c, obs))
        for k in ctrls:
            report(k, n, t[k])
        if not stagewise_only:
            f, s = (sorted(t[k])[BLOCKS // 2] for k in ("fused step", "stage-wise loop"))
            print(f"  stage-wise / fused at N = {n}: {s / f:.2f}x", flush=True)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("no GPU: this tool measures and has nothing to say without one")
    main()
