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
  python tools/cem_step_bench.py --batch B [--dtype f32|f64] [--sizes 512,4096]
                                               B planners: blocks of batched steps (``icem_plan_step_cem_batch``, each ending in
                                               the one device-to-host copy of its results) alternating with blocks of B solo
                                               ``icem_plan_step_cem`` steps issued back to back (each block step ending in one
                                               synchronisation) -- what these callers had before the batched entry; B may be a
                                               list (2,4,8,16).  With --trace: TRACE_STEPS steps of each and nothing else.
  python tools/cem_step_bench.py --learned [--batch B]
                                               the same legs through the learned dynamics: ``MpcCemStdHip`` with ``DeviceRSSMModel``
                                               at N = 1024, h = 12, d = 6, K = 10, 5 iterations -- the learned configuration's
                                               population on the CEM baseline -- ``icem_plan_step_cem_learned`` against the loop
                                               (``fused_step=False``), and with --batch ``icem_plan_step_cem_learned_batch`` against B
                                               solo fused steps.  The solo leg also prints the device time per launch of the three
                                               stages (sampler, rollout, update + bounds: each operator launched back to back between
                                               two events).  --stagewise runs on the parent commit's library as above.
  python tools/cem_step_bench.py --models [--cases 1x2,1x5,4x1,4x5] [--stagewise]
                                               the learned shape through MODELS OF THEIR OWN (``icem_plan_step_cem_learned_models``): B
                                               controllers x E members -- E > 1: one ``DeviceRSSMEnsemble`` of E seeds for all of them,
                                               E = 1: a ``DeviceRSSMModel`` each (``get_action_batch_own_models``) -- ``fused_step=True`` against
                                               ``fused_step=False`` (each controller's stage-wise loop: sampler, ensemble rollout +
                                               reduction, update, bounds), ``get_action`` for B = 1 and ``get_action_batch`` beyond,
                                               alternating blocks in one process.  --stagewise: the loop alone (also on the parent
                                               commit's library).
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
MODELS = "--models" in sys.argv
LEARNED = "--learned" in sys.argv or MODELS
if LEARNED:   # BASELINE configs[4]'s population on the CEM baseline; the RSSM's observation is [h (200) | z (30)]
    H, O_, SIZES = 12, 230, (1024,)
WARMUP, BLOCK, BLOCKS, TRACE_STEPS = 20, 200, 9, 50


def bind_what_the_library_has():
    """An older library lacks the newest entries: the stage-wise loop needs none of them."""
    have = C.CDLL(L.lib_path())
    L.SYMBOLS[:] = [s for s in L.SYMBOLS if hasattr(have, s[0])]


_rssm = []


def rssm():
    from icem_amd import DeviceRSSMModel
    if not _rssm:
        _rssm.append(DeviceRSSMModel(seed=3))
    return _rssm[0]


def controller(n, fused, model=None, seed=1):
    from icem_amd import DeviceSyntheticModel, MpcCemStdHip, halfcheetah_env
    if model is None:
        model = rssm() if LEARNED else DeviceSyntheticModel.make(O_, D, kind=0)
    c = MpcCemStdHip(env=halfcheetah_env(17 if LEARNED else O_), forward_model=model, horizon=H,
                     num_simulated_trajectories=n, cost_along_trajectory="sum", verbose=False, dtype="f32", seed=seed,
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


def _arg(flag, default):
    return sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else default


BATCH_BLOCK, BATCH_BLOCKS, BATCH_WARMUP = 30, 7, 10


def batch_planners(n, B, dtype):
    """B planners at the HalfCheetah shape (seeds of their own) with their distributions, as ``MpcCemStdHip`` holds them."""
    from icem_amd import DeviceSyntheticModel, IcemConfig, IcemPlanner, halfcheetah_env
    env = halfcheetah_env(17 if LEARNED else O_)
    out = []
    for i in range(B):
        cfg = IcemConfig(horizon=H, act_dim=D, num_traj=n, elites_size=10, opt_iters=ITERS, cost_mode="sum", use_mean_actions=False,
                         keep_previous_elites=False, shift_elites=False, factor_decrease=1.0, alpha=0.1, init_std=0.5, dtype=dtype,
                         seed=1 + i)
        pl = IcemPlanner(cfg, env.action_space.low, env.action_space.high)
        if not LEARNED:   # (the learned-dynamics step needs no built-in model)
            m = DeviceSyntheticModel.make(O_, D, kind=0)
            pl.set_model(m.kind, m.A, m.B)
            pl.set_cost_spec(env.cost_spec)
        pl.new_episode()
        mean = torch.empty((H, D), dtype=pl.dt, device=pl.device)
        std = torch.empty_like(mean)
        pl.reset_distribution(mean, std)
        lower, upper = pl.cem_bounds(mean, std, False)
        pl.mpc_step = 0
        out.append((pl, (mean, std, lower, upper)))
    return out


def main_batch():
    from icem_amd import IcemPlanner
    trace = "--trace" in sys.argv
    Bs = [int(x) for x in _arg("--batch", "8").split(",")]
    dtype = _arg("--dtype", "f32")
    sizes = [int(x) for x in _arg("--sizes", ",".join(str(n) for n in SIZES)).split(",")]
    lib = L.load_library()
    print(f"build {lib.icem_build_hash().decode()}  device {torch.cuda.get_device_name(0)}  h = {H}, d = {D}, o = {O_}, "
          f"{ITERS} iterations, {dtype}; warm-up {BATCH_WARMUP} steps; {BATCH_BLOCKS} blocks of {BATCH_BLOCK} steps per variant, alternating",
          flush=True)
    flags = dict(like_levine=False, shift_means=True, execute_best_elite=True)
    for n in sizes:
        for B in Bs:
            both = {"batched": batch_planners(n, B, dtype), "solo": batch_planners(n, B, dtype)}
            obs = [torch.as_tensor(0.1 * np.random.RandomState(i).randn(O_), dtype=both["solo"][0][0].dt, device="cuda") for i in range(B)]
            obs_all = torch.stack(obs)   # (the learned batch takes the table where it lies)

            def step(kind):
                ps = both[kind]
                if kind == "batched":
                    if LEARNED:
                        IcemPlanner.plan_step_cem_learned_batch([p for p, _ in ps], rssm(), obs_all, [dist for _, dist in ps], **flags)
                    else:
                        IcemPlanner.plan_step_cem_batch([p for p, _ in ps], obs, [dist for _, dist in ps], **flags)
                    return ps[0][0].cem_batch_results.cpu()   # the batch's one device-to-host copy
                for (p, dist), ob in zip(ps, obs):
                    if LEARNED:
                        p.plan_step_cem_learned(rssm(), ob, *dist, **flags)
                    else:
                        p.plan_step_cem(ob, *dist, **flags)
                torch.cuda.synchronize()
                return None

            def block(kind, reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    step(kind)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / reps * 1e3

            for kind in both:
                block(kind, BATCH_WARMUP)
            if trace:
                for kind in both:
                    block(kind, TRACE_STEPS)
                continue
            same = all(torch.equal(a[0].cem_result, b[0].cem_result) and torch.equal(a[1][0], b[1][0]) for a, b in zip(both["batched"], both["solo"]))
            t = {k: [] for k in both}
            for _ in range(BATCH_BLOCKS):
                for kind in both:
                    t[kind].append(block(kind, BATCH_BLOCK))
            b, s = sorted(t["batched"]), sorted(t["solo"])
            print(f"  {dtype} N = {n:5d} B = {B:2d}: batched median {b[len(b) // 2]:7.4f} ms per step of the batch (min {b[0]:.4f}, max {b[-1]:.4f}) | "
                  f"{B} solo steps median {s[len(s) // 2]:7.4f} (min {s[0]:.4f}, max {s[-1]:.4f}) | solo median / batched median "
                  f"{s[len(s) // 2] / b[len(b) // 2]:.2f}x | batched median < solo min: {b[len(b) // 2] < s[0]} | equal bits: {same}; "
                  f"launches per batched step {both['batched'][0][0].cem_batch_launches}, uploads {both['batched'][0][0].batch_uploads}", flush=True)


def stage_times(n, reps=200):
    """Device time per launch of the three stages of one CEM iteration through the RSSM: each operator launched `reps` times back to
    back between two events (the step's kernels run the operators' bodies)."""
    (pl, (mean, std, lower, upper)), = batch_planners(n, 1, "f32")
    m, obs = rssm(), (0.1 * np.random.RandomState(0).randn(O_)).astype(np.float32)
    actions = pl.sample_truncnorm(n, mean, std, lower, upper, None, offset=0)
    costs = m.rollout_cost(obs, actions, 0)

    def update():
        pl.update_distribution(costs, actions, pl.K, mean, std)
        pl.cem_bounds(mean, std, False)
    stages = {"sampler": lambda: pl.sample_truncnorm(n, mean, std, lower, upper, None, offset=1, out=actions),
              "rollout": lambda: m.rollout_cost(obs, actions, 0), "update + bounds (2 launches)": update}
    for name, launch in stages.items():
        for _ in range(20):
            launch()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            launch()
        b.record()
        torch.cuda.synchronize()
        print(f"  N = {n}: {name:<30s} {a.elapsed_time(b) / reps * 1e3:7.1f} us per call, back to back", flush=True)


def main():
    stagewise_only, trace = "--stagewise" in sys.argv, "--trace" in sys.argv
    if stagewise_only:
        bind_what_the_library_has()
    lib = L.load_library()
    print(f"build {lib.icem_build_hash().decode()}  device {torch.cuda.get_device_name(0)}  h = {H}, d = {D}, o = {O_}, "
          f"{ITERS} iterations, f32{', learned dynamics (DeviceRSSMModel)' if LEARNED else ''}; warm-up {WARMUP} calls", flush=True)
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
        if LEARNED:
            stage_times(n)


MODELS_BLOCK, MODELS_BLOCKS = 100, 9


def main_models():
    from icem_amd import DeviceRSSMEnsemble, DeviceRSSMModel, MpcCemStdHip
    stagewise_only = "--stagewise" in sys.argv
    if stagewise_only:
        bind_what_the_library_has()
    lib = L.load_library()
    n = SIZES[0]
    cases = [tuple(int(x) for x in c.split("x")) for c in _arg("--cases", "1x2,1x5,4x1,4x5").split(",")]
    print(f"build {lib.icem_build_hash().decode()}  device {torch.cuda.get_device_name(0)}  N = {n}, h = {H}, d = {D}, K = 10, {ITERS} iterations, "
          f"f32, models of their own; warm-up {WARMUP} steps; {MODELS_BLOCKS} blocks of {MODELS_BLOCK} steps per variant, alternating", flush=True)
    for B, E in cases:
        def group(fused):
            if E == 1:
                models = [DeviceRSSMModel(seed=3 + i) for i in range(B)]
            else:
                models = [DeviceRSSMEnsemble(seeds=list(range(3, 3 + E)))] * B
            return [controller(n, fused, model=m, seed=1 + i) for i, m in enumerate(models)]
        groups = {"stage-wise": group(False)}
        if not stagewise_only:
            groups = {"fused": group(True), **groups}
        obs = [0.1 * np.random.RandomState(i).randn(O_) for i in range(B)]

        def step(cs):   # (every step ends in its device-to-host copy of the result)
            return [cs[0].get_action(obs[0], None)] if B == 1 else (MpcCemStdHip.get_action_batch_own_models if E == 1 else MpcCemStdHip.get_action_batch)(cs, obs)

        def block(cs, reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                step(cs)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / reps * 1e3
        for cs in groups.values():
            block(cs, WARMUP)
        extra = ""
        if not stagewise_only:   # the same seeds, the same steps so far: the two groups agree bit for bit
            got, want = step(groups["fused"]), step(groups["stage-wise"])
            same = all(np.array_equal(a, b) for a, b in zip(got, want)) and all(np.array_equal(a.mean, b.mean) for a, b in zip(*groups.values()))
            extra = f" | equal bits: {same}; launches per fused step {groups['fused'][0].planner.cem_batch_launches}"
        t = {k: [] for k in groups}
        for _ in range(MODELS_BLOCKS):
            for k, cs in groups.items():
                t[k].append(block(cs, MODELS_BLOCK))
        line = " | ".join(f"{k} median {sorted(v)[len(v) // 2]:7.4f} ms per step (min {min(v):.4f}, max {max(v):.4f})" for k, v in t.items())
        if not stagewise_only:
            f, s_ = (sorted(t[k])[MODELS_BLOCKS // 2] for k in ("fused", "stage-wise"))
            extra = f" | stage-wise / fused {s_ / f:.2f}x | fused median < stage-wise min: {f < min(t['stage-wise'])}" + extra
        print(f"  B = {B} E = {E}: {line}{extra}", flush=True)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("no GPU: this tool measures and has nothing to say without one")
    if MODELS:
        main_models()
    elif "--batch" in sys.argv:
        main_batch()
    else:
        main()
