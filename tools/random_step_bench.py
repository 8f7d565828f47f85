"""ms per ``MpcRandomHip.get_action`` at the HalfCheetah shape (h = 30, d = 6, o = 17, ``action_change_frequency`` 4, f32),
N in {512, 4096}: the fused step (``icem_plan_step_random``) against the operator chain (``fused_step=False``), same process, warm,
in alternating blocks -- a host clock around BLOCK calls, each of which ends in its device-to-host copy; min / median / max over
BLOCKS blocks.

  python tools/random_step_bench.py [--sizes 512,4096]
                                                 fused and chain, both sizes (+ the launch count and an equality check)
  python tools/random_step_bench.py --stagewise  the operator chain alone.  It binds only what the library exports, so it also
                                                 runs on a library from before the entry -- the parent commit's chain, same box:
                                                     ICEM_HIP_LIB=<parent's libicem_hip.so> python tools/random_step_bench.py --stagewise
  python tools/random_step_bench.py --trace      TRACE_STEPS steps of each variant and nothing else, for the kernels' own times --
                                                 the step's sampler (random_sample_kernel) against the operator's
                                                 (sample_piecewise_kernel), the selection launch against the operator's top-k -- in
                                                 a run of its own:
                                                     rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o t -- \\
                                                         python tools/random_step_bench.py --trace
  python tools/random_step_bench.py --batch B [--dtype f32|f64] [--sizes 512,4096]
                                                 B planners: blocks of batched steps (``icem_plan_step_random_batch``, each ending in
                                                 the one device-to-host copy of its results) alternating with blocks of B solo
                                                 ``icem_plan_step_random`` steps issued back to back (each block step ending in one
                                                 synchronisation); B may be a list (2,4,8,16).
  ... --learned                                  every mode above through the learned dynamics (``DeviceRSSMModel``; N = 1024, h = 12,
                                                 hold 4): ``icem_plan_step_random_learned`` against the chain, ``--stagewise`` for the
                                                 chain alone (also on the parent commit's library), ``--batch B`` for
                                                 ``icem_plan_step_random_learned_batch`` against B solo fused steps
  python tools/random_step_bench.py --learned --events [--batch 2,4,8,16]
                                                 device times from HIP events around EVENT_REPS back-to-back launches, per launch:
                                                 the chain's sampler, rollout and selection one by one, the solo fused step as a
                                                 whole, and per B the batched step as a whole and its batched rollout alone (the
                                                 difference is the batch's sampler + selection)
  python tools/random_step_bench.py --models [--cases 1x2,1x5,4x1,4x5] [--stagewise]
                                                 the learned shape through MODELS OF THEIR OWN (``icem_plan_step_random_learned_models``):
                                                 B controllers x E members -- E > 1: one ``DeviceRSSMEnsemble`` of E seeds for all of
                                                 them, E = 1: a ``DeviceRSSMModel`` each (``get_action_batch_own_models``) -- ``fused_step=True``
                                                 against ``fused_step=False`` (each controller's operator chain), ``get_action`` for
                                                 B = 1 and ``get_action_batch`` beyond, alternating blocks in one process.
                                                 --stagewise: the chain alone (also on the parent commit's library).
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from icem_amd import _lib as L  # noqa: E402

H, D, O_, FREQ, SIZES = 30, 6, 17, 4, (512, 4096)
WARMUP, BLOCK, BLOCKS, TRACE_STEPS = 20, 200, 9, 50
BATCH_BLOCK, BATCH_BLOCKS, BATCH_WARMUP = 30, 7, 10
MODELS = "--models" in sys.argv
LEARNED = "--learned" in sys.argv or MODELS
if LEARNED:   # the declared RSSM's shape (BASELINE configs[4])
    H, O_, SIZES = 12, 230, (1024,)
EVENT_REPS, EVENT_BLOCKS = 50, 5
_model = {}


def rssm():
    from icem_amd import DeviceRSSMModel
    if "m" not in _model:
        _model["m"] = DeviceRSSMModel(seed=3)
    return _model["m"]


def bind_what_the_library_has():
    """An older library lacks the newest entries: the operator chain needs none of them."""
    have = C.CDLL(L.lib_path())
    L.SYMBOLS[:] = [s for s in L.SYMBOLS if hasattr(have, s[0])]


def controller(n, fused, model=None, seed=1):
    from icem_amd import DeviceSyntheticModel, MpcRandomHip, halfcheetah_env
    if model is None:
        model = rssm() if LEARNED else DeviceSyntheticModel.make(O_, D, kind=0)
    c = MpcRandomHip(env=halfcheetah_env(17 if LEARNED else O_), forward_model=model, horizon=H,
                     num_simulated_trajectories=n, cost_along_trajectory="sum", verbose=False, dtype="f32", seed=seed, fused_step=fused,
                     action_sampler_params=dict(action_change_frequency=FREQ))
    c.beginning_of_rollout(observation=np.zeros(O_), state=None, mode="train")
    return c


def block_ms(c, obs, reps=BLOCK):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        c.get_action(obs, None)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def report(what, n, ms):
    ms = sorted(ms)
    print(f"  {what:<18s} N = {n:5d}: median {ms[len(ms) // 2]:7.4f} ms per get_action (min {ms[0]:.4f}, max {ms[-1]:.4f}; "
          f"{len(ms)} blocks of {BLOCK})", flush=True)


def _arg(flag, default):
    return sys.argv[sys.argv.index(flag) + 1] if flag in sys.argv else default


def batch_planners(n, B, dtype):
    from icem_amd import DeviceSyntheticModel, IcemConfig, IcemPlanner, halfcheetah_env
    env = halfcheetah_env(17 if LEARNED else O_)
    out = []
    for i in range(B):
        pl = IcemPlanner(IcemConfig(horizon=H, act_dim=D, num_traj=n, elites_size=2, opt_iters=1, cost_mode="sum", dtype=dtype, seed=1 + i),
                         env.action_space.low, env.action_space.high)
        if not LEARNED:
            m = DeviceSyntheticModel.make(O_, D, kind=0)
            pl.set_model(m.kind, m.A, m.B)
            pl.set_cost_spec(env.cost_spec)
        out.append(pl)
    return out


def main_batch():
    from icem_amd import IcemPlanner
    Bs = [int(x) for x in _arg("--batch", "8").split(",")]
    dtype = _arg("--dtype", "f32")
    sizes = [int(x) for x in _arg("--sizes", ",".join(str(n) for n in SIZES)).split(",")]
    lib = L.load_library()
    print(f"build {lib.icem_build_hash().decode()}  device {torch.cuda.get_device_name(0)}  h = {H}, d = {D}, o = {O_}, hold {FREQ}, {dtype}; "
          f"warm-up {BATCH_WARMUP} steps; {BATCH_BLOCKS} blocks of {BATCH_BLOCK} steps per variant, alternating", flush=True)
    for n in sizes:
        for B in Bs:
            both = {"batched": batch_planners(n, B, dtype), "solo": batch_planners(n, B, dtype)}
            calls = {"batched": 0, "solo": 0}
            obs = [torch.as_tensor(0.1 * np.random.RandomState(i).randn(O_), dtype=both["solo"][0].dt, device="cuda") for i in range(B)]

            def step(kind):
                ps, off = both[kind], calls[kind]
                calls[kind] += n * H
                if kind == "batched":
                    if LEARNED:
                        IcemPlanner.plan_step_random_learned_batch(ps, rssm(), obs, [off] * B, FREQ)
                    else:
                        IcemPlanner.plan_step_random_batch(ps, obs, [off] * B, FREQ)
                    return ps[0].random_batch_results.cpu()   # the batch's one device-to-host copy
                for p, ob in zip(ps, obs):
                    if LEARNED:
                        p.plan_step_random_learned(rssm(), ob, off, FREQ)
                    else:
                        p.plan_step_random(ob, off, FREQ)
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
            same = all(torch.equal(a.random_result, b.random_result) and torch.equal(a.random_costs, b.random_costs)
                       for a, b in zip(both["batched"], both["solo"]))
            t = {k: [] for k in both}
            for _ in range(BATCH_BLOCKS):
                for kind in both:
                    t[kind].append(block(kind, BATCH_BLOCK))
            b, s = sorted(t["batched"]), sorted(t["solo"])
            print(f"  {dtype} N = {n:5d} B = {B:2d}: batched median {b[len(b) // 2]:7.4f} ms per step of the batch (min {b[0]:.4f}, max {b[-1]:.4f}) | "
                  f"{B} solo steps median {s[len(s) // 2]:7.4f} (min {s[0]:.4f}, max {s[-1]:.4f}) | solo median / batched median "
                  f"{s[len(s) // 2] / b[len(b) // 2]:.2f}x | equal bits: {same}; launches per batched step "
                  f"{both['batched'][0].random_batch_launches}, uploads {both['batched'][0].batch_uploads}", flush=True)


def event_us(fn, reps=EVENT_REPS, blocks=EVENT_BLOCKS):
    """us per call of fn from HIP events around `reps` back-to-back calls: (min, median, max) over `blocks` blocks."""
    for _ in range(5):
        fn()
    out = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps * 1e3)
    out.sort()
    return out[0], out[len(out) // 2], out[-1]


def main_events():
    """Device times per launch (HIP events; the host enqueues ahead, so these are the launches' own times plus the gaps between
    launches of one stream)."""
    from icem_amd import IcemPlanner
    n = SIZES[0]
    lib = L.load_library()
    print(f"build {lib.icem_build_hash().decode()}  device {torch.cuda.get_device_name(0)}  N = {n}, h = {H}, d = {D}, hold {FREQ}, f32; "
          f"HIP events around {EVENT_REPS} back-to-back calls, {EVENT_BLOCKS} blocks: min / median / max us per call", flush=True)
    pl = batch_planners(n, 1, "f32")[0]
    m = rssm()
    obs = (0.3 * np.random.RandomState(0).randn(O_)).astype(np.float32)
    actions = pl.sample_piecewise(n, 0, FREQ, None, 0)
    costs = m.rollout_cost(obs, actions, 0)
    show = lambda what, t: print(f"  {what:<58s} {t[0]:8.2f} / {t[1]:8.2f} / {t[2]:8.2f}", flush=True)   # noqa: E731
    show("chain: sample_piecewise", event_us(lambda: pl.sample_piecewise(n, 0, FREQ, None, 0)))
    show("chain: rollout_cost (icem_rssm_rollout_cost)", event_us(lambda: m.rollout_cost(obs, actions, 0)))
    show("chain: topk_sorted(costs, 1)", event_us(lambda: pl.topk_sorted(costs, 1)))
    obs_t = torch.as_tensor(obs, device="cuda")
    show("fused solo step (3 launches)", event_us(lambda: pl.plan_step_random_learned(m, obs_t, 0, FREQ)))
    for B in [int(x) for x in _arg("--batch", "2,4,8,16").split(",")]:
        ps = batch_planners(n, B, "f32")
        ob = [obs_t] * B
        t = event_us(lambda: IcemPlanner.plan_step_random_learned_batch(ps, m, ob, [0] * B, FREQ))
        pool = torch.cat([p.random_actions for p in ps])
        table = obs_t.repeat(B, 1).contiguous()
        r = event_us(lambda: m.rollout_cost_batch(table, pool, [n] * B, 0))
        show(f"batched step B = {B:2d} (3 launches)", t)
        show(f"  its batched rollout alone; per problem of the step {t[1] / B:.2f} us", r)


def main():
    stagewise_only, trace = "--stagewise" in sys.argv, "--trace" in sys.argv
    if stagewise_only:
        bind_what_the_library_has()
    lib = L.load_library()
    print(f"build {lib.icem_build_hash().decode()}  device {torch.cuda.get_device_name(0)}  h = {H}, d = {D}, o = {O_}, hold {FREQ}, f32; "
          f"warm-up {WARMUP} calls", flush=True)
    obs = (0.3 if LEARNED else 0.1) * np.random.RandomState(0).randn(O_)
    for n in [int(x) for x in _arg("--sizes", ",".join(str(n) for n in SIZES)).split(",")]:
        # (a library without the entry: False never asks the library for it)
        ctrls = {"operator chain": controller(n, False)}
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
            a, b = ctrls["fused step"], ctrls["operator chain"]
            same = (np.array_equal(a.get_action(obs, None), b.get_action(obs, None)) and a.best_traj_idx == b.best_traj_idx
                    and torch.equal(a._last_costs, b._last_costs))
            print(f"  N = {n}: fused == chain: {same}; launches per fused step: {a.planner.random_step_launches}", flush=True)
        t = {k: [] for k in ctrls}
        for _ in range(BLOCKS):
            for k, c in ctrls.items():
                t[k].append(block_ms(c, obs))
        for k in ctrls:
            report(k, n, t[k])
        if not stagewise_only:
            f, s = (sorted(t[k])[BLOCKS // 2] for k in ("fused step", "operator chain"))
            print(f"  chain / fused at N = {n}: {s / f:.2f}x", flush=True)


MODELS_BLOCK, MODELS_BLOCKS = 200, 9


def main_models():
    from icem_amd import DeviceRSSMEnsemble, DeviceRSSMModel, MpcRandomHip
    stagewise_only = "--stagewise" in sys.argv
    if stagewise_only:
        bind_what_the_library_has()
    lib = L.load_library()
    n = SIZES[0]
    cases = [tuple(int(x) for x in c.split("x")) for c in _arg("--cases", "1x2,1x5,4x1,4x5").split(",")]
    print(f"build {lib.icem_build_hash().decode()}  device {torch.cuda.get_device_name(0)}  N = {n}, h = {H}, d = {D}, hold {FREQ}, f32, "
          f"models of their own; warm-up {WARMUP} steps; {MODELS_BLOCKS} blocks of {MODELS_BLOCK} steps per variant, alternating", flush=True)
    for B, E in cases:
        def group(fused):
            if E == 1:
                models = [DeviceRSSMModel(seed=3 + i) for i in range(B)]
            else:
                models = [DeviceRSSMEnsemble(seeds=list(range(3, 3 + E)))] * B
            return [controller(n, fused, model=m, seed=1 + i) for i, m in enumerate(models)]
        groups = {"chain": group(False)}
        if not stagewise_only:
            groups = {"fused": group(True), **groups}
        obs = [0.1 * np.random.RandomState(i).randn(O_) for i in range(B)]

        def step(cs):   # (every step ends in its device-to-host copy of the result)
            return [cs[0].get_action(obs[0], None)] if B == 1 else (MpcRandomHip.get_action_batch_own_models if E == 1 else MpcRandomHip.get_action_batch)(cs, obs)

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
            got, want = step(groups["fused"]), step(groups["chain"])
            same = all(np.array_equal(a, b) for a, b in zip(got, want)) and all(
                a.best_traj_idx == b.best_traj_idx and torch.equal(a._last_costs, b._last_costs) for a, b in zip(*groups.values()))
            extra = f" | equal bits: {same}; launches per fused step {groups['fused'][0].planner.random_batch_launches}"
        t = {k: [] for k in groups}
        for _ in range(MODELS_BLOCKS):
            for k, cs in groups.items():
                t[k].append(block(cs, MODELS_BLOCK))
        line = " | ".join(f"{k} median {sorted(v)[len(v) // 2]:7.4f} ms per step (min {min(v):.4f}, max {max(v):.4f})" for k, v in t.items())
        if not stagewise_only:
            f, s_ = (sorted(t[k])[MODELS_BLOCKS // 2] for k in ("fused", "chain"))
            extra = f" | chain / fused {s_ / f:.2f}x | fused median < chain min: {f < min(t['chain'])}" + extra
        print(f"  B = {B} E = {E}: {line}{extra}", flush=True)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("no GPU: this tool measures and has nothing to say without one")
    if MODELS:
        main_models()
    elif LEARNED and "--events" in sys.argv:
        main_events()
    elif "--batch" in sys.argv:
        main_batch()
    else:
        main()
