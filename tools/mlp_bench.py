"""Feed-forward learned dynamics (GPU box): DeviceMLPModel.rollout_cost -- rollout and env cost fused into one launch -- against
the TorchForwardModel graph-replay path on the SAME module (h graph-replayed torch steps + icem_trajectory_cost), and
MpcICemHip.get_action on both models.  HalfCheetah shape (o = 17, d = 6, h = 30), N = 1024 and 4096, 2 and 4 hidden layers,
relu and swish.  Both paths run in one process, alternating window by window; every shape is warmed up; a window is timed
with device events and lasts at least 0.5 s; the line gives the median window and the spread (min .. max) per path.
usage: python tools/mlp_bench.py [--windows 5] [--seconds 0.5]

--models: several models in ONE launch against a launch each, same shape (2-layer relu and 4-layer swish, N = 1024 and 4096
rows per model): DeviceMLPEnsemble.rollout_cost for E = 2, 5, 8 members against E DeviceMLPModel.rollout_cost calls + a torch
mean, and mlp_rollout_cost_models for B = 4, 8 problems with a model each against B solo calls.  The two arms alternate window
by window as above.

--step: one MpcICemHip MPC step (get_action: 3 iterations, kept and shifted elites, one device-to-host copy of the result)
through a DeviceMLPEnsemble of E = 1 and E = 5 two-layer relu members two ways -- the stage-wise loop (development option
mlp_step = 0: per iteration a sampler, a rollout, a reduction and an update call from Python) and the fused call
(icem_plan_step_mlp: 3 launches per iteration, + 1 for the shifted elites) -- at N = 128 and at the benchmark's headline
population, N = 4096.  Two equal controllers, warmed up into the steady state (steps that shift elites), first checked to execute
the same bits, then timed alternating window by window as above; the line also gives the fused step's launch count."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from icem_amd import (DeviceMLPEnsemble, DeviceMLPModel, MpcICemHip, TorchForwardModel, declared_mlp, halfcheetah_env,  # noqa: E402
                      mlp_rollout_cost_models)

O, D, H = 17, 6, 30
DEV = "cuda:0"


def controller(model, N):
    asp = dict(alpha=0.1, elites_size=10, opt_iterations=3, init_std=0.5, use_mean_actions=True, keep_previous_elites=True,
               shift_elites_over_time=True, fraction_elites_reused=0.3, noise_beta=2.0)
    return MpcICemHip(env=halfcheetah_env(O), forward_model=model, horizon=H, num_simulated_trajectories=N, factor_decrease_num=1.25,
                      cost_along_trajectory="sum", dtype="f32", seed=1, action_sampler_params=asp)


def window(fn, seconds):
    """us per call of fn over one window of at least `seconds`, by device events."""
    reps, done, total_ms = 8, 0, 0.0
    while total_ms < seconds * 1e3:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        total_ms += a.elapsed_time(b)
        done += reps
        reps = min(reps * 2, 4096)
    return total_ms * 1e3 / done


def alternate(fns, windows, seconds):
    """{name: [us per call per window]} with the paths taking turns window by window."""
    out = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            out[k].append(window(fn, seconds))
    return out


def fmt(v):
    return f"{np.median(v):9.1f} us ({min(v):.1f} .. {max(v):.1f})"


def models_bench(args):
    """One launch for several models against a launch per model."""
    rs = np.random.RandomState(0)
    obs = 0.1 * rs.randn(O)
    for layers, act in ((2, "relu"), (4, "swish")):
        members = []
        for seed in range(8):
            net = declared_mlp(O, D, layers=layers, activation=act, seed=seed, device="cpu").module
            with torch.no_grad():
                net.out.weight.mul_(0.1)   # keeps the random network's state bounded over 30 steps
            members.append(DeviceMLPModel(module=net, env=halfcheetah_env(O), device=DEV))
        for N in (1024, 4096):
            actions = torch.as_tensor(rs.uniform(-1, 1, (N, H, D)), dtype=torch.float32, device=DEV)
            for E in (2, 5, 8):
                ens = DeviceMLPEnsemble(models=members[:E])
                fns = {"one": lambda: ens.rollout_cost(obs, actions),
                       "each": lambda: torch.stack([m.rollout_cost(obs, actions) for m in members[:E]]).mean(0)}
                for fn in fns.values():
                    for _ in range(5):
                        fn()
                torch.cuda.synchronize()
                assert torch.equal(ens.member_costs, torch.stack([m.rollout_cost(obs, actions) for m in members[:E]]))
                r = alternate(fns, args.windows, args.seconds)
                print(f"ensemble  L={layers} {act:5s} N={N:5d} E={E}  one launch + reduce {fmt(r['one'])}  E launches + torch mean {fmt(r['each'])}  "
                      f"ratio {np.median(r['each']) / np.median(r['one']):5.2f}", flush=True)
            for B in (4, 8):
                many = torch.as_tensor(rs.uniform(-1, 1, (B * N, H, D)), dtype=torch.float32, device=DEV)
                slices = [many[b * N:(b + 1) * N] for b in range(B)]
                obs_dev = torch.as_tensor(np.tile(obs.astype(np.float32), (B, 1)), device=DEV)
                fns = {"one": lambda: mlp_rollout_cost_models(members[:B], obs_dev, many, [N] * B),
                       "each": lambda: [m.rollout_cost(obs, a) for m, a in zip(members[:B], slices)]}
                for fn in fns.values():
                    for _ in range(5):
                        fn()
                torch.cuda.synchronize()
                assert torch.equal(fns["one"](), torch.cat(fns["each"]()))
                r = alternate(fns, args.windows, args.seconds)
                print(f"models    L={layers} {act:5s} N={N:5d} B={B}  one launch {fmt(r['one'])}  B launches {fmt(r['each'])}  "
                      f"ratio {np.median(r['each']) / np.median(r['one']):5.2f}", flush=True)


def step_bench(args):
    """One MPC step through a DeviceMLPEnsemble: the stage-wise loop against the fused call."""
    from icem_amd import _lib as L
    rs = np.random.RandomState(0)
    obs = 0.1 * rs.randn(O)
    members = []
    for seed in range(5):
        net = declared_mlp(O, D, layers=2, activation="relu", seed=seed, device="cpu").module
        with torch.no_grad():
            net.out.weight.mul_(0.1)   # keeps the random network's state bounded over 30 steps
        members.append(DeviceMLPModel(module=net, env=halfcheetah_env(O), device=DEV))
    for E in (1, 5):
        for N in (128, 4096):
            legs = {"stage": controller(DeviceMLPEnsemble(models=members[:E]), N), "fused": controller(DeviceMLPEnsemble(models=members[:E]), N)}

            def step(name):
                L.set_option("mlp_step", 1 if name == "fused" else 0)
                try:
                    return legs[name].get_action(obs, None)
                finally:
                    L.set_option("mlp_step", 1)
            for c in legs.values():
                c.beginning_of_rollout(observation=obs, state=None, mode="train")
            for k in range(5):   # warm-up into the steady state, and the two arrangements' bits
                a, b = step("stage"), step("fused")
                assert np.array_equal(a, b) and legs["stage"].last_min_cost == legs["fused"].last_min_cost, (E, N, k)
            launches = legs["fused"].planner.mlp_step_launches
            assert launches == 3 * 3 + 1 and legs["stage"].planner.mlp_step_launches == 0, "which path each leg took"
            r = alternate({k: (lambda k=k: step(k)) for k in legs}, args.windows, args.seconds)
            print(f"mpc step  E={E} N={N:5d}  stage-wise {fmt(r['stage'])}  fused {fmt(r['fused'])}  "
                  f"ratio {np.median(r['stage']) / np.median(r['fused']):5.2f}  fused launches {launches}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--models", action="store_true", help="several models in one launch against a launch each")
    ap.add_argument("--step", action="store_true", help="one MPC step through an ensemble: the stage-wise loop against the fused call")
    args = ap.parse_args()
    rs = np.random.RandomState(0)
    obs = 0.1 * rs.randn(O)
    print(f"# {torch.cuda.get_device_name(0)}; o={O} d={D} h={H}; {args.windows} windows of >= {args.seconds} s per path, alternating", flush=True)
    if args.models:
        return models_bench(args)
    if args.step:
        return step_bench(args)
    for layers in (2, 4):
        for act in ("relu", "swish"):
            net = declared_mlp(O, D, layers=layers, activation=act, seed=0, device="cpu").module
            with torch.no_grad():
                net.out.weight.mul_(0.1)   # keeps the random network's state bounded over 30 steps
            dev_model = DeviceMLPModel(module=net, env=halfcheetah_env(O), device=DEV)
            torch_model = TorchForwardModel(net, None, O, D, device=DEV, env=halfcheetah_env(O))
            for N in (1024, 4096):
                cd, ct = controller(dev_model, N), controller(torch_model, N)
                assert cd.rssm_path and ct.torch_path and ct.torch_spec_cost
                actions = torch.as_tensor(rs.uniform(-1, 1, (N, H, D)), dtype=torch.float32, device=DEV)
                fns = {"fused": lambda: cd._costs_of(obs, actions), "torch": lambda: ct._costs_of(obs, actions)}
                for fn in fns.values():   # warm-up: the graph capture of the torch chain, lazy initialisations
                    for _ in range(5):
                        fn()
                torch.cuda.synchronize()
                a, b = fns["fused"]().float(), fns["torch"]().float()
                diff = float((a - b).abs().max() / (1 + b.abs().max()))
                r = alternate(fns, args.windows, args.seconds)
                print(f"rollout_cost  L={layers} {act:5s} N={N:5d}  fused {fmt(r['fused'])}  torch graph {fmt(r['torch'])}  "
                      f"ratio {np.median(r['torch']) / np.median(r['fused']):5.2f}  max cost diff {diff:.1e} (bf16 vs f32 operands)", flush=True)
                for c in (cd, ct):
                    c.beginning_of_rollout(observation=obs, state=None, mode="train")
                steps = {"fused": lambda: cd.get_action(obs, None), "torch": lambda: ct.get_action(obs, None)}
                for fn in steps.values():
                    for _ in range(3):
                        fn()
                g = alternate(steps, max(args.windows // 2, 2), args.seconds)
                print(f"get_action    L={layers} {act:5s} N={N:5d}  fused {fmt(g['fused'])}  torch graph {fmt(g['torch'])}  "
                      f"ratio {np.median(g['torch']) / np.median(g['fused']):5.2f}", flush=True)


if __name__ == "__main__":
    main()
