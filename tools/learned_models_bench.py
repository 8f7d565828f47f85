"""The MPC step through ensembles and through a model per controller, two ways, at N = 1024, h = 12, d = 6, K = 10, 5 CEM
iterations, for (B controllers, E members) = (1, 2), (1, 5), (4, 1: a plain model each, own_models=True), (4, 5), (6, 5): in one
process, warm, on twin controllers that start from the same state, the two legs timed in alternating blocks (median of
BLOCKS blocks of at least BLOCK_S seconds each; a step ends in its device-to-host copy of the result, so every step is
synchronised):
  (a) get_action / get_action_batch as they come: icem_plan_step_learned_models, 3 launches per iteration (+ 1 with shifted elites);
  (b) the same call under set_option("learned_step", 0): the stage-wise loop -- per controller a sampler and an update launch per
      iteration, one scoring launch, the reduction launch, and Python between them.  This is the path before the entry existed.
Printed per shape: us per MPC step of both legs, the ratio, the min .. max of the blocks (the run-to-run spread a difference has
to exceed), the launches of a fused step, and whether the twins executed the same actions throughout (they must: same bits).

  python tools/learned_models_bench.py              the table
  python tools/learned_models_bench.py --trace B E  200 fused steps and 200 stage-wise steps at one shape, for a kernel trace of
                                                    its own (rocprofv3 --kernel-trace --stats -d DIR -- python tools/... --trace 4 5):
                                                    update_small_members_batch_kernel against update_small_kernel +
                                                    rssm_ensemble_reduce_kernel, per launch
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from icem_amd import DeviceRSSMEnsemble, DeviceRSSMModel, MpcICemHip, halfcheetah_env  # noqa: E402
from icem_amd import _lib as L  # noqa: E402
from icem_amd import build as B_  # noqa: E402

N, H, K, ITERS = 1024, 12, 10, 5
SHAPES = ((1, 2), (1, 5), (4, 1), (4, 5), (6, 5))
BLOCKS, BLOCK_S, WARMUP = 7, 0.25, 10
ASP = dict(alpha=0.1, elites_size=K, opt_iterations=ITERS, init_std=0.5, use_mean_actions=True, keep_previous_elites=True,
           shift_elites_over_time=True, fraction_elites_reused=0.3, noise_beta=0.25)


def controllers(B, E, models):
    """B controllers: on ONE E-member ensemble (E > 1), or with a plain model each (E == 1)."""
    ens = DeviceRSSMEnsemble(models=models[:E]) if E > 1 else None
    out = []
    for i in range(B):
        m = ens if ens is not None else models[i]
        out.append(MpcICemHip(env=halfcheetah_env(17), forward_model=m, horizon=H, num_simulated_trajectories=N, factor_decrease_num=1.25,
                              cost_along_trajectory="sum", dtype="f32", seed=i + 1, action_sampler_params=dict(ASP)))
    return out


class Leg:
    def __init__(self, B, E, models, fused, obs0):
        self.ctrls, self.fused, self.obs0, self.k, self.B, self.E = controllers(B, E, models), fused, obs0, 0, B, E
        for c, ob in zip(self.ctrls, obs0):
            c.beginning_of_rollout(observation=ob, state=None, mode="train")
        self.actions = []

    def step(self):
        obs = [ob + 0.001 * (self.k % 50) for ob in self.obs0]
        self.k += 1
        L.set_option("learned_step", 1 if self.fused else 0)
        if self.B == 1:
            a = [self.ctrls[0].get_action(obs[0], None)]
        else:
            a = MpcICemHip.get_action_batch(self.ctrls, obs, own_models=self.E == 1)
        L.set_option("learned_step", 1)
        return a

    def block(self):
        torch.cuda.synchronize()
        t0, calls = time.perf_counter(), 0
        while True:
            for _ in range(5):
                self.actions.append(np.stack(self.step()))
            calls += 5
            if time.perf_counter() - t0 >= BLOCK_S:
                break
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / calls * 1e6


def main():
    if not torch.cuda.is_available():
        sys.exit("no GPU: this tool measures and has nothing to say without one")
    models = [DeviceRSSMModel(seed=10 + e) for e in range(6)]
    rs = np.random.RandomState(1)
    if "--trace" in sys.argv:
        at = sys.argv.index("--trace")
        B, E = int(sys.argv[at + 1]), int(sys.argv[at + 2])
        obs0 = [0.3 * rs.randn(230) for _ in range(B)]
        for fused in (True, False):
            leg = Leg(B, E, models, fused, obs0)
            for _ in range(200):
                leg.step()
            torch.cuda.synchronize()
            print(f"200 {'fused' if fused else 'stage-wise'} steps at B = {B}, E = {E}; launches of a fused step: "
                  f"{leg.ctrls[0].planner.learned_step_launches}")
        return
    print(f"build {B_.build_info()['built_from']}  device {torch.cuda.get_device_name(0)}  N = {N}, h = {H}, K = {K}, {ITERS} iterations; "
          f"median of {BLOCKS} alternating blocks of >= {BLOCK_S} s, us per MPC step (all B controllers)")
    print("  B  E | (a) fused us  [min .. max] | (b) stage-wise us  [min .. max] | (a)/(b) | launches (a) | same actions")
    for B, E in SHAPES:
        obs0 = [0.3 * rs.randn(230) for _ in range(B)]
        a, b = Leg(B, E, models, True, obs0), Leg(B, E, models, False, obs0)
        for leg in (a, b):
            for _ in range(WARMUP):
                leg.actions.append(np.stack(leg.step()))
        launches = a.ctrls[0].planner.learned_step_launches
        assert launches > 0 and b.ctrls[0].planner.learned_step_launches == 0, "which path each leg took"
        ta, tb = [], []
        for _ in range(BLOCKS):
            ta.append(a.block())
            tb.append(b.block())
        n = min(len(a.actions), len(b.actions))
        same = all(np.array_equal(x, y) for x, y in zip(a.actions[:n], b.actions[:n]))
        ma, mb = float(np.median(ta)), float(np.median(tb))
        print(f" {B:2d} {E:2d} | {ma:10.1f}  [{min(ta):.1f} .. {max(ta):.1f}] | {mb:10.1f}  [{min(tb):.1f} .. {max(tb):.1f}] | {ma / mb:7.3f} | "
              f"{launches:12d} | {same}")


if __name__ == "__main__":
    main()
