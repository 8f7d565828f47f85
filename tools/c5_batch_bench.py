"""The batched learned-dynamics launch (icem_rssm_rollout_cost_batch) against its two alternatives, same process, warm,
bracketed by events (as tools/c5_bench.py does), B problems of 1024 rows at h = 12 with distinct observations:
  (a) one batched launch;  (b) B launches of 1024 rows;  (c) one launch of B * 1024 rows (one observation: the yardstick --
      the batch is that launch plus a table scan and B - 1 further observation reads).
The three are timed in turns, ROUNDS times, and the medians printed.  Then ms per MPC step of
MpcICemHip.get_action_batch over B controllers (BASELINE configs[4]: N = 1024 x 5 iterations) against B x get_action.

  python tools/c5_batch_bench.py            the table
  python tools/c5_batch_bench.py --solo     icem_rssm_rollout_cost alone at N = 1024 and 8192 through plain ctypes -- it
                                            binds nothing else, so it also runs on a library from before the batched entry
                                            (tools/experiments/ab_libs.sh "python tools/c5_batch_bench.py --solo" 0 P 0 P)
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from icem_amd import _lib as L  # noqa: E402
from icem_amd import build as B_  # noqa: E402
from icem_amd.models import declared_rssm, pack_rssm  # noqa: E402

H, D, ROWS, REPS, ROUNDS = 12, 6, 1024, 20, 5
VP = C.c_void_p


def timed(fn, reps=REPS):
    """us per call of fn over `reps` back-to-back calls between two events."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / reps


def check(lib, rc):
    if rc != 0:
        raise RuntimeError(f"rc {rc}: {lib.icem_last_error().decode()}")


def solo_only():
    lib = C.CDLL(L.lib_path())
    lib.icem_rssm_rollout_cost.restype = C.c_int
    lib.icem_rssm_rollout_cost.argtypes = [C.c_int32] * 3 + [VP] * 5
    lib.icem_last_error.restype = C.c_char_p
    lib.icem_build_hash.restype = C.c_char_p
    params = pack_rssm(declared_rssm(seed=3, device="cuda:0").module).to("cuda:0")
    obs = torch.as_tensor((0.3 * np.random.RandomState(1).randn(230)).astype(np.float32), device="cuda")
    st = VP(torch.cuda.current_stream().cuda_stream)
    for n in (1024, 8192):
        acts = torch.rand(n, H, D, device="cuda") * 2 - 1
        costs = torch.empty(n, device="cuda")
        run = lambda: check(lib, lib.icem_rssm_rollout_cost(n, H, 0, VP(params.data_ptr()), VP(obs.data_ptr()), VP(acts.data_ptr()),  # noqa: E731
                                                             VP(costs.data_ptr()), st))
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        us = sorted(timed(run, 50) for _ in range(7))
        print(f"build {lib.icem_build_hash().decode()}  icem_rssm_rollout_cost n={n:5d} h={H}: median {us[3]:7.1f} us per launch "
              f"(min {us[0]:.1f}, max {us[-1]:.1f}; 7 x 50 launches)  checksum {float(costs.sum()):.6f}")


def launches():
    from icem_amd import DeviceRSSMModel
    m = DeviceRSSMModel(seed=3)
    lib, st, par = m.lib, VP(torch.cuda.current_stream().cuda_stream), VP(m.params.data_ptr())
    rs = np.random.RandomState(1)
    print(f"build {B_.build_info()['built_from']}  device {torch.cuda.get_device_name(0)}  {ROWS} rows per problem, h = {H}, "
          f"{REPS} launches per timing, median of {ROUNDS} rounds")
    print("   B | (a) batched us | (b) B solo us | (c) one B*1024 us | (a)/(c) | (a)/(b) | us per problem (a)")
    for nb in (1, 2, 4, 8, 16):
        obs = torch.as_tensor((0.3 * rs.randn(nb, 230)).astype(np.float32), device="cuda")
        acts = torch.rand(nb * ROWS, H, D, device="cuda") * 2 - 1
        costs = torch.empty(nb * ROWS, device="cuda")
        rows = (C.c_int32 * nb)(*([ROWS] * nb))
        a_, c_, o_ = acts.data_ptr(), costs.data_ptr(), obs.data_ptr()

        def batched():
            check(lib, lib.icem_rssm_rollout_cost_batch(nb, rows, H, 0, par, VP(o_), VP(a_), VP(c_), st))

        def solos():
            for p in range(nb):
                check(lib, lib.icem_rssm_rollout_cost(ROWS, H, 0, par, VP(o_ + 920 * p), VP(a_ + 4 * p * ROWS * H * D), VP(c_ + 4 * p * ROWS), st))

        def one():
            check(lib, lib.icem_rssm_rollout_cost(nb * ROWS, H, 0, par, VP(o_), VP(a_), VP(c_), st))

        for f in (one, solos, batched):   # (the largest first: it sizes the staging area)
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        t = {f.__name__: [] for f in (batched, solos, one)}
        for _ in range(ROUNDS):
            for f in (batched, solos, one):
                t[f.__name__].append(timed(f))
        a, b, c = (float(np.median(t[k])) for k in ("batched", "solos", "one"))
        print(f"  {nb:2d} | {a:14.1f} | {b:13.1f} | {c:17.1f} | {a / c:7.3f} | {a / b:7.3f} | {a / nb:8.1f}")


def controllers():
    from icem_amd import DeviceRSSMModel, MpcICemHip, halfcheetah_env
    m = DeviceRSSMModel(seed=3)
    env = halfcheetah_env(17)
    asp = dict(alpha=0.1, elites_size=10, opt_iterations=5, init_std=0.5, use_mean_actions=True, keep_previous_elites=True,
               shift_elites_over_time=True, fraction_elites_reused=0.3, noise_beta=0.25)
    rs = np.random.RandomState(2)
    print("   B | get_action_batch ms per MPC step | B x get_action ms | per controller: batch / alone")
    for nb in (1, 2, 4, 8, 16):
        ctrls = [MpcICemHip(env=env, forward_model=m, horizon=H, num_simulated_trajectories=ROWS, factor_decrease_num=1.25,
                            cost_along_trajectory="sum", dtype="f32", seed=i + 1, action_sampler_params=asp) for i in range(nb)]
        obs = [0.3 * rs.randn(230) for _ in range(nb)]
        for c, ob in zip(ctrls, obs):
            c.beginning_of_rollout(observation=ob, state=None, mode="train")

        def together():
            MpcICemHip.get_action_batch(ctrls, obs)

        def alone():
            for c, ob in zip(ctrls, obs):
                c.get_action(ob, None)

        res = {}
        for f in (together, alone):
            for _ in range(3):
                f()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(REPS):
                f()
            torch.cuda.synchronize()
            res[f.__name__] = (time.perf_counter() - t0) / REPS * 1e3
        print(f"  {nb:2d} | {res['together']:32.3f} | {res['alone']:17.3f} | {res['together'] / nb:.3f} / {res['alone'] / nb:.3f}")


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("no GPU: this tool measures and has nothing to say without one")
    if "--solo" in sys.argv:
        solo_only()
    else:
        launches()
        controllers()
