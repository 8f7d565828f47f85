"""An ensemble's population score through the learned dynamics, three ways, at N = 1024 rows, h = 12, d = 6 and E = 2 / 4 / 5 /
8 members, in one process, warm, the legs timed in alternating blocks (median of BLOCKS blocks of at least BLOCK_S seconds
each, every block ended by a device synchronise):
  (a) one icem_rssm_rollout_cost_ensemble call: ONE split launch of E problems that share the action rows + the reduction;
  (b) what a caller did before that entry existed: E icem_rssm_rollout_cost_w launches + torch.stack(...).mean(0) -- the
      baseline; this leg binds nothing new (plain ctypes), so it runs identically on an older library (--baseline-only);
  (c) the floor: the same-weights icem_rssm_rollout_cost_batch_w with B = E (E problems of N rows, ONE parameter buffer).
(a) - (c) is the price of distinct weights (E models' GRU weights instead of one through the L2s) plus the reduction launch.

  python tools/rssm_ensemble_bench.py                    the table
  python tools/rssm_ensemble_bench.py --baseline-only    leg (b) alone
  python tools/rssm_ensemble_bench.py --trace E          leg (a) alone at E members, 200 calls, for a kernel trace of its own
                                                         (rocprofv3 --kernel-trace --stats -d DIR -- python tools/... --trace 8)
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from icem_amd import _lib as L  # noqa: E402
from icem_amd.models import declared_rssm, pack_rssm  # noqa: E402

N, H, D = 1024, 12, 6
MEMBERS = (2, 4, 5, 8)
BLOCKS, BLOCK_S, WARMUP = 7, 0.25, 20
VP = C.c_void_p


def check(lib, rc):
    if rc != 0:
        raise RuntimeError(f"rc {rc}: {lib.icem_last_error().decode()}")


def block(fn):
    """us per call of fn over one block: calls back to back for at least BLOCK_S seconds, then a device synchronise."""
    torch.cuda.synchronize()
    t0, calls = time.perf_counter(), 0
    while True:
        for _ in range(50):
            fn()
        calls += 50
        if time.perf_counter() - t0 >= BLOCK_S:
            break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def plain_library():
    lib = C.CDLL(L.lib_path())
    lib.icem_last_error.restype = C.c_char_p
    lib.icem_build_hash.restype = C.c_char_p
    lib.icem_rssm_rollout_cost_w.restype = C.c_int
    lib.icem_rssm_rollout_cost_w.argtypes = [C.c_int32] * 4 + [VP] * 5
    return lib


def inputs(E):
    params = [pack_rssm(declared_rssm(seed=10 + e, device="cuda:0").module).to("cuda:0") for e in range(E)]
    rs = np.random.RandomState(1)
    obs = torch.as_tensor((0.3 * rs.randn(E, 230)).astype(np.float32), device="cuda")   # (row 0: the ensemble's observation)
    acts = torch.as_tensor(rs.uniform(-1, 1, (N, H, D)).astype(np.float32), device="cuda")
    return params, obs, acts


def leg_solos(lib, params, obs, acts, st):
    E = len(params)
    member = [torch.empty(N, device="cuda") for _ in range(E)]

    def solos():
        for e in range(E):
            check(lib, lib.icem_rssm_rollout_cost_w(N, H, D, 0, VP(params[e].data_ptr()), VP(obs.data_ptr()), VP(acts.data_ptr()),
                                                    VP(member[e].data_ptr()), st))
        return torch.stack(member).mean(0)

    return solos


def main():
    if not torch.cuda.is_available():
        sys.exit("no GPU: this tool measures and has nothing to say without one")
    st = VP(torch.cuda.current_stream().cuda_stream)
    plain = plain_library()
    print(f"build {plain.icem_build_hash().decode()}  device {torch.cuda.get_device_name(0)}  N = {N}, h = {H}, d = {D}; median of "
          f"{BLOCKS} alternating blocks of >= {BLOCK_S} s, us per population score")
    if "--baseline-only" in sys.argv:
        print("   E | (b) E solo + torch mean us")
        for E in MEMBERS:
            params, obs, acts = inputs(E)
            f = leg_solos(plain, params, obs, acts, st)
            for _ in range(WARMUP):
                f()
            print(f"  {E:2d} | {float(np.median([block(f) for _ in range(BLOCKS)])):10.1f}")
        return
    lib = L.load_library()
    if "--trace" in sys.argv:
        E = int(sys.argv[sys.argv.index("--trace") + 1])
        params, obs, acts = inputs(E)
        ptrs = (VP * E)(*[p.data_ptr() for p in params])
        mc, costs = torch.empty(E, N, device="cuda"), torch.empty(N, device="cuda")
        for _ in range(200):
            check(lib, lib.icem_rssm_rollout_cost_ensemble(E, ptrs, N, H, D, 0, 0, VP(obs.data_ptr()), VP(acts.data_ptr()),
                                                           VP(mc.data_ptr()), VP(costs.data_ptr()), st))
        torch.cuda.synchronize()
        print(f"200 ensemble calls at E = {E}; checksum {float(costs.sum()):.6f}")
        return
    print("   E | (a) ensemble us | (b) E solo + mean us | (c) same-weights batch us | (a)/(b) | (a)-(c) us | (a) == (b) bits")
    for E in MEMBERS:
        params, obs, acts = inputs(E)
        ptrs = (VP * E)(*[p.data_ptr() for p in params])
        mc, costs = torch.empty(E, N, device="cuda"), torch.empty(N, device="cuda")
        acts_b, costs_b = acts.repeat(E, 1, 1).contiguous(), torch.empty(E * N, device="cuda")
        rows = (C.c_int32 * E)(*([N] * E))

        def ensemble():
            check(lib, lib.icem_rssm_rollout_cost_ensemble(E, ptrs, N, H, D, 0, 0, VP(obs.data_ptr()), VP(acts.data_ptr()),
                                                           VP(mc.data_ptr()), VP(costs.data_ptr()), st))

        def batch():
            check(lib, lib.icem_rssm_rollout_cost_batch_w(E, rows, H, D, 0, VP(params[0].data_ptr()), VP(obs.data_ptr()),
                                                          VP(acts_b.data_ptr()), VP(costs_b.data_ptr()), st))

        solos = leg_solos(plain, params, obs, acts, st)
        legs = (ensemble, solos, batch)
        for f in legs:
            for _ in range(WARMUP):
                f()
        torch.cuda.synchronize()
        same = bool(torch.equal(costs, solos()))   # (mean: the same three float32 operations in the same order)
        t = {f.__name__: [] for f in legs}
        for _ in range(BLOCKS):
            for f in legs:
                t[f.__name__].append(block(f))
        a, b, c = (float(np.median(t[k])) for k in ("ensemble", "solos", "batch"))
        print(f"  {E:2d} | {a:15.1f} | {b:20.1f} | {c:24.1f} | {a / b:7.3f} | {a - c:10.1f} | {same}")


if __name__ == "__main__":
    main()
