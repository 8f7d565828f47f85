"""Cases of the learned-dynamics rollout at action widths other than the declared six (a plain module, no fixtures), shared by
test_rssm_width_sensitivity_cpu.py and test_gpu_rssm_widths.py.  The criterion is rssm_cases.py's, bounds and all
(``violations``: median 1.9e-7, share of rows above 2e-5 at most 0.314, maximum 3.4e-2); the reference is the same float64
emulation of the kernel's rounding points (oracle/rssm_oracle.py::emulated_costs, which takes any width), the model
``declared_rssm(act_dim=d)`` with every weight matrix times the case's gain.

The widths are the edges of what the kernels do with an action row: a lane holds four entries (1, 2, 3, 4, 5, 7, 8, 9), a
wave's lane quads sixteen (16, 17), the action K block thirty-two (31, 32); 6 is the control.  Every width runs 1007 x 12 in
'sum' and 'best' (seed / gain / observation of rssm_cases.py's cases of that shape); widths 1, 5 and 32 also 4097 x 12 (the
257th tile: two tiles per recurrence workgroup), h = 1 (no transition: the initial staging alone) and h = 2 (one), and on
the fused kernel 17 rows (one ragged tile and one row of the next) and 8205 x 2 (513 workgroups, the last with 13 rows: at
these widths the fused launch keeps one tile per workgroup at every population).
Small populations pool several launches with observations and actions of their own, as rssm_cases.py's do.
"""
from collections import namedtuple

import numpy as np

import rssm_cases as RC
from oracle import rssm_oracle as RO

WIDTHS = [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 32]
CONTROL = 6
DEEP_WIDTHS = [1, 5, 32]          # ... also at the shapes that take another path through the launch
MUTANT_WIDTHS = [1, 5, 17, 32]    # test_rssm_width_sensitivity_cpu.py

WCase = namedtuple("WCase", "name d wseed gain obs n h mode launches kernel")


def _table():
    out = []
    for d in sorted(WIDTHS + [CONTROL]):
        out.append(WCase(f"d{d}-s3g1-randn-sum-1007x12", d, 3, 1.0, ("randn", 4, 0.3), 1007, 12, "sum", 1, "split"))
        out.append(WCase(f"d{d}-s0g1.5-settled-best-1007x12", d, 0, 1.5, ("settled", 10, 8), 1007, 12, "best", 1, "split"))
    for d in DEEP_WIDTHS:
        out.append(WCase(f"d{d}-s1g1-settled-best-4097x12", d, 1, 1.0, ("settled", 11, 8), 4097, 12, "best", 1, "split"))
        out.append(WCase(f"d{d}-s3g1-settled-best-13x1", d, 3, 1.0, ("settled", 40, 8), 13, 1, "best", 10, "split"))
        out.append(WCase(f"d{d}-s0g1.5-settled-best-509x2", d, 0, 1.5, ("settled", 51, 8), 509, 2, "best", 1, "split"))
        out.append(WCase(f"d{d}-s3g1-randn-sum-17x12-fused", d, 3, 1.0, ("randn", 4, 0.3), 17, 12, "sum", 8, "fused"))
        out.append(WCase(f"d{d}-s1g1-settled-best-8205x2-fused", d, 1, 1.0, ("settled", 11, 8), 8205, 2, "best", 1, "fused"))
    return out


CASES = _table()
WIDE_CASES = [c for c in CASES if c.n == 1007]

_modules = {}


def module(case):
    """The f32 torch module of the case (CPU): declared_rssm(act_dim = d, seed = wseed), every weight matrix times gain."""
    import torch
    from icem_amd.models import declared_rssm
    key = (case.d, case.wseed, case.gain)
    if key not in _modules:
        net = declared_rssm(act_dim=case.d, seed=case.wseed, device="cpu").module
        with torch.no_grad():
            for p in net.parameters():
                if p.ndim > 1:
                    p.mul_(case.gain)
        _modules[key] = net
    return _modules[key]


def params(case) -> dict:
    return RO.params_from_state_dict(module(case).state_dict())


def launches(case, rows=None):
    """[(obs [230], actions [n, h, d])] of the case; ``rows`` caps the rows of a launch (the CPU sensitivity test)."""
    P = params(case)
    n = case.n if rows is None else min(case.n, rows)
    out = []
    for i in range(case.launches):
        kind, seed, arg = case.obs
        rs = np.random.RandomState(seed + 1000 * i)
        if kind == "randn":
            ob = arg * rs.randn(RC.DET + RC.STOCH)
        else:
            ob = 0.3 * rs.randn(1, RC.DET + RC.STOCH)
            for _ in range(arg):
                ob = RO.step(P, ob, rs.uniform(-1, 1, (1, case.d)))
            ob = ob[0]
        out.append((ob, np.random.RandomState(seed + 1000 * i + 500).uniform(-1, 1, (n, case.h, case.d))))
    return out


def over_launches(case, fn, rows=None) -> np.ndarray:
    return np.concatenate([fn(ob, acts) for ob, acts in launches(case, rows)], 0)


def want(case, rows=None) -> np.ndarray:
    """The float64 emulation of the kernel's rounding points."""
    P = params(case)
    return over_launches(case, lambda ob, a: RO.emulated_costs(P, ob, a, case.mode, q=RO.bf16), rows)


def kernel_standin(case, rows=None, seed=0, actions=None) -> np.ndarray:
    """rssm_cases.py::kernel_standin at the case's width: float32, K blocked by 32, activations off by up to +-2 ulp.
    ``actions``: what a (wrong) staging makes of a launch's action tensor -- the mutants of the CPU test."""
    P = params(case)
    rng = np.random.RandomState(seed)
    kw = dict(q=RO.bf16, dtype=np.float32, kblock=32, act_ulp=2.0, rng=rng)
    see = actions or (lambda a: a)
    return over_launches(case, lambda ob, a: RO.emulated_costs(P, ob, see(a), case.mode, **kw), rows).astype(np.float64)


errors, violations, agree = RC.errors, RC.violations, RC.agree
