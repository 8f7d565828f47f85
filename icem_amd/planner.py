"""Torch-tensor level wrapper of the C ABI: one :class:`IcemPlanner` per controller.

PyTorch is plumbing here (device memory, streams, ``torch.distributed``); all
arithmetic happens in ``libicem_hip.so``.  Each method names the reference
call site it replaces (paths relative to ``/root/reference``).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Callable, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .distributed import exchange_records, shard_range


@dataclass
class IcemConfig:
    """Constructor kwargs of the reference's ``MpcICem`` (icem/controllers/icem.py:213-233,
    icem/controllers/mpc.py:22) plus the device-side knobs."""
    horizon: int
    act_dim: int
    num_traj: int
    elites_size: int = 10
    opt_iters: int = 3
    cost_mode: str = "sum"
    use_mean_actions: bool = True
    keep_previous_elites: bool = True
    shift_elites: bool = True
    factor_decrease: float = 1.25
    alpha: float = 0.1
    init_std: float = 0.5
    fraction_reused: float = 0.3
    noise_beta: float = 0.25
    dtype: str = "f32"
    rng_rounds: int = 10
    seed: int = 0
    rank: int = 0
    world: int = 1

    @property
    def num_elites(self) -> int:
        # icem/controllers/icem.py:235-240
        return max(2, min(self.elites_size, self.num_traj // 2))

    @property
    def torch_dtype(self):
        return torch.float64 if self.dtype == "f64" else torch.float32

    def to_c(self) -> L.IcemConfigC:
        if self.cost_mode not in L.COST_MODES:
            raise NotImplementedError(
                "Implement method {} to compute cost along trajectory".format(self.cost_mode))
        return L.IcemConfigC(
            horizon=self.horizon, act_dim=self.act_dim, num_traj=self.num_traj, num_elites=self.num_elites,
            elites_size=self.elites_size, opt_iters=self.opt_iters, cost_mode=L.COST_MODES[self.cost_mode],
            use_mean_actions=int(self.use_mean_actions), keep_previous_elites=int(self.keep_previous_elites),
            shift_elites=int(self.shift_elites), dtype=L.ICEM_F64 if self.dtype == "f64" else L.ICEM_F32,
            rng_rounds=self.rng_rounds, rank=self.rank, world=self.world, factor_decrease=self.factor_decrease,
            alpha=self.alpha, init_std=self.init_std, fraction_reused=self.fraction_reused,
            noise_beta=self.noise_beta, seed=self.seed & 0xFFFFFFFFFFFFFFFF)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


# noise callback of the parity mode: noise(num_traj) -> (z_r, z_i) float64 arrays [num, d, F]
# (noise_beta <= 0, the white branch of icem.py:77: -> (randn [num, h, d], None))
NoiseFn = Callable[[int], Tuple[np.ndarray, np.ndarray]]


class IcemPlanner:
    """Owns one ``icem_handle`` and the device buffers of one controller."""

    def __init__(self, cfg: IcemConfig, low, high, device="cuda:0", process_group=None):
        self.lib = L.load_library()
        L.maybe_follow_environment()   # (tools only: icem_amd._lib.follow_environment)
        if not torch.cuda.is_available():
            raise RuntimeError("icem_amd needs a HIP device (torch.cuda.is_available() is False); "
                               "there is no CPU fallback")
        self.cfg = cfg
        self.device = torch.device(device)
        self.dt = cfg.torch_dtype
        self.group = process_group
        torch.cuda.set_device(self.device)
        self._h = C.c_void_p()
        ccfg = cfg.to_c()
        L.check(self.lib.icem_create(C.byref(ccfg), C.byref(self._h)))
        if L._FOLLOW_ENV and os.environ.get("ICEM_TILE_ARITH", "") != "":   # (tools only; the arithmetic is the HANDLE's)
            L.check(self.lib.icem_set_tile_arith(self._h, int(os.environ["ICEM_TILE_ARITH"])))
        self.h, self.d, self.K = cfg.horizon, cfg.act_dim, cfg.num_elites
        self.F = self.h // 2 + 1
        self.low = torch.as_tensor(np.asarray(low, dtype=np.float64), dtype=self.dt, device=self.device).contiguous()
        self.high = torch.as_tensor(np.asarray(high, dtype=np.float64), dtype=self.dt, device=self.device).contiguous()
        if self.low.shape != (self.d,) or self.high.shape != (self.d,):
            raise ValueError("low/high must have shape [act_dim]")
        pops = (C.c_int32 * cfg.opt_iters)()
        L.check(self.lib.icem_population_sizes(self._h, pops))
        self.population_sizes = list(pops)
        self.n_reuse = int(self.K * cfg.fraction_reused)
        self.obs_dim = 0
        self._bufs = None
        self.mpc_step = 0
        self.episode = 0           # folded into the device noise streams (icem_set_episode)
        self._episodes_started = 0
        self._topk_ws = None

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self.lib.icem_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # ------------------------------------------------------------------ model / cost
    def set_model(self, kind: int, A: np.ndarray, B: np.ndarray):
        """Built-in batched model ``o' = act(o@A + a@B)`` (predict contract of
        icem/models/abstract_models.py:17-26)."""
        A = np.ascontiguousarray(A, dtype=np.float64)
        B = np.ascontiguousarray(B, dtype=np.float64)
        o = A.shape[0]
        if A.shape != (o, o) or B.shape != (self.d, o):
            raise ValueError("A must be [o,o] and B [act_dim,o]")
        L.check(self.lib.icem_set_model(self._h, kind, o, A.ctypes.data_as(C.POINTER(C.c_double)),
                                        B.ctypes.data_as(C.POINTER(C.c_double))))
        self.obs_dim = o
        self._bufs = None
        self._cem = None
        self._random = None

    def set_cost(self, ctrl_weight=0.1, lin_idx=8, lin_weight=-1.0, flip_idx=1, flip_penalty=10.0,
                 flip_thresh=float(np.pi / 2)):
        """Parametric HalfCheetah / HumanoidStandup cost (icem/environments/mujoco.py:67-99, 259-277)."""
        spec = L.IcemCostSpecC(ctrl_weight, lin_weight, flip_penalty, flip_thresh, lin_idx, flip_idx)
        L.check(self.lib.icem_set_cost(self._h, C.byref(spec)))

    def sample_piecewise(self, n: int, call_offset: int, change_freq: int, u=None, first_block: int = 0) -> torch.Tensor:
        """``MpcRandom.sample_action_sequences`` (icem/controllers/mpc.py:96-109): ``[n, h, d]`` uniform actions held
        over consecutive ``sample()`` calls (``icem_sample_piecewise``).  ``u``: the draws ``[*, d]`` of blocks
        ``first_block..`` (parity), or None for the device's Philox streams."""
        actions = torch.empty((n, self.h, self.d), dtype=self.dt, device=self.device)
        u_t = None if u is None else self._t(u)
        L.check(self.lib.icem_sample_piecewise(self._h, n, int(call_offset), int(change_freq), int(first_block),
                                               _ptr(self.low), _ptr(self.high), _ptr(u_t), _ptr(actions), self._stream()))
        return actions

    def set_cost_spec(self, spec):
        """The whole parametric cost of an env (``envs.CostSpec``): the HalfCheetah / HumanoidStandup form plus the
        Ant / Hopper / Humanoid / Reacher / Fetch terms (``icem_set_cost_terms``)."""
        self.set_cost(spec.ctrl_weight, spec.lin_idx, spec.lin_weight, spec.flip_idx, spec.flip_penalty, spec.flip_thresh)
        if not getattr(spec, "extended", False):
            L.check(self.lib.icem_set_cost_terms(self._h, None))
            return
        if len(spec.terms) > L.MAX_COST_TERMS:
            raise ValueError(f"at most {L.MAX_COST_TERMS} cost terms")
        t = L.IcemCostTermsC(
            diff_weight=spec.diff_weight, health_penalty=spec.health_penalty, health_lo=spec.health_lo,
            health_hi=spec.health_hi, box_lo=spec.box_lo, box_hi=spec.box_hi, diff_idx=spec.diff_idx,
            health_idx=spec.health_idx, health_closed=int(spec.health_closed), box_from=spec.box_from,
            n_terms=len(spec.terms))
        for j, tm in enumerate(spec.terms):
            t.terms[j] = L.IcemCostTermC(weight=tm.weight, thresh=tm.thresh, gate_thresh=tm.gate_thresh, kind=tm.kind,
                                         a=tm.a, b=tm.b, len=tm.len, gate_idx=tm.gate_idx)
        L.check(self.lib.icem_set_cost_terms(self._h, C.byref(t)))

    def trajectory_cost(self, observations, actions, next_observations=None) -> torch.Tensor:
        """``trajectory_cost_fn`` (abstract_controller.py:74-91) on the device for rollouts held as tensors:
        ``observations`` / ``next_observations`` ``[n, h, o]`` (any strides over n and h, entries of a row
        contiguous -- a transposed view of a step-major ``[h, n, o]`` buffer works), ``actions [n, h, d]``."""
        n, h, o = observations.shape
        if h != self.h or observations.dtype != self.dt or observations.stride(2) != 1:
            raise ValueError("observations must be [n, horizon, o] of the planner dtype with contiguous rows")
        if next_observations is not None and (next_observations.shape != observations.shape
                                              or next_observations.stride() != observations.stride()
                                              or next_observations.dtype != self.dt):
            raise ValueError("next_observations must match observations in shape, strides and dtype")
        actions = self._t(actions, (n, self.h, self.d))
        costs = torch.empty((n,), dtype=self.dt, device=self.device)
        L.check(self.lib.icem_trajectory_cost(
            self._h, n, o, _ptr(observations), _ptr(next_observations) if next_observations is not None else None,
            observations.stride(0), observations.stride(1), _ptr(actions), _ptr(costs), self._stream()))
        return costs

    # ------------------------------------------------------------------ helpers
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _t(self, x, shape=None) -> torch.Tensor:
        t = torch.as_tensor(x, dtype=self.dt, device=self.device).contiguous()
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t

    def noise_tables(self) -> Tuple[np.ndarray, np.ndarray]:
        cr = np.zeros((self.F, self.h))
        ci = np.zeros((self.F, self.h))
        L.check(self.lib.icem_noise_tables_host(self.h, self.cfg.noise_beta, cr.ctypes.data_as(C.POINTER(C.c_double)),
                                                ci.ctypes.data_as(C.POINTER(C.c_double))))
        return cr, ci

    # ------------------------------------------------------------------ stateless operators
    def sample_clip(self, n: int, mean, std, z_r=None, z_i=None, offset: int = 0, first_index: int = 0,
                    t_begin: int = 0, row0_mean: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """K1: ``MpcICem.sample_action_sequences`` (icem/controllers/icem.py:61-82)."""
        mean = self._t(mean, (self.h, self.d))
        std = self._t(std, (self.h, self.d))
        if z_r is not None and self.cfg.noise_beta <= 0:  # white branch (icem.py:77): the randn(n, h, d) draw itself
            z_r, z_i = self._t(z_r, (n, self.h, self.d)), None
        elif z_r is not None:
            z_r = self._t(z_r, (n, self.d, self.F))
            z_i = self._t(z_i, (n, self.d, self.F))
        if out is None:
            out = torch.empty((n, self.h, self.d), dtype=self.dt, device=self.device)
        L.check(self.lib.icem_sample_clip(self._h, n, first_index, _ptr(mean), _ptr(std), _ptr(self.low),
                                          _ptr(self.high), _ptr(z_r), _ptr(z_i), offset, t_begin, int(row0_mean),
                                          _ptr(out), self._stream()))
        return out

    def philox_normals(self, n: int, offset: int = 0, first_index: int = 0):
        z_r = torch.empty((n, self.d, self.F), dtype=self.dt, device=self.device)
        z_i = torch.empty_like(z_r)
        L.check(self.lib.icem_philox_normals(self._h, n, first_index, offset, _ptr(z_r), _ptr(z_i), self._stream()))
        return z_r, z_i

    def rollout_cost(self, obs0, actions: torch.Tensor, return_observations: bool = False):
        """K2: ``simulate_trajectories`` + ``trajectory_cost_fn`` (icem/controllers/mpc.py:56-67,
        icem/controllers/abstract_controller.py:74-91) with the built-in model."""
        obs0 = self._t(obs0, (self.obs_dim,))
        actions = self._t(actions)
        n = actions.shape[0]
        if tuple(actions.shape[1:]) != (self.h, self.d):
            raise ValueError("actions must be [n, h, d]")
        costs = torch.empty((n,), dtype=self.dt, device=self.device)
        obs = torch.empty((n, self.h, self.obs_dim), dtype=self.dt, device=self.device) if return_observations else None
        L.check(self.lib.icem_rollout_cost(self._h, n, _ptr(obs0), _ptr(actions), _ptr(costs), _ptr(obs), self._stream()))
        return (costs, obs) if return_observations else costs

    def cost_reduce(self, step_costs) -> torch.Tensor:
        step_costs = self._t(step_costs)
        n = step_costs.shape[0]
        if step_costs.shape[1] != self.h:
            raise ValueError("step_costs must be [n, h]")
        costs = torch.empty((n,), dtype=self.dt, device=self.device)
        L.check(self.lib.icem_cost_reduce(self._h, n, _ptr(step_costs), _ptr(costs), self._stream()))
        return costs

    def topk_sorted(self, costs, k: Optional[int] = None):
        """K3: ``np.array(costs).argsort()[:K]`` (icem/controllers/icem.py:199)."""
        costs = self._t(costs)
        n = costs.shape[0]
        k = self.K if k is None else k
        nbytes = self.lib.icem_topk_workspace_bytes(self._h, n, k)
        if self._topk_ws is None or self._topk_ws.numel() < nbytes:
            self._topk_ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=self.device)
        out_c = torch.empty((k,), dtype=self.dt, device=self.device)
        out_i = torch.empty((k,), dtype=torch.int32, device=self.device)
        L.check(self.lib.icem_topk_sorted(self._h, n, _ptr(costs), k, _ptr(out_c), _ptr(out_i), _ptr(self._topk_ws),
                                          self._stream()))
        return out_c, out_i

    def gather_refit(self, actions: torch.Tensor, idx: torch.Tensor, mean: torch.Tensor, std: torch.Tensor):
        """K4: ``update_distributions`` (icem/controllers/icem.py:201-211); mean/std updated in place."""
        assert mean.dtype == self.dt and std.dtype == self.dt and mean.is_contiguous() and std.is_contiguous()
        actions = self._t(actions)
        idx = idx.to(device=self.device, dtype=torch.int32).contiguous()
        k = idx.shape[0]
        elites = torch.empty((k, self.h, self.d), dtype=self.dt, device=self.device)
        L.check(self.lib.icem_gather_refit(self._h, _ptr(actions), _ptr(idx), k, _ptr(mean), _ptr(std), _ptr(elites),
                                           self._stream()))
        return elites

    def can_update_in_one_launch(self, n_all: int, k: int) -> bool:
        """Does this handle serve ``icem_update_distribution`` for ``n_all`` candidates and ``k`` elites?  (f32, pools of at
        most 16 384 candidates, k <= 32 -- and the fast-path switch the HANDLE latched at ``icem_create``: asked of the
        handle, not re-read from the environment.)"""
        return bool(self.lib.icem_update_distribution_ok(self._h, int(n_all), int(k)))

    def update_distribution(self, costs: torch.Tensor, pool: torch.Tensor, k: int, mean: torch.Tensor, std: torch.Tensor,
                            keep_costs: Optional[torch.Tensor] = None, keep_actions: Optional[torch.Tensor] = None):
        """``update_distributions`` (icem/controllers/icem.py:194-211) with the kept elites appended behind the pool
        (icem.py:143-145) in ONE launch: -> (elite costs [k], indices [k] into [pool | kept], elites [k, h, d]); ``mean`` /
        ``std`` refitted in place.  Same bits as ``topk_sorted`` over the concatenation + ``gather_refit``."""
        assert mean.dtype == self.dt and std.dtype == self.dt and mean.is_contiguous() and std.is_contiguous()
        n = costs.shape[0]
        costs, pool = self._t(costs, (n,)), self._t(pool, (n, self.h, self.d))
        n_keep = 0 if keep_costs is None else keep_costs.shape[0]
        if n_keep:
            keep_costs, keep_actions = self._t(keep_costs, (n_keep,)), self._t(keep_actions, (n_keep, self.h, self.d))
        elites = torch.empty((k, self.h, self.d), dtype=self.dt, device=self.device)
        ec = torch.empty(k, dtype=self.dt, device=self.device)
        idx = torch.empty(k, dtype=torch.int32, device=self.device)
        L.check(self.lib.icem_update_distribution(self._h, n, _ptr(costs), _ptr(pool), n_keep,
                                                  _ptr(keep_costs) if n_keep else None, _ptr(keep_actions) if n_keep else None,
                                                  k, _ptr(mean), _ptr(std), _ptr(elites), _ptr(ec), _ptr(idx), self._stream()))
        return ec, idx, elites

    def sample_truncnorm(self, n: int, mean, std, lower, upper, u=None, offset: int = 0, first_index: int = 0,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``MpcCemStd.sample_action_sequences`` (icem/controllers/mpc.py:188-198): truncated-normal samples
        ``[n, h, d]``; ``lower`` / ``upper`` are ``[h, d]`` in standard-normal units; ``u`` = scipy's uniform draws
        ``[n, h, d]`` (parity mode) or None (device RNG)."""
        mean, std = self._t(mean, (self.h, self.d)), self._t(std, (self.h, self.d))
        lower, upper = self._t(lower, (self.h, self.d)), self._t(upper, (self.h, self.d))
        if u is not None:
            u = self._t(u, (n, self.h, self.d))
        if out is None:
            out = torch.empty((n, self.h, self.d), dtype=self.dt, device=self.device)
        L.check(self.lib.icem_sample_truncnorm(self._h, n, first_index, _ptr(mean), _ptr(std), _ptr(lower), _ptr(upper),
                                               _ptr(u), offset, _ptr(out), self._stream()))
        return out

    def cem_bounds(self, mean: torch.Tensor, std: torch.Tensor, like_levine: bool):
        """``MpcCemStd._update_bounds`` (icem/controllers/mpc.py:290-301): returns (lower, upper) ``[h, d]``;
        ``std`` is capped in place when ``like_levine``."""
        assert mean.dtype == self.dt and std.dtype == self.dt and mean.is_contiguous() and std.is_contiguous()
        lower = torch.empty((self.h, self.d), dtype=self.dt, device=self.device)
        upper = torch.empty_like(lower)
        L.check(self.lib.icem_cem_bounds(self._h, int(like_levine), _ptr(mean), _ptr(std), _ptr(self.low), _ptr(self.high),
                                         _ptr(lower), _ptr(upper), self._stream()))
        return lower, upper

    def shift(self, mean: torch.Tensor, std: torch.Tensor):
        """Epilogue of get_action (icem/controllers/icem.py:167-175), in place."""
        L.check(self.lib.icem_shift(self._h, _ptr(mean), _ptr(std), _ptr(self.low), _ptr(self.high), self._stream()))

    def reset_distribution(self, mean: torch.Tensor, std: torch.Tensor):
        """beginning_of_rollout (icem/controllers/icem.py:31-59), in place."""
        L.check(self.lib.icem_reset_distribution(self._h, _ptr(mean), _ptr(std), _ptr(self.low), _ptr(self.high),
                                                 self._stream()))

    def set_tile_arith(self, mode="auto"):
        """16 <= padded obs_dim <= 20: the arithmetic of the tile kernels' model step (``icem_set_tile_arith``): ``"f32"`` / 0
        the exact fmaf chain, ``"f16x2"`` / 1 two fp16 planes per operand on the 16-bit matrix cores, ``"auto"`` / -1 by the
        configuration's global population.  Returns the arithmetic now in effect (0 / 1)."""
        m = {"auto": -1, "f32": 0, "f16x2": 1}.get(mode, mode)
        L.check(self.lib.icem_set_tile_arith(self._h, int(m)))
        return self.tile_arith

    @property
    def tile_arith(self):
        return int(self.lib.icem_tile_arith(self._h))

    @property
    def tile_growth(self) -> float:
        """Reachable maximum of |state entry| / max(|obs0|, action bound) over the horizon for the handle's model
        (``icem_tile_growth``): what decides whether the fp16-plane tiles are served (<= 2^10)."""
        return float(self.lib.icem_tile_growth(self._h))

    def nonfinite_costs(self) -> int:
        """Trajectories since the planner was made whose cost left a tile kernel NaN (``icem_nonfinite_costs``;
        synchronises the launch stream)."""
        n = C.c_int64()
        L.check(self.lib.icem_nonfinite_costs(self._h, C.byref(n), self._stream()))
        return int(n.value)

    F64_ARITH = {"chain": 0, "mfma": 1}

    def set_f64_arith(self, mode="chain"):
        """dtype f64: which arithmetic the rollout's model step runs in (``icem_set_f64_arith``), by NAME: ``"chain"`` / 0 the
        generic kernels' fma chain (obs_dim <= 32, the default), ``"mfma"`` / 1 the f64 matrix cores -- sixteen trajectories
        per workgroup, every obs_dim up to 384, float64 rounding in blocks of four (not the chain's bits).  Set it BEFORE
        ``set_model`` for a model wider than 32.  Returns the arithmetic now in effect (a name)."""
        m = self.F64_ARITH.get(mode, mode)
        L.check(self.lib.icem_set_f64_arith(self._h, int(m)))
        return self.f64_arith

    @property
    def f64_arith(self):
        """The float64 arithmetic in effect: ``"chain"`` / ``"mfma"`` (``"chain"`` on an f32 planner)."""
        return {0: "chain", 1: "mfma"}[int(self.lib.icem_f64_arith(self._h))]

    WIDE_ARITH = {"auto": -1, "f16x2": 0, "fp16x2": 0, "f32": 1, "bf16x3": 2}

    def set_wide_arith(self, mode="auto"):
        """obs_dim > 32: which arithmetic the model step's GEMM runs in (``icem_set_wide_arith``), by NAME: ``"f32"`` the
        exact-f32 matrix pipe (bitwise an fmaf chain -- strict parity), ``"f16x2"`` two fp16 planes per operand (three
        products per multiply-add), ``"bf16x3"`` three bf16 planes (six products, operands exact at any magnitude),
        ``"auto"`` (the library's default) f16x2 unless the balanced model keeps a row or column more than 2^13 below its
        largest weight -- then bf16x3.  Returns the arithmetic now in effect (a name)."""
        m = self.WIDE_ARITH.get(mode, mode)
        L.check(self.lib.icem_set_wide_arith(self._h, int(m)))
        return self.wide_arith

    @property
    def wide_arith(self):
        """The wide arithmetic in effect for the current model: ``"f16x2"`` / ``"f32"`` / ``"bf16x3"``."""
        return {0: "f16x2", 1: "f32", 2: "bf16x3"}[int(self.lib.icem_wide_arith(self._h))]

    @property
    def wide_imbalance_log2(self):
        return int(self.lib.icem_wide_imbalance_log2(self._h))

    def set_wide_exact(self, on=True):
        """ABI <= 3 spelling of :meth:`set_wide_arith`: ``False`` / 0 the fp16 planes, ``True`` / 1 exact f32, 2 the bf16
        planes (``on`` defaults to exact f32; the LIBRARY's default is ``"auto"``)."""
        L.check(self.lib.icem_set_wide_exact(self._h, int(on)))

    # ------------------------------------------------------------------ measurement
    def profile_enable(self, on: bool = True):
        L.check(self.lib.icem_profile_enable(self._h, int(on)))

    def profile_read(self):
        """{kernel: (total_ms, launches, units)} since the last read (HIP events on the launch stream)."""
        n = len(L.KERNEL_NAMES)
        ms, cnt, units = (C.c_double * n)(), (C.c_int64 * n)(), (C.c_int64 * n)()
        L.check(self.lib.icem_profile_read(self._h, ms, cnt, units))
        return {L.KERNEL_NAMES[i]: (ms[i], cnt[i], units[i]) for i in range(n) if cnt[i]}

    def profile_overhead(self, reps: int = 200, spin_us: float = 15.0) -> Tuple[float, float]:
        """(event-pair time around a one-wave kernel spinning for ``spin_us``, how long that kernel really ran) in
        microseconds, on the launch stream (``icem_profile_overhead``): their difference is the bracket's share of every
        ``profile_read`` span."""
        pair, kern = C.c_double(), C.c_double()
        L.check(self.lib.icem_profile_overhead(self._stream(), reps, spin_us, C.byref(pair), C.byref(kern)))
        return pair.value, kern.value

    def get_action_host(self, obs) -> Tuple[np.ndarray, float]:
        """One MPC step for a host caller (``icem_get_action``): float64 observation in, ``(executed action [d] float64,
        best cost of the last pool)`` out; one H2D copy, the step's launches, one D2H copy and one synchronisation, all
        inside the library.  Device noise, world == 1."""
        self._ensure_buffers()
        self._cb.z_r = self._cb.z_i = self._cb.z_r_shift = self._cb.z_i_shift = None
        ob = np.ascontiguousarray(obs, dtype=np.float64)
        if ob.shape != (self.obs_dim,):
            raise ValueError(f"expected an observation of shape ({self.obs_dim},)")
        act = np.empty(self.d, dtype=np.float64)
        best = C.c_double()
        rc = self.lib.icem_get_action(self._h, C.byref(self._cb), self.mpc_step, ob.ctypes.data_as(C.POINTER(C.c_double)),
                                      act.ctypes.data_as(C.POINTER(C.c_double)), C.byref(best), self._stream())
        if rc in (0, L.ICEM_E_RANGE):
            self.mpc_step += 1   # (ICEM_E_RANGE: the step ran and its outputs are filled -- but they are not the reference's)
        L.check(rc)
        return act, best.value

    def plan_step_resident(self):
        """plan_step with the observation already in ``self.obs0`` (Philox noise): no host work besides
        the launches (and, for world > 1, the one all-gather per iteration) -- the bench's timed region."""
        self._cb.z_r = self._cb.z_i = self._cb.z_r_shift = self._cb.z_i_shift = None
        st = self._stream()
        if self.cfg.world == 1:
            L.check(self.lib.icem_plan_step(self._h, C.byref(self._cb), self.mpc_step, st))
        elif getattr(self, "_exchange", False) or getattr(self, "_rccl", False):
            # in-library exchange (or, failing that, the library's own RCCL all-gather on the launch stream): one C call
            # per MPC step, no host-side collective
            L.check(self.lib.icem_plan_step_sharded(self._h, C.byref(self._cb), self.mpc_step, st))
        else:
            # non-last merges ride in the next iteration's launch (nobody looks at mean / std in between)
            self._set_deferral(True)
            gather = self._resident_gather()
            local, merge, cb, h, step = self.lib.icem_plan_iter_local, self.lib.icem_plan_iter_merge, C.byref(self._cb), self._h, self.mpc_step
            for it in range(self.cfg.opt_iters):
                L.check(local(h, cb, step, it, st))
                gather()
                L.check(merge(h, cb, step, it, st))
        self.mpc_step += 1

    # ------------------------------------------------------------------ B independent planners, one launch per stage
    @staticmethod
    def plan_step_batch(planners: Sequence["IcemPlanner"], observations=None):
        """One MPC step of every planner of ``planners`` (one configuration; models, costs, seeds and observations of their
        own) as ``icem_plan_step_batch``: the reference's parallel episodes (icem/misc/rollout_utils.py:46-58, 129-152),
        every stage one launch for all of them.  Served: the o <= 20 tile shapes (HalfCheetah ...), the TileHN shapes -- Door,
        Relocate, FetchPickAndPlace at h = 30, planners that share the compiled term program of their cost terms -- and the
        GEMM-kernel shapes at h = 30 -- HumanoidStandup (o = 378), Humanoid, Ant, Hopper, Reacher, FetchReach: planners that share
        the observation width, the wide arithmetic in effect (:attr:`wide_arith`) and all or none carry cost terms -- at up to
        8192 rows per iteration; anything else raises ``IcemError`` (``ICEM_E_UNSUPPORTED`` / ``ICEM_E_INVALID``) before
        anything runs.  ``observations``: one per planner (``None``: already in ``planner.obs0``).
        Each planner's buffers afterwards are bit for bit those of its own :meth:`plan_step`.  Returns the executed actions
        (device tensors, no host sync)."""
        return IcemPlanner._step_batch("icem_plan_step_batch", planners, observations)

    @staticmethod
    def _step_batch(entry: str, planners, observations):
        """The host side the batched plan entries share: buffers, one ``mpc_step``, observations, the C call ``entry``."""
        pls = list(planners)
        n = len(pls)
        if n == 0:
            return []
        lib = pls[0].lib
        step = pls[0].mpc_step
        for i, pl in enumerate(pls):
            pl._ensure_buffers()
            if pl.mpc_step != step:
                raise ValueError("the planners of a batch advance together: same mpc_step")
            pl._cb.z_r = pl._cb.z_i = pl._cb.z_r_shift = pl._cb.z_i_shift = None
            if observations is not None:
                pl.obs0.copy_(torch.as_tensor(np.asarray(observations[i], dtype=np.float64), dtype=pl.dt), non_blocking=False)
        hs = (C.c_void_p * n)(*[pl._h for pl in pls])
        bs = (L.IcemPlanBuffersC * n)(*[pl._cb for pl in pls])
        L.check(getattr(lib, entry)(hs, n, bs, step, pls[0]._stream()))
        for pl in pls:
            pl.mpc_step += 1
        return [pl.executed for pl in pls]

    @staticmethod
    def plan_step_batch_f64(planners: Sequence["IcemPlanner"], observations=None):
        """:meth:`plan_step_batch` for planners in the strict-parity arithmetic (``dtype="f64"``), as
        ``icem_plan_step_batch_f64``: the generic kernels' sampler, rollout and one-launch selection, each ONE launch for all
        planners -- 3 launches per iteration, 2 more in a step with shifted elites, whatever the number of planners.  Served:
        one GPU, device noise, at most 8192 rows per iteration, the default arrangement of the generic kernels; anything else
        raises ``IcemError`` (``ICEM_E_UNSUPPORTED`` / ``ICEM_E_INVALID``) before anything runs.  Each planner's buffers
        afterwards are bit for bit those of its own :meth:`plan_step`.  Returns the executed actions (device tensors, no host
        sync)."""
        return IcemPlanner._step_batch("icem_plan_step_batch_f64", planners, observations)

    @property
    def batch_uploads(self) -> int:
        return int(self.lib.icem_batch_uploads(self._h))

    @property
    def batch_f64_launches(self) -> int:
        """Kernel launches of the last float64 batch step this planner led (``icem_batch_f64_launches``)."""
        return int(self.lib.icem_batch_f64_launches(self._h))

    # ------------------------------------------------------------------ the learned-dynamics step (declared RSSM)
    def _bind_rssm(self, model) -> bool:
        """Tell the handle the action width of ``model`` (``icem_set_rssm_act_dim``) where that is the planner's own -- the
        library cannot see the width a ``params`` buffer was packed at, and serves a handle that was never told at the declared
        six only.  A model of another width (or none: no ``act_dim``) leaves the handle alone, so the entry refuses it as it
        always has.  Returns whether the handle is now bound to ``model``'s width."""
        w = getattr(model, "act_dim", None)
        if w is None or int(w) != self.d or not 1 <= int(w) <= 32:
            return False
        if int(self.lib.icem_rssm_act_dim(self._h)) != int(w):
            L.check(self.lib.icem_set_rssm_act_dim(self._h, int(w)))
        return True

    def _learned_ok(self, ask, model) -> bool:
        """``ask(handle)`` as it stands (``model`` None), or for a step through ``model``: false where its width is not the
        planner's, else asked of the handle bound to that width (as the step itself would bind it)."""
        if model is not None and not self._bind_rssm(model):
            return False
        return bool(ask(self._h))

    def learned_step_ok(self, model=None) -> bool:
        """Does ``icem_plan_step_learned`` serve THIS handle?  (f32, one GPU, the RSSM's action width -- six unless the handle is
        bound to its own, 1 .. 32 --, a horizon of the folded sampler, the default generator, option ``learned_step`` on ...:
        asked of the handle.)  ``model``: ask for a step through this model, whose ``act_dim`` must be the planner's."""
        return self._learned_ok(self.lib.icem_plan_step_learned_ok, model)

    @property
    def learned_step_launches(self) -> int:
        """Kernel launches of the last learned step this planner led (``icem_learned_step_launches``)."""
        return int(self.lib.icem_learned_step_launches(self._h))

    def _learned_buffers(self, obs0_ptr) -> "L.IcemPlanBuffersC":
        self._ensure_buffers(learned=True)
        cb = L.IcemPlanBuffersC.from_buffer_copy(self._cb)
        cb.mean, cb.std = self.mean.data_ptr(), self.std.data_ptr()   # (the controller owns them between episodes)
        cb.obs0 = obs0_ptr
        cb.z_r = cb.z_i = cb.z_r_shift = cb.z_i_shift = None
        return cb

    def plan_step_learned(self, model, obs) -> torch.Tensor:
        """One MPC step through ``model`` (a ``DeviceRSSMModel``: its packed ``params``) as ``icem_plan_step_learned``: every
        CEM iteration's sampling, rollout and update and the step's epilogue inside the library, no host synchronisation.
        ``obs``: the observation ``[230]``.  Afterwards ``mean`` / ``std`` are shifted, :meth:`current_elites` is the step's
        elite set, ``executed`` / ``best_cost`` hold the step's result.  Returns ``executed`` (device tensor, no host sync).
        Raises ``IcemError`` (``ICEM_E_UNSUPPORTED``) before anything runs where :meth:`learned_step_ok` is false."""
        self._ensure_buffers(learned=True)
        ob = np.ascontiguousarray(obs, dtype=np.float32).reshape(-1)
        if ob.shape != (L.RSSM_OBS_DIM,):
            raise ValueError(f"expected an observation of shape ({L.RSSM_OBS_DIM},)")
        self.obs_rssm.copy_(torch.as_tensor(ob), non_blocking=False)
        cb = self._learned_buffers(self.obs_rssm.data_ptr())
        self._bind_rssm(model)
        L.check(self.lib.icem_plan_step_learned(self._h, C.byref(cb), C.c_void_p(model.params.data_ptr()), self.mpc_step,
                                                self._stream()))
        self.mpc_step += 1
        return self.executed

    @staticmethod
    def plan_step_learned_batch(planners: Sequence["IcemPlanner"], model, observations) -> torch.Tensor:
        """One MPC step of every planner of ``planners`` (one configuration; seeds, episodes, step counts and observations
        of their own) through ``model`` as ``icem_plan_step_learned_batch``: every stage one launch for all of them.  Each
        planner's buffers afterwards are bit for bit those of its own :meth:`plan_step_learned`.  Returns the results
        ``[B, d + 1]`` (executed action | best cost per planner; device tensor, no host sync).  Raises ``IcemError`` before
        anything runs -- and before any planner has advanced -- where the batch is not served."""
        pls = list(planners)
        n = len(pls)
        if n == 0:   # (the entry's own refusal: n outside [1, 32])
            L.check(L.load_library().icem_plan_step_learned_batch(None, 0, None, None, None, None, None))
        p0 = pls[0]
        obs = np.ascontiguousarray(np.asarray(observations, dtype=np.float32).reshape(n, -1))
        if obs.shape[1] != L.RSSM_OBS_DIM:
            raise ValueError(f"expected observations of shape ({n}, {L.RSSM_OBS_DIM})")
        obs_dev = torch.as_tensor(obs, device=p0.device)   # one host-to-device copy for the whole batch
        hs = (C.c_void_p * n)(*[pl._h for pl in pls])
        bs = (L.IcemPlanBuffersC * n)(*[pl._learned_buffers(obs_dev[i].data_ptr()) for i, pl in enumerate(pls)])
        steps = (C.c_int32 * n)(*[pl.mpc_step for pl in pls])
        results = torch.empty((n, p0.d + 1), dtype=torch.float32, device=p0.device)
        for pl in pls:
            pl._bind_rssm(model)
        L.check(p0.lib.icem_plan_step_learned_batch(hs, n, bs, C.c_void_p(model.params.data_ptr()), steps, _ptr(results), p0._stream()))
        for pl in pls:
            pl.mpc_step += 1
        return results

    # ------------------------------------------------------------------ ... through ensembles and a model per planner
    def learned_models_step_ok(self, n: int = 1, members: int = 1) -> bool:
        """Does ``icem_plan_step_learned_models`` serve a batch of ``n`` handles like THIS one through ``members`` models per
        problem?  (:meth:`learned_step_ok`'s conditions of the handle as it is bound, ``n * members <= 32``, and the tiles of
        every iteration of such a batch within the rollout's limit.)"""
        return bool(self.lib.icem_plan_step_learned_models_ok(self._h, int(n), int(members)))

    def _step_rows(self, it: int) -> int:
        """Rows iteration ``it`` of this planner's NEXT step scores (the shifted elites behind iteration 0's population)."""
        shift = it == 0 and self.cfg.shift_elites and self.mpc_step > 0 and self.n_reuse > 0
        return self.population_sizes[it] + (self.n_reuse if shift else 0)

    @staticmethod
    def _ensembles_each(models):
        """``models`` as the list of ``DeviceRSSMEnsemble`` (or of ``DeviceMLPEnsemble``: :meth:`plan_step_mlp`) it is where every
        planner plans through an ensemble of its own, else None."""
        from .models import DeviceMLPEnsemble, DeviceMLPModel, DeviceRSSMEnsemble
        if isinstance(models, (DeviceRSSMEnsemble, DeviceMLPEnsemble, DeviceMLPModel)):
            return None
        models = list(models)
        for kind in (DeviceRSSMEnsemble, DeviceMLPEnsemble):
            if models and all(isinstance(m, kind) for m in models):
                return models
        return None

    @staticmethod
    def _leave_member_costs(ens, models, member_costs, members: int, rows):
        """What a step through ensembles leaves in their ``member_costs``, as their own ``rollout_cost`` calls would: the last
        rollout's ``[members, rows of all planners]`` with a shared ensemble, planner p's columns of it (a view) with an
        ensemble each."""
        if member_costs is None:
            return
        total = sum(rows)
        table = member_costs[:members * total].view(members, total)
        if ens is not None:
            ens.member_costs = table
            return
        row0 = 0
        for m, r in zip(IcemPlanner._ensembles_each(models) or [], rows):
            m.member_costs = table[:, row0:row0 + r]
            row0 += r

    @staticmethod
    def _models_table(models, n: int, reduce, who: str):
        """``models`` of a step through models of their own -> ``(ens, table, width_of, reduce)``: the shared
        ``DeviceRSSMEnsemble`` or None, the parameter pointers ``[n][members]``, a model that stands for the action width, and
        the reduction's name (None: the ensemble's own -- of the first where every planner has one --, else ``"mean"``)."""
        from .models import DeviceRSSMEnsemble, DeviceRSSMModel
        ens = models if isinstance(models, DeviceRSSMEnsemble) else None
        if ens is not None:
            table = [ens._param_ptrs()] * n
            width_of = ens
            reduce = ens.reduce if reduce is None else reduce
        else:
            models = list(models)
            if models and all(isinstance(m, DeviceRSSMEnsemble) for m in models):   # an ensemble each: the launch reads its stacked params
                if len(models) != n:
                    raise ValueError(f"{n} planners but models for {len(models)}")
                if len({m.reduce for m in models}) > 1 and reduce is None:
                    raise ValueError("the planners' ensembles reduce differently: name one reduce for the step")
                if len({m.members for m in models}) > 1:
                    raise ValueError(f"every planner needs the same number (>= 1) of models, got {[m.members for m in models]}")
                if len({m.act_dim for m in models}) > 1 or len({m.params.device for m in models}) > 1:
                    raise ValueError("learned-dynamics models of one step need one action width on one device")
                reduce = models[0].reduce if reduce is None else reduce
                if reduce not in L.RSSM_REDUCE:
                    raise ValueError(f"reduce must be 'mean' or 'max', not {reduce!r}")
                return None, [m._param_ptrs() for m in models], models[0], reduce
            per = [[m] if isinstance(m, DeviceRSSMModel) else list(m) for m in models]
            if len(per) != n:
                raise ValueError(f"{n} planners but models for {len(per)}")
            if n and (len(per[0]) < 1 or any(len(ms) != len(per[0]) for ms in per)):
                raise ValueError(f"every planner needs the same number (>= 1) of models, got {[len(ms) for ms in per]}")
            flat = [m for ms in per for m in ms]
            if not all(isinstance(m, DeviceRSSMModel) for m in flat):
                raise ValueError(f"the models of {who} are DeviceRSSMModels (or one DeviceRSSMEnsemble)")
            if len({m.act_dim for m in flat}) > 1 or len({m.params.device for m in flat}) > 1:
                raise ValueError("learned-dynamics models of one step need one action width on one device")
            table = [[m.params.data_ptr() for m in ms] for ms in per]
            width_of = flat[0] if flat else None
            reduce = "mean" if reduce is None else reduce
        if reduce not in L.RSSM_REDUCE:
            raise ValueError(f"reduce must be 'mean' or 'max', not {reduce!r}")
        return ens, table, width_of, reduce

    @staticmethod
    def plan_step_learned_models(planners: Sequence["IcemPlanner"], models, observations, reduce=None, member_costs=None) -> torch.Tensor:
        """One MPC step of every planner of ``planners`` (one configuration; seeds, episodes, step counts and observations of
        their own) as ``icem_plan_step_learned_models``: :meth:`plan_step_learned_batch` with the rollout of every problem
        through models of its own.  ``models``: a ``DeviceRSSMEnsemble`` every planner plans through; a list of
        ``DeviceRSSMModel`` (one per planner); or a list of ``DeviceRSSMEnsemble`` / of lists (every planner its own ensemble, all
        of one size; ensembles bring their stacked ``params`` and, unless ``reduce`` is given, their common reduction).  A plan's
        cost is the mean or the worst of its problem's members: ``reduce`` ``"mean"`` / ``"max"`` (None: the ensemble's own,
        else ``"mean"``).  Every stage is one launch for all problems and members, 3 per CEM iteration (+ 1 in a step that
        shifts elites).  Each planner's buffers afterwards are bit for bit those of its own step with its members.  Returns
        the results ``[B, d + 1]`` (executed action | best cost per planner; device tensor, no host sync; kept with the first
        planner -- its next call of this batch size overwrites it).  The members' costs
        of the LAST iteration, ``[members, its rows of all planners]``, are left in ``member_costs`` (an f32 device tensor of
        at least ``members * B * max rows`` elements) when one is given, and with a ``DeviceRSSMEnsemble`` in its
        ``member_costs`` as its ``rollout_cost_batch`` leaves them.  Raises ``IcemError`` before anything runs -- and before
        any planner has advanced -- where the batch is not served."""
        pls = list(planners)
        n = len(pls)
        ens, table, width_of, reduce = IcemPlanner._models_table(models, n, reduce, "plan_step_learned_models")
        if n == 0:   # (the entry's own refusal: n outside [1, 32])
            L.check(L.load_library().icem_plan_step_learned_models(None, 0, None, 1, None, 0, None, None, None, None))
        members = len(table[0])
        p0 = pls[0]
        obs = np.ascontiguousarray(np.asarray(observations, dtype=np.float32).reshape(n, -1))
        if obs.shape[1] != L.RSSM_OBS_DIM:
            raise ValueError(f"expected observations of shape ({n}, {L.RSSM_OBS_DIM})")
        need = members * n * max(p0.population_sizes[it] + (p0.n_reuse if it == 0 else 0) for it in range(len(p0.population_sizes)))
        member_costs = IcemPlanner._models_member_costs(p0, ens, member_costs, need, models)
        # (the observations and the results of a batch size live with the first planner: the results' address sits in the argument blocks)
        kept = p0.__dict__.setdefault("_models_step_io", {})
        if n not in kept:
            kept[n] = (torch.empty((n, L.RSSM_OBS_DIM), dtype=torch.float32, device=p0.device),
                       torch.empty((n, p0.d + 1), dtype=torch.float32, device=p0.device))
        obs_dev, results = kept[n]
        obs_dev.copy_(torch.as_tensor(obs), non_blocking=False)   # one host-to-device copy for the whole batch
        hs = (C.c_void_p * n)(*[pl._h for pl in pls])
        bs = (L.IcemPlanBuffersC * n)(*[pl._learned_buffers(obs_dev[i].data_ptr()) for i, pl in enumerate(pls)])
        steps = (C.c_int32 * n)(*[pl.mpc_step for pl in pls])
        ptrs = (C.c_void_p * (n * members))(*[p for row in table for p in row])
        last_rows = [pl._step_rows(len(pl.population_sizes) - 1) for pl in pls]
        for pl in pls:
            pl._bind_rssm(width_of)
        L.check(p0.lib.icem_plan_step_learned_models(hs, n, bs, members, ptrs, L.RSSM_REDUCE[reduce], steps,
                                                     None if member_costs is None else _ptr(member_costs), _ptr(results), p0._stream()))
        for pl in pls:
            pl.mpc_step += 1
        IcemPlanner._leave_member_costs(ens, models, member_costs, members, last_rows)
        return results

    # ------------------------------------------------------------------ the same step through the feed-forward model (DeviceMLPModel)
    def mlp_step_ok(self, n: int = 1, members: int = 1, model=None) -> bool:
        """Does ``icem_plan_step_mlp`` serve a batch of ``n`` handles like THIS one through ``members`` MLPs per problem?  (f32,
        one GPU, a horizon of the folded sampler, the default generator, option ``mlp_step`` on, ``n * members <= 32`` ...:
        asked of the handle; no RSSM binding is involved.)  ``model``: ask for a step through this ``DeviceMLPModel`` /
        ``DeviceMLPEnsemble``, whose ``act_dim`` must be the planner's and whose parameters must be on its device."""
        if model is not None and (int(getattr(model, "act_dim", -1)) != self.d or model.params.device != self.device):
            return False
        return bool(self.lib.icem_plan_step_mlp_ok(self._h, int(n), int(members)))

    @property
    def mlp_step_launches(self) -> int:
        """Kernel launches of the last ``icem_plan_step_mlp`` this planner led (``icem_mlp_step_launches``)."""
        return int(self.lib.icem_mlp_step_launches(self._h))

    @staticmethod
    def _mlp_models_table(models, n: int, reduce):
        """``models`` of :meth:`plan_step_mlp` -> ``(ens, per, table, reduce)``: the ``DeviceMLPEnsemble`` all planners share or
        None, the model or ensemble of every planner, the parameter pointers ``[n][members]`` and the reduction's name (None:
        the ensembles' own, else ``"mean"``).  One kind for all planners, and ``_check_mlp_models``' rules: one shape, one
        activation, one device, one cost program; ensembles of one size and -- unless ``reduce`` names one -- one reduction."""
        from .models import DeviceMLPEnsemble, DeviceMLPModel, _check_mlp_models
        per = [models] * n if isinstance(models, (DeviceMLPModel, DeviceMLPEnsemble)) else list(models)
        if len(per) != n:
            raise ValueError(f"{n} planners but models for {len(per)}")
        each_ens = bool(per) and all(isinstance(m, DeviceMLPEnsemble) for m in per)
        if per and not each_ens and not all(isinstance(m, DeviceMLPModel) for m in per):
            raise ValueError("the models of plan_step_mlp are DeviceMLPModels or DeviceMLPEnsembles (one kind for all planners)")
        distinct = list({id(m): m for m in per}.values())
        if 1 <= len(distinct) <= L.MLP_MAX_PROBLEMS:   # (an ensemble carries its members' shape, activation, cost and device)
            _check_mlp_models(distinct)
        if each_ens:
            if len({m.members for m in per}) > 1:
                raise ValueError(f"every planner needs the same number (>= 1) of models, got {[m.members for m in per]}")
            if len({m.reduce for m in per}) > 1 and reduce is None:
                raise ValueError("the planners' ensembles reduce differently: name one reduce for the step")
            reduce = per[0].reduce if reduce is None else reduce
            table = [m._param_ptrs() for m in per]
        else:
            reduce = "mean" if reduce is None else reduce
            table = [[m.params.data_ptr()] for m in per]
        if reduce not in L.RSSM_REDUCE:
            raise ValueError(f"reduce must be 'mean' or 'max', not {reduce!r}")
        ens = per[0] if each_ens and len(distinct) == 1 else None
        return ens, per, table, reduce

    @staticmethod
    def plan_step_mlp(planners: Sequence["IcemPlanner"], models, observations, reduce=None, member_costs=None) -> torch.Tensor:
        """One MPC step of every planner of ``planners`` (one configuration; seeds, episodes, step counts and observations of
        their own) through feed-forward models as ``icem_plan_step_mlp``: :meth:`plan_step_learned_models` with the MLP launch
        in the rollout's place.  ``models``: a ``DeviceMLPModel`` or a ``DeviceMLPEnsemble`` for all planners, or a list with
        one of either per planner (one shape, one activation, one device, one cost program; ensembles of one size and one
        reduction).  ``observations``: ``[B, obs_dim]``.  A plan's cost is the mean or the worst of its problem's members:
        ``reduce`` ``"mean"`` / ``"max"`` (None: the ensembles' own, else ``"mean"``).  Every stage is one launch for all
        problems and members, 3 per CEM iteration (+ 1 in a step that shifts elites: :attr:`mlp_step_launches` of the first
        planner).  Each planner's ``mean``, ``std``, elites, ``executed`` and ``best_cost`` afterwards are bit for bit those of
        the stage-wise loop through its members' ``rollout_cost``; with one planner ``actions`` / ``costs`` hold the last pool
        as well.  Returns the results ``[B, d + 1]`` (executed action | best cost per planner; device tensor, no host sync;
        kept with the first planner -- its next call of this batch size overwrites it).  The members' costs of the LAST
        iteration, ``[members, its rows of all planners]``, are left in ``member_costs`` (an f32 device tensor of at least
        ``members * B * max rows`` elements) when one is given, and in the ensembles' ``member_costs`` as their own
        ``rollout_cost`` / ``rollout_cost_batch`` would leave them (with an ensemble each: its planner's columns, a view).
        Raises ``IcemError`` before anything is launched -- and before any planner has advanced -- where the batch is not served
        (the observations have then been copied into the first planner's private ``[B, obs_dim]`` tensor, nothing else).  That
        tensor and the results are kept per ``(B, obs_dim)`` with the first planner and released with it."""
        pls = list(planners)
        n = len(pls)
        ens, per, table, reduce = IcemPlanner._mlp_models_table(models, n, reduce)
        if n == 0:   # (the entry's own refusal: n outside [1, 32])
            L.check(L.load_library().icem_plan_step_mlp(None, 0, None, None, 1, None, 0, None, None, None, None))
        members = len(table[0])
        p0, m0 = pls[0], per[0]
        obs = np.ascontiguousarray(np.asarray(observations, dtype=np.float32).reshape(n, -1))
        if obs.shape[1] != m0.obs_dim:
            raise ValueError(f"expected observations of shape ({n}, {m0.obs_dim})")
        need = members * n * max(p0.population_sizes[it] + (p0.n_reuse if it == 0 else 0) for it in range(len(p0.population_sizes)))
        member_costs = IcemPlanner._models_member_costs(p0, ens, member_costs, need, per)
        # (the observations and the results of a batch size live with the first planner for as long as it does -- their addresses
        #  sit in the argument blocks, so the steady state uploads nothing; the observations are copied there before the entry
        #  can refuse, which no planner's state sees)
        kept = p0.__dict__.setdefault("_mlp_step_io", {})
        if (n, m0.obs_dim) not in kept:
            kept[(n, m0.obs_dim)] = (torch.empty((n, m0.obs_dim), dtype=torch.float32, device=p0.device),
                                     torch.empty((n, p0.d + 1), dtype=torch.float32, device=p0.device))
        obs_dev, results = kept[(n, m0.obs_dim)]
        obs_dev.copy_(torch.as_tensor(obs), non_blocking=False)   # one host-to-device copy for the whole batch
        hs = (C.c_void_p * n)(*[pl._h for pl in pls])
        bs = (L.IcemPlanBuffersC * n)(*[pl._learned_buffers(obs_dev[i].data_ptr()) for i, pl in enumerate(pls)])
        steps = (C.c_int32 * n)(*[pl.mpc_step for pl in pls])
        ptrs = (C.c_void_p * (n * members))(*[p for row in table for p in row])
        last_rows = [pl._step_rows(len(pl.population_sizes) - 1) for pl in pls]
        model_c = L.IcemMlpStepModelC(m0.obs_dim, m0.layers, L.MLP_ACTIVATIONS[m0.activation], C.pointer(m0._cost_c),
                                      C.pointer(m0._terms_c) if m0._terms_c is not None else None)
        L.check(p0.lib.icem_plan_step_mlp(hs, n, bs, C.byref(model_c), members, ptrs, L.RSSM_REDUCE[reduce], steps,
                                          None if member_costs is None else _ptr(member_costs), _ptr(results), p0._stream()))
        for pl in pls:
            pl.mpc_step += 1
        IcemPlanner._leave_member_costs(ens, per, member_costs, members, last_rows)
        return results

    # ------------------------------------------------------------------ the CEM baseline's step (MpcCemStd)
    def cem_step_ok(self) -> bool:
        """Does ``icem_plan_step_cem`` serve THIS handle?  (One GPU, profiling off, ``factor_decrease == 1``, no kept or
        shifted elites, a pool the one-launch update / selection of the handle's dtype admits, option ``cem_step`` on:
        asked of the handle.)"""
        return bool(self.lib.icem_plan_step_cem_ok(self._h))

    @property
    def cem_step_launches(self) -> int:
        """Kernel launches of the last CEM step of this planner (``icem_cem_step_launches``): 3 per iteration."""
        return int(self.lib.icem_cem_step_launches(self._h))

    def _cem_buffers(self, obs: Optional[str] = None):
        """The step's buffers, owned by the planner: the last pool and its costs, the elite set, its costs and indices,
        and ``[executed | best_cost]`` as one tensor (one device-to-host copy fetches both).  ``obs``: also the observation
        buffer of one of the two steps -- ``"obs0"`` ``[obs_dim]`` of the planner dtype for the built-in model (which must
        be set), ``"obs_rssm"`` ``[230]`` f32 for the learned-dynamics step, which needs no built-in model."""
        b = getattr(self, "_cem", None)
        new = lambda *shape, dt=self.dt: torch.zeros(shape, dtype=dt, device=self.device)  # noqa: E731
        if b is None:
            n = self.cfg.num_traj
            b = self._cem = dict(actions=new(n, self.h, self.d), costs=new(n), elites=new(self.K, self.h, self.d),
                                 elite_costs=new(self.K), elite_idx=new(self.K, dt=torch.int32), obs0=None, obs_rssm=None,
                                 result=new(self.d + 1), cb=None, key=None)
        if obs is not None and b[obs] is None:
            if obs == "obs0" and self.obs_dim == 0:
                raise RuntimeError("set_model()/set_cost() must be called before planning")
            b[obs] = new(self.obs_dim) if obs == "obs0" else new(L.RSSM_OBS_DIM, dt=torch.float32)
        return b

    def plan_step_cem(self, obs, mean: torch.Tensor, std: torch.Tensor, lower: torch.Tensor, upper: torch.Tensor, *,
                      like_levine: bool, shift_means: bool, execute_best_elite: bool) -> torch.Tensor:
        """One MPC step of the truncated-normal CEM (``MpcCemStd.get_action``, icem/controllers/mpc.py:200-262) as
        ``icem_plan_step_cem``: every iteration's sampling, rollout, update and bounds and the step's epilogue inside the
        library, no host synchronisation.  ``mean`` / ``std`` / ``lower`` / ``upper`` ``[h, d]`` are the caller's and are
        updated in place (afterwards: shifted / reset for the next step).  The planner's ``cem_elites`` / ``cem_elite_costs``
        / ``cem_elite_idx`` / ``cem_actions`` / ``cem_costs`` hold the last iteration's elite set and pool, ``cem_result``
        is ``[executed | best_cost]``.  Returns ``executed`` (device tensor, no host sync) and advances ``mpc_step``.
        Raises ``IcemError`` (``ICEM_E_UNSUPPORTED``) before anything runs where :meth:`cem_step_ok` is false."""
        cb = self._cem_cb(obs, mean, std, lower, upper)
        prm = L.IcemCemParamsC(int(bool(like_levine)), int(bool(shift_means)), int(bool(execute_best_elite)), 0)
        L.check(self.lib.icem_plan_step_cem(self._h, C.byref(cb), C.byref(prm), self.mpc_step, self._stream()))
        self.mpc_step += 1
        return self._cem_buffers()["result"][:self.d]

    def _cem_cb(self, obs, mean, std, lower, upper, which: str = "obs0", obs_ptr: Optional[int] = None) -> "L.IcemCemBuffersC":
        """The observation into the planner's own buffer and the step's ``icem_cem_buffers`` (kept while the caller's tensors
        stay where they are).  ``which``: the built-in model's observation buffer or the learned-dynamics step's
        (:meth:`_cem_buffers`); ``obs_ptr``: the observation already lies on the device there (a row of a batch's table) --
        nothing is copied."""
        b = self._cem_buffers(None if obs_ptr is not None else which)
        for t in (mean, std, lower, upper):
            if t.dtype != self.dt or t.device != self.device or tuple(t.shape) != (self.h, self.d) or not t.is_contiguous():
                raise ValueError("mean / std / lower / upper must be contiguous [h, d] device tensors of the planner dtype")
        if obs_ptr is None:
            dst = b[which]
            if isinstance(obs, torch.Tensor) and obs.device == self.device:
                if obs.numel() != dst.numel():
                    raise ValueError(f"expected an observation of {dst.numel()} values")
                dst.copy_(obs.reshape(-1))
            else:
                dst.copy_(torch.as_tensor(np.asarray(obs, dtype=np.float64).reshape(dst.numel()), dtype=dst.dtype))
            obs_ptr = dst.data_ptr()
        key = (mean.data_ptr(), std.data_ptr(), lower.data_ptr(), upper.data_ptr(), obs_ptr)
        if b["key"] != key:
            r = b["result"]
            b["cb"] = L.IcemCemBuffersC(
                mean=key[0], std=key[1], lower=key[2], upper=key[3], low=self.low.data_ptr(), high=self.high.data_ptr(),
                obs0=obs_ptr, actions=b["actions"].data_ptr(), costs=b["costs"].data_ptr(),
                elites=b["elites"].data_ptr(), elite_costs=b["elite_costs"].data_ptr(), elite_idx=b["elite_idx"].data_ptr(),
                executed=r.data_ptr(), best_cost=r[self.d:].data_ptr(), workspace=None)
            b["key"] = key
        return b["cb"]

    @staticmethod
    def plan_step_cem_batch(planners: Sequence["IcemPlanner"], observations, dists, *, like_levine: bool, shift_means: bool,
                            execute_best_elite: bool) -> torch.Tensor:
        """:meth:`plan_step_cem` of every planner of ``planners`` (one configuration; models, costs, seeds, episodes, step
        counts and observations of their own) as ``icem_plan_step_cem_batch``: the reference's side-by-side CEM episodes
        (icem/misc/rollout_utils.py:46-58, 129-152), every iteration 3 launches for all of them.  ``dists[i]``: planner i's
        ``(mean, std, lower, upper)``, updated in place.  Each planner's ``cem_*`` views afterwards are bit for bit those of
        its own :meth:`plan_step_cem`, and each ``mpc_step`` has advanced by one.  Returns the executed actions ``[B, d]`` -- a
        view of the batch's results ``[B, d + 1]`` (executed | best cost; ``planners[0].cem_batch_results``), the one tensor a
        caller copies to the host.  Raises ``IcemError`` before anything runs, and before any planner has advanced, where
        the batch is not served."""
        pls = list(planners)
        n = len(pls)
        if n == 0:   # (the entry's own refusal: n outside [1, 32])
            L.check(L.load_library().icem_plan_step_cem_batch(None, 0, None, None, None, None, None))
        p0 = pls[0]
        observations, dists = list(observations), list(dists)
        if len(observations) != n or len(dists) != n:
            raise ValueError("one observation and one (mean, std, lower, upper) per planner")
        cbs = [pl._cem_cb(ob, *dist) for pl, ob, dist in zip(pls, observations, dists)]
        hs = (C.c_void_p * n)(*[pl._h for pl in pls])
        bs = (L.IcemCemBuffersC * n)(*cbs)
        steps = (C.c_int32 * n)(*[pl.mpc_step for pl in pls])
        res = getattr(p0, "_cem_batch_results", None)   # (kept per batch size: a captured step replays into the same tensor)
        if res is None or res.shape[0] != n:
            res = p0._cem_batch_results = torch.zeros((n, p0.d + 1), dtype=p0.dt, device=p0.device)
        prm = L.IcemCemParamsC(int(bool(like_levine)), int(bool(shift_means)), int(bool(execute_best_elite)), 0)
        L.check(p0.lib.icem_plan_step_cem_batch(hs, n, bs, C.byref(prm), steps, _ptr(res), p0._stream()))
        for pl in pls:
            pl.mpc_step += 1
        return res[:, :p0.d]

    cem_batch_results = property(lambda self: getattr(self, "_cem_batch_results", None))

    @property
    def cem_batch_launches(self) -> int:
        """Kernel launches of the last batched CEM step this planner led (``icem_cem_batch_launches``): 3 per iteration."""
        return int(self.lib.icem_cem_batch_launches(self._h))

    # ------------------------------------------------------------------ the random-shooting baseline's step (MpcRandom)
    def random_step_ok(self) -> bool:
        """Does ``icem_plan_step_random`` serve THIS handle?  (One GPU, profiling and stamps off, option ``random_step`` on:
        asked of the handle.)"""
        return bool(self.lib.icem_plan_step_random_ok(self._h))

    @property
    def random_step_launches(self) -> int:
        """Kernel launches of the last random-shooting step of this planner (``icem_random_step_launches``)."""
        return int(self.lib.icem_random_step_launches(self._h))

    @property
    def random_batch_launches(self) -> int:
        """Kernel launches of the last batched random-shooting step this planner led (``icem_random_batch_launches``)."""
        return int(self.lib.icem_random_batch_launches(self._h))

    def _random_buffers(self, obs: Optional[str] = None):
        """The step's buffers, owned by the planner (a captured step replays into the same tensors): the pool and its
        costs, the cheapest row, ``result`` = ``[executed | best cost | best index]`` (one device-to-host copy fetches all
        three).  ``obs``: also the observation buffer of that name -- ``"obs0"`` ``[obs_dim]`` for the built-in model,
        ``"obs_rssm"`` ``[230]`` f32 for the learned-dynamics step (no model need be set for it) -- and under ``"cb_" + obs``
        the step's ``icem_random_buffers`` with it."""
        b = getattr(self, "_random", None)
        new = lambda *shape, dt=self.dt: torch.zeros(shape, dtype=dt, device=self.device)  # noqa: E731
        if b is None:
            n = self.cfg.num_traj
            b = self._random = dict(actions=new(n, self.h, self.d), costs=new(n), best_actions=new(self.h, self.d),
                                    result=new(self.d + 2), obs0=None, obs_rssm=None)
        if obs is not None and b[obs] is None:
            if obs == "obs0" and self.obs_dim == 0:
                raise RuntimeError("set_model()/set_cost() must be called before planning")
            b[obs] = new(self.obs_dim) if obs == "obs0" else new(L.RSSM_OBS_DIM, dt=torch.float32)
            b["cb_" + obs] = L.IcemRandomBuffersC(
                low=self.low.data_ptr(), high=self.high.data_ptr(), obs0=b[obs].data_ptr(), actions=b["actions"].data_ptr(),
                costs=b["costs"].data_ptr(), best_actions=b["best_actions"].data_ptr(), result=b["result"].data_ptr())
        return b

    def _random_cb(self, obs, which: str = "obs0") -> "L.IcemRandomBuffersC":
        """The observation into the planner's own buffer (``which``: the built-in model's or the learned-dynamics step's,
        :meth:`_random_buffers`); the step's ``icem_random_buffers``."""
        b = self._random_buffers(which)
        dst = b[which]
        if isinstance(obs, torch.Tensor) and obs.device == self.device:
            if obs.numel() != dst.numel():
                raise ValueError(f"expected an observation of {dst.numel()} values")
            dst.copy_(obs.reshape(-1))
        else:
            dst.copy_(torch.as_tensor(np.asarray(obs, dtype=np.float64).reshape(dst.numel()), dtype=dst.dtype))
        return b["cb_" + which]

    random_actions = property(lambda self: self._random_buffers()["actions"])
    random_costs = property(lambda self: self._random_buffers()["costs"])
    random_best_actions = property(lambda self: self._random_buffers()["best_actions"])
    random_result = property(lambda self: self._random_buffers()["result"])

    def plan_step_random(self, obs, call_offset: int, change_freq: int, u=None, first_block: int = 0) -> torch.Tensor:
        """One MPC step of random shooting (``MpcRandom.get_action``, icem/controllers/mpc.py:114-138) as
        ``icem_plan_step_random``: :meth:`sample_piecewise` at ``call_offset`` (``MpcRandom``'s counter of ``sample()`` calls:
        the caller's -- the planner keeps none), :meth:`rollout_cost`, ``topk_sorted(costs, 1)`` and the gathers, no host
        synchronisation.  ``u``: the draws ``[*, d]`` of blocks ``first_block..`` (parity), or None for the device's Philox
        streams.  Afterwards ``random_actions`` / ``random_costs`` hold the pool, ``random_best_actions`` its cheapest row,
        ``random_result`` is ``[executed | best cost | best index]``.  Returns ``executed`` (device tensor, no host sync).
        Raises ``IcemError`` before anything runs where the step is refused."""
        cb = self._random_cb(obs)
        u_t = None if u is None else self._t(u)
        L.check(self.lib.icem_plan_step_random(self._h, C.byref(cb), int(change_freq), int(call_offset), int(first_block),
                                               _ptr(u_t), self._stream()))
        return self._random_buffers()["result"][:self.d]

    @staticmethod
    def plan_step_random_batch(planners: Sequence["IcemPlanner"], observations, call_offsets, change_freq: int) -> torch.Tensor:
        """:meth:`plan_step_random` of every planner of ``planners`` (one configuration; models, costs, seeds, observations
        and call offsets of their own) as ``icem_plan_step_random_batch``: the same three stages, each ONE launch for all of
        them.  Each planner's ``random_*`` views afterwards are bit for bit those of its own :meth:`plan_step_random`.
        Returns the executed actions ``[B, d]`` -- a view of the batch's results ``[B, d + 2]``
        (``planners[0].random_batch_results``), the one tensor a caller copies to the host.  Raises ``IcemError`` before
        anything runs where the batch is not served."""
        pls = list(planners)
        n = len(pls)
        if n == 0:   # (the entry's own refusal: n outside [1, 32])
            L.check(L.load_library().icem_plan_step_random_batch(None, 0, None, 0, None, None, None))
        p0 = pls[0]
        observations, call_offsets = list(observations), list(call_offsets)
        if len(observations) != n or len(call_offsets) != n:
            raise ValueError("one observation and one call offset per planner")
        cbs = [pl._random_cb(ob) for pl, ob in zip(pls, observations)]
        hs = (C.c_void_p * n)(*[pl._h for pl in pls])
        bs = (L.IcemRandomBuffersC * n)(*cbs)
        offs = (C.c_int64 * n)(*[int(o) for o in call_offsets])
        res = getattr(p0, "_random_batch_results", None)   # (kept per batch size: a captured step replays into the same tensor)
        if res is None or res.shape[0] != n:
            res = p0._random_batch_results = torch.zeros((n, p0.d + 2), dtype=p0.dt, device=p0.device)
        L.check(p0.lib.icem_plan_step_random_batch(hs, n, bs, int(change_freq), offs, _ptr(res), p0._stream()))
        return res[:, :p0.d]

    random_batch_results = property(lambda self: getattr(self, "_random_batch_results", None))

    def random_learned_step_ok(self, model=None) -> bool:
        """Does ``icem_plan_step_random_learned`` serve THIS handle?  (:meth:`random_step_ok`'s conditions, f32, the RSSM's
        action width -- six unless the handle is bound to its own, 1 .. 32 --, a population the RSSM's split launch takes: asked
        of the handle.)  ``model``: as :meth:`learned_step_ok`'s."""
        return self._learned_ok(self.lib.icem_plan_step_random_learned_ok, model)

    def plan_step_random_learned(self, model, obs, call_offset: int, change_freq: int) -> torch.Tensor:
        """:meth:`plan_step_random` through ``model`` (a ``DeviceRSSMModel``: its packed ``params``) as
        ``icem_plan_step_random_learned``.  ``obs``: the observation ``[230]`` (array-like, or a device tensor); no built-in
        model or cost need be set; the uniforms are the device's.  The same views, return value and launch count
        (:attr:`random_step_launches`) as :meth:`plan_step_random`, and the same bits as the operator chain
        (``sample_piecewise``, ``model.rollout_cost``, ``topk_sorted(costs, 1)`` and the gathers).  Raises ``IcemError``
        before anything runs where the step is refused."""
        cb = self._random_cb(obs, "obs_rssm")
        self._bind_rssm(model)
        L.check(self.lib.icem_plan_step_random_learned(self._h, C.byref(cb), C.c_void_p(model.params.data_ptr()), int(change_freq),
                                                       int(call_offset), self._stream()))
        return self._random_buffers()["result"][:self.d]

    @staticmethod
    def plan_step_random_learned_batch(planners: Sequence["IcemPlanner"], model, observations, call_offsets, change_freq: int) -> torch.Tensor:
        """:meth:`plan_step_random_learned` of every planner of ``planners`` (one configuration; seeds, observations and call
        offsets of their own) through the one ``model`` as ``icem_plan_step_random_learned_batch``: 3 launches for all of
        them.  Each planner's ``random_*`` views afterwards -- its pool and costs included -- are bit for bit those of its own
        :meth:`plan_step_random_learned`.  Returns the executed actions ``[B, d]``, a view of
        ``planners[0].random_batch_results`` ``[B, d + 2]`` (kept per batch size).  Raises ``IcemError`` before anything runs
        where the batch is not served."""
        pls = list(planners)
        n = len(pls)
        if n == 0:   # (the entry's own refusal: n outside [1, 32])
            L.check(L.load_library().icem_plan_step_random_learned_batch(None, 0, None, None, 0, None, None, None))
        p0 = pls[0]
        observations, call_offsets = list(observations), list(call_offsets)
        if len(observations) != n or len(call_offsets) != n:
            raise ValueError("one observation and one call offset per planner")
        cbs = [pl._random_cb(ob, "obs_rssm") for pl, ob in zip(pls, observations)]
        hs = (C.c_void_p * n)(*[pl._h for pl in pls])
        bs = (L.IcemRandomBuffersC * n)(*cbs)
        offs = (C.c_int64 * n)(*[int(o) for o in call_offsets])
        res = getattr(p0, "_random_batch_results", None)   # (kept per batch size: a captured step replays into the same tensor)
        if res is None or res.shape[0] != n:
            res = p0._random_batch_results = torch.zeros((n, p0.d + 2), dtype=p0.dt, device=p0.device)
        for pl in pls:
            pl._bind_rssm(model)
        L.check(p0.lib.icem_plan_step_random_learned_batch(hs, n, bs, C.c_void_p(model.params.data_ptr()), int(change_freq), offs,
                                                           _ptr(res), p0._stream()))
        return res[:, :p0.d]

    # ------------------------------------------------------------------ ... through the learned dynamics (declared RSSM)
    def cem_learned_step_ok(self, model=None) -> bool:
        """Does ``icem_plan_step_cem_learned`` serve THIS handle?  (:meth:`cem_step_ok`'s conditions, f32, the RSSM's action
        width -- six unless the handle is bound to its own, 1 .. 32 --, a population the RSSM's split launch takes: asked of the
        handle.)  ``model``: as :meth:`learned_step_ok`'s."""
        return self._learned_ok(self.lib.icem_plan_step_cem_learned_ok, model)

    def plan_step_cem_learned(self, model, obs, mean: torch.Tensor, std: torch.Tensor, lower: torch.Tensor, upper: torch.Tensor, *,
                              like_levine: bool, shift_means: bool, execute_best_elite: bool) -> torch.Tensor:
        """:meth:`plan_step_cem` through ``model`` (a ``DeviceRSSMModel``: its packed ``params``) as
        ``icem_plan_step_cem_learned`` -- the planner PlaNet uses.  ``obs``: the observation ``[230]`` (array-like, or a
        device tensor); no built-in model or cost need be set.  The same arguments, views, return value and launch count
        (:attr:`cem_step_launches`) as :meth:`plan_step_cem`, and the same bits as the operator loop
        (``sample_truncnorm``, ``model.rollout_cost``, ``update_distribution``, ``cem_bounds``).  Raises ``IcemError``
        (``ICEM_E_UNSUPPORTED``) before anything runs where :meth:`cem_learned_step_ok` is false."""
        cb = self._cem_cb(obs, mean, std, lower, upper, "obs_rssm")
        prm = L.IcemCemParamsC(int(bool(like_levine)), int(bool(shift_means)), int(bool(execute_best_elite)), 0)
        self._bind_rssm(model)
        L.check(self.lib.icem_plan_step_cem_learned(self._h, C.byref(cb), C.byref(prm), C.c_void_p(model.params.data_ptr()),
                                                    self.mpc_step, self._stream()))
        self.mpc_step += 1
        return self._cem_buffers()["result"][:self.d]

    @staticmethod
    def _cem_learned_batch_io(pls, observations, dists, like_levine, shift_means, execute_best_elite):
        """What a batched learned-dynamics CEM step hands the library: the handles, every planner's ``icem_cem_buffers`` (the
        observations in ONE table kept with the first planner), the step counts, the results tensor and the flags."""
        p0, n = pls[0], len(pls)
        dists = list(dists)
        if len(dists) != n:
            raise ValueError("one (mean, std, lower, upper) per planner")
        obs_dev = getattr(p0, "_cem_learned_obs", None)   # (kept per batch size, as the results)
        if obs_dev is None or obs_dev.shape[0] != n:
            obs_dev = p0._cem_learned_obs = torch.zeros((n, L.RSSM_OBS_DIM), dtype=torch.float32, device=p0.device)
        if isinstance(observations, torch.Tensor) and observations.device == p0.device:
            src = observations.reshape(n, -1)
            if src.dtype == torch.float32 and src.is_contiguous() and src.shape[1] == L.RSSM_OBS_DIM:
                obs_dev = src
            else:
                obs_dev.copy_(src)
        else:
            host = np.ascontiguousarray(np.asarray(observations, dtype=np.float32).reshape(n, -1))
            if host.shape[1] != L.RSSM_OBS_DIM:
                raise ValueError(f"expected observations of shape ({n}, {L.RSSM_OBS_DIM})")
            obs_dev.copy_(torch.as_tensor(host))   # one host-to-device copy for the whole batch
        cbs = [pl._cem_cb(None, *dist, obs_ptr=obs_dev[i].data_ptr()) for i, (pl, dist) in enumerate(zip(pls, dists))]
        hs = (C.c_void_p * n)(*[pl._h for pl in pls])
        bs = (L.IcemCemBuffersC * n)(*cbs)
        steps = (C.c_int32 * n)(*[pl.mpc_step for pl in pls])
        res = getattr(p0, "_cem_batch_results", None)   # (kept per batch size: a captured step replays into the same tensor)
        if res is None or res.shape[0] != n:
            res = p0._cem_batch_results = torch.zeros((n, p0.d + 1), dtype=p0.dt, device=p0.device)
        prm = L.IcemCemParamsC(int(bool(like_levine)), int(bool(shift_means)), int(bool(execute_best_elite)), 0)
        return hs, bs, steps, res, prm

    # ------------------------------------------------------------------ ... through ensembles and a model per planner
    def cem_learned_models_step_ok(self, n: int = 1, members: int = 1) -> bool:
        """Does ``icem_plan_step_cem_learned_models`` serve a batch of ``n`` handles like THIS one through ``members`` models per
        problem?  (:meth:`cem_learned_step_ok`'s conditions of the handle as it is bound, ``n * members <= 32``, the tiles of
        such a rollout within the launch's limit.)"""
        return bool(self.lib.icem_plan_step_cem_learned_models_ok(self._h, int(n), int(members)))

    def random_learned_models_step_ok(self, n: int = 1, members: int = 1) -> bool:
        """Does ``icem_plan_step_random_learned_models`` serve a batch of ``n`` handles like THIS one through ``members`` models
        per problem?  (:meth:`random_learned_step_ok`'s conditions, ``n * members <= 32``, the rollout's tiles.)"""
        return bool(self.lib.icem_plan_step_random_learned_models_ok(self._h, int(n), int(members)))

    @staticmethod
    def _models_member_costs(p0, ens, member_costs, need: int, models=None):
        """The ``member_costs`` tensor of a step through models of their own: the caller's (checked), the one kept with a
        shared ensemble -- or, where every planner has an ensemble of its own, with the first of them -- (its address sits in
        the step's argument blocks), or None (the library's scratch: plain models keep no member costs)."""
        if ens is None and models is not None:
            each = IcemPlanner._ensembles_each(models)
            ens = each[0] if each else None
        if ens is not None and member_costs is None:
            member_costs = getattr(ens, "_step_member_costs", None)
            if member_costs is None or member_costs.numel() < need or member_costs.device != p0.device:
                member_costs = ens._step_member_costs = torch.empty((need,), dtype=torch.float32, device=p0.device)
        if member_costs is not None and (member_costs.dtype != torch.float32 or not member_costs.is_contiguous()
                                         or member_costs.numel() < need or member_costs.device != p0.device):
            raise ValueError(f"member_costs must be a contiguous float32 tensor of at least {need} elements on the planners' device")
        return member_costs

    @staticmethod
    def plan_step_cem_learned_models(planners: Sequence["IcemPlanner"], models, observations, dists, *, like_levine: bool,
                                     shift_means: bool, execute_best_elite: bool, reduce=None, member_costs=None) -> torch.Tensor:
        """:meth:`plan_step_cem_learned_batch` with the rollout of every problem through models of its own, as
        ``icem_plan_step_cem_learned_models``: the planner PETS and PlaNet use, through an ensemble.  ``models``, ``reduce`` and
        ``member_costs`` as :meth:`plan_step_learned_models` takes them (a ``DeviceRSSMEnsemble`` for all planners, a list of
        ``DeviceRSSMModel`` -- one each --, or a list of ``DeviceRSSMEnsemble`` / of lists -- an ensemble each, all of one size);
        ``member_costs`` needs ``members * B * num_traj`` elements and holds the last iteration's ``[members, B * num_traj]``.
        3 launches per CEM iteration whatever B and the member count (:attr:`cem_batch_launches` of the first planner); every
        planner's ``mean`` / ``std`` / ``lower`` / ``upper``, ``cem_elites`` / ``cem_elite_costs`` / ``cem_elite_idx`` and its
        row of the results are bit for bit the operator loop's through its members; with one planner ``cem_actions`` /
        ``cem_costs`` hold the last pool as well, with more they are scratch.  Returns the executed actions ``[B, d]``, a view
        of ``planners[0].cem_batch_results`` ``[B, d + 1]``.  Raises ``IcemError`` before anything runs, and before any planner
        has advanced, where the batch is not served."""
        pls = list(planners)
        n = len(pls)
        ens, table, width_of, reduce = IcemPlanner._models_table(models, n, reduce, "plan_step_cem_learned_models")
        if n == 0:   # (the entry's own refusal: n outside [1, 32])
            L.check(L.load_library().icem_plan_step_cem_learned_models(None, 0, None, None, 1, None, 0, None, None, None, None))
        members = len(table[0])
        p0 = pls[0]
        member_costs = IcemPlanner._models_member_costs(p0, ens, member_costs, members * n * p0.cfg.num_traj, models)
        hs, bs, steps, res, prm = IcemPlanner._cem_learned_batch_io(pls, observations, dists, like_levine, shift_means, execute_best_elite)
        ptrs = (C.c_void_p * (n * members))(*[p for row in table for p in row])
        for pl in pls:
            pl._bind_rssm(width_of)
        L.check(p0.lib.icem_plan_step_cem_learned_models(hs, n, bs, C.byref(prm), members, ptrs, L.RSSM_REDUCE[reduce], steps,
                                                         None if member_costs is None else _ptr(member_costs), _ptr(res), p0._stream()))
        for pl in pls:
            pl.mpc_step += 1
        IcemPlanner._leave_member_costs(ens, models, member_costs, members, [p0.cfg.num_traj] * n)
        return res[:, :p0.d]

    @staticmethod
    def plan_step_random_learned_models(planners: Sequence["IcemPlanner"], models, observations, call_offsets, change_freq: int,
                                        reduce=None, member_costs=None) -> torch.Tensor:
        """:meth:`plan_step_random_learned_batch` with the rollout of every problem through models of its own, as
        ``icem_plan_step_random_learned_models``: random shooting through an ensemble (PETS), or with a trained model per
        planner.  ``models``, ``reduce`` and ``member_costs`` as :meth:`plan_step_cem_learned_models` takes them.  3 launches
        whatever B and the member count (:attr:`random_batch_launches` of the first planner); every planner's ``random_*``
        views -- its pool and the reduced costs included -- are bit for bit the operator chain's through its members.  Returns
        the executed actions ``[B, d]``, a view of ``planners[0].random_batch_results`` ``[B, d + 2]``.  Raises ``IcemError``
        before anything runs where the batch is not served."""
        pls = list(planners)
        n = len(pls)
        ens, table, width_of, reduce = IcemPlanner._models_table(models, n, reduce, "plan_step_random_learned_models")
        if n == 0:   # (the entry's own refusal: n outside [1, 32])
            L.check(L.load_library().icem_plan_step_random_learned_models(None, 0, None, 1, None, 0, 0, None, None, None, None))
        members = len(table[0])
        p0 = pls[0]
        observations, call_offsets = list(observations), list(call_offsets)
        if len(observations) != n or len(call_offsets) != n:
            raise ValueError("one observation and one call offset per planner")
        member_costs = IcemPlanner._models_member_costs(p0, ens, member_costs, members * n * p0.cfg.num_traj, models)
        cbs = [pl._random_cb(ob, "obs_rssm") for pl, ob in zip(pls, observations)]
        hs = (C.c_void_p * n)(*[pl._h for pl in pls])
        bs = (L.IcemRandomBuffersC * n)(*cbs)
        offs = (C.c_int64 * n)(*[int(o) for o in call_offsets])
        res = getattr(p0, "_random_batch_results", None)   # (kept per batch size: a captured step replays into the same tensor)
        if res is None or res.shape[0] != n:
            res = p0._random_batch_results = torch.zeros((n, p0.d + 2), dtype=p0.dt, device=p0.device)
        ptrs = (C.c_void_p * (n * members))(*[p for row in table for p in row])
        for pl in pls:
            pl._bind_rssm(width_of)
        L.check(p0.lib.icem_plan_step_random_learned_models(hs, n, bs, members, ptrs, L.RSSM_REDUCE[reduce], int(change_freq), offs,
                                                            None if member_costs is None else _ptr(member_costs), _ptr(res), p0._stream()))
        IcemPlanner._leave_member_costs(ens, models, member_costs, members, [p0.cfg.num_traj] * n)
        return res[:, :p0.d]

    @staticmethod
    def plan_step_cem_learned_batch(planners: Sequence["IcemPlanner"], model, observations, dists, *, like_levine: bool,
                                    shift_means: bool, execute_best_elite: bool) -> torch.Tensor:
        """:meth:`plan_step_cem_learned` of every planner of ``planners`` (one configuration; seeds, episodes, step counts
        and observations of their own) through the one ``model`` as ``icem_plan_step_cem_learned_batch``: every iteration 3
        launches for all of them.  ``observations``: ``[B, 230]`` array-like -- one host-to-device copy for the batch -- or
        an f32 device tensor, used where it lies.  ``dists[i]``: planner i's ``(mean, std, lower, upper)``, updated in
        place.  Each planner's ``cem_elites`` / ``cem_elite_costs`` / ``cem_elite_idx`` / ``cem_result`` afterwards are bit
        for bit those of its own :meth:`plan_step_cem_learned`; its ``cem_actions`` / ``cem_costs`` are scratch for B > 1
        (the batch scores its rows in a pool of the first planner's handle).  Returns the executed actions ``[B, d]``, a
        view of ``planners[0].cem_batch_results`` ``[B, d + 1]`` (kept per batch size).  Raises ``IcemError`` before anything
        runs, and before any planner has advanced, where the batch is not served."""
        pls = list(planners)
        n = len(pls)
        if n == 0:   # (the entry's own refusal: n outside [1, 32])
            L.check(L.load_library().icem_plan_step_cem_learned_batch(None, 0, None, None, None, None, None, None))
        p0 = pls[0]
        hs, bs, steps, res, prm = IcemPlanner._cem_learned_batch_io(pls, observations, dists, like_levine, shift_means, execute_best_elite)
        for pl in pls:
            pl._bind_rssm(model)
        L.check(p0.lib.icem_plan_step_cem_learned_batch(hs, n, bs, C.byref(prm), C.c_void_p(model.params.data_ptr()), steps, _ptr(res),
                                                        p0._stream()))
        for pl in pls:
            pl.mpc_step += 1
        return res[:, :p0.d]

    cem_actions = property(lambda self: self._cem_buffers()["actions"])
    cem_costs = property(lambda self: self._cem_buffers()["costs"])
    cem_elites = property(lambda self: self._cem_buffers()["elites"])
    cem_elite_costs = property(lambda self: self._cem_buffers()["elite_costs"])
    cem_elite_idx = property(lambda self: self._cem_buffers()["elite_idx"])
    cem_result = property(lambda self: self._cem_buffers()["result"])

    # ------------------------------------------------------------------ in-library elite exchange (world > 1)
    def connect_exchange(self, group=None):
        """Set up the in-library elite exchange between the ranks' processes (``icem_exchange_create`` /
        ``icem_exchange_connect``): every rank allocates its exchange block, the 64-byte IPC handles travel ONCE over
        ``torch.distributed`` (any backend), and from then on an MPC step makes no host-side collective: the records
        move as peer-to-peer stores issued by the library's own kernels (xGMI between GPUs)."""
        import torch.distributed as dist
        self._ensure_buffers()
        group = self.group if group is None else group
        mine = (C.c_ubyte * L.IPC_HANDLE_BYTES)()
        err = None
        try:
            L.check(self.lib.icem_exchange_create(self._h, mine))
        except L.IcemError as e:
            err = e
        handles = [None] * self.cfg.world
        dist.all_gather_object(handles, None if err else bytes(mine), group=group)
        if err is None and all(hd is not None for hd in handles):
            blob = (C.c_ubyte * (L.IPC_HANDLE_BYTES * self.cfg.world)).from_buffer_copy(b"".join(handles))
            try:
                L.check(self.lib.icem_exchange_connect(self._h, blob, None))
            except L.IcemError as e:
                err = e
        elif err is None:
            err = L.IcemError(L.ICEM_E_HIP if hasattr(L, "ICEM_E_HIP") else -3, "a peer could not create its exchange block")
        # all ranks or none: one rank that cannot map its peers sends everybody back to the host-driven all-gather
        oks = [None] * self.cfg.world
        dist.all_gather_object(oks, err is None, group=group)
        if all(oks):
            # ... and it has to WORK, not only map: a few real exchanges (every rank pushes to every rank and waits for
            # all of them); a rank whose waits time out (peer stores that never land) sends everybody back as well
            self._exchange = True
            try:
                self.exchange_probe(rounds=4)
                ok = self.exchange_status()[0] == 0
            except L.IcemError as e:
                ok, err = False, e
            dist.all_gather_object(oks, ok, group=group)
            if all(oks):
                return True
            if err is None:
                err = L.IcemError(-3, "the exchange self-test timed out on a rank")
        self.lib.icem_exchange_disable(self._h)
        self._exchange = False
        self.exchange_error = str(err) if err is not None else "a peer failed to connect"
        return False

    def degrade_exchange(self, group=None) -> str:
        """COLLECTIVE, after a run-time failure of the records' path (a bounded wait for a peer ran out: the next
        ``icem_plan_step_sharded`` raises): every rank leaves the path it was on and takes the next one in the order in-library
        exchange -> the library's RCCL all-gather -> host-driven all-gather; the distribution is re-initialised (the steps
        since the failure planned on garbage).  Returns the path now in use: ``"rccl"`` or ``"host"``."""
        torch.cuda.synchronize(self.device)
        was_exchange = bool(getattr(self, "_exchange", False))
        if was_exchange:
            status = self.exchange_status()[0] | int(getattr(self, "_xchg_status_seen", 0))   # read and clear
            self._xchg_status_seen = 0
            why = getattr(self, "_degrade_reason", None)   # (set by the caller when the trigger was not a timeout)
            self._degrade_reason = None
            self.exchange_error = (f"run time: {why} (status word {status})" if why and not (status & 1) else
                                   f"run time: a wait for a peer's elite records timed out (status word {status})")
            L.check(self.lib.icem_exchange_disable(self._h))
            self._exchange = False
        elif getattr(self, "_rccl", False):
            self.rccl_error = "run time: the in-library all-gather failed"
            self.lib.icem_rccl_disconnect(self._h)
            self._rccl = False
        self._gather_fn = None
        self.reset()
        if was_exchange and self.connect_rccl(group):
            return "rccl"
        return "host"

    def connect_rccl(self, group=None) -> bool:
        """The fallback of :meth:`connect_exchange`: an RCCL communicator owned by the library (``icem_rccl_connect``) so
        that ``icem_plan_step_sharded`` gathers the ranks' records with ``ncclAllGather`` on the launch stream
        (``icem_allgather_elites``) -- still one C call per MPC step and no host-side collective.  The 128-byte
        ``ncclUniqueId`` travels once over ``torch.distributed`` (any backend).  All ranks or none."""
        import torch.distributed as dist
        self._ensure_buffers()
        group = self.group if group is None else group
        err = None
        ident = [None]
        # RCCL wants one GPU per rank (two ranks on one device: "duplicate GPU", or a hang inside ncclCommInitRank):
        # find out BEFORE anybody enters the blocking call
        import socket
        where = [None] * self.cfg.world
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        mine = (socket.gethostname(), dev_index,
                tuple(os.environ.get(k, "") for k in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES")))
        dist.all_gather_object(where, mine, group=group)
        if len(set(where)) < self.cfg.world:
            self._rccl = False
            self.rccl_error = "two ranks share a GPU: RCCL needs one device per rank"
            return False
        try:
            # bind the copy of RCCL this process already carries (torch's), else torch's file, else the system's
            # (ICEM_RCCL_LIB names another one: read HERE, in the tooling -- the library reads no environment variable)
            L.check(self.lib.icem_rccl_load((os.environ.get("ICEM_RCCL_LIB") or
                                             os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")).encode()))
            if self.cfg.rank == 0:
                buf = (C.c_ubyte * L.RCCL_ID_BYTES)()
                L.check(self.lib.icem_rccl_unique_id(buf))
                ident = [bytes(buf)]
        except L.IcemError as e:
            err = e
        dist.broadcast_object_list(ident, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        oks = [None] * self.cfg.world
        dist.all_gather_object(oks, err is None and ident[0] is not None, group=group)
        if all(oks):   # (ncclCommInitRank blocks until every rank has called it: only enter it together)
            try:
                blob = (C.c_ubyte * L.RCCL_ID_BYTES).from_buffer_copy(ident[0])
                with torch.cuda.device(self.device):   # ncclCommInitRank binds the CURRENT device: the planner's, not torch's default
                    L.check(self.lib.icem_rccl_connect(self._h, blob))
                    # ... and one real all-gather, checked: every rank's K record slots marked with its number
                    K, r = self.K, self.cfg.rank
                    self.records.zero_()
                    self.records[r * K:(r + 1) * K] = float(r + 1)
                    L.check(self.lib.icem_allgather_elites(self._h, _ptr(self.records), self._stream()))
                    torch.cuda.synchronize(self.device)
                    want = torch.arange(1, self.cfg.world + 1, device=self.device, dtype=self.dt).repeat_interleave(K)
                    if not bool((self.records == want[:, None]).all().item()):
                        raise RuntimeError("the in-library all-gather returned other ranks' records in the wrong slots or not at all")
                    self.records.zero_()
            except (L.IcemError, RuntimeError) as e:
                err = e
            dist.all_gather_object(oks, err is None, group=group)
            if all(oks):
                self._rccl = True
                return True
        self.lib.icem_rccl_disconnect(self._h)
        self._rccl = False
        self.rccl_error = str(err) if err is not None else "a peer failed to create the communicator"
        return False

    @staticmethod
    def connect_exchange_local(planners: Sequence["IcemPlanner"]):
        """The same for ranks that live in ONE process (tests, several GPUs driven by one host thread): the blocks are
        handed over as device pointers, no IPC."""
        for pl in planners:
            pl._ensure_buffers()
            scratch = (C.c_ubyte * L.IPC_HANDLE_BYTES)()
            L.check(pl.lib.icem_exchange_create(pl._h, scratch))
        blocks = (C.c_void_p * len(planners))(*[pl.lib.icem_exchange_block(pl._h) for pl in planners])
        for pl in planners:
            L.check(pl.lib.icem_exchange_connect(pl._h, None, blocks))
            pl._exchange = True

    def exchange_status(self) -> Tuple[int, bool]:
        """(status, finegrained): status != 0 means a device-side wait for a peer timed out since the last call."""
        s, f = C.c_int32(), C.c_int32()
        L.check(self.lib.icem_exchange_status(self._h, C.byref(s), C.byref(f)))
        return s.value, bool(f.value)

    def exchange_probe(self, rounds: int = 200) -> float:
        """Average latency [us] of one in-library exchange (collective: all ranks call it together)."""
        us = C.c_double()
        L.check(self.lib.icem_exchange_probe(self._h, rounds, self._stream(), C.byref(us)))
        return us.value

    def _resident_gather(self):
        """The per-iteration all-gather of the bench loop with everything that does not change hoisted out: on RCCL
        it is one in-place ``all_gather_into_tensor`` of this rank's K records."""
        g = getattr(self, "_gather_fn", None)
        if g is None:
            import torch.distributed as dist
            rank, world, K, records, group = self.cfg.rank, self.cfg.world, self.K, self.records, self.group
            if records.is_cuda and dist.get_backend(group) == "nccl":
                mine = records[rank * K:(rank + 1) * K]
                g = lambda: dist.all_gather_into_tensor(records, mine, group=group)  # noqa: E731
            else:
                g = lambda: exchange_records(records, K, rank, world, group)  # noqa: E731
            self._gather_fn = g
        return g

    def _set_deferral(self, on: bool):
        if getattr(self, "_deferral", False) != on:
            L.check(self.lib.icem_set_merge_deferral(self._h, int(on)))
            self._deferral = on

    # ------------------------------------------------------------------ fused MPC step
    def _ensure_buffers(self, learned: bool = False):
        """``learned``: for the learned-dynamics step, which needs no built-in model (``obs0`` then stays empty; the step's
        observation lives in ``obs_rssm``, 230 f32)."""
        if learned and getattr(self, "obs_rssm", None) is None:
            self.obs_rssm = torch.zeros((L.RSSM_OBS_DIM,), dtype=torch.float32, device=self.device)
        if self._bufs is not None:
            return
        if self.obs_dim == 0 and not learned:
            raise RuntimeError("set_model()/set_cost() must be called before planning")
        names = ["mean", "std", "low", "high", "obs0", "actions", "costs", "elites", "records", "workspace",
                 "executed", "best_cost"]
        t = {}
        for which, name in enumerate(names):
            nbytes = self.lib.icem_plan_buffer_bytes(self._h, which)
            if name in ("low", "high"):
                t[name] = self.low if name == "low" else self.high
                continue
            t[name] = torch.zeros((max(1, nbytes),), dtype=torch.uint8, device=self.device)
        self._bufs = t
        self.mean = t["mean"].view(self.dt).view(self.h, self.d)
        self.std = t["std"].view(self.dt).view(self.h, self.d)
        self.obs0 = t["obs0"].view(self.dt)
        self.executed = t["executed"].view(self.dt)
        self.best_cost = t["best_cost"].view(self.dt)
        self.actions = t["actions"].view(self.dt).view(-1, self.h, self.d)
        self.costs = t["costs"].view(self.dt)
        rs = self.h * self.d + 2
        self.records = t["records"].view(self.dt).view(self.cfg.world * self.K, rs)
        el = t["elites"].view(self.dt)
        khd = self.K * self.h * self.d
        self.elites_actions = el[:2 * khd].view(2, self.K, self.h, self.d)
        self.elites_costs = el[2 * khd:].view(2, self.K)
        self._cb = L.IcemPlanBuffersC(**{n: t[n].data_ptr() for n in names})
        self._cb.z_r = self._cb.z_i = self._cb.z_r_shift = self._cb.z_i_shift = None

    def reset(self):
        """``MpcICem.beginning_of_rollout`` (icem/controllers/icem.py:31-43)."""
        self._ensure_buffers()
        self.reset_distribution(self.mean, self.std)
        self.mpc_step = 0

    def new_episode(self) -> int:
        """Move the device noise streams on to the next episode (``icem_set_episode``): the reference's ``np.random``
        stream runs on across episodes (icem/controllers/icem.py:73-77), so rollouts must not replay each other's
        exploration noise.  The first call selects episode 0.  Returns the episode number."""
        self.episode = self._episodes_started
        self._episodes_started += 1
        L.check(self.lib.icem_set_episode(self._h, self.episode))
        return self.episode

    def noise_offset(self, call: int) -> int:
        """Stream offset of sampling call ``call`` of the current episode (what ``icem_plan_*`` use internally)."""
        return (self.episode << 32) + int(call)

    def current_elites(self):
        """Elite actions [K,h,d] and costs [K] of the latest iteration (best first)."""
        g = (self.mpc_step * self.cfg.opt_iters) & 1
        return self.elites_actions[g], self.elites_costs[g]

    def local_count(self, it: int) -> int:
        lo, hi = shard_range(self.population_sizes[it], self.cfg.rank, self.cfg.world)
        return hi - lo

    def plan_step(self, obs, noise: Optional[NoiseFn] = None, on_iteration=None) -> torch.Tensor:
        """One MPC step = the loop of ``MpcICem.get_action`` (icem/controllers/icem.py:123-175).
        Returns the executed action as a device tensor ``[d]`` (no host sync).  ``noise`` switches to
        the parity mode: the white draws come from the callback (in the reference's call order)."""
        self._ensure_buffers()
        self.obs0.copy_(torch.as_tensor(np.asarray(obs, dtype=np.float64), dtype=self.dt), non_blocking=False)
        cfg = self.cfg
        st = self._stream()
        xchg = getattr(self, "_exchange", False)
        if noise is None and on_iteration is None and (cfg.world == 1 or xchg or getattr(self, "_rccl", False)):
            self._cb.z_r = self._cb.z_i = self._cb.z_r_shift = self._cb.z_i_shift = None
            L.check(self.lib.icem_plan_step_sharded(self._h, C.byref(self._cb), self.mpc_step, st))
        else:
            self._set_deferral(False)  # callers of this form look at the buffers between iterations
            keep = []
            for it in range(cfg.opt_iters):
                self._cb.z_r = self._cb.z_i = self._cb.z_r_shift = self._cb.z_i_shift = None
                if noise is not None:
                    n_it = self.population_sizes[it]
                    lo, hi = shard_range(n_it, cfg.rank, cfg.world)
                    z_r, z_i = noise(n_it)  # the reference draws the whole batch (icem.py:73 / :77)
                    zr = self._t(z_r[lo:hi])
                    zi = self._t(z_i[lo:hi]) if z_i is not None and cfg.noise_beta > 0 else None
                    keep += [zr, zi]
                    self._cb.z_r, self._cb.z_i = zr.data_ptr(), (zi.data_ptr() if zi is not None else None)
                    if it == 0 and cfg.shift_elites and self.mpc_step > 0 and self.n_reuse > 0:
                        s_r, s_i = noise(self.n_reuse)  # icem.py:102
                        sr = self._t(s_r)
                        si = self._t(s_i) if s_i is not None and cfg.noise_beta > 0 else None
                        keep += [sr, si]
                        self._cb.z_r_shift = sr.data_ptr()
                        self._cb.z_i_shift = si.data_ptr() if si is not None else None
                L.check(self.lib.icem_plan_iter_local(self._h, C.byref(self._cb), self.mpc_step, it, st))
                if cfg.world > 1 and not xchg:  # (connected exchange: the local call has pushed the records already)
                    exchange_records(self.records, self.K, cfg.rank, cfg.world, self.group)
                L.check(self.lib.icem_plan_iter_merge(self._h, C.byref(self._cb), self.mpc_step, it, st))
                if on_iteration is not None:
                    on_iteration(it)
            if keep:
                torch.cuda.current_stream(self.device).synchronize()  # z tensors must outlive the kernels
        self.mpc_step += 1
        return self.executed
