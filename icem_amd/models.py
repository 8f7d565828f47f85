"""Forward-model side of the boundary.

``ForwardModel`` mirrors the reference's batched model contract
(icem/misc/base_types.py:62-118, icem/models/abstract_models.py:8-53): ``predict`` maps
``([N,o], states, [N,d]) -> ([N,o], states, [N,1])`` and ``predict_n_steps`` rolls a policy out
for ``horizon`` steps.  ``DeviceSyntheticModel`` is the built-in analytic model the HIP rollout
kernel evaluates on the GPU; its NumPy ``predict`` exists so the same object can be driven
through the reference-style interface (used by the host-model path and by tests).
"""
from __future__ import annotations

import math
from abc import ABC, abstractmethod

import numpy as np

MODEL_LINEAR, MODEL_TANH = 0, 1


class TrajectoryBatch:
    """What ``predict_n_steps`` returns here instead of N ``Rollout`` objects (the reference
    spends ~90 % of a step building those -- icem/misc/rolloutbuffer.py:16-39,155-172): flat
    arrays ``[N,h,.]``.  Indexing yields per-trajectory dict views so reference-style consumers
    (``r["observations"]``, ``buffer.as_array("actions")``) keep working."""

    fields = ("observations", "next_observations", "actions", "rewards")

    def __init__(self, **arrays):
        self._a = {k: np.asarray(v) for k, v in arrays.items()}
        n = {len(v) for v in self._a.values()}
        if len(n) > 1:
            raise TypeError("Turning rollout structure into numpy array failed. Rollouts of unequal length?")

    def __len__(self):
        return len(next(iter(self._a.values()))) if self._a else 0

    def __bool__(self):
        return len(self) > 0

    def as_array(self, key):
        return self._a[key]

    def __getitem__(self, item):
        if isinstance(item, str):
            return self._a[item].reshape((-1,) + self._a[item].shape[2:])
        if isinstance(item, (int, np.integer)):
            return {k: v[item] for k, v in self._a.items()}
        return TrajectoryBatch(**{k: v[item] for k, v in self._a.items()})

    def __iter__(self):
        for i in range(len(self)):
            yield self[i]

    # -- the mutating half of RolloutBuffer's sequence interface (icem/misc/rolloutbuffer.py:112-123, 156-172, 277) ----------
    @property
    def is_empty(self):
        return len(self) == 0

    def extend(self, other):
        """Add trajectories: another ``TrajectoryBatch`` (its arrays are concatenated along N) or an iterable of
        per-trajectory dict views as ``self[i]`` hands them out.  An empty batch takes the other's fields; otherwise the
        fields must be the same and of the same horizon -- the reference's "Rollouts of unequal length?" error."""
        if not isinstance(other, TrajectoryBatch):
            rows = list(other)
            if not rows:
                return
            try:
                other = TrajectoryBatch(**{k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0]})
            except (ValueError, KeyError) as e:
                raise TypeError(f"Concatenating rollouts failed with error {e}")
        if len(other) == 0:
            return
        if not self._a:
            self._a = {k: np.array(v) for k, v in other._a.items()}
            return
        if set(other._a) != set(self._a) or any(other._a[k].shape[1:] != v.shape[1:] for k, v in self._a.items()):
            raise TypeError("Turning rollout structure into numpy array failed. Rollouts of unequal length?")
        self._a = {k: np.concatenate([v, other._a[k]], axis=0) for k, v in self._a.items()}

    def append(self, item):
        self.extend([item])

    @property
    def flat(self):
        """All transitions of all trajectories, ``{field: [N * h, ...]}`` (``RolloutBuffer.flat``: the concatenation of the
        rollouts' transition records); per-trajectory scalars such as ``costs`` are left out."""
        return {k: v.reshape((-1,) + v.shape[2:]) for k, v in self._a.items() if v.ndim >= 2}


class ForwardModel(ABC):
    supports_stochastic = False

    def __init__(self, *, env=None):
        self.env = env

    def reset(self, observation):
        return None

    def got_actual_observation_and_env_state(self, *, observation, env_state=None, model_state=None):
        return None

    @abstractmethod
    def predict(self, *, observations, states, actions):
        """-> (next_observations [N,o], next_states, rewards [N,1])"""

    def rollout_generator(self, start_states, start_observations, horizon, policy, mode=None):
        states, obs = start_states, start_observations
        for _ in range(horizon):
            actions = policy.get_action(obs, state=states, mode=mode)
            next_obs, next_states, r = self.predict(observations=obs, states=states, actions=actions)
            yield obs, next_obs, actions, states, r
            states, obs = next_states, next_obs

    def rollout_field_names(self):
        return TrajectoryBatch.fields

    def predict_n_steps(self, *, start_observations, start_states, policy, horizon):
        if start_observations.ndim != 2:
            raise AttributeError("call predict_n_steps with a batch of states")
        if len(start_observations) != len(start_states):
            raise AttributeError("number of observations and states have to be the same")
        obs, nxt, act, states, rew = zip(*self.rollout_generator(start_states, start_observations, horizon, policy))
        tr = lambda x: np.asarray(x).transpose((1, 0, 2))
        return TrajectoryBatch(observations=tr(obs), next_observations=tr(nxt), actions=tr(act),
                               rewards=tr(rew)), states[-1]

    def train(self, buffer):
        pass

    def save(self, path):
        pass

    def load(self, path):
        pass


class DeviceSyntheticModel(ForwardModel):
    """``o' = act(o @ A + a @ B)``, ``A [o,o]``, ``B [d,o]``; ``kind`` linear or tanh; ``band >= 0``
    zeroes ``A`` outside ``|row-col| <= band``."""

    def __init__(self, A, B, kind: int = MODEL_LINEAR, band: int = -1, env=None):
        super().__init__(env=env)
        A = np.array(A, dtype=np.float64)
        B = np.array(B, dtype=np.float64)
        if band >= 0:
            r = np.arange(A.shape[0])
            A = np.where(np.abs(r[:, None] - r[None, :]) <= band, A, 0.0)
        self.A, self.B, self.kind, self.band = A, B, kind, band
        self.obs_dim, self.act_dim = A.shape[0], B.shape[0]

    @staticmethod
    def make(obs_dim: int, act_dim: int, kind: int = MODEL_LINEAR, band: int = -1, seed_a: int = 0,
             seed_b: int = 1, env=None) -> "DeviceSyntheticModel":
        """The synthetic dynamics of the benchmark configs: ``A = 0.95 I + 0.05 N(0,1)/sqrt(o)``
        (RandomState(seed_a)), ``B = 0.1 N(0,1)`` (RandomState(seed_b))."""
        A = 0.95 * np.eye(obs_dim) + 0.05 * np.random.RandomState(seed_a).randn(obs_dim, obs_dim) / math.sqrt(obs_dim)
        B = 0.1 * np.random.RandomState(seed_b).randn(act_dim, obs_dim)
        return DeviceSyntheticModel(A, B, kind, band, env)

    def predict(self, *, observations, states, actions):
        observations = np.asarray(observations, dtype=np.float64)
        actions = np.asarray(actions, dtype=np.float64)
        nxt = np.zeros_like(observations)
        for k in range(self.obs_dim):
            nxt = nxt + observations[..., k:k + 1] * self.A[k]
        for j in range(self.act_dim):
            nxt = nxt + actions[..., j:j + 1] * self.B[j]
        if self.kind == MODEL_TANH:
            nxt = np.tanh(nxt)
        # a model that carries its environment reports the environment's reward, like the reference's ground-truth
        # models do (env.step's reward = -cost_fn); without one there is no reward to report
        if self.env is not None and hasattr(self.env, "reward_fn"):
            rew = np.asarray(self.env.reward_fn(observations, actions, nxt), dtype=np.float64)[..., None]
        else:
            rew = np.zeros(observations.shape[:-1] + (1,))
        return nxt, None, rew


class TorchForwardModel(ForwardModel):
    """Adapter for a learned, device-resident dynamics model (the README's PlaNet column has no
    code in the reference, so the architecture is the caller's).  ``module(obs[N,o], act[N,d]) -> next_obs[N,o]``
    is any ``torch.nn.Module`` on the GPU (its GEMMs run on the matrix cores through hipBLASLt, bf16 if the
    module is bf16); ``cost(obs, act) -> [N]`` is a torch callable.  ``MpcICemHip`` keeps the whole CEM loop on
    the device with it; ``predict`` serves the reference-style NumPy interface."""

    def __init__(self, module, cost, obs_dim: int, act_dim: int, dtype=None, device="cuda:0", env=None, use_graph=True):
        super().__init__(env=env)
        import torch
        self.use_graph = use_graph   # replay the h-step chain of torch launches as a HIP graph (MpcController._costs_of)
        self.module = module.to(device)
        self.cost = cost
        self.obs_dim, self.act_dim = obs_dim, act_dim
        self.device = torch.device(device)
        self.dtype = dtype or next(module.parameters()).dtype

    def torch_step(self, obs, act):
        import torch
        with torch.no_grad():
            return self.module(obs, act)

    def torch_cost(self, obs, act):
        import torch
        with torch.no_grad():
            return self.cost(obs, act)

    def predict(self, *, observations, states, actions):
        import torch
        o = torch.as_tensor(np.asarray(observations), dtype=self.dtype, device=self.device)
        a = torch.as_tensor(np.asarray(actions), dtype=self.dtype, device=self.device)
        single = o.ndim == 1
        if single:
            o, a = o[None], a[None]
        nxt = self.torch_step(o, a).float().cpu().numpy().astype(np.float64)
        if single:
            nxt = nxt[0]
        return nxt, None, np.zeros(nxt.shape[:-1] + (1,))


def declared_rssm(act_dim: int = 6, det: int = 200, stoch: int = 30, hidden: int = 200, seed: int = 0, dtype=None,
                  device="cuda:0", env=None) -> TorchForwardModel:
    """The learned-dynamics stand-in declared for BASELINE config 5 (N=1024, h=12: "PlaNet learned dynamics" -- the
    reference ships no such model, README.md:21-29 only quotes its results): a recurrent state-space model in the
    PlaNet shape, rolled out on its prior mean.  Planner observation = ``[h (det) | z (stoch)]``;
    ``x = relu(W1 [z, a])``, ``h' = GRUCell(x, h)``, ``z' = W3 relu(W2 h')`` and a two-layer reward head on
    ``[h', z']``; cost of a step = minus the predicted reward of the state it starts from.  Random weights
    (``seed``); ``dtype=torch.bfloat16`` runs the GEMMs on the bf16 matrix cores through hipBLASLt."""
    import torch

    class RSSM(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.det, self.stoch = det, stoch
            self.inp = torch.nn.Linear(stoch + act_dim, hidden)
            self.gru = torch.nn.GRUCell(hidden, det)
            self.prior1 = torch.nn.Linear(det, hidden)
            self.prior2 = torch.nn.Linear(hidden, stoch)
            self.rew1 = torch.nn.Linear(det + stoch, hidden)
            self.rew2 = torch.nn.Linear(hidden, hidden)
            self.rew3 = torch.nn.Linear(hidden, 1)

        def forward(self, obs, act):
            h, z = obs[:, :self.det], obs[:, self.det:]
            x = torch.relu(self.inp(torch.cat([z, act], dim=-1)))
            h2 = self.gru(x, h)
            z2 = self.prior2(torch.relu(self.prior1(h2)))
            return torch.cat([h2, z2], dim=-1)

        def reward(self, obs):
            return self.rew3(torch.relu(self.rew2(torch.relu(self.rew1(obs))))).squeeze(-1)

    gen = torch.Generator().manual_seed(seed)
    net = RSSM()
    with torch.no_grad():
        for p in net.parameters():   # reproducible weights, independent of torch's global RNG state
            bound = 1.0 / math.sqrt(p.shape[-1]) if p.ndim > 1 else 0.05
            p.copy_((torch.rand(p.shape, generator=gen) * 2 - 1) * bound)
    if dtype is not None:
        net = net.to(dtype)
    return TorchForwardModel(net, lambda o, a: -net.reward(o), det + stoch, act_dim, dtype=dtype, device=device, env=env)


def pack_rssm(module):
    """The packed bf16 parameter buffer ``icem_rssm_rollout_cost_w`` reads (layout: icem_amd/csrc/icem_rssm.h) from a
    ``declared_rssm`` module of any action width 1 .. 32: every weight padded (outputs to multiples of 16, contraction to
    multiples of 32), cut into 16 x 32 blocks stored as ``v_mfma_f32_16x16x32_bf16`` A operands
    ``[out block][k block][lane = 16*g + i][v]`` = ``W[16*ob + i][32*kb + 8*g + v]``, each layer followed by its f32 bias.
    The action columns of the input layer fill the front of its second K block (columns 32 .. 32 + act of ``[z | a]``) with
    zeros behind them, so the buffer has the same size at every width."""
    import torch
    sd = {k: v.detach().float().cpu() for k, v in module.state_dict().items()}
    det, st = module.det, module.stoch
    act = sd["inp.weight"].shape[1] - st
    assert (det, st) == (200, 30) and sd["inp.weight"].shape[0] == 200 and 1 <= act <= 32, \
        "icem_rssm_rollout_cost is compiled for the declared sizes (200 / 30 / 200) and 1 to 32 action dimensions"

    def pad(w, rows, cols, col_map=None):
        out = torch.zeros(rows, cols)
        if col_map is None:
            out[:w.shape[0], :w.shape[1]] = w
        else:
            for (s0, s1, d0) in col_map:
                out[:w.shape[0], d0:d0 + (s1 - s0)] = w[:, s0:s1]
        return out

    def gates(w, cols):   # [3*200, k] -> [3*208, cols]: each gate padded separately
        return torch.cat([pad(w[i * det:(i + 1) * det], 208, cols) for i in range(3)], dim=0)

    def gate_bias(b):
        return torch.cat([pad(b[i * det:(i + 1) * det][None], 1, 208)[0] for i in range(3)])

    layers = [
        (pad(sd["inp.weight"], 208, 64, [(0, st, 0), (st, st + act, 32)]), pad(sd["inp.bias"][None], 1, 208)[0]),
        (gates(sd["gru.weight_ih"], 224), gate_bias(sd["gru.bias_ih"])),
        (gates(sd["gru.weight_hh"], 224), gate_bias(sd["gru.bias_hh"])),
        (pad(sd["prior1.weight"], 208, 224), pad(sd["prior1.bias"][None], 1, 208)[0]),
        (pad(sd["prior2.weight"], 32, 224), pad(sd["prior2.bias"][None], 1, 32)[0]),
        (pad(sd["rew1.weight"], 208, 256, [(0, det, 0), (det, det + st, 224)]), pad(sd["rew1.bias"][None], 1, 208)[0]),
        (pad(sd["rew2.weight"], 208, 224), pad(sd["rew2.bias"][None], 1, 208)[0]),
        (pad(sd["rew3.weight"], 16, 224), pad(sd["rew3.bias"][None], 1, 16)[0]),
    ]
    chunks = []
    for w, b in layers:
        ob, kb = w.shape[0] // 16, w.shape[1] // 32
        blocks = w.reshape(ob, 16, kb, 4, 8).permute(0, 2, 3, 1, 4).contiguous()   # [ob, kb, g, i, v]
        chunks.append(blocks.to(torch.bfloat16).view(torch.int16).reshape(-1))
        chunks.append(b.contiguous().view(torch.int16).reshape(-1))                 # f32 bias as two 16-bit words each
    return torch.cat(chunks)


class DeviceRSSMModel(ForwardModel):
    """The declared RSSM with its whole h-step rollout + cost fused into one HIP launch on the bf16 matrix cores
    (``icem_rssm_rollout_cost_w``); ``MpcICemHip`` scores a population with it in a single kernel.  ``reference`` is the
    f32 torch module the weights come from (``predict`` serves the reference-style NumPy interface through it):
    ``declared_rssm(act_dim, seed=seed)``'s, or a copy of the caller's ``module`` -- any module of the declared sizes with the
    declared parameter names, e.g. a ``declared_rssm(...).module`` whose weights were trained or edited.  ``act_dim``
    (1 .. 32) is the action width: the argument's, or with a ``module`` that of its input layer."""

    act_dim = 6   # the declared width (an instance carries its own; the shape checks of the wrappers read it first)

    def __init__(self, seed: int = 0, device="cuda:0", env=None, module=None, act_dim: int = 6):
        super().__init__(env=env)
        import torch
        from . import _lib as L
        if module is None:
            if not 1 <= int(act_dim) <= 32:
                raise ValueError(f"the device RSSM takes 1 to 32 action dimensions, not {act_dim}")
            self._tm = declared_rssm(act_dim=int(act_dim), seed=seed, device=device)
        else:
            import copy
            net = copy.deepcopy(module).float()
            act_dim = net.inp.in_features - net.stoch
            self._tm = TorchForwardModel(net, lambda o, a: -net.reward(o), net.det + net.stoch, act_dim, device=device, env=env)
        self.reference = self._tm.module
        self.obs_dim, self.act_dim = 230, int(act_dim)
        self.device = torch.device(device)
        self.params = pack_rssm(self.reference).to(self.device)
        self.lib = L.load_library()
        L.maybe_follow_environment()   # (tools only: icem_amd._lib.follow_environment)
        self._obs_host = self._obs_dev = None
        if self.params.numel() != self.lib.icem_rssm_param_elems():
            raise RuntimeError("packed RSSM parameters do not match the library's layout")

    def rollout_cost(self, obs, actions, cost_mode: int = 0):
        """costs ``[n]`` (f32 device tensor) of f32 device action sequences ``[n, h, act_dim]`` from observation ``obs [230]``."""
        import ctypes as C
        import torch
        from . import _lib as L
        if actions.ndim != 3 or actions.shape[2] != self.act_dim:
            raise ValueError(f"actions must be [n, h, {self.act_dim}], got {tuple(actions.shape)}")
        actions = actions.to(torch.float32).contiguous()
        n, h, _ = actions.shape
        ob = np.asarray(obs, dtype=np.float32)
        if self._obs_host is None or not np.array_equal(ob, self._obs_host):   # the CEM iterations of a step share it
            self._obs_host, self._obs_dev = ob.copy(), torch.as_tensor(ob, device=self.device)
        o = self._obs_dev
        costs = torch.empty((n,), dtype=torch.float32, device=self.device)
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib.icem_rssm_rollout_cost_w(n, h, self.act_dim, cost_mode, C.c_void_p(self.params.data_ptr()), C.c_void_p(o.data_ptr()),
                                                  C.c_void_p(actions.data_ptr()), C.c_void_p(costs.data_ptr()), st))
        return costs

    def rollout_cost_batch(self, observations, actions, rows, cost_mode: int = 0):
        """``rollout_cost`` of B problems in ONE launch (``icem_rssm_rollout_cost_batch_w``): problem p scores its ``rows[p]``
        action sequences -- back to back in ``actions [sum rows, h, act_dim]`` (f32 device tensor) -- from ``observations[p]``
        (``[B, 230]`` array-like, or an f32 device tensor that is used as is).  -> costs ``[sum rows]``, every problem's
        slice bit for bit what ``rollout_cost`` gives for it alone; B = 1 is ``rollout_cost``."""
        import ctypes as C
        import torch
        from . import _lib as L
        rows = [int(r) for r in rows]
        if actions.ndim != 3 or actions.shape[2] != self.act_dim:
            raise ValueError(f"actions must be [sum rows, h, {self.act_dim}], got {tuple(actions.shape)}")
        if sum(rows) != actions.shape[0]:
            raise ValueError(f"rows sum to {sum(rows)} but actions has {actions.shape[0]} rows")
        on_device = isinstance(observations, torch.Tensor) and observations.is_cuda
        if not on_device:
            observations = np.asarray(observations, dtype=np.float32)
        if tuple(observations.shape) != (len(rows), 230):
            raise ValueError(f"observations must be [{len(rows)}, 230] (one start state per problem), got {tuple(observations.shape)}")
        if on_device and (observations.dtype != torch.float32 or not observations.is_contiguous()):
            raise ValueError("a device tensor of observations must be contiguous float32")
        o = observations if on_device else torch.as_tensor(observations, device=self.device)
        actions = actions.to(torch.float32).contiguous()
        costs = torch.empty((actions.shape[0],), dtype=torch.float32, device=self.device)
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib.icem_rssm_rollout_cost_batch_w(len(rows), (C.c_int32 * len(rows))(*rows), actions.shape[1], self.act_dim, cost_mode,
                                                        C.c_void_p(self.params.data_ptr()), C.c_void_p(o.data_ptr()),
                                                        C.c_void_p(actions.data_ptr()), C.c_void_p(costs.data_ptr()), st))
        return costs

    def predict(self, *, observations, states, actions):
        return self._tm.predict(observations=observations, states=states, actions=actions)


def _rssm_models_launch(lib, device, act_dim, params_ptrs, obs_rows, arow0, rows, obs_dev, n_obs, actions, cost_mode, out=None):
    """One ``icem_rssm_rollout_cost_models`` launch: problem p = (params_ptrs[p], obs_rows[p], arow0[p], rows[p]) over the f32
    device tensors ``obs_dev [n_obs, 230]`` and ``actions [n_action_rows, h, act_dim]`` -> costs ``[sum rows]`` (``out``, or new)."""
    import ctypes as C
    import torch
    from . import _lib as L
    n = len(rows)
    costs = torch.empty((sum(rows),), dtype=torch.float32, device=device) if out is None else out
    problems = (L.IcemRssmProblemC * n)(*[L.IcemRssmProblemC(int(params_ptrs[p]), int(arow0[p]), int(rows[p]), int(obs_rows[p]))
                                           for p in range(n)])
    st = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    L.check(lib.icem_rssm_rollout_cost_models(n, problems, actions.shape[1], act_dim, cost_mode, C.c_void_p(obs_dev.data_ptr()), n_obs,
                                              C.c_void_p(actions.data_ptr()), actions.shape[0], C.c_void_p(costs.data_ptr()), st))
    return costs


def _check_problem_shapes(act_dim, n_problems, observations, actions, rows, action_row0, obs_dim: int = 230):
    """The shape checks of ``rollout_cost_batch`` for problems that may share action rows (needs nothing of a device);
    ``obs_dim``: the width of a start observation (the RSSM's 230, or an MLP's own).
    -> (rows, action_row0, observations: a device tensor as it came, or an f32 array)."""
    import torch
    rows = [int(r) for r in rows]
    if len(rows) != n_problems:
        raise ValueError(f"{n_problems} problems but {len(rows)} row counts")
    if actions.ndim != 3 or actions.shape[2] != act_dim:
        raise ValueError(f"actions must be [rows, h, {act_dim}], got {tuple(actions.shape)}")
    if any(r < 1 for r in rows):
        raise ValueError(f"every problem needs at least one row, got {rows}")
    if action_row0 is None:   # back to back
        if sum(rows) != actions.shape[0]:
            raise ValueError(f"rows sum to {sum(rows)} but actions has {actions.shape[0]} rows")
        action_row0 = [sum(rows[:p]) for p in range(len(rows))]
    else:
        action_row0 = [int(a) for a in action_row0]
        if len(action_row0) != len(rows):
            raise ValueError(f"{len(rows)} row counts but {len(action_row0)} first action rows")
        for a, r in zip(action_row0, rows):
            if a < 0 or a + r > actions.shape[0]:
                raise ValueError(f"action rows {a} .. {a + r} lie outside actions' {actions.shape[0]} rows")
    on_device = isinstance(observations, torch.Tensor) and observations.is_cuda
    if not on_device:
        observations = np.asarray(observations, dtype=np.float32)
    if tuple(observations.shape) != (len(rows), obs_dim):
        raise ValueError(f"observations must be [{len(rows)}, {obs_dim}] (one start state per problem), got {tuple(observations.shape)}")
    if on_device and (observations.dtype != torch.float32 or not observations.is_contiguous()):
        raise ValueError("a device tensor of observations must be contiguous float32")
    return rows, action_row0, observations


def rssm_rollout_cost_models(models, observations, actions, rows, action_row0=None, cost_mode: int = 0):
    """``DeviceRSSMModel.rollout_cost`` of B problems with a MODEL EACH in ONE launch (``icem_rssm_rollout_cost_models``; the
    reference's parallel episodes, icem/misc/rollout_utils.py:46-58, 129-152, each with its own trained model): problem p
    scores ``rows[p]`` action sequences of ``actions [n, h, act_dim]`` (f32 device tensor) -- from row ``action_row0[p]`` on, or
    back to back with ``action_row0=None``; the rows of different problems may overlap or coincide -- from ``observations[p]``
    (``[B, 230]`` array-like, or an f32 device tensor that is used as is) through ``models[p]`` (``DeviceRSSMModel``s of one
    action width on one device; the same model may serve several problems).  -> costs ``[sum rows]``, problem p's rows back
    to back in problem order, each bit for bit what ``models[p].rollout_cost`` gives for it alone.  B <= 32."""
    import torch
    models = list(models)
    if not 1 <= len(models) <= 32:
        raise ValueError(f"one launch takes 1 to 32 problems, not {len(models)}")
    act_dim = models[0].act_dim
    if any(m.act_dim != act_dim for m in models):
        raise ValueError(f"the models must share one action width, got {[m.act_dim for m in models]}")
    rows, action_row0, observations = _check_problem_shapes(act_dim, len(models), observations, actions, rows, action_row0)
    m0 = models[0]
    if any(m.params.device != m0.params.device for m in models):
        raise ValueError("the models' parameter buffers must be on one device")
    o = observations if isinstance(observations, torch.Tensor) else torch.as_tensor(observations, device=m0.device)
    actions = actions.to(torch.float32).contiguous()
    return _rssm_models_launch(m0.lib, m0.device, act_dim, [m.params.data_ptr() for m in models], range(len(models)), action_row0, rows,
                               o, len(models), actions, cost_mode)


class DeviceRSSMEnsemble(ForwardModel):
    """E ``DeviceRSSMModel``s that score every candidate plan together (the model loop of the reference's
    icem/models/abstract_models.py:17-53, with members trained from different seeds): a plan's cost is the members' mean
    (``reduce="mean"``) or the worst member's (``"max"``, the cautious planner), so that one model's error is not exploited.
    Built from ``models=[DeviceRSSMModel, ...]`` or from ``seeds=[...]`` (+ ``act_dim``, default: the models' width, or 6);
    1 to 32 members of one action width.  ``rollout_cost`` is ONE learned-dynamics launch for all members
    (``icem_rssm_rollout_cost_ensemble``) + the reduction; ``member_costs`` holds the last ``[E, n]`` (row e: member e alone,
    bit for bit).  ``params`` are the members' packed buffers stacked ``[E, elems]`` on one device -- the launch reads these.

    It is deliberately NOT a ``DeviceRSSMModel``: the library's fused ``*_learned`` steps know one parameter buffer.
    ``MpcICemHip`` takes the whole MPC step through it as one library call (``icem_plan_step_learned_models``: the members'
    reduction inside the update launch) where that entry serves the planner, and so do the CEM and random-shooting baselines
    (``icem_plan_step_cem_learned_models`` / ``icem_plan_step_random_learned_models``: the reduction inside the update /
    the selection launch); all leave ``member_costs`` as the stage-wise loop does: the last iteration's ``[E, rows]`` (with
    an ensemble per planner, each ensemble's is its planner's columns of the step's one table: a view).  ``predict`` -- the reference-style interface needs ONE successor state -- delegates to
    member 0."""

    obs_dim = 230

    def __init__(self, models=None, seeds=None, act_dim=None, reduce: str = "mean", device="cuda:0", env=None):
        super().__init__(env=env)
        import torch
        from . import _lib as L
        if reduce not in L.RSSM_REDUCE:
            raise ValueError(f"reduce must be 'mean' or 'max', not {reduce!r}")
        if (models is None) == (seeds is None):
            raise ValueError("give either models=[DeviceRSSMModel, ...] or seeds=[...]")
        count = len(models) if models is not None else len(seeds)
        if not 1 <= count <= L.RSSM_BATCH_MAX:
            raise ValueError(f"an ensemble has 1 to {L.RSSM_BATCH_MAX} members (one launch serves them all), not {count}")
        if models is None:
            models = [DeviceRSSMModel(seed=int(s), device=device, env=env, act_dim=6 if act_dim is None else int(act_dim)) for s in seeds]
        models = list(models)
        if not all(isinstance(m, DeviceRSSMModel) for m in models):
            raise ValueError("the members of a DeviceRSSMEnsemble are DeviceRSSMModels")
        widths = sorted({m.act_dim for m in models})
        if len(widths) != 1 or (act_dim is not None and widths[0] != int(act_dim)):
            raise ValueError(f"the members must share one action width{'' if act_dim is None else f' ({act_dim})'}, got {widths}")
        self.models, self.members, self.reduce = models, len(models), reduce
        self.act_dim = widths[0]
        self.device = models[0].device
        self.params = torch.stack([m.params.to(self.device) for m in models])
        self.lib = models[0].lib
        self.member_costs = None
        self._obs_host = self._obs_dev = None

    def _param_ptrs(self):
        stride = self.params.shape[1] * self.params.element_size()
        return [self.params.data_ptr() + e * stride for e in range(self.members)]

    def rollout_cost(self, obs, actions, cost_mode: int = 0):
        """costs ``[n]`` (f32 device tensor): the members' reduced costs of f32 device action sequences ``[n, h, act_dim]`` from
        observation ``obs [230]``; ``member_costs [E, n]`` is kept."""
        import ctypes as C
        import torch
        from . import _lib as L
        if actions.ndim != 3 or actions.shape[2] != self.act_dim:
            raise ValueError(f"actions must be [n, h, {self.act_dim}], got {tuple(actions.shape)}")
        if actions.shape[0] < 1:
            raise ValueError("actions must have at least one row")
        ob = np.asarray(obs, dtype=np.float32)
        if ob.shape != (230,):
            raise ValueError(f"obs must be [230], got {ob.shape}")
        actions = actions.to(torch.float32).contiguous()
        n, h, _ = actions.shape
        if self._obs_host is None or not np.array_equal(ob, self._obs_host):   # the CEM iterations of a step share it
            self._obs_host, self._obs_dev = ob.copy(), torch.as_tensor(ob, device=self.device)
        member_costs = torch.empty((self.members, n), dtype=torch.float32, device=self.device)
        costs = torch.empty((n,), dtype=torch.float32, device=self.device)
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib.icem_rssm_rollout_cost_ensemble(self.members, (C.c_void_p * self.members)(*self._param_ptrs()), n, h, self.act_dim,
                                                         cost_mode, L.RSSM_REDUCE[self.reduce], C.c_void_p(self._obs_dev.data_ptr()),
                                                         C.c_void_p(actions.data_ptr()), C.c_void_p(member_costs.data_ptr()),
                                                         C.c_void_p(costs.data_ptr()), st))
        self.member_costs = member_costs
        return costs

    def rollout_cost_batch(self, observations, actions, rows, cost_mode: int = 0):
        """``rollout_cost`` of B planners in ONE launch of B x E problems (+ one reduction): planner b scores its ``rows[b]``
        action sequences -- back to back in ``actions [sum rows, h, act_dim]`` -- from ``observations[b]`` through every
        member.  -> costs ``[sum rows]``; ``member_costs [E, sum rows]`` is kept.  One launch holds 32 problems: B x E beyond
        that raises a ``ValueError`` (step fewer planners together)."""
        import ctypes as C
        import torch
        from . import _lib as L
        rows = [int(r) for r in rows]
        if len(rows) * self.members > L.RSSM_BATCH_MAX:
            raise ValueError(f"{len(rows)} planners x {self.members} members = {len(rows) * self.members} problems, but one "
                             f"learned-dynamics launch holds {L.RSSM_BATCH_MAX}: step at most {L.RSSM_BATCH_MAX // self.members} planners together")
        rows, row0, observations = _check_problem_shapes(self.act_dim, len(rows), observations, actions, rows, None)
        o = observations if isinstance(observations, torch.Tensor) else torch.as_tensor(observations, device=self.device)
        actions = actions.to(torch.float32).contiguous()
        B, total = len(rows), sum(rows)
        member_costs = torch.empty((self.members, total), dtype=torch.float32, device=self.device)
        ptrs = self._param_ptrs()
        # member-major: problem e * B + b writes member_costs[e, row0[b] : row0[b] + rows[b]]
        _rssm_models_launch(self.lib, self.device, self.act_dim, [ptrs[e] for e in range(self.members) for _ in range(B)],
                            list(range(B)) * self.members, row0 * self.members, rows * self.members, o, B, actions, cost_mode,
                            out=member_costs.view(-1))
        costs = torch.empty((total,), dtype=torch.float32, device=self.device)
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib.icem_rssm_ensemble_reduce(self.members, total, L.RSSM_REDUCE[self.reduce], C.c_void_p(member_costs.data_ptr()),
                                                   C.c_void_p(costs.data_ptr()), st))
        self.member_costs = member_costs
        return costs

    def predict(self, *, observations, states, actions):
        """Member 0's successor state (the reference-style interface returns one; the planning costs are the ensemble's)."""
        return self.models[0].predict(observations=observations, states=states, actions=actions)


# ---- feed-forward learned dynamics (PETS / MBPO style): icem_amd/csrc/icem_mlp.h, icem_mlp_rollout_cost ---------------------
MLP_ACTIVATIONS = ("relu", "swish")


def declared_mlp(obs_dim: int, act_dim: int, hidden: int = 200, layers: int = 2, activation: str = "relu", seed: int = 0, dtype=None,
                 device="cuda:0", env=None) -> TorchForwardModel:
    """An observation-space MLP that predicts the next observation as a residual -- the model most people who train dynamics
    for MPC have (PETS, MBPO), and the one the reference's ``cost_fn``s presuppose:
    ``x1 = act(W1 [s | a] + b1)``, ``xk = act(Wk x(k-1) + bk)`` for ``k = 2 .. layers``, ``s' = s + Wout x_layers + bout`` with
    ``act`` = ``"relu"`` or ``"swish"`` (``x * sigmoid(x)``, PETS's).  Random weights reproducible from ``seed`` (in
    ``declared_rssm``'s manner).  The module has ``hidden`` (the ``layers`` hidden ``Linear``s), ``out`` and ``activation``;
    it comes back as a ``TorchForwardModel`` with ``cost=None``: the controllers score its graph-replayed torch rollout with
    the env's ``cost_spec``.  ``DeviceMLPModel`` runs the same module (``hidden`` = 200, ``layers`` 1 .. 4, ``obs_dim`` 1 .. 64,
    ``act_dim`` 1 .. 32) with rollout and cost fused into one HIP launch."""
    import torch
    if activation not in MLP_ACTIVATIONS:
        raise ValueError(f"activation must be 'relu' or 'swish', not {activation!r}")
    if layers < 1 or obs_dim < 1 or act_dim < 1 or hidden < 1:
        raise ValueError("obs_dim, act_dim, hidden and layers must be >= 1")

    class MLP(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.obs_dim, self.act_dim, self.activation = obs_dim, act_dim, activation
            self.hidden = torch.nn.ModuleList([torch.nn.Linear(obs_dim + act_dim if k == 0 else hidden, hidden) for k in range(layers)])
            self.out = torch.nn.Linear(hidden, obs_dim)

        def forward(self, obs, act):
            x = torch.cat([obs, act], dim=-1)
            for lin in self.hidden:
                x = lin(x)
                x = torch.relu(x) if self.activation == "relu" else x * torch.sigmoid(x)
            return obs + self.out(x)

    gen = torch.Generator().manual_seed(seed)
    net = MLP()
    with torch.no_grad():
        for p in net.parameters():   # reproducible weights, independent of torch's global RNG state
            bound = 1.0 / math.sqrt(p.shape[-1]) if p.ndim > 1 else 0.05
            p.copy_((torch.rand(p.shape, generator=gen) * 2 - 1) * bound)
    if dtype is not None:
        net = net.to(dtype)
    return TorchForwardModel(net, None, obs_dim, act_dim, dtype=dtype, device=device, env=env)


def fold_input_norm(weight, bias, in_mean, in_std):
    """``(W', b')`` (float64) of an input layer that takes the raw ``[s | a]`` where ``(weight, bias)`` takes the normalised
    ``([s | a] - mean) / std``: ``W' = W / std`` column by column, ``b' = b - W' mean``."""
    import torch
    w, b = weight.detach().double().cpu(), bias.detach().double().cpu()
    mean = torch.zeros(w.shape[1], dtype=torch.float64) if in_mean is None else torch.as_tensor(np.asarray(in_mean, dtype=np.float64))
    std = torch.ones(w.shape[1], dtype=torch.float64) if in_std is None else torch.as_tensor(np.asarray(in_std, dtype=np.float64))
    if mean.shape != (w.shape[1],) or std.shape != (w.shape[1],):
        raise ValueError(f"in_mean / in_std must have the input layer's {w.shape[1]} entries ([s | a])")
    if not bool((std != 0).all()):
        raise ValueError("in_std must not contain zeros")
    w2 = w / std[None, :]
    return w2, b - w2 @ mean


def _mlp_shape(module):
    """(obs_dim, act_dim, layers, activation) of a ``declared_mlp``-shaped module, checked against what the device kernel serves."""
    hidden = list(module.hidden)
    o = module.out.out_features
    d = hidden[0].in_features - o
    act = getattr(module, "activation", "relu")
    ok = (1 <= len(hidden) <= 4 and 1 <= o <= 64 and 1 <= d <= 32 and act in MLP_ACTIVATIONS and module.out.in_features == 200
          and all(lin.out_features == 200 for lin in hidden) and all(lin.in_features == 200 for lin in hidden[1:]))
    if not ok:
        raise ValueError("icem_mlp_rollout_cost is compiled for hidden width 200, 1 to 4 hidden layers, 1 to 64 observation and 1 to 32 "
                         "action dimensions, relu or swish")
    return o, d, len(hidden), act


def pack_mlp(module, in_mean=None, in_std=None):
    """The packed bf16 parameter buffer ``icem_mlp_rollout_cost`` reads (layout: icem_amd/csrc/icem_mlp.h) from a
    ``declared_mlp``-shaped module: every weight padded (outputs to multiples of 16, contractions to multiples of 32) and cut
    into 16 x 32 blocks stored as ``v_mfma_f32_16x16x32_bf16`` A operands ``[out block][k block][lane = 16*g + i][v]`` =
    ``W[16*ob + i][32*kb + 8*g + v]``, each layer followed by its f32 bias.  The input layer's state columns sit at
    ``0 .. obs_dim - 1`` and its action columns at ``32*SK ..`` (``SK = ceil(obs_dim / 32)``), zeros elsewhere.  ``in_mean`` /
    ``in_std`` (``[obs_dim + act_dim]``): an input normalisation ``([s | a] - mean) / std`` in front of the module, folded into
    the input layer (``fold_input_norm``) before it is rounded."""
    import torch
    o, d, L, _ = _mlp_shape(module)
    sk, ob_n = (o + 31) // 32, (o + 15) // 16
    hidden = list(module.hidden)
    w1, b1 = fold_input_norm(hidden[0].weight, hidden[0].bias, in_mean, in_std)

    def pad(w, rows, cols, col_map=None):
        out = torch.zeros(rows, cols)
        w = w.detach().float().cpu()
        for (s0, s1, d0) in (col_map or [(0, w.shape[1], 0)]):
            out[:w.shape[0], d0:d0 + (s1 - s0)] = w[:, s0:s1]
        return out

    def vec(b, n):
        return pad(b.detach().float().cpu()[None], 1, n)[0]

    layers = [(pad(w1, 208, 32 * (sk + 1), [(0, o, 0), (o, o + d, 32 * sk)]), vec(b1, 208))]
    layers += [(pad(lin.weight, 208, 224), vec(lin.bias, 208)) for lin in hidden[1:]]
    layers.append((pad(module.out.weight, 16 * ob_n, 224), vec(module.out.bias, 16 * ob_n)))
    chunks = []
    for w, b in layers:
        ob, kb = w.shape[0] // 16, w.shape[1] // 32
        blocks = w.reshape(ob, 16, kb, 4, 8).permute(0, 2, 3, 1, 4).contiguous()   # [ob, kb, g, i, v]
        chunks.append(blocks.to(torch.bfloat16).view(torch.int16).reshape(-1))
        chunks.append(b.contiguous().view(torch.int16).reshape(-1))                 # f32 bias as two 16-bit words each
    return torch.cat(chunks)


class DeviceMLPModel(ForwardModel):
    """A ``declared_mlp``-shaped residual MLP with its whole h-step rollout AND the environment's parametric cost fused into one
    HIP launch on the bf16 matrix cores (``icem_mlp_rollout_cost``).  ``reference`` is the f32 torch module the weights come
    from -- ``declared_mlp(obs_dim, act_dim, layers=, activation=, seed=)``'s, or a copy of the caller's trained ``module``
    (hidden width 200; with ``in_mean`` / ``in_std`` the copy's input layer has the normalisation folded in, so that
    ``reference`` maps raw ``[s | a]`` like the device buffer does); ``predict`` serves the reference-style NumPy interface
    through it.  The cost is ``cost_spec``, or else ``env.cost_spec`` (an ``envs.CostSpec``).  ``MpcICemHip`` takes the whole MPC step
    through it as one library call (``icem_plan_step_mlp``) where that entry serves the planner -- a model whose
    ``rollout_cost`` was replaced to time or record the rollouts is called stage by stage, as the two baselines always call it
    (``rollout_cost`` + ``params``).  Several models in ONE launch: ``mlp_rollout_cost_models`` (a model per problem) and
    ``DeviceMLPEnsemble`` (the members of an ensemble).  The model itself has no ``rollout_cost_batch``: controllers that want
    to step together (``MpcICemHip.get_action_batch``) share a ``DeviceMLPEnsemble`` -- one member is allowed and gives this
    model's bits -- or bring a model each and say ``own_models=True``."""

    def __init__(self, obs_dim=None, act_dim=None, layers: int = 2, activation: str = "relu", seed: int = 0, device="cuda:0", env=None,
                 module=None, cost_spec=None, in_mean=None, in_std=None):
        super().__init__(env=env)
        import copy
        import torch
        from . import _lib as L
        if cost_spec is None:
            cost_spec = getattr(env, "cost_spec", None)
        if cost_spec is None:
            raise ValueError("DeviceMLPModel scores its rollouts with a parametric cost: give cost_spec= or an env that has one")
        if module is None:
            if obs_dim is None or act_dim is None:
                raise ValueError("give obs_dim and act_dim, or a module")
            if not (1 <= int(obs_dim) <= L.MLP_MAX_OBS_DIM and 1 <= int(act_dim) <= L.MLP_MAX_ACT_DIM and 1 <= int(layers) <= L.MLP_MAX_LAYERS):
                raise ValueError(f"the device MLP takes 1 to {L.MLP_MAX_OBS_DIM} observation and 1 to {L.MLP_MAX_ACT_DIM} action dimensions and "
                                 f"1 to {L.MLP_MAX_LAYERS} hidden layers, not ({obs_dim}, {act_dim}, {layers})")
            net = declared_mlp(int(obs_dim), int(act_dim), hidden=L.MLP_HIDDEN, layers=int(layers), activation=activation, seed=seed,
                               device="cpu").module
        else:
            net = copy.deepcopy(module).float().cpu()
        self.obs_dim, self.act_dim, self.layers, self.activation = _mlp_shape(net)
        if in_mean is not None or in_std is not None:
            w1, b1 = fold_input_norm(net.hidden[0].weight, net.hidden[0].bias, in_mean, in_std)
            with torch.no_grad():
                net.hidden[0].weight.copy_(w1.float())
                net.hidden[0].bias.copy_(b1.float())
        self.cost_spec = cost_spec
        self._cost_c, self._terms_c = L.cost_spec_structs(cost_spec)
        self.device = torch.device(device)
        self.lib = L.load_library()
        L.maybe_follow_environment()   # (tools only: icem_amd._lib.follow_environment)
        self._tm = TorchForwardModel(net, None, self.obs_dim, self.act_dim, device=device, env=env)
        self.reference = self._tm.module
        self.params = pack_mlp(self.reference).to(self.device)
        self._obs_host = self._obs_dev = None
        if self.params.numel() != self.lib.icem_mlp_param_elems(self.obs_dim, self.act_dim, self.layers):
            raise RuntimeError("packed MLP parameters do not match the library's layout")

    def rollout_cost(self, obs, actions, cost_mode: int = 0, return_observations: bool = False):
        """costs ``[n]`` (f32 device tensor) of f32 device action sequences ``[n, h, act_dim]`` from observation ``obs [obs_dim]``
        under the model's cost (``cost_mode``: 0 sum, 1 best, 2 final).  ``return_observations=True``: ``(costs, states)`` with
        states ``[n, h + 1, obs_dim]`` = ``s_0 .. s_h`` -- one more than the h observations a controller's rollout holds: its
        "last predicted observation" (the one in front of the last action) is index ``h - 1``, not ``-1``.  The costs are the
        same bit for bit with and without the states."""
        import ctypes as C
        import torch
        from . import _lib as L
        if actions.ndim != 3 or actions.shape[2] != self.act_dim:
            raise ValueError(f"actions must be [n, h, {self.act_dim}], got {tuple(actions.shape)}")
        actions = actions.to(torch.float32).contiguous()
        n, h, _ = actions.shape
        ob = np.asarray(obs, dtype=np.float32)
        if ob.shape != (self.obs_dim,):
            raise ValueError(f"obs must be [{self.obs_dim}], got {ob.shape}")
        if self._obs_host is None or not np.array_equal(ob, self._obs_host):   # the CEM iterations of a step share it
            self._obs_host, self._obs_dev = ob.copy(), torch.as_tensor(ob, device=self.device)
        costs = torch.empty((n,), dtype=torch.float32, device=self.device)
        states = torch.empty((n, h + 1, self.obs_dim), dtype=torch.float32, device=self.device) if return_observations else None
        if n == 0:   # (empty tensors have no address to hand over; the entry launches nothing for n == 0 either)
            return (costs, states) if return_observations else costs
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib.icem_mlp_rollout_cost(n, h, self.obs_dim, self.act_dim, self.layers, L.MLP_ACTIVATIONS[self.activation], cost_mode,
                                               C.byref(self._cost_c), C.byref(self._terms_c) if self._terms_c is not None else None,
                                               C.c_void_p(self.params.data_ptr()), C.c_void_p(self._obs_dev.data_ptr()),
                                               C.c_void_p(actions.data_ptr()), C.c_void_p(costs.data_ptr()),
                                               C.c_void_p(states.data_ptr()) if states is not None else None, st))
        return (costs, states) if return_observations else costs

    def predict(self, *, observations, states, actions):
        return self._tm.predict(observations=observations, states=states, actions=actions)


def _mlp_cost_bytes(model) -> bytes:
    """The cost program of a ``DeviceMLPModel`` as the library reads it: the bytes of the two ctypes structs."""
    import ctypes as C
    terms = model._terms_c
    return C.string_at(C.addressof(model._cost_c), C.sizeof(model._cost_c)) + (b"" if terms is None else C.string_at(C.addressof(terms), C.sizeof(terms)))


def _check_mlp_models(models):
    """``models`` (``DeviceMLPModel``s) may share a launch: 1 to 32 of one shape, one activation, one device and one cost
    program (compared by the bytes of the ctypes structs).  Needs nothing of a device.  -> the list."""
    from . import _lib as L
    models = list(models)
    if not 1 <= len(models) <= L.MLP_MAX_PROBLEMS:
        raise ValueError(f"one launch takes 1 to {L.MLP_MAX_PROBLEMS} problems, not {len(models)}")
    m0 = models[0]
    shapes = [(m.obs_dim, m.act_dim, m.layers) for m in models]
    if any(sh != shapes[0] for sh in shapes):
        raise ValueError(f"the models must share one shape (obs_dim, act_dim, layers), got {sorted(set(shapes))}")
    if any(m.activation != m0.activation for m in models):
        raise ValueError(f"the models must share one activation, got {sorted({m.activation for m in models})}")
    if any(m.params.device != m0.params.device for m in models):
        raise ValueError("the models' parameter buffers must be on one device")
    cost = _mlp_cost_bytes(m0)
    if any(_mlp_cost_bytes(m) != cost for m in models[1:]):
        raise ValueError("the models must share one cost program (the launch scores every problem with the same cost_spec)")
    return models


def _mlp_models_launch(m0, params_ptrs, obs_rows, arow0, rows, obs_dev, n_obs, actions, cost_mode, out=None, states=None):
    """One ``icem_mlp_rollout_cost_models`` launch with ``m0``'s shape, activation and cost: problem p = (params_ptrs[p],
    obs_rows[p], arow0[p], rows[p]) over the f32 device tensors ``obs_dev [n_obs, obs_dim]`` and ``actions [n_action_rows, h,
    act_dim]`` -> costs ``[sum rows]`` (``out``, or new); ``states``: None, or ``[sum rows, h + 1, obs_dim]`` to fill."""
    import ctypes as C
    import torch
    from . import _lib as L
    n = len(rows)
    costs = torch.empty((sum(rows),), dtype=torch.float32, device=m0.device) if out is None else out
    problems = (L.IcemMlpProblemC * n)(*[L.IcemMlpProblemC(int(params_ptrs[p]), int(arow0[p]), int(rows[p]), int(obs_rows[p]))
                                          for p in range(n)])
    st = C.c_void_p(torch.cuda.current_stream(m0.device).cuda_stream)
    L.check(m0.lib.icem_mlp_rollout_cost_models(n, problems, actions.shape[1], m0.obs_dim, m0.act_dim, m0.layers, L.MLP_ACTIVATIONS[m0.activation],
                                                cost_mode, C.byref(m0._cost_c), C.byref(m0._terms_c) if m0._terms_c is not None else None,
                                                C.c_void_p(obs_dev.data_ptr()), n_obs, C.c_void_p(actions.data_ptr()), actions.shape[0],
                                                C.c_void_p(costs.data_ptr()), C.c_void_p(states.data_ptr()) if states is not None else None, st))
    return costs


def mlp_rollout_cost_models(models, observations, actions, rows, action_row0=None, cost_mode: int = 0, return_observations: bool = False):
    """``DeviceMLPModel.rollout_cost`` of B problems with a MODEL EACH in ONE launch (``icem_mlp_rollout_cost_models``; the
    sibling of ``rssm_rollout_cost_models``: parallel episodes, each with its own trained model): problem p scores ``rows[p]``
    action sequences of ``actions [n, h, act_dim]`` (f32 device tensor) -- from row ``action_row0[p]`` on, or back to back with
    ``action_row0=None``; the rows of different problems may overlap or coincide -- from ``observations[p]`` (``[B, obs_dim]``
    array-like, or an f32 device tensor that is used as is) through ``models[p]`` (``DeviceMLPModel``s of one shape, one
    activation and one cost program on one device, otherwise ``ValueError``; the same model may serve several problems).
    -> costs ``[sum rows]``, problem p's rows back to back in problem order, each bit for bit what ``models[p].rollout_cost``
    gives for it alone; ``return_observations=True``: ``(costs, states [sum rows, h + 1, obs_dim])``, the states laid out and
    equal in the same way.  B <= 32."""
    import torch
    models = _check_mlp_models(models)
    m0 = models[0]
    rows, action_row0, observations = _check_problem_shapes(m0.act_dim, len(models), observations, actions, rows, action_row0, m0.obs_dim)
    o = observations if isinstance(observations, torch.Tensor) else torch.as_tensor(observations, device=m0.device)
    actions = actions.to(torch.float32).contiguous()
    states = (torch.empty((sum(rows), actions.shape[1] + 1, m0.obs_dim), dtype=torch.float32, device=m0.device)
              if return_observations else None)
    costs = _mlp_models_launch(m0, [m.params.data_ptr() for m in models], range(len(models)), action_row0, rows, o, len(models), actions,
                               cost_mode, states=states)
    return (costs, states) if return_observations else costs


class DeviceMLPEnsemble(ForwardModel):
    """E ``DeviceMLPModel``s that score every candidate plan together (PETS plans through about five such networks, trained
    from different seeds): a plan's cost is the members' mean (``reduce="mean"``) or the worst member's (``"max"``), so that
    one model's error is not exploited.  Built from ``models=[DeviceMLPModel, ...]`` or from ``seeds=[...]`` (+
    ``DeviceMLPModel``'s shape keywords: ``obs_dim``, ``act_dim``, ``layers``, ``activation``, ``cost_spec`` / ``env``, ...); 1 to
    32 members of one shape, one activation and one cost program.  ``rollout_cost`` is ONE launch for all members
    (``icem_mlp_rollout_cost_ensemble``) + the reduction; ``member_costs`` holds the last ``[E, n]`` (row e: member e alone, bit
    for bit).  ``params`` are the members' packed buffers stacked ``[E, elems]`` on one device -- the launch reads these.

    The sibling of ``DeviceRSSMEnsemble``, and deliberately neither a subclass of it nor a ``DeviceMLPModel``: the library's
    fused ``*_learned_models`` steps run the RSSM.  ``MpcICemHip`` takes the whole MPC step through it as one library call of
    its own (``icem_plan_step_mlp``: one launch of all members per iteration, their reduction inside the update launch) where
    that entry serves the planner, ``get_action_batch`` likewise for controllers that share one ensemble or, with
    ``own_models=True``, have one each; it leaves ``member_costs`` as the stage-wise loop does (with an ensemble per planner:
    its planner's columns of the step's one table, a view).  An instrumented ensemble and the two baselines plan through it
    stage by stage (``rollout_cost`` / ``rollout_cost_batch`` + ``params``); one member is allowed and gives the plain model's
    bits.  ``predict`` -- the
    reference-style interface needs ONE successor state -- delegates to member 0."""

    def __init__(self, models=None, seeds=None, reduce: str = "mean", **model_kw):
        import torch
        from . import _lib as L
        super().__init__(env=model_kw.get("env"))
        if reduce not in L.RSSM_REDUCE:
            raise ValueError(f"reduce must be 'mean' or 'max', not {reduce!r}")
        if (models is None) == (seeds is None):
            raise ValueError("give either models=[DeviceMLPModel, ...] or seeds=[...]")
        count = len(models) if models is not None else len(seeds)
        if not 1 <= count <= L.MLP_MAX_PROBLEMS:
            raise ValueError(f"an ensemble has 1 to {L.MLP_MAX_PROBLEMS} members (one launch serves them all), not {count}")
        if models is None:
            if "seed" in model_kw or "module" in model_kw:
                raise ValueError("seeds=[...] builds every member from its seed: give neither seed= nor module=")
            models = [DeviceMLPModel(seed=int(s), **model_kw) for s in seeds]
        elif model_kw:
            raise ValueError(f"models=[...] come with their own shape: unexpected {sorted(model_kw)}")
        models = list(models)
        if not all(isinstance(m, DeviceMLPModel) for m in models):
            raise ValueError("the members of a DeviceMLPEnsemble are DeviceMLPModels")
        _check_mlp_models(models)
        m0 = models[0]
        self.models, self.members, self.reduce = models, len(models), reduce
        self.obs_dim, self.act_dim, self.layers, self.activation = m0.obs_dim, m0.act_dim, m0.layers, m0.activation
        self.cost_spec, self._cost_c, self._terms_c = m0.cost_spec, m0._cost_c, m0._terms_c
        self.device = m0.device
        self.params = torch.stack([m.params.to(self.device) for m in models])
        self.lib = m0.lib
        self.member_costs = None
        self._obs_host = self._obs_dev = None

    def _param_ptrs(self):
        stride = self.params.shape[1] * self.params.element_size()
        return [self.params.data_ptr() + e * stride for e in range(self.members)]

    def rollout_cost(self, obs, actions, cost_mode: int = 0):
        """costs ``[n]`` (f32 device tensor): the members' reduced costs of f32 device action sequences ``[n, h, act_dim]`` from
        observation ``obs [obs_dim]``; ``member_costs [E, n]`` is kept."""
        import ctypes as C
        import torch
        from . import _lib as L
        if actions.ndim != 3 or actions.shape[2] != self.act_dim:
            raise ValueError(f"actions must be [n, h, {self.act_dim}], got {tuple(actions.shape)}")
        if actions.shape[0] < 1:
            raise ValueError("actions must have at least one row")
        ob = np.asarray(obs, dtype=np.float32)
        if ob.shape != (self.obs_dim,):
            raise ValueError(f"obs must be [{self.obs_dim}], got {ob.shape}")
        actions = actions.to(torch.float32).contiguous()
        n, h, _ = actions.shape
        if self._obs_host is None or not np.array_equal(ob, self._obs_host):   # the CEM iterations of a step share it
            self._obs_host, self._obs_dev = ob.copy(), torch.as_tensor(ob, device=self.device)
        member_costs = torch.empty((self.members, n), dtype=torch.float32, device=self.device)
        costs = torch.empty((n,), dtype=torch.float32, device=self.device)
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib.icem_mlp_rollout_cost_ensemble(self.members, (C.c_void_p * self.members)(*self._param_ptrs()), n, h, self.obs_dim,
                                                        self.act_dim, self.layers, L.MLP_ACTIVATIONS[self.activation], cost_mode,
                                                        L.RSSM_REDUCE[self.reduce], C.byref(self._cost_c),
                                                        C.byref(self._terms_c) if self._terms_c is not None else None,
                                                        C.c_void_p(self._obs_dev.data_ptr()), C.c_void_p(actions.data_ptr()),
                                                        C.c_void_p(member_costs.data_ptr()), C.c_void_p(costs.data_ptr()), st))
        self.member_costs = member_costs
        return costs

    def rollout_cost_batch(self, observations, actions, rows, cost_mode: int = 0):
        """``rollout_cost`` of B planners in ONE launch of B x E problems (+ one reduction): planner b scores its ``rows[b]``
        action sequences -- back to back in ``actions [sum rows, h, act_dim]`` -- from ``observations[b]`` (``[B, obs_dim]``)
        through every member.  -> costs ``[sum rows]``; ``member_costs [E, sum rows]`` is kept.  One launch holds 32 problems:
        B x E beyond that raises a ``ValueError`` (step fewer planners together)."""
        import ctypes as C
        import torch
        from . import _lib as L
        rows = [int(r) for r in rows]
        if len(rows) * self.members > L.MLP_MAX_PROBLEMS:
            raise ValueError(f"{len(rows)} planners x {self.members} members = {len(rows) * self.members} problems, but one "
                             f"launch holds {L.MLP_MAX_PROBLEMS}: step at most {L.MLP_MAX_PROBLEMS // self.members} planners together")
        rows, row0, observations = _check_problem_shapes(self.act_dim, len(rows), observations, actions, rows, None, self.obs_dim)
        o = observations if isinstance(observations, torch.Tensor) else torch.as_tensor(observations, device=self.device)
        actions = actions.to(torch.float32).contiguous()
        B, total = len(rows), sum(rows)
        member_costs = torch.empty((self.members, total), dtype=torch.float32, device=self.device)
        ptrs = self._param_ptrs()
        # member-major: problem e * B + b writes member_costs[e, row0[b] : row0[b] + rows[b]]
        _mlp_models_launch(self, [ptrs[e] for e in range(self.members) for _ in range(B)], list(range(B)) * self.members,
                           row0 * self.members, rows * self.members, o, B, actions, cost_mode, out=member_costs.view(-1))
        costs = torch.empty((total,), dtype=torch.float32, device=self.device)
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib.icem_rssm_ensemble_reduce(self.members, total, L.RSSM_REDUCE[self.reduce], C.c_void_p(member_costs.data_ptr()),
                                                   C.c_void_p(costs.data_ptr()), st))
        self.member_costs = member_costs
        return costs

    def predict(self, *, observations, states, actions):
        """Member 0's successor state (the reference-style interface returns one; the planning costs are the ensemble's)."""
        return self.models[0].predict(observations=observations, states=states, actions=actions)
