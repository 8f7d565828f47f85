"""NumPy restatement of the declared recurrent state-space model (icem_amd/models.py::declared_rssm) -- TEST
INFRASTRUCTURE ONLY, like everything under oracle/: the checker of tests/ and the timed CPU baseline of
``bench.py --workload c5``.  The reference ships no learned-dynamics model (README.md:21-29 quotes PlaNet results
only), so this restates the build's own declared architecture: ``x = relu(W1 [z, a])``, ``h' = GRUCell(x, h)`` (torch
gate order r, u, n), ``z' = W5 relu(W4 h')``, reward head ``W8 relu(W7 relu(W6 [h, z]))``; cost of a step = minus the
reward of the state it starts from."""
import numpy as np


def params_from_state_dict(sd) -> dict:
    return {k: np.asarray(v.detach().cpu().double().numpy() if hasattr(v, "detach") else v, dtype=np.float64) for k, v in sd.items()}


def step(P: dict, obs: np.ndarray, act: np.ndarray, det: int = 200) -> np.ndarray:
    h, z = obs[:, :det], obs[:, det:]
    x = np.maximum(np.concatenate([z, act], -1) @ P["inp.weight"].T + P["inp.bias"], 0)
    gi = x @ P["gru.weight_ih"].T + P["gru.bias_ih"]
    gh = h @ P["gru.weight_hh"].T + P["gru.bias_hh"]
    r = 1.0 / (1.0 + np.exp(-(gi[:, :det] + gh[:, :det])))
    u = 1.0 / (1.0 + np.exp(-(gi[:, det:2 * det] + gh[:, det:2 * det])))
    n = np.tanh(gi[:, 2 * det:] + r * gh[:, 2 * det:])
    h2 = (1 - u) * n + u * h
    z2 = np.maximum(h2 @ P["prior1.weight"].T + P["prior1.bias"], 0) @ P["prior2.weight"].T + P["prior2.bias"]
    return np.concatenate([h2, z2], -1)


def reward(P: dict, obs: np.ndarray) -> np.ndarray:
    a = np.maximum(obs @ P["rew1.weight"].T + P["rew1.bias"], 0)
    a = np.maximum(a @ P["rew2.weight"].T + P["rew2.bias"], 0)
    return (a @ P["rew3.weight"].T + P["rew3.bias"])[:, 0]


def rollout_costs(P: dict, obs0: np.ndarray, actions: np.ndarray, mode: str = "sum") -> np.ndarray:
    ob = np.broadcast_to(np.asarray(obs0, dtype=np.float64), (actions.shape[0], len(obs0))).copy()
    steps = []
    for t in range(actions.shape[1]):
        steps.append(-reward(P, ob))
        ob = step(P, ob, actions[:, t])
    s = np.stack(steps, 1)
    return {"sum": s.sum(1), "best": s.min(1), "final": s[:, -1]}[mode]


# ---------------------------------------------------------------------------------------------------------------------
# The same rollout with the roundings of icem_rssm_rollout_cost (icem_amd/csrc/icem_rssm.hip, icem_rssm_split.hip) put
# where the kernel puts them: weights and every matrix operand in bf16, accumulation, biases, activations and the
# recurrent state h in the working type (the kernel: f32), z carried as a bf16 operand only.
# ---------------------------------------------------------------------------------------------------------------------

def bf16(x) -> np.ndarray:
    """Round to bfloat16 (nearest, ties to even -- rssm_dev.h::to_bf16), returned in the type it came in."""
    x = np.asarray(x)
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32).astype(x.dtype if x.dtype.kind == "f" else np.float64)


def reduce_costs(s: np.ndarray, mode: str) -> np.ndarray:
    """[n, h] per-step costs -> [n]; ``sum`` adds the steps in order in the array's own type, as the kernel does."""
    if mode == "sum":
        acc = s[:, 0].copy()
        for t in range(1, s.shape[1]):
            acc = acc + s[:, t]
        return acc
    return {"best": s.min(1), "final": s[:, -1]}[mode]


def emulated_step_costs(P: dict, obs0, actions, q=None, dtype=np.float64, act_ulp: float = 0.0, rng=None, kblock: int = 0,
                        state_q=None, active: dict = None, tanh=np.tanh) -> np.ndarray:
    """Per-step costs ``[n, h]`` of ``actions [n, h, 6]`` from ``obs0 [230]`` (one observation, or ``[n, 230]``: one per row).

    ``q``        rounding applied to the weights and to every matrix operand (``bf16``: the kernel's rounding points;
                 ``None``: none -- in float64 that is ``rollout_costs``);
    ``dtype``    the type of accumulators, biases, activations and the recurrent state;
    ``kblock``   > 0: contractions accumulate block by block of that many inputs, bias first (the matrix instruction's
                 K = 32), instead of in one product;
    ``act_ulp``  > 0: every sigmoid and tanh output is multiplied by ``1 + e``, ``e`` uniform in ``+-act_ulp * 2^-23``
                 (``rng``: a ``RandomState``) -- the hardware exp / rcp the kernel builds them from;
    ``state_q``  rounding applied to the recurrent state when it is stored (the kernel: none, it stays f32);
    ``active``   a dict that receives, per ReLU layer, which units were positive on some row at some step;
    ``tanh``     the n gate's tanh (to try a kernel's own spelling of it in the working type)."""
    q = q or (lambda x: x)
    ft = np.dtype(dtype).type
    W = {k: (q(np.asarray(v, np.float64)) if v.ndim > 1 else np.asarray(v, np.float64)).astype(ft) for k, v in P.items()}
    actions = np.asarray(actions)
    n, h, _ = actions.shape
    det = W["gru.weight_hh"].shape[1]
    ob = np.asarray(obs0, dtype=np.float32).astype(ft)   # the kernel reads the observation as f32
    ob = np.broadcast_to(ob, (n, ob.shape[-1]))
    hh, z = ob[:, :det].copy(), ob[:, det:].copy()
    one, eps = ft(1), ft(act_ulp * 2.0 ** -23)

    def dense(x, name):
        w, b = (W[name + ".weight"], W[name + ".bias"]) if name + ".weight" in W else (W[name], W[name.replace("weight", "bias")])
        if kblock <= 0:
            return x @ w.T + b
        acc = np.broadcast_to(b, (x.shape[0], w.shape[0])).astype(ft)
        for k0 in range(0, w.shape[1], kblock):
            acc = acc + x[:, k0:k0 + kblock] @ w[:, k0:k0 + kblock].T
        return acc

    def fast(y):   # an activation's output as the hardware's exp and rcp leave it
        return y * (one + eps * rng.uniform(-1, 1, y.shape).astype(ft)) if act_ulp > 0 else y

    def relu(y, layer):
        if active is not None:
            active[layer] = active.get(layer, False) | (y > 0).any(0)
        return np.maximum(y, 0)

    sig = lambda x: fast(one / (one + np.exp(-x)))  # noqa: E731
    steps = []
    for t in range(h):
        hq, zq = q(hh), q(z)
        a1 = q(relu(dense(np.concatenate([hq, zq], -1), "rew1"), "rew1"))
        a2 = q(relu(dense(a1, "rew2"), "rew2"))
        steps.append(-dense(a2, "rew3")[:, 0])
        if t + 1 == h:
            break   # the transition behind the last scored state is never taken
        x = q(relu(dense(np.concatenate([zq, q(actions[:, t].astype(ft))], -1), "inp"), "inp"))
        gi, gh = dense(x, "gru.weight_ih"), dense(hq, "gru.weight_hh")
        r = sig(gi[:, :det] + gh[:, :det])
        u = sig(gi[:, det:2 * det] + gh[:, det:2 * det])
        nn = fast(tanh(gi[:, 2 * det:] + r * gh[:, 2 * det:]))
        hh = (one - u) * nn + u * hh
        if state_q is not None:
            hh = state_q(hh)
        z = dense(q(relu(dense(q(hh), "prior1"), "prior1")), "prior2")
    return np.stack(steps, 1)


def emulated_costs(P: dict, obs0, actions, mode: str = "sum", **kw) -> np.ndarray:
    return reduce_costs(emulated_step_costs(P, obs0, actions, **kw), mode)
