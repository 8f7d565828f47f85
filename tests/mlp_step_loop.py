"""The reference of test_gpu_mlp_step.py: one iCEM MPC step through feed-forward models driven operator by operator through the
public stage-wise entries -- the sampling operator (``IcemPlanner.sample_clip``), the models' own ``rollout_cost``
(``icem_mlp_rollout_cost`` for a ``DeviceMLPModel``, ``icem_mlp_rollout_cost_ensemble`` for a ``DeviceMLPEnsemble``),
``icem_update_distribution`` with the kept elites, the shifted elites' copy + draw, and ``icem_shift``.  It is the loop of
``MpcICemHip._get_action_stagewise`` restated on a bare planner (as tests/test_gpu_learned_step.py::operator_step restates it
for the RSSM), so that nothing ``icem_plan_step_mlp`` calls internally is called here except those operators.  The planners of
a batch are independent problems: their reference is this loop per planner; :func:`member_table` lays their members' costs out
as one launch of all of them would."""
import numpy as np
import torch

DEV = "cuda:0"
ITERS, K = 3, 10

# the two shapes of the issue: the existing controller tests' (whole first tile count: rows 128 (+3), 102, 81), and one on the
# SK = 2 instantiation (obs_dim > 32) whose every row count is off a multiple of 16: 100 (+3), 76, 58 (factor_decrease 1.3)
SHAPES = {
    "o17": dict(o=17, d=6, h=12, layers=2, activation="swish", n=128, factor_decrease=1.25),
    "o40": dict(o=40, d=3, h=10, layers=1, activation="relu", n=100, factor_decrease=1.3),
}
_models = {}


def np_(t):
    return t.detach().cpu().numpy()


def cost_spec(shape):
    """HalfCheetah's cost at o = 17; at o = 40 the same form plus a term that reads the observation's last entries (33 .. 39:
    beyond the first 32-wide block of the state)."""
    from icem_amd import halfcheetah_env
    from icem_amd.envs import TERM_SUMSQ, CostSpec, CostTerm
    if SHAPES[shape]["o"] == 17:
        return halfcheetah_env(17).cost_spec
    return CostSpec(ctrl_weight=0.1, lin_idx=8, lin_weight=-1.0, flip_idx=1, terms=(CostTerm(TERM_SUMSQ, a=33, len=7, weight=0.05),))


def model(shape, seed):
    """Cached ``DeviceMLPModel(seed=...)`` of a shape (never instrumented: twins may share it)."""
    from icem_amd import DeviceMLPModel
    if (shape, seed) not in _models:
        s = SHAPES[shape]
        _models[(shape, seed)] = DeviceMLPModel(s["o"], s["d"], layers=s["layers"], activation=s["activation"], seed=seed,
                                                cost_spec=cost_spec(shape), device=DEV)
    return _models[(shape, seed)]


def ensemble(shape, seeds, reduce="mean"):
    """A fresh ``DeviceMLPEnsemble`` on the cached members (``member_costs`` is the object's own)."""
    from icem_amd import DeviceMLPEnsemble
    return DeviceMLPEnsemble(models=[model(shape, s) for s in seeds], reduce=reduce)


def planner(shape, seed, **kw):
    """A bare planner of the issue's configuration: 3 iterations, kept and shifted elites, 0.3 of them reused, the mean as row 0
    of the last iteration, colored noise (beta 0.25), K = 10."""
    from icem_amd import IcemConfig, IcemPlanner
    s = SHAPES[shape]
    cfg = IcemConfig(horizon=kw.pop("horizon", s["h"]), act_dim=s["d"], num_traj=kw.pop("n", s["n"]), elites_size=K, opt_iters=ITERS,
                     factor_decrease=s["factor_decrease"], use_mean_actions=True, keep_previous_elites=True, shift_elites=True,
                     fraction_reused=0.3, noise_beta=0.25, seed=seed, **kw)
    p = IcemPlanner(cfg, -np.ones(s["d"]), np.ones(s["d"]))
    p._ensure_buffers(learned=True)
    p.reset_distribution(p.mean, p.std)
    return p


def restart(p):
    """A new episode of a bare planner, as ``MpcICemHip.beginning_of_rollout`` starts one."""
    p.new_episode()
    p.reset_distribution(p.mean, p.std)
    p.mpc_step = 0


def observations(shape, n, seed=9):
    rs = np.random.RandomState(seed)
    return [0.3 * rs.randn(SHAPES[shape]["o"]) for _ in range(n)]


def operator_step(p, m, ob, elites):
    """One MPC step of planner ``p`` through ``m`` (a ``DeviceMLPModel`` or a ``DeviceMLPEnsemble``) from observation ``ob``;
    ``elites`` = (actions, costs) of the step before, or None behind a (re)start.  -> dict: ``result`` (executed | best cost),
    ``elites`` / ``before`` (the last iteration's set and the one before it), the last pool's ``actions`` / ``costs`` and, with
    an ensemble, its ``member_costs`` [E, rows]."""
    from icem_amd._lib import COST_MODES
    cfg, it_n = p.cfg, p.cfg.opt_iters
    base = p.noise_offset(p.mpc_step * (it_n + 1))
    before = None
    for i, n_i in enumerate(p.population_sizes):
        shift = i == 0 and cfg.shift_elites and elites is not None and p.n_reuse > 0
        acts = torch.empty((n_i + (p.n_reuse if shift else 0), p.h, p.d), dtype=p.dt, device=p.device)
        p.sample_clip(n_i, p.mean, p.std, offset=base + i, row0_mean=bool(cfg.use_mean_actions and i == it_n - 1), out=acts[:n_i])
        if shift:
            acts[n_i:, :-1] = elites[0][:p.n_reuse, 1:]
            p.sample_clip(p.n_reuse, p.mean, p.std, offset=base + it_n, t_begin=p.h - 1, out=acts[n_i:])
        costs = m.rollout_cost(ob, acts, COST_MODES[cfg.cost_mode])
        keep = i > 0 and cfg.keep_previous_elites and p.n_reuse > 0
        before = elites
        ec, _, ea = p.update_distribution(costs, acts, p.K, p.mean, p.std, elites[1][:p.n_reuse] if keep else None,
                                          elites[0][:p.n_reuse] if keep else None)
        elites = (ea, ec)
    p.shift(p.mean, p.std)
    p.mpc_step += 1
    mc = getattr(m, "member_costs", None)
    return dict(result=np_(torch.cat([elites[0][0, 0], elites[1][:1]])), elites=elites, before=before, actions=np_(acts).copy(),
                costs=np_(costs).copy(), member_costs=None if mc is None else np_(mc).copy())


def member_table(steps):
    """The members' costs of the last iteration of several planners' reference steps as ONE launch of all of them leaves them:
    [members, the planners' rows back to back].  A plain model's step has one member: its costs."""
    return np.concatenate([s["costs"][None] if s["member_costs"] is None else s["member_costs"] for s in steps], axis=1)


def launches(p, step):
    """The design's count: sample, rollout and update per iteration, + the shifted elites' launch in a step that has them."""
    return 3 * p.cfg.opt_iters + (1 if step > 0 and p.cfg.shift_elites and p.n_reuse > 0 else 0)
