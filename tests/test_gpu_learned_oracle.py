"""The stage-wise loop of the learned-dynamics MPC step (MpcICemHip on DeviceRSSMModel) against the float64 oracle, per
iteration, with the costs teacher-forced (learned_loop.py): the anchor of everything test_gpu_learned_step.py and
test_gpu_rssm_batch.py hold bit for bit to that loop.  Every case records 5 MPC steps of a controller under
learned_step = 0, steps a twin on the fused entry alongside (bit-equal executed action, mean, std, elites, last_min_cost
after every step: the run held to the oracle is the run the fused entry reproduces), then checks the record: pools, row
counts, elite index sets, elite rows and costs, refits, epilogue, and the device costs on the planner's own pools under
rssm_cases' criterion (pooled over the case's 15 rollout calls; not for sum at h = 30, where the CPU reference pair itself
breaks the share cap).  test_learned_loop_sensitivity_cpu.py shows what the checker rejects.

First run on an MI355X ([record] lines; before best_settled existed and with h30_best on the observation of "best"): every
case passed, each under 1 s.  Elite index sets identical in every iteration
of every step.  Worst absolute deviations: pool 5.9e-7, mean 2.9e-7, std 1.4e-7, step end 2.9e-7 (asymmetric bounds, range up
to 5: 8.6e-7 / 5.3e-7 / 2.3e-7 / 5.2e-7).  Pooled costs (1542 .. 1619 rows; n24_floor 332): median 3.9e-8 .. 5.6e-8 (bound
1.9e-7), share of rows above ROW_BOUND 0.056 .. 0.086 (cap 0.314), maximum 5.6e-4 .. 5.2e-3 (bound 3.4e-2); sum at h = 30,
reported only: median 7.6e-8, share 0.133, maximum 5.4e-4.  "best" from 0.3 N(0, 1): median 1.4e-7, share 0.006 -- every
minimum sits on step 0 or 1 and step 0 is one cost for all rows (exact ties, broken by index as the oracle breaks them), so
the median is the accumulation-order error of that one cost; best_settled and h30_best plan from a settled state, where the
minima spread over the steps -- those two were added behind that run and are NOT yet run on a GPU (on the CPU reference
pair: median <= 3.0e-8, share 0.034 / 0.169).  Clipped entries per dimension under the asymmetric bounds: 299 .. 1952
at low, 313 .. 1398 at high.
"""
import numpy as np
import pytest

import learned_loop as LL
import test_gpu_learned_step as S
from oracle import rssm_oracle as RO
from oracle_loop import DeviceNormals, record

pytestmark = pytest.mark.gpu

_P = {}


def model_params():
    if "P" not in _P:
        _P["P"] = RO.params_from_state_dict(S.model().reference.state_dict())
    return _P["P"]


def test_the_case_table_covers_every_variant():
    """A variant added to test_gpu_learned_step.VARIANTS cannot go unanchored: the table restates each of them."""
    assert LL.ASP == S.ASP
    assert {k: LL.CASES.get(k) for k in S.VARIANTS} == S.VARIANTS
    assert [n for n in CONTROLLER_CASES if n in S.VARIANTS] == list(S.VARIANTS)


def controller_kwargs(name):
    return {k: v for k, v in LL.CASES[name].items() if k in ("horizon", "n", "cost", "asp")}


def device_noise(name, planner):
    cs = LL.case_settings(name)
    return DeviceNormals(LL.EpisodeNormals(planner), cs["asp"]["opt_iterations"], shift=cs["asp"]["shift_elites_over_time"],
                         white=cs["asp"]["noise_beta"] <= 0)


def check_and_report(name, rec, noise, tag=None):
    cs = LL.case_settings(name)
    out = LL.check(rec, noise, P=model_params(), cost_criterion=cs["criterion"])
    c = out["cost"]
    record(dict(case=tag or name, rows=c["rows"], cost_median=c["median"], cost_share=c["share"], cost_max=c["max"],
                criterion=cs["criterion"], pool=out["pool"], mean=out["mean"], std=out["std"], step_end=out["end"]))
    return out


def run_controllers(name, seeds, batch):
    """Recorded stage-wise controllers, their twins on the fused entry (``batch``: through get_action_batch) and a third
    set that only draws the normals; -> the records, checked."""
    from icem_amd import MpcICemHip
    kw = controller_kwargs(name)
    staged, fused, drawers = ([S.controller(sd, **kw) for sd in seeds] for _ in range(3))
    obs0 = LL.first_observations(name, model_params(), len(seeds))
    for group in (staged, fused, drawers):
        for c, ob in zip(group, obs0):
            S.begin(c, ob)
    recorders = [LL.ControllerRecorder(c) for c in staged]
    for k in range(LL.N_STEPS):
        obs = [ob + 0.01 * k for ob in obs0]
        want = [r.step(ob) for r, ob in zip(recorders, obs)]
        got = MpcICemHip.get_action_batch(fused, obs) if batch else [fused[0].get_action(obs[0], None)]
        assert fused[0].planner.learned_step_launches > 0, "the twin took the fused entry"
        for i in range(len(seeds)):
            assert np.array_equal(got[i], want[i]), (name, k, i)
            S.assert_same_state(fused[i], staged[i], (name, k, i))
    for i, r in enumerate(recorders):
        assert len(r.record["steps"]) == LL.N_STEPS
        check_and_report(name, r.record, device_noise(name, drawers[i].planner), tag=name if len(seeds) == 1 else f"{name}[{i}]")
    return [r.record for r in recorders]


CONTROLLER_CASES = [n for n in LL.CASES if "low" not in LL.CASES[n]]


@pytest.mark.parametrize("name", CONTROLLER_CASES)
def test_stagewise_loop_against_the_oracle(name):
    rec, = run_controllers(name, [5], batch=False)
    rows = [len(it["costs"]) for it in rec["steps"][1]["iters"]]
    p = rec["params"]
    n_reuse = int(p.num_elites * p.fraction_elites_reused) if p.shift_elites_over_time else 0
    want = {"n24_floor": [24, 20, 20], "n126_full_last_workgroup": [126, 100, 80]}.get(name, [128, 102, 81])
    assert rows == [want[0] + n_reuse] + want[1:], rows


def test_batch_of_three_against_the_oracle():
    """B = 3 controllers of different seeds and observations through get_action_batch against their three recorded twins."""
    run_controllers("h12", [1, 2, 3], batch=True)


def test_asymmetric_bounds_through_the_planner():
    """Per-dimension low / high (learned_loop.LOW / HIGH: every learned-path test else plans in [-1, 1]^6) through
    IcemPlanner alone: plan_step_learned against the recorded operator loop bit for bit, the record against the oracle.
    Every dimension has entries clipped at both ends in the recorded pools."""
    import torch
    from icem_amd import IcemConfig, IcemPlanner
    cs = LL.case_settings("bounds")

    def planner():
        cfg = IcemConfig(horizon=12, act_dim=6, num_traj=128, elites_size=10, opt_iters=3, factor_decrease=1.25, seed=11)
        pl = IcemPlanner(cfg, cs["low"], cs["high"])
        pl._ensure_buffers(learned=True)
        pl.reset_distribution(pl.mean, pl.std)
        return pl
    m = S.model()
    p, q, drawer = planner(), planner(), planner()
    rec = LL.new_record(LL.oracle_params(horizon=12, n=128, **cs["asp"]), cs["low"], cs["high"])
    elites = None
    for k, ob in enumerate(LL.step_observations(LL.first_observations("bounds", model_params(), seed=4)[0])):
        p.plan_step_learned(m, ob)
        want, elites, before = LL.record_operator_step(rec, q, m, ob, elites)
        assert p.mpc_step == q.mpc_step == k + 1 and p.learned_step_launches > 0
        assert np.array_equal(LL.host(torch.cat([p.executed, p.best_cost])), want), k
        assert np.array_equal(LL.host(p.mean), LL.host(q.mean)) and np.array_equal(LL.host(p.std), LL.host(q.std)), k
        g = (p.mpc_step * p.cfg.opt_iters) & 1
        for half, (ea, ec) in ((g, elites), (g ^ 1, before)):
            assert np.array_equal(LL.host(p.elites_actions[half]), LL.host(ea)) and np.array_equal(LL.host(p.elites_costs[half]), LL.host(ec)), k
    pools = np.concatenate([it["pool"].reshape(-1, 6) for st in rec["steps"] for it in st["iters"]])
    at_low, at_high = (pools == cs["low"].astype(np.float32)).sum(0), (pools == cs["high"].astype(np.float32)).sum(0)
    print("entries clipped at low / high per dimension:", at_low.tolist(), at_high.tolist())
    assert np.all(at_low > 0) and np.all(at_high > 0)
    check_and_report("bounds", rec, device_noise("bounds", drawer))
