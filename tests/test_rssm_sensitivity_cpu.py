"""The test of the learned-dynamics tests (no GPU): with the CPU emulation standing in for the kernel, the acceptance
criterion of rssm_cases.py passes the reference pair on every case, every deliberately wrong variant of the rollout
fails it on some case by a factor of ten, and the case table keeps the properties that make it discriminating."""
import numpy as np
import pytest

import rssm_cases as RC
from oracle import rssm_oracle as RO

ROWS = 128   # rows per launch for the mutants


def test_emulation_without_rounding_is_the_float64_network():
    case = RC.FULL_CASES[2]
    P = RC.params(case)
    (ob, acts), = RC.launches(case, rows=40)
    for mode in RC.MODES:
        np.testing.assert_allclose(RO.emulated_costs(P, ob.astype(np.float32), acts, mode), RO.rollout_costs(P, ob.astype(np.float32), acts, mode),
                                   rtol=1e-12, atol=1e-12)
    s = RO.emulated_step_costs(P, ob, acts)
    assert s.shape == (40, case.h)
    for mode in RC.MODES:
        assert np.array_equal(RO.reduce_costs(s, mode), RO.emulated_costs(P, ob, acts, mode))


def test_bf16_rounding_is_nearest_even():
    import torch
    x = np.concatenate([np.random.RandomState(0).randn(4096) * 10.0 ** np.random.RandomState(1).randint(-6, 6, 4096),
                        [0.0, -0.0, 1.0, 1.00390625, 1.01171875, -1.00390625, 3.3895313892515355e38]])   # ties both ways
    want = torch.as_tensor(x.astype(np.float32)).to(torch.bfloat16).to(torch.float64).numpy()
    assert np.array_equal(RO.bf16(x), want) and RO.bf16(x).dtype == np.float64
    assert RO.bf16(x.astype(np.float32)).dtype == np.float32


@pytest.mark.parametrize("case", RC.CASES, ids=lambda c: c.name)
def test_reference_pair_agrees(case):
    """(a) the float32, K-blocked emulation with perturbed activations against the float64 one: what the bounds were
    measured on must pass them (with the margins rssm_cases.py states)."""
    want = RC.want(case)
    for seed in (0, 1):
        got = RC.kernel_standin(case, seed=seed)
        assert RC.agree(got, want), (RC.violations(got, want), RC.errors(got, want))


def _tanh_by_sigmoid(x):   # 2 sigma(2x) - 1 in f32, the last step one fused multiply-add: what rssm_dev.h::tanhf_ was
    f = np.float32
    s = (f(1) / (f(1) + np.exp(f(-2) * x.astype(f)))).astype(np.float64)
    return (2 * s - 1).astype(f)


def _tanh_of_the_kernel(x):   # rssm_dev.h::tanhf_: odd series below 1/4, (1 - e) / (1 + e) beyond
    f = np.float32
    a = np.abs(x.astype(f))
    e, x2 = np.exp(f(-2) * a), a * a
    p = f(62 / 2835)
    for c in (-17 / 315, 2 / 15, -1 / 3):
        p = p * x2 + f(c)
    return np.copysign(np.where(a < f(0.25), a + a * (x2 * p), (f(1) - e) * (f(1) / (f(1) + e))), x).astype(f)


def test_a_tanh_that_cancels_around_zero_is_rejected():
    """What the GPU test found in the kernel: tanh spelled 2 sigma(2x) - 1 is good to 1e-7 ABSOLUTE, 1e-6 of a candidate
    state of 0.1, and flips twice as many of the bf16 roundings of h' as f32 accumulation does.  On the MI355X the share
    of rows above ROW_BOUND was 0.372 on the h = 30 case (cap 0.314; 0.27 - 0.28 on the two seed-3 cases, 0.26 on
    1x12) with the median in bounds; this emulation of that spelling gives the same picture, and the spelling the
    kernel has now (3 ulp of tanh's own value) is back at the reference pair's share."""
    case, = [c for c in RC.FULL_CASES if c.name == "s1g1-settled-best-333x30"]
    want = RC.want(case)
    old = RC.errors(RC.kernel_standin(case, tanh=_tanh_by_sigmoid), want)
    new = RC.errors(RC.kernel_standin(case, tanh=_tanh_of_the_kernel), want)
    assert old["share"] > RC.SHARE_CAP and old["median"] <= RC.MEDIAN_BOUND, old
    assert RC.agree(RC.kernel_standin(case, tanh=_tanh_of_the_kernel), want) and new["share"] <= 0.157, new
    x = np.linspace(-6, 6, 400001).astype(np.float32)
    x = x[x != 0]
    rel = np.abs(_tanh_of_the_kernel(x).astype(np.float64) - np.tanh(x.astype(np.float64))) / np.abs(np.tanh(x.astype(np.float64)))
    assert rel.max() <= 4 * 2.0 ** -23, rel.max() / 2.0 ** -23


# ---- (b) the mutants -----------------------------------------------------------------------------------------------------
D = RC.DET


def _edit(fn):
    def params(P):
        P = {k: v.copy() for k, v in P.items()}
        fn(P)
        return P
    return params


def _zero(name, rows=None, cols=None):
    def fn(P):
        if rows is not None:
            P[name][list(rows)] = 0
        if cols is not None:
            P[name][:, list(cols)] = 0
    return _edit(fn)


def _swap_cols(name, a, b):
    def fn(P):
        P[name][:, [a, b]] = P[name][:, [b, a]]
    return _edit(fn)


def _swap_gates(a, b):   # the kernel reading gate block a where b is meant and the other way round
    def fn(P):
        for name in ("gru.weight_ih", "gru.weight_hh", "gru.bias_ih", "gru.bias_hh"):
            blocks = [P[name][i * D:(i + 1) * D].copy() for i in range(3)]
            blocks[a], blocks[b] = blocks[b], blocks[a]
            P[name] = np.concatenate(blocks, 0)
    return _edit(fn)


def _bias_outside(P):   # n = tanh(i_n + r (W_hn h) + b_hn) instead of tanh(i_n + r (W_hn h + b_hn))
    P["gru.bias_ih"][2 * D:] += P["gru.bias_hh"][2 * D:]
    P["gru.bias_hh"][2 * D:] = 0


def _inp_swapped(P):   # x = relu(W1 [a, z]) instead of [z, a]
    w = P["inp.weight"]
    P["inp.weight"] = np.concatenate([w[:, RC.ACT:], w[:, :RC.ACT]], 1)   # the same thing seen from [z, a]


GATE_ROWS = (D - 1, 2 * D - 1, 3 * D - 1)
# name -> dict(params=, state_q=, shift=, reduce=)
MUTANTS = {
    # the last valid unit of every padded block: output rows and contraction columns, layer by layer
    "inp: output unit 199 dropped": dict(params=_zero("inp.weight", rows=[D - 1])),
    "inp: z[29] dropped": dict(params=_zero("inp.weight", cols=[RC.STOCH - 1])),
    "inp: action 5 dropped": dict(params=_zero("inp.weight", cols=[RC.STOCH + RC.ACT - 1])),
    "weight_ih: the three rows of unit 199 dropped": dict(params=_zero("gru.weight_ih", rows=GATE_ROWS)),
    "weight_ih: x[199] dropped": dict(params=_zero("gru.weight_ih", cols=[D - 1])),
    "weight_hh: the three rows of unit 199 dropped": dict(params=_zero("gru.weight_hh", rows=GATE_ROWS)),
    "weight_hh: h[199] dropped": dict(params=_zero("gru.weight_hh", cols=[D - 1])),
    "weight_hh: columns 198 and 199 swapped": dict(params=_swap_cols("gru.weight_hh", D - 2, D - 1)),
    "prior1: output unit 199 dropped": dict(params=_zero("prior1.weight", rows=[D - 1])),
    "prior1: h[199] dropped": dict(params=_zero("prior1.weight", cols=[D - 1])),
    "prior2: z[29] not produced": dict(params=_zero("prior2.weight", rows=[RC.STOCH - 1])),
    "prior2: p[199] dropped": dict(params=_zero("prior2.weight", cols=[D - 1])),
    "rew1: output unit 199 dropped": dict(params=_zero("rew1.weight", rows=[D - 1])),
    "rew1: h[199] dropped": dict(params=_zero("rew1.weight", cols=[D - 1])),
    "rew1: z[29] dropped": dict(params=_zero("rew1.weight", cols=[D + RC.STOCH - 1])),
    "rew2: output unit 199 dropped": dict(params=_zero("rew2.weight", rows=[D - 1])),
    "rew2: r1[199] dropped": dict(params=_zero("rew2.weight", cols=[D - 1])),
    "rew3: r2[199] dropped": dict(params=_zero("rew3.weight", cols=[D - 1])),
    # every bias vector's last element
    "inp.bias[199] dropped": dict(params=_zero("inp.bias", rows=[D - 1])),
    "bias_ih: n gate of unit 199 dropped": dict(params=_zero("gru.bias_ih", rows=[3 * D - 1])),
    "bias_hh: n gate of unit 199 dropped": dict(params=_zero("gru.bias_hh", rows=[3 * D - 1])),
    "bias_hh: u gate of unit 199 dropped": dict(params=_zero("gru.bias_hh", rows=[2 * D - 1])),
    "prior1.bias[199] dropped": dict(params=_zero("prior1.bias", rows=[D - 1])),
    "prior2.bias[29] dropped": dict(params=_zero("prior2.bias", rows=[RC.STOCH - 1])),
    "rew1.bias[199] dropped": dict(params=_zero("rew1.bias", rows=[D - 1])),
    "rew2.bias[199] dropped": dict(params=_zero("rew2.bias", rows=[D - 1])),
    "rew3.bias dropped": dict(params=_zero("rew3.bias", rows=[0])),
    # structure
    "bias_hh of the whole n gate dropped": dict(params=_zero("gru.bias_hh", rows=range(2 * D, 3 * D))),
    "gates read as u, r, n": dict(params=_swap_gates(0, 1)),
    "gates read as r, n, u": dict(params=_swap_gates(1, 2)),
    "n gate's hidden bias outside the product with r": dict(params=_edit(_bias_outside)),
    "z and the action swapped in inp's input": dict(params=_edit(_inp_swapped)),
    "recurrent state kept in bf16": dict(state_q=RO.bf16),
    "reward of the state after the step": dict(shift=1),
    "best over steps 1 .. h-1": dict(reduce=lambda s, mode: RO.reduce_costs(s[:, 1:] if mode == "best" and s.shape[1] > 1 else s, mode)),
    "best over steps 0 .. h-2": dict(reduce=lambda s, mode: RO.reduce_costs(s[:, :-1] if mode == "best" and s.shape[1] > 1 else s, mode)),
    "final taken one step early": dict(reduce=lambda s, mode: RO.reduce_costs(s[:, :-1] if mode == "final" and s.shape[1] > 1 else s, mode)),
}


def mutant_costs(case, params=None, state_q=None, shift=0, reduce=RO.reduce_costs, rows=ROWS):
    """The kernel stand-in of rssm_cases.py with one thing wrong."""
    P = RC.params(case)
    P = params(P) if params else P
    rng = np.random.RandomState(0)

    def run(ob, acts):
        if shift:   # one more state: the last transition is taken as well
            acts = np.concatenate([acts, np.zeros_like(acts[:, :shift])], 1)
        s = RO.emulated_step_costs(P, ob, acts, q=RO.bf16, dtype=np.float32, kblock=32, act_ulp=2.0, rng=rng, state_q=state_q)
        return reduce(s[:, shift:], case.mode)
    return RC.over_launches(case, run, rows).astype(np.float64)


def miss_factors(case, want, **mutant):
    """By what factor the mutant misses the median part and the share part on this case (the share part: the largest
    f with more than SHARE_CAP of the rows above f * ROW_BOUND)."""
    s = RC.errors(mutant_costs(case, **mutant), want)
    return s["median"] / RC.MEDIAN_BOUND, s["quantile"] / RC.ROW_BOUND


_want = {}


def small_want(case):
    if case.name not in _want:
        _want[case.name] = RC.want(case, rows=ROWS)
    return _want[case.name]


@pytest.mark.parametrize("name", MUTANTS, ids=lambda s: s.replace(" ", "_"))
def test_every_mutant_fails_some_case_tenfold(name):
    """(b) both robust parts of the criterion, each by a factor of at least 10, on one and the same case."""
    best = (0.0, None)
    for case in RC.CASES:
        f = min(miss_factors(case, small_want(case), **MUTANTS[name]))
        if f > best[0]:
            best = (f, case.name)
        if f >= 10:
            return
    pytest.fail(f"{name}: best case {best[1]} misses by {best[0]:.3g} only")


# ---- (c) the case table ----------------------------------------------------------------------------------------------------

def argmin_histogram(case):
    P = RC.params(case)
    s = RC.over_launches(case, lambda ob, a: RO.emulated_step_costs(P, ob, a))   # the float64 network
    return np.bincount(s.argmin(1), minlength=case.h) / len(s)


@pytest.mark.parametrize("case", RC.BEST_CASES, ids=lambda c: c.name)
def test_best_cases_spread_their_minimum_over_the_steps(case):
    """No step holds more than half of the rows' minima and at least four steps hold 5 % each (at h = 12; the h = 30 case
    has 30 steps to spread them over and is asked for the same per step: 5 % * 12 / 30)."""
    hist = argmin_histogram(case)
    assert hist.max() <= 0.5 and (hist >= 0.05 * 12 / case.h).sum() >= 4, hist


def test_lopsided_best_cases_favour_the_first_and_the_last_step():
    """... and the two h = 2 cases put 60-85 % of the minima on one step, one on the first and one on the last: the
    median row then sees a reduction that leaves that step out."""
    favoured = set()
    for case in RC.LOPSIDED_BEST_CASES:
        hist = argmin_histogram(case)
        assert 0.6 <= hist.max() <= 0.85, hist
        favoured.add(int(hist.argmax()))
    assert favoured == {0, 1}


def test_every_relu_unit_is_active_somewhere_in_the_table():
    active = {}
    for case in RC.FULL_CASES:
        P = RC.params(case)
        RC.over_launches(case, lambda ob, a: RO.emulated_step_costs(P, ob, a, q=RO.bf16, active=active), rows=ROWS)
    assert set(active) == {"inp", "prior1", "rew1", "rew2"}
    for layer, on in active.items():
        assert on.shape == (200,) and on.all(), (layer, np.flatnonzero(~on))


@pytest.mark.parametrize("case", RC.FULL_CASES, ids=lambda c: c.name)
def test_costs_are_spread(case):
    """max - min of the costs at least a tenth of their magnitude: a criterion normalised by max|cost| then resolves the
    differences between rows, not a common offset."""
    c = RC.want(case)
    assert len(c) > 1 and c.max() - c.min() >= 0.1 * np.abs(c).max()
