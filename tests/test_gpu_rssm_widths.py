"""icem_rssm_rollout_cost_w / icem_rssm_rollout_cost_batch_w: the learned-dynamics rollout at every action width from 1 to 32.

Against the float64 emulation of the kernel's rounding points (oracle/rssm_oracle.py, which takes any width) on the table of
rssm_width_cases.py under rssm_cases.py's criterion, bounds unchanged (test_rssm_width_sensitivity_cpu.py: the reference pair
passes them at these widths, every single staging fault misses them tenfold).  The widths are the edges of the staging: four
entries per lane, sixteen per wave, thirty-two in the K block.  Width 6 through the new entries is the old entries bit for
bit.  An action tensor that ends where its last row ends -- the front of an allocation whose remainder is NaN -- gives finite
costs, the same bits as a tensor of its own: no entry past a row's d is read and none of the neighbour's enters.  A batch's
problems are bit for bit their own launches."""
import ctypes as C

import numpy as np
import pytest
import torch

import rssm_cases as RC
import rssm_width_cases as WC

pytestmark = pytest.mark.gpu

_models, _want = {}, {}


def np_(t):
    return t.detach().cpu().numpy()


def device_model(case):
    from icem_amd import DeviceRSSMModel
    key = (case.d, case.wseed, case.gain)
    if key not in _models:
        _models[key] = DeviceRSSMModel(module=WC.module(case))
        assert _models[key].act_dim == case.d
    return _models[key]


def seeded_model(d, seed=3):
    from icem_amd import DeviceRSSMModel
    key = ("seed", d, seed)
    if key not in _models:
        _models[key] = DeviceRSSMModel(seed=seed, act_dim=d)
    return _models[key]


def wanted(case):
    if case.name not in _want:
        _want[case.name] = WC.want(case)
    return _want[case.name]


@pytest.mark.parametrize("case", WC.CASES, ids=lambda c: c.name)
def test_every_width_against_the_emulation(case):
    from icem_amd import _lib as L
    m = device_model(case)
    L.set_option("rssm_split", 1 if case.kernel == "split" else 0)   # (back to the default behind every test: conftest.py)

    def run(ob, acts):
        return np_(m.rollout_cost(ob, torch.as_tensor(acts, dtype=torch.float32, device="cuda"), RC.MODES[case.mode])).astype(np.float64)
    got = WC.over_launches(case, run)
    want = wanted(case)
    print(case.name, WC.errors(got, want))
    assert got.shape == want.shape
    assert WC.agree(got, want), (WC.violations(got, want), WC.errors(got, want))


def _raw(lib, m, n, h, d, mode, obs, acts, width_entry):
    costs = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = (C.c_void_p(m.params.data_ptr()), C.c_void_p(obs.data_ptr()), C.c_void_p(acts.data_ptr()), C.c_void_p(costs.data_ptr()), st)
    rc = lib.icem_rssm_rollout_cost_w(n, h, d, mode, *args) if width_entry else lib.icem_rssm_rollout_cost(n, h, mode, *args)
    assert rc == 0, lib.icem_last_error()
    return np_(costs)


@pytest.mark.parametrize("n", [17, 250, 4097])
def test_width_six_through_the_new_entries_is_the_old_entries_bit_for_bit(n):
    from icem_amd import _lib as L
    m = seeded_model(6)
    rs = np.random.RandomState(n)
    obs = torch.as_tensor(0.3 * rs.randn(2, 230), dtype=torch.float32, device="cuda")
    acts = torch.as_tensor(rs.uniform(-1, 1, (n, 12, 6)), dtype=torch.float32, device="cuda")
    for mode in (0, 1):
        old, new = _raw(m.lib, m, n, 12, 6, mode, obs, acts, False), _raw(m.lib, m, n, 12, 6, mode, obs, acts, True)
        assert np.isfinite(old).all() and np.array_equal(old, new), mode
    # ... and the batch entry: two problems that split the rows
    rows = [n // 3 + 1, n - n // 3 - 1]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = []
    for width_entry in (False, True):
        costs = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
        tail = (C.c_void_p(m.params.data_ptr()), C.c_void_p(obs.data_ptr()), C.c_void_p(acts.data_ptr()), C.c_void_p(costs.data_ptr()), st)
        r = (C.c_int32 * 2)(*rows)
        rc = m.lib.icem_rssm_rollout_cost_batch_w(2, r, 12, 6, 0, *tail) if width_entry else m.lib.icem_rssm_rollout_cost_batch(2, r, 12, 0, *tail)
        assert rc == 0, m.lib.icem_last_error()
        out.append(np_(costs))
    assert np.isfinite(out[0]).all() and np.array_equal(out[0], out[1])
    assert np.array_equal(out[0][:rows[0]], _raw(m.lib, m, rows[0], 12, 6, 0, obs, acts, False))
    # widths the action K block does not hold are refused, nothing launched
    for d in (0, 33, 64):
        costs = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
        tail = (C.c_void_p(m.params.data_ptr()), C.c_void_p(obs.data_ptr()), C.c_void_p(acts.data_ptr()), C.c_void_p(costs.data_ptr()), st)
        assert m.lib.icem_rssm_rollout_cost_w(n, 12, d, 0, *tail) == L.ICEM_E_UNSUPPORTED
        assert m.lib.icem_rssm_rollout_cost_batch_w(2, (C.c_int32 * 2)(*rows), 12, d, 0, *tail) == L.ICEM_E_UNSUPPORTED
        assert (np_(costs) == 7.0).all()


@pytest.mark.parametrize("kernel", ["split", "fused"])
@pytest.mark.parametrize("d", [1, 5, 7, 17, 31])
def test_nothing_behind_a_rows_own_entries_is_read(d, kernel):
    """The action tensor as a view at the front of a larger allocation whose remainder is NaN (an entry read past a row's d, or
    past the last row, would be one of them -- and in a tensor of its own the neighbouring row's or step's entry): finite
    costs, and the same bits as the same call on a tensor of its own."""
    from icem_amd import _lib as L
    L.set_option("rssm_split", 1 if kernel == "split" else 0)
    m = seeded_model(d)
    for n in (17, 33):
        for h in (1, 2, 12):
            rs = np.random.RandomState(100 * n + h)
            ob = 0.3 * rs.randn(230)
            a = rs.uniform(-1, 1, (n, h, d)).astype(np.float32)
            arena = torch.full((n * h * d + 4096,), float("nan"), dtype=torch.float32, device="cuda")
            view = arena[:n * h * d].view(n, h, d)
            view.copy_(torch.as_tensor(a))
            own = torch.as_tensor(a, device="cuda").clone()
            for mode in (0, 1):
                got, want = np_(m.rollout_cost(ob, view, mode)), np_(m.rollout_cost(ob, own, mode))
                assert np.isfinite(got).all(), (n, h, mode)
                assert np.array_equal(got, want), (n, h, mode)
            assert torch.isnan(arena[n * h * d:]).all()


@pytest.mark.parametrize("rows", [[1, 17, 250], [4000, 90, 30]], ids=["1-17-250", "past-256-tiles"])
@pytest.mark.parametrize("d", [1, 5, 32])
def test_every_problem_of_a_batch_is_its_own_launch(d, rows):
    """[4000, 90, 30]: 250 + 6 + 2 = 258 tiles, two tiles per recurrence workgroup, the second problem off a multiple of 32 rows."""
    m = seeded_model(d)
    rs = np.random.RandomState(d)
    obs = (0.3 * rs.randn(len(rows), 230)).astype(np.float32)
    acts = torch.as_tensor(rs.uniform(-1, 1, (sum(rows), 12, d)), dtype=torch.float32, device="cuda")
    for mode in (0, 1):
        got = np_(m.rollout_cost_batch(obs, acts, rows, mode))
        assert np.isfinite(got).all()
        r0 = 0
        for p, r in enumerate(rows):
            alone = np_(m.rollout_cost(obs[p], acts[r0:r0 + r], mode))
            assert np.array_equal(got[r0:r0 + r], alone), (p, mode)
            r0 += r


def test_the_models_shape_errors_name_its_own_width():
    m = seeded_model(2)
    assert m.act_dim == 2 and m.params.numel() == m.lib.icem_rssm_param_elems()
    six = torch.zeros((16, 12, 6), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match=r"\[n, h, 2\]"):
        m.rollout_cost(np.zeros(230), six)
    with pytest.raises(ValueError, match=r"\[sum rows, h, 2\]"):
        m.rollout_cost_batch(np.zeros((1, 230)), six, [16])
    from icem_amd import DeviceRSSMModel
    with pytest.raises(ValueError):
        DeviceRSSMModel(act_dim=33)
