"""The action width of the learned-dynamics path without a device: the packer at widths 1, 5, 32 (the buffer's size, where the
action columns sit, zeros behind them; width 6 as it always was), the new symbols with their argument types, the bind / refuse
rules of icem_set_rssm_act_dim on handles made without a GPU call, the runtime-width kernels in the built objects."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from icem_amd import _lib as L
from icem_amd.models import declared_rssm, pack_rssm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {
    "icem_rssm_rollout_cost_w": "int (int32_t n, int32_t horizon, int32_t act_dim, int32_t cost_mode, const void* params, const void* obs0, "
                                "const void* actions, void* costs, void* stream)",
    "icem_rssm_rollout_cost_batch_w": "int (int32_t n_problems, const int32_t* rows_host, int32_t horizon, int32_t act_dim, int32_t cost_mode, "
                                      "const void* params, const void* obs0, const void* actions, void* costs, void* stream)",
    "icem_set_rssm_act_dim": "int (icem_handle* h, int32_t act_dim)",
    "icem_rssm_act_dim": "int32_t (const icem_handle* h)",
}
BLK, HIDB, K1K = 64 * 8, 13, 2   # icem_amd/csrc/icem_rssm.h


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.lib_path()):
        import __graft_entry__ as g
        g.build()
    return L.load_library()


def _w1(packed):
    """The input layer out of a packed buffer: [208 outputs, 64 contraction columns] as floats (bf16 values)."""
    blocks = packed[:HIDB * K1K * BLK].view(torch.bfloat16).float().reshape(HIDB, K1K, 4, 16, 8)   # [ob, kb, g, i, v]
    return blocks.permute(0, 3, 1, 2, 4).reshape(HIDB * 16, K1K * 32).numpy()


@pytest.mark.parametrize("d", [1, 5, 6, 32])
def test_the_packer_puts_the_action_columns_at_32(d, lib):
    net = declared_rssm(act_dim=d, seed=2, device="cpu").module
    packed = pack_rssm(net)
    assert packed.numel() == lib.icem_rssm_param_elems() and packed.dtype == torch.int16
    w = net.inp.weight.detach().to(torch.bfloat16).float().numpy()   # [200, 30 + d]
    got = _w1(packed)
    assert np.array_equal(got[:200, :30], w[:, :30]) and np.array_equal(got[:200, 32:32 + d], w[:, 30:])
    assert (got[:200, 32:32 + d] != 0).all()
    assert not got[:, 30:32].any() and not got[:, 32 + d:].any() and not got[200:].any()


def test_width_six_packs_as_it_always_did():
    """Against the layout written out by hand for the declared width: the bytes of the input layer, and everything behind it
    equal to the same network packed at another width (the other layers know no action)."""
    net = declared_rssm(seed=4, device="cpu").module
    packed = pack_rssm(net)
    w = torch.zeros(208, 64)
    w[:200, :30], w[:200, 32:38] = net.inp.weight.detach()[:, :30], net.inp.weight.detach()[:, 30:36]
    want = w.reshape(13, 16, 2, 4, 8).permute(0, 2, 3, 1, 4).contiguous().to(torch.bfloat16).view(torch.int16).reshape(-1)
    assert torch.equal(packed[:want.numel()], want)
    wide = declared_rssm(act_dim=9, seed=4, device="cpu").module
    sd = {k: v for k, v in net.state_dict().items() if not k.startswith("inp.")}
    wide.load_state_dict({**wide.state_dict(), **sd})
    assert torch.equal(pack_rssm(wide)[want.numel() + 2 * 16 * 13:], packed[want.numel() + 2 * 16 * 13:])


def test_the_packer_refuses_what_the_layout_does_not_hold():
    for d in (33, 64):
        with pytest.raises(AssertionError):
            pack_rssm(declared_rssm(act_dim=d, device="cpu").module)
    with pytest.raises(AssertionError):
        pack_rssm(declared_rssm(det=100, device="cpu").module)


def _squash(s):
    return re.sub(r"\s+", " ", s).strip()


def test_the_header_declares_the_entries_with_these_signatures():
    hdr = open(os.path.join(ROOT, "include", "icem_hip.h")).read()
    assert re.search(r"#define\s+ICEM_RSSM_MAX_ACT_DIM\s+32\b", hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, sig in SIGNATURES.items():
        m = re.search(rf"^(\w+)\s+{name}\s*\(([^)]*)\)\s*;", hdr, flags=re.M)
        assert m, name
        assert _squash(f"{m.group(1)} ({_squash(m.group(2))})") == sig, name


def test_the_library_exports_them_and_lib_binds_them(lib):
    bound = {name: (res, args) for name, res, args in L.SYMBOLS}
    VP, I32 = C.c_void_p, C.c_int32
    assert bound["icem_rssm_rollout_cost_w"] == (C.c_int, [I32, I32, I32, I32, VP, VP, VP, VP, VP])
    assert bound["icem_rssm_rollout_cost_batch_w"] == (C.c_int, [I32, C.POINTER(I32), I32, I32, I32, VP, VP, VP, VP, VP])
    assert bound["icem_set_rssm_act_dim"] == (C.c_int, [VP, I32])
    assert bound["icem_rssm_act_dim"] == (I32, [VP])
    assert lib.icem_abi_version() == L.ABI_VERSION == 6   # an added symbol breaks no caller
    if shutil.which("nm") is not None:
        exported = subprocess.check_output(["nm", "-D", "--defined-only", L.lib_path()], text=True)
        for name in list(SIGNATURES) + ["icem_rssm_rollout_cost", "icem_rssm_rollout_cost_batch"]:
            assert re.search(rf"\bT {name}$", exported, flags=re.M), name


def test_argument_errors_need_no_device(lib):
    p = C.c_void_p(8)   # (never dereferenced)
    assert lib.icem_rssm_rollout_cost_w(16, 12, 6, 0, None, p, p, p, None) == L.ICEM_E_INVALID
    assert lib.icem_rssm_rollout_cost_w(16, 0, 6, 0, p, p, p, p, None) == L.ICEM_E_INVALID
    for d in (0, -1, 33, 64):
        assert lib.icem_rssm_rollout_cost_w(16, 12, d, 0, p, p, p, p, None) == L.ICEM_E_UNSUPPORTED, d
        assert b"act_dim" in lib.icem_last_error()
        assert lib.icem_rssm_rollout_cost_batch_w(1, (C.c_int32 * 1)(16), 12, d, 0, p, p, p, p, None) == L.ICEM_E_UNSUPPORTED, d
    assert lib.icem_rssm_rollout_cost_batch_w(1, None, 12, 6, 0, p, p, p, p, None) == L.ICEM_E_INVALID
    assert lib.icem_rssm_rollout_cost_batch_w(0, (C.c_int32 * 1)(16), 12, 6, 0, p, p, p, p, None) == L.ICEM_E_INVALID
    assert lib.icem_set_rssm_act_dim(None, 6) == L.ICEM_E_INVALID and lib.icem_rssm_act_dim(None) == 0


def _handle(lib, d, dtype="f32"):
    """A handle straight from icem_create; None where creating one needs a device this machine does not have."""
    from icem_amd import IcemConfig
    cfg = IcemConfig(horizon=12, act_dim=d, num_traj=64, dtype=dtype).to_c()
    h = C.c_void_p()
    if lib.icem_create(C.byref(cfg), C.byref(h)) != 0:
        return None
    return h


def test_bind_and_refuse(lib):
    """act_dim must be the handle's own (ICEM_E_INVALID) and at most 32 (ICEM_E_UNSUPPORTED); a refused call leaves the binding
    as it was; a handle never bound reads 6.  (Run on the handles icem_create hands out here: skipped where it needs a GPU.)"""
    hs = {d: _handle(lib, d) for d in (2, 6, 32, 33, 64)}
    if any(h is None for h in hs.values()):
        pytest.skip("icem_create needs a device here")
    try:
        for d, h in hs.items():
            assert lib.icem_rssm_act_dim(h) == 6, d
        assert lib.icem_set_rssm_act_dim(hs[2], 6) == L.ICEM_E_INVALID and lib.icem_rssm_act_dim(hs[2]) == 6
        assert lib.icem_set_rssm_act_dim(hs[2], 2) == 0 and lib.icem_rssm_act_dim(hs[2]) == 2
        assert lib.icem_set_rssm_act_dim(hs[2], 3) == L.ICEM_E_INVALID and lib.icem_rssm_act_dim(hs[2]) == 2
        assert lib.icem_set_rssm_act_dim(hs[2], 33) == L.ICEM_E_INVALID and lib.icem_rssm_act_dim(hs[2]) == 2
        assert lib.icem_set_rssm_act_dim(hs[32], 32) == 0 and lib.icem_rssm_act_dim(hs[32]) == 32
        for d in (33, 64):
            assert lib.icem_set_rssm_act_dim(hs[d], d) == L.ICEM_E_UNSUPPORTED and lib.icem_rssm_act_dim(hs[d]) == 6, d
            assert lib.icem_set_rssm_act_dim(hs[d], 6) == L.ICEM_E_INVALID, d
        assert lib.icem_set_rssm_act_dim(hs[6], 6) == 0 and lib.icem_rssm_act_dim(hs[6]) == 6
        # the served-questions follow the binding: a bound d = 2 handle is asked like a d = 6 one, an unbound one is refused
        other = _handle(lib, 2)
        for ok in (lib.icem_plan_step_learned_ok, lib.icem_plan_step_cem_learned_ok, lib.icem_plan_step_random_learned_ok):
            assert ok(other) == 0
            assert ok(hs[2]) == ok(hs[6])
        lib.icem_destroy(other)
    finally:
        for h in hs.values():
            lib.icem_destroy(h)


def test_the_python_layers_carry_the_width():
    from icem_amd import DeviceRSSMModel, IcemPlanner
    assert inspect.signature(DeviceRSSMModel.__init__).parameters["act_dim"].default == 6
    for name in ("learned_step_ok", "cem_learned_step_ok", "random_learned_step_ok"):
        assert inspect.signature(getattr(IcemPlanner, name)).parameters["model"].default is None, name
    assert callable(IcemPlanner._bind_rssm)


def test_the_runtime_width_kernels_are_in_the_objects():
    from icem_amd import build as B
    if B.build_info()["stale"]:
        import __graft_entry__ as g
        g.build()
    if shutil.which("nm") is None or shutil.which("c++filt") is None:
        pytest.skip("nm / c++filt not in this image")
    want = {"icem_rssm.hip": ["rssm_rollout_w_kernel<1>", "rssm_rollout_kernel<1>", "rssm_rollout_kernel<2>"],
            "icem_rssm_split.hip": ["rssm_split_w_kernel<1>", "rssm_split_w_kernel<2>", "rssm_split_batch_w_kernel<1>",
                                    "rssm_split_batch_w_kernel<2>", "rssm_split_kernel<1>", "rssm_split_kernel<2>",
                                    "rssm_split_batch_kernel<1>", "rssm_split_batch_kernel<2>"]}
    for unit, names in want.items():
        obj = B.object_path(unit)
        assert os.path.exists(obj), obj
        syms = subprocess.check_output(["nm", obj], text=True)
        dem = subprocess.check_output(["c++filt"], input=syms, text=True)
        for name in names:
            assert re.search(rf"__device_stub__{re.escape(name)}\(", dem), (unit, name)
