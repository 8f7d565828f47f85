"""The CEM baseline's step through the learned dynamics (icem_plan_step_cem_learned / _batch, cem_step.hip + k_cem.hip) without a
device: the three symbols are declared, exported, bound and callable and the ABI version stays 6; the planner's methods exist;
argument errors are reported before any device is looked for; the batch's first sampler launch -- the one new kernel -- is in
k_cem.hip's gfx950 object for both generators, takes its argument blocks as a pointer and keeps its registers; the kernels the step
shares are still there under their names."""
import ctypes as C
import os
import re
import subprocess

import pytest

from icem_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
LIMIT = 8
NEW = ["icem_plan_step_cem_learned_ok", "icem_plan_step_cem_learned", "icem_plan_step_cem_learned_batch"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.lib_path()):
        import __graft_entry__ as g
        g.build()
    return L.load_library()


def test_symbols_are_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "icem_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(icem_[a-z_0-9]+)\s*\(", hdr))
    bound = {name for name, _, _ in L.SYMBOLS}
    for name in NEW:
        assert name in declared and name in bound and hasattr(lib, name), name
    assert lib.icem_abi_version() == 6   # an added symbol breaks no caller
    assert L.ABI_VERSION == 6


def test_the_planner_and_the_controller_have_the_way_up():
    from icem_amd import IcemPlanner, MpcCemStdHip, MpcICemHip
    for attr in ("cem_learned_step_ok", "plan_step_cem_learned", "plan_step_cem_learned_batch"):
        assert callable(getattr(IcemPlanner, attr)), attr
    # one rule for "the model is the library's own RSSM", where both controllers reach it
    assert MpcCemStdHip._model_is_the_library_rssm is MpcICemHip._model_is_the_library_rssm


def test_argument_errors_need_no_device(lib):
    h = C.c_void_p(1)   # (never dereferenced: every call below fails on another argument first)
    params = C.c_void_p(8)
    cb, prm = L.IcemCemBuffersC(), L.IcemCemParamsC()
    solo = lib.icem_plan_step_cem_learned
    assert lib.icem_plan_step_cem_learned_ok(None) == 0
    for args in ((None, C.byref(cb), C.byref(prm), params), (h, None, C.byref(prm), params), (h, C.byref(cb), None, params),
                 (h, C.byref(cb), C.byref(prm), None)):
        assert solo(*args, 0, None) == L.ICEM_E_INVALID
        assert b"icem_plan_step_cem_learned" in lib.icem_last_error()
    assert solo(h, C.byref(cb), C.byref(prm), params, -1, None) == L.ICEM_E_INVALID    # a negative step
    assert b"negative mpc_step" in lib.icem_last_error()
    assert solo(h, C.byref(cb), C.byref(prm), params, 0, None) == L.ICEM_E_INVALID     # null buffers
    assert b"null buffer" in lib.icem_last_error()


def test_batch_argument_errors_need_no_device(lib):
    batch = lib.icem_plan_step_cem_learned_batch
    params = C.c_void_p(8)
    hs = (C.c_void_p * 33)(*[1 + i for i in range(33)])   # (never dereferenced)
    bs, prm, steps = (L.IcemCemBuffersC * 33)(), L.IcemCemParamsC(), (C.c_int32 * 33)()
    for n in (0, 33, -1):
        assert batch(hs, n, bs, C.byref(prm), params, steps, None, None) == L.ICEM_E_INVALID, n
        assert b"icem_plan_step_cem_learned_batch" in lib.icem_last_error()
    for args in ((None, 2, bs, C.byref(prm), params, steps), (hs, 2, None, C.byref(prm), params, steps), (hs, 2, bs, None, params, steps),
                 (hs, 2, bs, C.byref(prm), None, steps), (hs, 2, bs, C.byref(prm), params, None)):
        assert batch(*args, None, None) == L.ICEM_E_INVALID
    null_handle = (C.c_void_p * 2)(1, None)
    assert batch(null_handle, 2, bs, C.byref(prm), params, steps, None, None) == L.ICEM_E_INVALID
    twice = (C.c_void_p * 2)(1, 1)
    assert batch(twice, 2, bs, C.byref(prm), params, steps, None, None) == L.ICEM_E_INVALID
    assert b"twice" in lib.icem_last_error()


@pytest.fixture(scope="module")
def spills(tmp_path_factory):
    from icem_amd import build as B
    from test_register_hygiene_cpu import kernel_spills
    if B.build_info()["stale"]:
        import __graft_entry__ as g
        g.build()
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.skip(f"{tool} not in this image")
    obj = B.object_path("k_cem.hip")
    assert os.path.exists(obj), obj
    tot = kernel_spills(obj, str(tmp_path_factory.mktemp("co")))
    names = list(tot)
    dem = subprocess.check_output(["c++filt"], input="\n".join(names), text=True).splitlines()
    return {d: tot[n] for n, d in zip(names, dem)}


def _one(spills, pattern):
    hit = {k: v for k, v in spills.items() if re.search(pattern, k)}
    assert len(hit) == 1, (pattern, sorted(hit))
    return next(iter(hit.values()))


def test_the_gathering_sampler_exists_and_keeps_its_registers(spills):
    for rounds in (7, 10):
        n = _one(spills, rf"cem_sample_gather_batch_kernel<float, {rounds}>\(icem::CemSampleArgs<float> const\*, icem::BatchBases, icem::ObsGather\)")
        assert n <= LIMIT, (rounds, n)


def test_the_shared_kernels_are_still_there_under_their_names(spills):
    for t in ("float", "double"):
        for rounds in (7, 10):
            _one(spills, rf"cem_sample_batch_kernel<{t}, {rounds}>\(icem::CemSampleArgs<{t}> const\*, icem::BatchBases\)")
            _one(spills, rf"cem_sample_kernel<{t}, {rounds}>\(icem::CemSampleArgs<{t}>\)")
    _one(spills, r"cem_update_f32_kernel\(icem::UpdateSmallArgs, icem::CemTailArgs<float>\)")
    _one(spills, r"cem_update_f64_kernel\(icem::SelectArgs<double>, int\*, icem::CemTailArgs<double>\)")
    _one(spills, r"cem_update_f32_batch_kernel\(icem::CemUpdateF32Args const\*\)")
    _one(spills, r"cem_update_f64_batch_kernel\(icem::CemUpdateF64Args const\*\)")
