"""The CEM baseline's step entry (icem_plan_step_cem, cem_step.hip + k_cem.hip) without a device: the three symbols are
exported, declared and bound; the two structs have the header's sizes; the development option that switches the entry exists
and is on; argument errors are reported before any device is looked for; the new kernels are in the built gfx950 objects and
keep their registers; the operators' kernels whose bodies the step's kernels share are still there under their names."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from icem_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
LIMIT = 8
NEW = ["icem_plan_step_cem_ok", "icem_plan_step_cem", "icem_cem_step_launches"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.lib_path()):
        import __graft_entry__ as g
        g.build()
    return L.load_library()


def test_symbols_are_exported_declared_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "icem_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(icem_[a-z_0-9]+)\s*\(", hdr))
    bound = {name for name, _, _ in L.SYMBOLS}
    for name in NEW:
        assert name in declared and name in bound and hasattr(lib, name), name
    assert re.search(r"typedef struct icem_cem_params\s*\{", hdr) and re.search(r"typedef struct icem_cem_buffers\s*\{", hdr)
    assert lib.icem_abi_version() == 6   # an added symbol breaks no caller
    from icem_amd import IcemPlanner
    for attr in ("cem_step_ok", "plan_step_cem", "cem_step_launches"):
        assert hasattr(IcemPlanner, attr), attr


def test_struct_sizes():
    # icem_cem_params: 4 int32; icem_cem_buffers: 15 pointers
    assert C.sizeof(L.IcemCemParamsC) == 16
    assert C.sizeof(L.IcemCemBuffersC) == 15 * 8
    assert [n for n, _ in L.IcemCemBuffersC._fields_] == [
        "mean", "std", "lower", "upper", "low", "high", "obs0", "actions", "costs", "elites", "elite_costs", "elite_idx",
        "executed", "best_cost", "workspace"]


def test_struct_sizes_match_c_compiler(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    hdr = os.path.join(ROOT, "include", "icem_hip.h")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu %%zu", '
                   'sizeof(icem_cem_params), sizeof(icem_cem_buffers), offsetof(icem_cem_buffers, elite_idx), '
                   'offsetof(icem_cem_buffers, workspace), offsetof(icem_cem_params, execute_best_elite));return 0;}' % hdr)
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(L.IcemCemParamsC), C.sizeof(L.IcemCemBuffersC), L.IcemCemBuffersC.elite_idx.offset,
                   L.IcemCemBuffersC.workspace.offset, L.IcemCemParamsC.execute_best_elite.offset]


def test_the_switch_is_an_option_and_on_by_default(lib):
    assert "cem_step" in L.option_names()
    L.reset_options()
    assert L.get_option("cem_step") == 1.0
    L.set_option("cem_step", 0)
    assert L.get_option("cem_step") == 0.0
    L.reset_options()


def test_argument_errors_need_no_device(lib):
    h = C.c_void_p(1)   # (never dereferenced: every call below fails on another argument first)
    cb, prm = L.IcemCemBuffersC(), L.IcemCemParamsC()
    assert lib.icem_plan_step_cem_ok(None) == 0
    assert lib.icem_cem_step_launches(None) == 0
    assert lib.icem_plan_step_cem(None, C.byref(cb), C.byref(prm), 0, None) == L.ICEM_E_INVALID
    assert lib.icem_plan_step_cem(h, None, C.byref(prm), 0, None) == L.ICEM_E_INVALID
    assert lib.icem_plan_step_cem(h, C.byref(cb), None, 0, None) == L.ICEM_E_INVALID
    assert b"icem_plan_step_cem" in lib.icem_last_error()
    assert lib.icem_plan_step_cem(h, C.byref(cb), C.byref(prm), -1, None) == L.ICEM_E_INVALID    # a negative step
    assert lib.icem_plan_step_cem(h, C.byref(cb), C.byref(prm), 0, None) == L.ICEM_E_INVALID     # null buffers
    assert b"null buffer" in lib.icem_last_error()


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
    tmp = str(tmp_path_factory.mktemp("co"))
    tot = {}
    for unit in ("k_cem.hip", "k_merge.hip", "generic_kernels.hip", "k_generic_batch.hip"):
        obj = B.object_path(unit)
        assert os.path.exists(obj), obj
        tot.update(kernel_spills(obj, tmp))
    names = list(tot)
    dem = subprocess.check_output(["c++filt"], input="\n".join(names), text=True).splitlines()
    return {d: tot[n] for n, d in zip(names, dem)}


def _one(spills, pattern):
    hit = {k: v for k, v in spills.items() if re.search(pattern, k)}
    assert len(hit) == 1, (pattern, sorted(hit))
    return next(iter(hit.values()))


def test_the_new_kernels_exist_and_keep_their_registers(spills):
    over = []
    pats = [r"cem_update_f32_kernel\(icem::UpdateSmallArgs, icem::CemTailArgs<float>\)",
            r"cem_update_f64_kernel\(icem::SelectArgs<double>, int\*, icem::CemTailArgs<double>\)"]
    pats += [rf"cem_sample_kernel<{t}, {r}>\(icem::CemSampleArgs<{t}>\)" for t in ("float", "double") for r in (7, 10)]
    for pat in pats:
        n = _one(spills, pat)
        if n > LIMIT:
            over.append((n, pat))
    assert not over, over


def test_the_operators_kernels_are_still_there_under_their_names(spills):
    _one(spills, r"update_small_kernel\(icem::UpdateSmallArgs\)")
    for finish in ("true", "false"):
        _one(spills, rf"update_small_batch_kernel<{finish}>\(icem::UpdateFinishArgs const\*\)")
    _one(spills, r"select_refit_kernel<double>\(icem::SelectArgs<double>\)")
    _one(spills, r"select_refit_kernel<float>\(icem::SelectArgs<float>\)")
    _one(spills, r"select_refit_batch_kernel\(icem::SelectArgs<double> const\*")
    for t in ("float", "double"):
        _one(spills, rf"cem_bounds_kernel<{t}>\(")
        for r in (7, 10):
            _one(spills, rf"sample_truncnorm_kernel<{t}, {r}>\(")
