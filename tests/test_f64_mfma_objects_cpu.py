"""The float64 matrix-core rollout (``icem_set_f64_arith``, k_rollout_f64.hip) as far as a machine without a GPU can see it:
the two entry points are declared, exported and bound, the translation unit is part of the build, and every instantiation of
its kernel is in the built object with at most 8 spilled VGPRs and the f64 matrix instruction in its code."""
import os
import re
import subprocess

import pytest

from icem_amd import _lib as L
from icem_amd import build as B
from test_register_hygiene_cpu import LLVM, kernel_spills

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = "k_rollout_f64.hip"
LIMIT = 8


@pytest.fixture(scope="module")
def built():
    if B.build_info()["stale"]:
        import __graft_entry__ as g
        g.build()
    return L.load_library()


def test_entry_points_are_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "icem_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+icem_set_f64_arith\s*\(\s*icem_handle\s*\*\s*h\s*,\s*int32_t\s+mode\s*\)\s*;", code)
    assert re.search(r"\bint\s+icem_f64_arith\s*\(\s*const\s+icem_handle\s*\*\s*h\s*\)\s*;", code)
    assert re.search(r"ICEM_F64_CHAIN\s*=\s*0\s*,\s*ICEM_F64_MFMA\s*=\s*1", code)
    assert "#define ICEM_ABI_VERSION 6" in hdr
    bound = {name for name, _, _ in L.SYMBOLS}
    for name in ("icem_set_f64_arith", "icem_f64_arith"):
        assert name in bound and hasattr(built, name)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", L.lib_path()], text=True)
    assert re.search(r"\bT icem_set_f64_arith\b", exported) and re.search(r"\bT icem_f64_arith\b", exported)
    # no handle: the arithmetic in effect is the default, a set call is refused -- neither touches a device
    assert built.icem_f64_arith(None) == 0
    assert built.icem_set_f64_arith(None, 1) == L.ICEM_E_INVALID


def test_the_planner_and_the_controller_expose_the_mode():
    import inspect
    from icem_amd import IcemPlanner, MpcICemHip
    assert callable(IcemPlanner.set_f64_arith) and isinstance(IcemPlanner.f64_arith, property)
    assert IcemPlanner.F64_ARITH == {"chain": 0, "mfma": 1}
    assert "f64_arith" in inspect.signature(MpcICemHip.__init__).parameters


def test_every_instantiation_is_built_and_does_not_spill(built, tmp_path):
    assert UNIT in B.UNITS
    obj = B.object_path(UNIT)
    assert os.path.exists(obj), obj
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump"):
        assert os.path.exists(os.path.join(LLVM, tool)), tool
    spills = kernel_spills(obj, str(tmp_path))
    names = list(spills)
    dem = subprocess.check_output(["c++filt"], input="\n".join(names), text=True).splitlines()
    got = {d: spills[n] for n, d in zip(names, dem) if "rollout_f64_mfma_kernel" in d}
    # model kind (linear / tanh) x term list x observations written: one kernel family, never instantiated on a width
    want = {f"<{kind}, {terms}, {obs}>" for kind in (0, 1) for terms in ("false", "true") for obs in ("false", "true")}
    assert {re.search(r"<[^>]*>", k).group(0) for k in got} == want, sorted(got)
    assert len(got) == 8
    for name, n in got.items():
        assert n <= LIMIT, (name, n)
    asm = subprocess.check_output([f"{LLVM}/llvm-objdump", "-d", os.path.join(str(tmp_path), "d.co")], text=True)
    assert asm.count("v_mfma_f64_16x16x4") >= 8
