"""The kernels of ``icem_plan_step_random`` / ``icem_plan_step_random_batch`` exist in the built gfx950 object of k_random.hip and
keep their registers: read from the code object's metadata as tests/test_cem_batch_objects_cpu.py does (no GPU, no recompilation).
The step's sampler by value and its batched twin for both dtypes and both generators, the selection kernel and its batched twin for
both dtypes -- the batched ones taking their arguments as a pointer to a device array, none with more than 8 spilled VGPRs (the
hygiene test's limit; its allow-list does not grow for them).  The operator's sampler is still there under its name."""
import os
import re
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
LIMIT = 8


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
    for unit in ("k_random.hip", "generic_kernels.hip"):
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


def test_the_samplers_exist_and_keep_their_registers(spills):
    for t in ("float", "double"):
        for rounds in (7, 10):
            assert _one(spills, rf"random_sample_kernel<{t}, {rounds}>\(icem::RandomSampleArgs<{t}>\)") <= LIMIT
            # the arguments come from a device array, the call offsets by value
            assert _one(spills, rf"random_sample_batch_kernel<{t}, {rounds}>\(icem::RandomSampleArgs<{t}> const\*, icem::BatchBases\)") <= LIMIT
            _one(spills, rf"sample_piecewise_kernel<{t}, {rounds}>\(")   # the operator's


def test_the_selection_kernels_exist_and_keep_their_registers(spills):
    for t in ("float", "double"):
        assert _one(spills, rf"random_select_kernel<{t}>\(icem::RandomSelectArgs<{t}>\)") <= LIMIT
        assert _one(spills, rf"random_select_batch_kernel<{t}>\(icem::RandomSelectArgs<{t}> const\*\)") <= LIMIT


def test_nothing_else_is_in_the_unit(spills):
    mine = [k for k in spills if "random_s" in k]
    assert len(mine) == 8 + 4, sorted(mine)
