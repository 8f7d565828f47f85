"""The kernels of ``icem_plan_step_random_learned_batch`` exist in the built gfx950 object of k_random_learned.hip and keep their
registers: read from the code object's metadata as tests/test_random_objects_cpu.py reads them (no GPU, no recompilation).  The
gathering sampler for both generators and the pool selection, f32 only, each taking its argument blocks as a pointer to a device
array and the pool by value, none with more than 8 spilled VGPRs (the hygiene test's limit; its allow-list does not grow for them)."""
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
    obj = B.object_path("k_random_learned.hip")
    assert os.path.exists(obj), obj
    tot = kernel_spills(obj, str(tmp_path_factory.mktemp("co")))
    names = list(tot)
    dem = subprocess.check_output(["c++filt"], input="\n".join(names), text=True).splitlines()
    return {d: tot[n] for n, d in zip(names, dem)}


def _one(spills, pattern):
    hit = {k: v for k, v in spills.items() if re.search(pattern, k)}
    assert len(hit) == 1, (pattern, sorted(hit))
    return next(iter(hit.values()))


def test_the_gathering_samplers_exist_and_keep_their_registers(spills):
    for rounds in (7, 10):
        # the blocks come from a device array; the call offsets, the observations' addresses and the pool by value
        assert _one(spills, rf"random_sample_gather_batch_kernel<float, {rounds}>\(icem::RandomSampleArgs<float> const\*, icem::BatchBases, "
                            r"icem::ObsGather, icem::RandomPool<float>\)") <= LIMIT


def test_the_pool_selection_exists_and_keeps_its_registers(spills):
    assert _one(spills, r"random_select_pool_batch_kernel<float>\(icem::RandomSelectArgs<float> const\*, icem::RandomPool<float>\)") <= LIMIT


def test_nothing_else_is_in_the_unit(spills):
    assert len(spills) == 3, sorted(spills)
