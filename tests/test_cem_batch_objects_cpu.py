"""The batched kernels of ``icem_plan_step_cem_batch`` exist in the built gfx950 objects and keep their registers: read from the code
objects' metadata as tests/test_batch_hn_objects_cpu.py does (no GPU, no recompilation).  ``rollout16_batch_kernel`` for every
``ICEM_FAST_SHAPES`` entry x both model kinds x both tile arithmetics (the exact one only where the observation takes two tiles,
O > 20) x the wave counts the by-value kernel has (at most 8 where O > 20), ``cem_sample_batch_kernel`` for both dtypes and both
generators, and the two batched update kernels -- each taking its arguments as a pointer to a device array, none with more than 8
spilled VGPRs (the hygiene test's limit; its allow-list does not grow for them)."""
import os
import re
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
LIMIT = 8
SHAPES = [(30, 6, 17), (30, 6, 18), (12, 6, 17), (13, 4, 17), (30, 17, 24)]   # ICEM_FAST_SHAPES (fused_dev.h)


@pytest.fixture(scope="module")
def spills(tmp_path_factory):
    from icem_amd import build as B
    from test_register_hygiene_cpu import kernel_spills
    if B.build_info()["stale"]:
        import __graft_entry__ as g
        g.build()
    if os.environ.get("ICEM_DEV_SHAPES"):
        pytest.skip("development build with a narrowed shape list")
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.skip(f"{tool} not in this image")
    tmp = str(tmp_path_factory.mktemp("co"))
    tot = {}
    for unit in ("k_rollout.hip", "k_cem.hip"):
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


def test_the_shape_list_is_the_headers():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "icem_amd", "csrc", "fused_dev.h")).read()
    line = re.search(r"#define ICEM_FAST_SHAPES\(X\)(.*)", src).group(1)
    assert [tuple(int(v) for v in m) for m in re.findall(r"X\((\d+), (\d+), (\d+)\)", line)] == SHAPES


def test_a_batched_tile_rollout_exists_for_every_by_value_instantiation(spills):
    over, want = [], 0
    for (h, d, o) in SHAPES:
        for kind in (0, 1):
            for arith in ((0, 1) if o <= 20 else (0,)):
                for waves in ((1, 2, 4, 8, 16) if o <= 20 else (1, 2, 4, 8)):
                    want += 1
                    args = rf"<{h}, {d}, {o}, {kind}, {waves}, {arith}>"
                    _one(spills, rf"rollout16_kernel{args}\(icem::FastRolloutArgs\)")
                    # the arguments come from a device array, not from the kernel-argument segment
                    n = _one(spills, rf"rollout16_batch_kernel{args}\(icem::FastRolloutArgs const\*\)")
                    if n > LIMIT:
                        over.append((n, args))
    assert not over, over
    by_value = [k for k in spills if re.search(r"rollout16_kernel<", k)]
    batched = [k for k in spills if re.search(r"rollout16_batch_kernel<", k)]
    assert len(by_value) == len(batched) == want


def test_the_batched_sampler_and_updates_exist(spills):
    for t in ("float", "double"):
        for rounds in (7, 10):
            assert _one(spills, rf"cem_sample_batch_kernel<{t}, {rounds}>\(icem::CemSampleArgs<{t}> const\*, icem::BatchBases\)") <= LIMIT
            _one(spills, rf"cem_sample_kernel<{t}, {rounds}>\(icem::CemSampleArgs<{t}>\)")
    assert _one(spills, r"cem_update_f32_batch_kernel\(icem::CemUpdateF32Args const\*\)") <= LIMIT
    assert _one(spills, r"cem_update_f64_batch_kernel\(icem::CemUpdateF64Args const\*\)") <= LIMIT
    # the solo kernels keep their by-value arguments
    _one(spills, r"cem_update_f32_kernel\(icem::UpdateSmallArgs, icem::CemTailArgs<float>\)")
    _one(spills, r"cem_update_f64_kernel\(icem::SelectArgs<double>, int\*, icem::CemTailArgs<double>\)")
