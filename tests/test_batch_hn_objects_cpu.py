"""The batched forms of a TileHN step's launches (icem_plan_step_batch on the Door / Relocate / FetchPickAndPlace shapes) exist in
the built gfx950 objects and keep their registers: read from the code objects' metadata as tests/test_register_hygiene_cpu.py
does (no GPU, no recompilation).  ``rollout_hn_batch_kernel`` for each compiled shape x both model kinds x the four term programs
x 1, 2 and 4 waves per workgroup, ``sample_folded_batch_kernel`` and ``sample_folded_merge_batch_kernel`` at h = 30 -- none with
more than 8 spilled VGPRs (the hygiene test's limit; its allow-list does not grow for them)."""
import os
import re
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
LIMIT = 8
SHAPES = [(30, 28, 39), (30, 30, 39), (30, 4, 28)]          # ICEM_HN_SHAPES: door, relocate, fpp
PROGRAMS = [(0, 0, 0), (0, 2, 0), (0, 4, 1), (1, 1, 4)]     # hn_cost_program


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
    for unit in ("k_rollout_hn.hip", "k_sample.hip"):
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


def test_a_batched_tilehn_rollout_exists_for_every_compiled_shape_kind_and_program(spills):
    over = []
    for (h, d, o) in SHAPES:
        for kind in (0, 1):
            for (n32, n4, npt) in PROGRAMS:
                for waves in (1, 2, 4):
                    pat = rf"rollout_hn_batch_kernel<{h}, {d}, {o}, {kind}, {waves}, {n32}, {n4}, {npt}>\("
                    n = _one(spills, pat)
                    if n > LIMIT:
                        over.append((n, pat))
    assert not over, over
    # the by-value kernels are still there, one per batched form: same template arguments, same body
    assert len([k for k in spills if re.search(r"rollout_hn_kernel<", k)]) == len([k for k in spills if re.search(r"rollout_hn_batch_kernel<", k)])


def test_the_batched_samplers_exist_at_the_tilehn_horizon(spills):
    assert _one(spills, r"sample_folded_batch_kernel<30, 10>\(") <= LIMIT
    assert _one(spills, r"sample_folded_merge_batch_kernel<30, 10, 12>\(") <= LIMIT
    # the arguments come from a device array, not from the kernel-argument segment
    assert [k for k in spills if re.search(r"sample_folded_batch_kernel<30, 10>\(icem::FastSampleArgs const\*", k)]
