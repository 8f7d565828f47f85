"""The batched forms of the GEMM-path rollout launches (icem_plan_step_batch on HumanoidStandup / Humanoid / Ant and the narrow
shapes no tile kernel serves) exist in the built gfx950 objects and keep their registers: read from the code objects' metadata as
tests/test_register_hygiene_cpu.py does (no GPU, no recompilation).  ``rollout_wide_batch_kernel`` for every NT x model kind x
term list on / off, ``rollout_rows_wide_batch_kernel`` for both model kinds, ``rollout_wide_split_batch_kernel`` for every
NCT x kind x term list x FIVE x planes -- none with more than 8 spilled VGPRs (the hygiene test's limit; its allow-list does not
grow for them: the twins of ``rollout_wide_split_kernel<3, [01], true, *, false>``, which that list carries at up to 16, stay
within 8 with their argument block read from memory and the development stamps compiled out)."""
import itertools
import os
import re
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
LIMIT = 8
B = ("false", "true")


@pytest.fixture(scope="module")
def spills(tmp_path_factory):
    from icem_amd import build as Bd
    from test_register_hygiene_cpu import kernel_spills
    if Bd.build_info()["stale"]:
        import __graft_entry__ as g
        g.build()
    if os.environ.get("ICEM_DEV_SHAPES"):
        pytest.skip("development build with a narrowed shape list")
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.skip(f"{tool} not in this image")
    tmp = str(tmp_path_factory.mktemp("co"))
    tot = {}
    for unit in ("k_rollout_wide.hip", "k_rollout_wide_batch.hip", "k_rollout_wide_split.hip", "k_rollout_wide_split_batch.hip"):
        obj = Bd.object_path(unit)
        assert os.path.exists(obj), obj
        tot.update(kernel_spills(obj, tmp))
    names = list(tot)
    dem = subprocess.check_output(["c++filt"], input="\n".join(names), text=True).splitlines()
    return {d: tot[n] for n, d in zip(names, dem)}


def _one(spills, pattern):
    hit = {k: v for k, v in spills.items() if re.search(pattern, k)}
    assert len(hit) == 1, (pattern, sorted(hit))
    return next(iter(hit.values()))


def test_a_batched_exact_rollout_exists_for_every_width_kind_and_term_switch(spills):
    over = []
    for nt, kind, ext in itertools.product((4, 8, 16, 24), (0, 1), B):
        _one(spills, rf"rollout_wide_kernel<{nt}, {kind}, 4, {ext}>\(icem::WideRolloutArgs\)")        # the by-value kernel is still there
        pat = rf"rollout_wide_batch_kernel<{nt}, {kind}, 4, {ext}>\(icem::WideRolloutArgs const\*\)"   # ... its twin reads a device array
        n = _one(spills, pat)
        if n > LIMIT:
            over.append((n, pat))
    for kind in (0, 1):
        _one(spills, rf"rollout_rows_wide_kernel<{kind}>\(icem::WideRowsArgs\)")
        pat = rf"rollout_rows_wide_batch_kernel<{kind}>\(icem::WideRowsArgs const\*\)"
        n = _one(spills, pat)
        if n > LIMIT:
            over.append((n, pat))
    assert not over, over
    assert len([k for k in spills if re.search(r"rollout_wide_kernel<", k)]) == len([k for k in spills if re.search(r"rollout_wide_batch_kernel<", k)])


def test_a_batched_plane_rollout_exists_for_every_instantiation(spills):
    over, served = [], 0
    for nct, kind, ext, five, f16 in itertools.product((1, 2, 3), (0, 1), B, B, B):
        _one(spills, rf"rollout_wide_split_kernel<{nct}, {kind}, {ext}, {five}, {f16}>\(icem::WideRolloutArgs\)")
        pat = rf"rollout_wide_split_batch_kernel<{nct}, {kind}, {ext}, {five}, {f16}>\(icem::WideRolloutArgs const\*\)"
        served += 1
        n = _one(spills, pat)
        if n > LIMIT:
            over.append((n, pat))
    assert served == 48
    assert not over, over
    assert len([k for k in spills if re.search(r"rollout_wide_split_batch_kernel<", k)]) == served
