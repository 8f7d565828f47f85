"""The code objects behind icem_plan_step_learned_models, read from the build (no GPU, no recompilation): the two new update
kernels -- update_small_members_batch_kernel<true / false>, the one-launch update that reduces the members' costs itself -- are
in k_merge.hip's gfx950 object and keep their registers (at most test_register_hygiene_cpu.LIMIT spilled VGPRs, and on no
allow-list); and the kernels that share their body (update_small_body.h, now with the cost source as a template parameter)
spill what they spilled before the parameter existed: nothing."""
import os
import re
import subprocess

import pytest

from test_register_hygiene_cpu import ALLOWED, LIMIT, LLVM, kernel_spills

# VGPR spill counts of the kernels on update_small_body before it took a cost source (read from that build's code objects)
BEFORE = {
    r"update_small_kernel\(icem::UpdateSmallArgs\)": 0,
    r"update_small_batch_kernel<true>\(icem::UpdateFinishArgs const\*\)": 0,
    r"update_small_batch_kernel<false>\(icem::UpdateFinishArgs const\*\)": 0,
    r"cem_update_f32_kernel\(icem::UpdateSmallArgs, icem::CemTailArgs<float>\)": 0,
    r"cem_update_f32_batch_kernel\(icem::CemUpdateF32Args const\*\)": 0,
}
NEW = [rf"update_small_members_batch_kernel<{finish}>\(icem::UpdateMembersArgs const\*\)" for finish in ("true", "false")]


@pytest.fixture(scope="module")
def spills(tmp_path_factory):
    from icem_amd import build as B
    if B.build_info()["stale"]:
        import __graft_entry__ as g
        g.build()
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.skip(f"{tool} not in this image")
    tmp = str(tmp_path_factory.mktemp("co"))
    out = {}
    for unit in ("k_merge.hip", "k_cem.hip"):
        obj = B.object_path(unit)
        assert os.path.exists(obj), obj
        tot = kernel_spills(obj, tmp)
        names = list(tot)
        dem = subprocess.check_output(["c++filt"], input="\n".join(names), text=True).splitlines()
        out[unit] = {d: tot[n] for n, d in zip(names, dem)}
    return out


def _one(table, pattern):
    hit = {k: v for k, v in table.items() if re.search(pattern, k)}
    assert len(hit) == 1, (pattern, sorted(hit))
    return next(iter(hit.items()))


def test_the_new_update_kernels_are_in_k_merges_object_and_keep_their_registers(spills):
    for pat in NEW:
        name, n = _one(spills["k_merge.hip"], pat)
        print(f"{n:3d} spilled VGPRs  {name}")
        assert n <= LIMIT, (name, n)
        assert not [p for p, _cap, _why in ALLOWED if re.search(p, name)], "not on the allow-list"
        assert not [k for k in spills["k_cem.hip"] if re.search(pat, k)]


def test_the_kernels_that_share_the_body_spill_what_they_did(spills):
    both = dict(spills["k_merge.hip"])
    both.update(spills["k_cem.hip"])
    for pat, before in BEFORE.items():
        name, n = _one(both, pat)
        assert n == before, (name, n, before)
