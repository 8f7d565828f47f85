"""The code objects behind icem_plan_step_cem_learned_models / icem_plan_step_random_learned_models, read from the build (no GPU, no
recompilation) as tests/test_learned_models_objects_cpu.py reads its own: the two new kernels -- cem_update_members_batch_kernel
(k_cem_members.hip) and random_select_members_batch_kernel (k_random_members.hip) -- are in the built gfx950 objects, take their
argument blocks as a pointer to a device array, spill nothing (no VGPR to scratch, no private segment) and stay within the 128
VGPRs that 1024 threads per workgroup leave; and the kernels whose bodies gained the cost source as a template parameter, or a
neighbour in their unit, spill what they spilled before: nothing."""
import os
import re
import subprocess

import pytest

from test_register_hygiene_cpu import ALLOWED, LLVM

NEW = {
    "k_cem_members.hip": r"cem_update_members_batch_kernel\(icem::CemUpdateMembersArgs const\*\)",
    "k_random_members.hip": r"random_select_members_batch_kernel\(icem::RandomSelectArgs<float> const\*, icem::RandomPool<float>, icem::RandomMembers\)",
}
BEFORE = {   # VGPR spill counts before this kernel had a neighbour / its body a cost source
    "k_cem.hip": [r"cem_update_f32_kernel\(icem::UpdateSmallArgs, icem::CemTailArgs<float>\)", r"cem_update_f32_batch_kernel\(icem::CemUpdateF32Args const\*\)"],
    "k_random_learned.hip": [r"random_select_pool_batch_kernel<float>\(icem::RandomSelectArgs<float> const\*, icem::RandomPool<float>\)"],
    "k_random.hip": [r"random_select_kernel<float>\(icem::RandomSelectArgs<float>\)", r"random_select_batch_kernel<double>\(icem::RandomSelectArgs<double> const\*\)"],
}
FIELDS = ("vgpr_count", "vgpr_spill_count", "sgpr_count", "private_segment_fixed_size", "max_flat_workgroup_size")


def kernel_notes(obj, tmp):
    """{mangled kernel name: {field: value}} from the code object's metadata (test_register_hygiene_cpu.kernel_spills, more fields)."""
    fat, co = os.path.join(tmp, "f.fatbin"), os.path.join(tmp, "d.co")
    subprocess.check_call([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj])
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
    notes = subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", co], text=True)
    # one block per kernel, from its first key (the keys are sorted: .agpr_count) to the next kernel's; the kernel's own .name
    # is the least indented one of its block (its arguments have names too)
    out = {}
    for block in re.split(r"\n(?=\s*- \.agpr_count:)", notes)[1:]:
        names = [(len(m.group(1)), m.group(2)) for m in re.finditer(r"^(\s*(?:- )?)\.name:\s+(\S+)", block, flags=re.M)]
        vals = {f: int(m.group(1)) for f in FIELDS for m in [re.search(rf"^\s*\.{f}:\s+(\d+)", block, flags=re.M)] if m}
        out[min(names)[1]] = vals
    return out


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    from icem_amd import build as B
    if B.build_info()["stale"]:
        import __graft_entry__ as g
        g.build()
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.skip(f"{tool} not in this image")
    tmp = str(tmp_path_factory.mktemp("co"))
    out = {}
    for unit in ("k_cem_members.hip", "k_cem.hip", "k_random_members.hip", "k_random_learned.hip", "k_random.hip"):
        obj = B.object_path(unit)
        assert os.path.exists(obj), obj
        tot = kernel_notes(obj, tmp)
        names = list(tot)
        dem = subprocess.check_output(["c++filt"], input="\n".join(names), text=True).splitlines()
        out[unit] = {d: tot[n] for n, d in zip(names, dem)}
    return out


def _one(table, pattern):
    hit = {k: v for k, v in table.items() if re.search(pattern, k)}
    assert len(hit) == 1, (pattern, sorted(table))
    return next(iter(hit.items()))


@pytest.mark.parametrize("unit", list(NEW))
def test_the_new_kernel_is_in_its_object_takes_a_pointer_and_keeps_its_registers(notes, unit):
    name, n = _one(notes[unit], NEW[unit])   # (the pattern: the argument blocks arrive as a pointer to a device array)
    print(n, name)
    assert n["vgpr_spill_count"] == 0 and n["private_segment_fixed_size"] == 0, (name, n)
    assert n["vgpr_count"] <= 128, (name, n)            # 1024 threads = 16 waves on 4 SIMDs: 512 / 4 registers each
    assert n["max_flat_workgroup_size"] == 1024, (name, n)
    assert not [p for p, _cap, _why in ALLOWED if re.search(p, name)], "not on the allow-list"


def test_the_new_kernels_have_units_of_their_own(notes):
    """(in k_cem.hip a third instantiation of update_small_body moved instructions in cem_update_f32_kernel and its batched twin;
    k_random_learned.hip's three kernels are counted by test_random_learned_objects_cpu.py)"""
    assert len(notes["k_cem_members.hip"]) == 1 and len(notes["k_random_members.hip"]) == 1
    assert not [k for k in notes["k_cem.hip"] if "members" in k] and not [k for k in notes["k_random_learned.hip"] if "members" in k]


def test_the_kernels_that_share_a_body_or_a_unit_spill_what_they_did(notes):
    for unit, pats in BEFORE.items():
        for pat in pats:
            name, n = _one(notes[unit], pat)
            assert n["vgpr_spill_count"] == 0 and n["private_segment_fixed_size"] == 0, (name, n)
