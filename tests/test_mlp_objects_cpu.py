"""The kernels of icem_mlp_rollout_cost in the built object of k_mlp_rollout.hip: the four instantiations (state K blocks 1 / 2 x
relu / swish) are there, none of them spills more than 8 VGPRs (the limit of test_register_hygiene_cpu.py, whose allow-list they
are not on) and none has scratch beyond its spills."""
import os
import re
import shutil
import subprocess

import pytest

from test_register_hygiene_cpu import LIMIT, LLVM

KERNELS = ["mlp_rollout_kernel<1, 0>", "mlp_rollout_kernel<1, 1>", "mlp_rollout_kernel<2, 0>", "mlp_rollout_kernel<2, 1>"]


@pytest.fixture(scope="module")
def obj():
    from icem_amd import build as B
    if B.build_info()["stale"]:
        import __graft_entry__ as g
        g.build()
    path = B.object_path("k_mlp_rollout.hip")
    assert os.path.exists(path), path
    return path


def test_the_unit_is_part_of_the_library():
    from icem_amd import build as B
    assert "k_mlp_rollout.hip" in B.UNITS


def test_the_kernels_are_in_the_object(obj):
    if shutil.which("nm") is None or shutil.which("c++filt") is None:
        pytest.skip("nm / c++filt not in this image")
    syms = subprocess.check_output(["nm", obj], text=True)
    dem = subprocess.check_output(["c++filt"], input=syms, text=True)
    for name in KERNELS:
        assert re.search(rf"__device_stub__{re.escape(name)}\(", dem), name


def test_none_of_them_spills_more_than_eight_registers_or_has_scratch_beyond(obj, tmp_path):
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.skip(f"{tool} not in this image")
    if shutil.which("c++filt") is None:
        pytest.skip("c++filt not in this image")
    from test_register_hygiene_cpu import kernel_spills
    raw = kernel_spills(obj, str(tmp_path))
    names = list(raw)
    dem = subprocess.check_output(["c++filt"], input="\n".join(names), text=True).splitlines()
    spills = {d: raw[n] for n, d in zip(names, dem)}
    notes = subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", os.path.join(str(tmp_path), "d.co")], text=True)
    # one record per kernel: .name, .private_segment_fixed_size (scratch bytes per lane) and .vgpr_spill_count
    records = re.split(r"\n\s*- \.agpr_count:", notes)[1:]
    scratch = {}
    for rec in records:
        nm = re.search(r"\.name:\s+(\S+)", rec)
        ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", rec)
        if nm and ps:
            scratch[nm.group(1)] = int(ps.group(1))
    for name in KERNELS:
        hit = {k: v for k, v in spills.items() if re.search(rf"\b{re.escape(name)}(\(|$)", k)}
        assert len(hit) == 1, (name, sorted(spills))
        assert max(hit.values()) <= LIMIT, hit
        mangled = [n for n, d in zip(names, dem) if d in hit]
        assert mangled[0] in scratch, (name, sorted(scratch))
        assert scratch[mangled[0]] <= 4 * raw[mangled[0]], (name, scratch[mangled[0]], raw[mangled[0]])
