"""The kernels of icem_mlp_rollout_cost_models in the built object of k_mlp_rollout.hip: the four instantiations (state K blocks
1 / 2 x relu / swish) are there beside the solo kernel's, none of them spills a vector register or has scratch (the problem
table must not be copied to private memory, and its resolution must not cost the step loop a register), and their LDS per
workgroup lets at least as many workgroups share a CU as the solo kernel's does -- both numbers read from the same object."""
import os
import re
import shutil
import subprocess

import pytest

from test_register_hygiene_cpu import LLVM, kernel_spills

SHAPES = ["<1, 0>", "<1, 1>", "<2, 0>", "<2, 1>"]
KERNELS = ["mlp_rollout_models_kernel" + s for s in SHAPES]


@pytest.fixture(scope="module")
def obj():
    from icem_amd import build as B
    if B.build_info()["stale"]:
        import __graft_entry__ as g
        g.build()
    path = B.object_path("k_mlp_rollout.hip")
    assert os.path.exists(path), path
    return path


def test_the_kernels_are_in_the_object(obj):
    if shutil.which("nm") is None or shutil.which("c++filt") is None:
        pytest.skip("nm / c++filt not in this image")
    syms = subprocess.check_output(["nm", obj], text=True)
    dem = subprocess.check_output(["c++filt"], input=syms, text=True)
    for name in KERNELS:
        assert re.search(rf"__device_stub__{re.escape(name)}\(", dem), name


@pytest.fixture(scope="module")
def records(obj, tmp_path_factory):
    """{demangled kernel name: {vgpr_spills, scratch, lds}} of the gfx950 code object."""
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.skip(f"{tool} not in this image")
    if shutil.which("c++filt") is None:
        pytest.skip("c++filt not in this image")
    tmp = str(tmp_path_factory.mktemp("co"))
    raw = kernel_spills(obj, tmp)
    notes = subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", os.path.join(tmp, "d.co")], text=True)
    out = {}
    for rec in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:   # one record per kernel
        nm = re.search(r"\.name:\s+(\S+)", rec)
        ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", rec)
        gs = re.search(r"\.group_segment_fixed_size:\s+(\d+)", rec)
        assert nm and ps and gs, rec[:200]
        dem = subprocess.check_output(["c++filt"], input=nm.group(1), text=True).strip()
        out[dem] = dict(vgpr_spills=raw[nm.group(1)], scratch=int(ps.group(1)), lds=int(gs.group(1)))
    return out


def _one(records, name):
    hit = [v for k, v in records.items() if re.search(rf"\b{re.escape(name)}(\(|$)", k)]
    assert len(hit) == 1, (name, sorted(records))
    return hit[0]


@pytest.mark.parametrize("name", KERNELS)
def test_none_of_them_spills_a_vector_register_or_has_scratch(records, name):
    r = _one(records, name)
    assert r["vgpr_spills"] == 0 and r["scratch"] == 0, r


@pytest.mark.parametrize("shape", SHAPES)
def test_their_lds_fits_a_cu_as_often_as_the_solo_kernels(records, shape):
    """A CU's LDS is shared by the workgroups on it: a workgroup that needs no more than the solo kernel's fits at least as
    often, whatever the CU's size."""
    solo, many = _one(records, "mlp_rollout_kernel" + shape), _one(records, "mlp_rollout_models_kernel" + shape)
    assert 0 < many["lds"] <= solo["lds"], (many, solo)
