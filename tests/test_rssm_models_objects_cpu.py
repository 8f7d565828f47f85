"""The kernels of the launches with a model per problem in the built object of icem_rssm_split.hip: the four instantiations
and the ensemble reduction are there, and none of them spills more than 8 VGPRs (the limit of
test_register_hygiene_cpu.py, whose allow-list they are not on)."""
import os
import re
import shutil
import subprocess

import pytest

from test_register_hygiene_cpu import LIMIT, LLVM, kernel_spills

KERNELS = ["rssm_split_models_kernel<1>", "rssm_split_models_kernel<2>", "rssm_split_models_w_kernel<1>", "rssm_split_models_w_kernel<2>",
           "rssm_ensemble_reduce_kernel"]


@pytest.fixture(scope="module")
def obj():
    from icem_amd import build as B
    if B.build_info()["stale"]:
        import __graft_entry__ as g
        g.build()
    path = B.object_path("icem_rssm_split.hip")
    assert os.path.exists(path), path
    return path


def test_the_kernels_are_in_the_object(obj):
    if shutil.which("nm") is None or shutil.which("c++filt") is None:
        pytest.skip("nm / c++filt not in this image")
    syms = subprocess.check_output(["nm", obj], text=True)
    dem = subprocess.check_output(["c++filt"], input=syms, text=True)
    for name in KERNELS:
        assert re.search(rf"__device_stub__{re.escape(name)}\(", dem), name


def test_none_of_them_spills_more_than_eight_registers(obj, tmp_path):
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.skip(f"{tool} not in this image")
    if shutil.which("c++filt") is None:
        pytest.skip("c++filt not in this image")
    raw = kernel_spills(obj, str(tmp_path))
    names = list(raw)
    dem = subprocess.check_output(["c++filt"], input="\n".join(names), text=True).splitlines()
    spills = {d: raw[n] for n, d in zip(names, dem)}
    for name in KERNELS:
        hit = {k: v for k, v in spills.items() if re.search(rf"\b{re.escape(name)}(\(|$)", k)}
        assert len(hit) == 1, (name, sorted(spills))
        assert max(hit.values()) <= LIMIT, hit
