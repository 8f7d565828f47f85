"""The batched forms of a float64 step's launches (``icem_plan_step_batch_f64``) exist in the built gfx950 objects and keep their
registers: read from the code objects' metadata as tests/test_register_hygiene_cpu.py does (no GPU, no recompilation).  The quad
sampler for both synthesis-table widths and both generators, the shifted elites' copy, the row-of-lanes rollout for every padded
width and both model kinds, the thread-form rollout for every width and kind but <32, tanh> (whose solo twin spills 56 registers:
it gets no batched twin and its handles are refused), the one-launch selection -- none with more than 8 spilled VGPRs (the hygiene
test's limit; its allow-list does not grow for them).  The solo kernels are still there under their old names, and the library
exports the entry and its launch counter."""
import os
import re
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
LIMIT = 8
WIDTHS = (8, 16, 17, 18, 24, 32)


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
    for unit in ("k_generic_batch.hip", "generic_kernels.hip"):
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


def test_the_library_exports_the_entry_and_the_bindings_carry_it():
    from icem_amd import _lib as L
    lib = L.load_library()
    names = [s[0] for s in L.SYMBOLS]
    for sym in ("icem_plan_step_batch_f64", "icem_batch_f64_launches"):
        assert sym in names and getattr(lib, sym) is not None
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "icem_hip.h")).read()
    assert "int icem_plan_step_batch_f64(icem_handle* const* handles, int32_t n," in header
    from icem_amd import IcemPlanner
    assert hasattr(IcemPlanner, "plan_step_batch_f64") and hasattr(IcemPlanner, "batch_f64_launches")


def test_every_batched_generic_kernel_exists_and_keeps_its_registers(spills):
    over = []

    def check(pat):
        n = _one(spills, pat)
        if n > LIMIT:
            over.append((n, pat))
    for hmax in (32, 64):
        for rounds in (7, 10):
            check(rf"sample_clip_quad_batch_kernel<{hmax}, {rounds}>\(icem::SampleArgs<double> const\*")
    check(r"shift_elites_batch_kernel\(icem::ShiftElitesArgs<double> const\*")
    check(r"select_refit_batch_kernel\(icem::SelectArgs<double> const\*")
    for o in WIDTHS:
        for kind in (0, 1):
            check(rf"rollout_cost_rows_batch_kernel<{o}, {kind}>\(icem::RolloutArgs<double> const\*")
            if (o, kind) != (32, 1):
                check(rf"rollout_cost_batch_kernel<{o}, {kind}>\(icem::RolloutArgs<double> const\*")
    assert not over, over
    # the instantiation whose solo twin is on the hygiene test's list has no batched twin (its handles are refused)
    assert not [k for k in spills if re.search(r"rollout_cost_batch_kernel<32, 1>", k)]


def test_the_solo_generic_kernels_are_still_there_under_their_names(spills):
    for hmax in (32, 64):
        for rounds in (7, 10):
            _one(spills, rf"sample_clip_quad_kernel<double, {hmax}, {rounds}>\(icem::SampleArgs<double>\)")
    _one(spills, r"shift_elites_kernel<double>\(")
    _one(spills, r"select_refit_kernel<double>\(icem::SelectArgs<double>\)")
    for o in WIDTHS:
        for kind in (0, 1):
            _one(spills, rf"rollout_cost_rows_kernel<double, {o}, {kind}>\(icem::RolloutArgs<double>\)")
            _one(spills, rf"rollout_cost_kernel<double, {o}, {kind}>\(icem::RolloutArgs<double>\)")
