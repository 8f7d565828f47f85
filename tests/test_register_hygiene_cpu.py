"""Register hygiene of the shipped gfx950 code: the VGPR spill count of EVERY kernel in the built objects (read from the
code objects' metadata: no GPU, no recompilation) stays at or under 8 -- or the kernel is on the list below with the
measurement that says the spilled form is still the fastest path for its shapes.  (every
``iter_ahead_kernel<30,17,24,*>`` spilled 112-156 registers and nobody had timed it; it lost by 38 % and is gone.)"""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
LIMIT = 8

# pattern of the demangled kernel name -> (spilled VGPRs allowed, why)
ALLOWED = [
    (r"sample_rollout_kernel<\d+, \d+, \d+, [01], 10, 2, 12, false, [01]>", 60,
     "two-tile slabs of the single-launch kernel (8k-16k rows): its selection wave spills; measured and left alone in "
     "EXPERIMENTS R3.13 -- 89-90 us per MPC step at N = 12 000-16 000, no faster path for those populations"),
    (r"sample_rollout_batch_kernel<\d+, \d+, \d+, [01], 10, 2, 12, [01]>", 60,
     "the same body as sample_rollout_kernel<..., 2, 12, false, ...> (icem_plan_step_batch reads its argument blocks from device "
     "memory): the same spills at two-tile slabs; a batch takes that slab size only between 2 and 4 problems of <= 2048 rows"),
    (r"iter_ahead_batch_kernel<30, 6, 1[78], [01], [48], [01], [01]>", 32,
     "the noise-ahead launch with its argument block read from device memory (icem_plan_step_batch, eight or more problems of "
     "4096 rows): the text of iter_ahead_kernel (iter_ahead_body.h) with the block's scalars held across the roles -- 9-23 "
     "spills on 128 registers, the same class as the by-value kernel's, and the batch is faster with it than on the "
     "single-launch kernels (EXPERIMENTS R6.3)"),
    (r"iter_ahead_kernel<30, 6, 17, [01], [48], [012], 1>", 16,
     "the fp16-plane tile (Tile16H: two operand planes of the model and of the state) on the 128 registers of the noise-ahead "
     "launch: 9-14 spills, at the staging points every ten steps -- and the launch wins by 11-14 %: 140.8 vs 157.2 us per MPC "
     "step at N = 65 536, 102.5 vs 116.4 at 32 768 on the same box (EXPERIMENTS R5.1)"),
    (r"iter_ahead_kernel<30, 6, 18, [01], [48], [012], [01]>", 32,
     "o = 18 (HalfCheetah with x position): 4-26 spills, and the launch still wins -- 268.5 vs 299.9 us per MPC step at "
     "N = 65 536 with the tanh model, 181.9 vs 239.0 with the linear one (EXPERIMENTS R4.6)"),
    (r"rollout_wide_split_kernel<3, [01], true, (true|false), false>", 16,
     "o = 378 on the bf16 matrix cores (icem_set_wide_exact 2) with icem_cost_terms: 4-11 spills at 256 registers, all in "
     "the batch prologue (EXPERIMENTS R4.9); the default fp16 form spills nothing"),
    (r"rollout_cost_kernel<double, 32, 1>", 56, "the generic float64 kernel at its widest observation: strict-parity path, not a throughput kernel"),
    (r"rssm_rollout_kernel<2>", 48, "the fused learned-dynamics kernel, populations above 65 536 only (the split launch serves the rest)"),
]


def kernel_spills(obj, tmp):
    fat, co = os.path.join(tmp, "f.fatbin"), os.path.join(tmp, "d.co")
    r = subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj], capture_output=True)
    if r.returncode != 0:   # a host-only translation unit (collective.hip binds RCCL with dlopen)
        return {}
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
    notes = subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", co], text=True)
    out, name = {}, None
    for line in notes.splitlines():
        m = re.search(r"\.name:\s+(\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"\.vgpr_spill_count:\s+(\d+)", line)
        if m and name:
            out[name] = int(m.group(1))
    return out


@pytest.fixture(scope="module")
def spills(tmp_path_factory):
    from icem_amd import build as B
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
    for obj in sorted(glob.glob(os.path.join(ROOT, "icem_amd", "csrc", "_obj", "*.o"))):
        tot.update(kernel_spills(obj, tmp))
    names = list(tot)
    dem = subprocess.check_output(["c++filt"], input="\n".join(names), text=True).splitlines()
    return {d: tot[n] for n, d in zip(names, dem)}


def test_every_kernel_is_accounted_for(spills):
    assert len(spills) > 250, "expected the metadata of a few hundred kernel instantiations"
    offenders = []
    for name, n in spills.items():
        if n <= LIMIT:
            continue
        for pat, cap, _why in ALLOWED:
            if re.search(pat, name):
                if n > cap:
                    offenders.append((n, name, f"allowed up to {cap}"))
                break
        else:
            offenders.append((n, name, "not on the list"))
    assert not offenders, "kernels spilling more than %d VGPRs:\n%s" % (LIMIT, "\n".join(f"{n:4d}  {k}  ({w})" for n, k, w in sorted(offenders, reverse=True)))


def test_the_benchmarked_instantiations_do_not_spill(spills):
    """The instantiations the bench lines run (c2, c4, c3, c5) stay at <= 4 spilled registers -- c4's noise-ahead launch on the
    fp16-plane tile at <= 13 (9 without the merge prologue, 13 with it since the step is the hand-interleaved one there too:
    EXPERIMENTS R6.15), none of them between the MFMAs of a tile's step chain (the spilled values belong to the merge
    prologue and the noise role, which share the launch's 128 registers: tools/dbg/kernel_isa.py)."""
    for pat, cap in ((r"iter_ahead_kernel<30, 6, 17, 0, 8, [01], 0>", 4), (r"iter_ahead_kernel<30, 6, 17, 0, 8, [01], 1>", 13),
                     (r"sample_rollout_kernel<30, 6, 17, 0, 10, 1, (0|12), false, 0>", 4),
                     (r"rssm_split_kernel<1>", 4), (r"merge_noise_kernel", 4), (r"merge_single_kernel", 4)):
        hit = {k: v for k, v in spills.items() if re.search(pat, k)}
        assert hit, pat
        assert max(hit.values()) <= cap, hit


def test_the_two_tile_shapes_are_not_on_the_noise_ahead_path(spills):
    assert not [k for k in spills if re.search(r"iter_ahead_kernel<\d+, \d+, 2[0-9],", k)]
    assert not [k for k in spills if re.search(r"rollout16_kernel<\d+, \d+, 2[0-9], [01], 16, [01]>", k)]
