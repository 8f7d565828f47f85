"""Issue slots of one model step of the headline rollout (c2: N = 4096, h = 30, d = 6, o = 17, fp16-plane tile), counted in the
disassembly of the built object (no GPU, no recompilation; the route and the skip rules of test_chain_isa_cpu.py).

One rollout wave per CU runs the step's 30 dependent repetitions alone on its SIMD, and a lone wave pays an issue slot for
EVERY instruction -- s_nop, s_waitcnt, v_mov and LDS reads as much as arithmetic (tools/ubench/lone_wave_ilp.hip: 2.0-2.2 ns
each).  Tile16H::step_lone_pairs (fused_dev.h) is written so that none is spent on a hazard filler, a repeated zero, a second
read or an unpacked product: 40 / 41 instructions per step, where the step it replaces had 47 / 48 (EXPERIMENTS R19.1).

A step here is the instructions from the first MFMA of one step up to the first MFMA of the next: every third v_mfma of the
kernel, the first and the last step left out (set-up before, cost and store behind).  Instruction classes are counted,
nothing else: no register, no order."""
import collections
import glob
import os
import re
import statistics
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
# the headline step's two rollout launches: merge-prologue (KREG = 12) and iteration 0, one rollout wave, fp16-plane tile
HEADLINE = r"sample_rollout_kernel<30, 6, 17, 0, 10, 1, (0|12), false, 1>"
MAX_MEDIAN_SLOTS = 43


def kernel_listings(obj, tmp):
    """{mangled kernel name: [instruction lines]} of one object's gfx950 code."""
    fat, co = os.path.join(tmp, "unit.fatbin"), os.path.join(tmp, "unit.co")
    subprocess.check_call([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj])
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
    text = subprocess.check_output([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], text=True)
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            name = m.group(1)
            out[name] = []
            continue
        ins = line.split("//")[0].strip()
        if name and ins and not ins.endswith(":"):
            out[name].append(ins)
    return out


def steps_of(ins):
    """The kernel's instructions cut at every third v_mfma; without the first and the last step."""
    at = [i for i, l in enumerate(ins) if l.startswith("v_mfma")]
    starts = at[::3]
    return [ins[a:b] for a, b in zip(starts[:-1], starts[1:])][1:-1]


@pytest.fixture(scope="module")
def headline(tmp_path_factory):
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump"):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.skip(f"{tool} not in this image")
    from icem_amd import build as B
    if B.build_info()["stale"]:   # no library, or one built from other sources: its objects say nothing about this tree
        pytest.skip("no objects built from the sources in the tree (python -m icem_amd.build)")
    if not os.path.isdir(B.OBJ) or not glob.glob(os.path.join(B.OBJ, "*.o")):
        pytest.skip("no built objects (icem_amd/csrc/_obj): the library was built elsewhere")
    obj = B.object_path("k_iter_small.hip")
    assert os.path.exists(obj), obj
    lst = kernel_listings(obj, str(tmp_path_factory.mktemp("slots")))
    names = list(lst)
    dem = subprocess.check_output(["c++filt"], input="\n".join(names), text=True).splitlines()
    hit = {d: lst[n] for n, d in zip(names, dem) if re.search(HEADLINE, d)}
    if not hit and any("ICEM_FAST_SHAPES" in f for f in B.FLAGS):
        pytest.skip("development build without the headline shape")
    assert len(hit) == 2, sorted(hit)
    return hit


def test_a_model_step_of_the_lone_wave_fits_its_slots(headline):
    for name, ins in sorted(headline.items()):
        steps = steps_of(ins)
        n_mfma = sum(1 for l in ins if l.startswith("v_mfma"))
        assert len(steps) >= 20, (name, len(steps))   # (h = 30, fully unrolled)
        lens = [len(s) for s in steps]
        hist = collections.Counter()
        for s in steps:
            hist.update(re.sub(r"_e(32|64)$", "", l.split()[0]) for l in s)
        print(f"\n{name}\n  instructions per step: {lens}  median {statistics.median(lens)}")
        for op, n in sorted(hist.items(), key=lambda kv: (-kv[1], kv[0])):
            print(f"  {n / len(steps):6.2f}  {op}")
        # three MFMAs per step, and the cut stands where a step's first MFMA does: that one starts the accumulation (its
        # accumulator operand is the constant 0), the two behind it accumulate onto a register quad
        for i, s in enumerate(steps):
            mf = [l for l in s if l.startswith("v_mfma")]
            assert len(mf) == 3 and s[0] is mf[0], (name, i, mf)
            assert re.search(r",\s*0$", mf[0]) and not any(re.search(r",\s*0$", l) for l in mf[1:]), (name, i, mf)
        assert n_mfma >= 3 * 29, (name, n_mfma)   # (h = 30; the last step's next state is dead, and so are MFMAs of it)
        nops = [(i, l) for i, s in enumerate(steps) for l in s if l.startswith("s_nop")]
        assert not nops, (name, nops[:4])
        assert statistics.median(lens) <= MAX_MEDIAN_SLOTS, (name, statistics.median(lens), lens)
