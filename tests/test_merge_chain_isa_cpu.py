"""The exact-K merge kernels of the headline MPC step (K = 10 known at compile time: ``sample_rollout_exactk_kernel``,
``merge_single_exactk_kernel``, ``merge_noise_exactk_kernel``), read from the disassembly of the built objects (no GPU, no
recompilation; the route and the skip rules of test_chain_isa_cpu.py).

 * Every exact-K kernel addresses memory as ``global_*`` / ``ds_*`` only (no FLAT access) and has no scratch.
 * Every exact-K kernel gathers exactly ten elite rows: ten ``global_load_dword`` between the barrier that ends the
   selection and the refit's first ``v_div_scale``, besides the two loads of the element's old mean and old std that every
   form of the merge issues in that stretch; the runtime-K kernels gather twelve rows there (one per register slot).  (The
   barrier is the last one in front of that ``v_div_scale``, not the kernel's first: ``merge_noise_*`` has its noise
   workgroups' code, barrier included, in front of the merge's.)
 * The exact-K headline rollout kernel meets what test_step_slots_cpu.py asks of the runtime-K ones: a median of at most 43
   issue slots per model step, no ``s_nop`` inside a step.

(A branch-free form of the survivors' compaction in ``merge_select_shallow`` was built together with a cap on its instruction
count -- 915 against 1279 between the threshold's ``ds_bpermute`` and the re-read of ``cand`` -- and measured slower on the
GPU; neither it nor its cap is in the tree: EXPERIMENTS R20.1.)
"""
import glob
import os
import re
import statistics
import subprocess

import pytest

LLVM = "/opt/rocm/lib/llvm/bin"
UNITS = ("k_iter_small", "k_merge")
EXACT_K = r"(sample_rollout_exactk_kernel|merge_single_exactk_kernel|merge_noise_exactk_kernel)<"
# the headline step's merge-prologue launch (one rollout wave, fp16-plane tile), exact-K and runtime-K
HEADLINE_EXACT = r"sample_rollout_exactk_kernel<30, 6, 17, 0, 10, 1, 12, 1, 10>"
HEADLINE_RUNTIME = r"sample_rollout_kernel<30, 6, 17, 0, 10, 1, 12, false, 1>"
MAX_MEDIAN_SLOTS = 43


def unit_kernels(obj, tmp):
    """{mangled kernel name: ([instruction lines], private segment bytes)} of one object's gfx950 code, and the symbols that
    are no kernel."""
    stem = os.path.basename(obj).split(".")[0]
    fat, co = os.path.join(tmp, stem + ".fatbin"), os.path.join(tmp, stem + ".co")
    subprocess.check_call([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj])
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
    notes = subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", co], text=True)
    private, name = {}, None
    for line in notes.splitlines():   # (a kernel's keys come alphabetically: .args with its own .name entries, then .name)
        m = re.search(r"\.name:\s+(\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"\.private_segment_fixed_size:\s+(\d+)", line)
        if m and name:
            private[name] = int(m.group(1))
    text = subprocess.check_output([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], text=True)
    out, strays, name = {}, [], None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            name = m.group(1) if m.group(1) in private else None
            if name:
                out[name] = ([], private[name])
            else:
                strays.append(m.group(1))
            continue
        ins = line.split("//")[0].strip()
        if name and ins and not ins.endswith(":"):
            out[name][0].append(ins)
    return out, strays


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump"):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.skip(f"{tool} not in this image")
    from icem_amd import build as B
    if B.build_info()["stale"]:   # no library, or one built from other sources: its objects say nothing about this tree
        pytest.skip("no objects built from the sources in the tree (python -m icem_amd.build)")
    objs = [B.object_path(u + ".hip") for u in UNITS]
    if not os.path.isdir(B.OBJ) or not glob.glob(os.path.join(B.OBJ, "*.o")):
        pytest.skip("no built objects (icem_amd/csrc/_obj): the library was built elsewhere")
    assert all(os.path.exists(o) for o in objs), [o for o in objs if not os.path.exists(o)]
    tmp = str(tmp_path_factory.mktemp("merge_isa"))
    tot, strays = {}, []
    for obj in objs:
        k, s = unit_kernels(obj, tmp)
        tot.update(k)
        strays += s
    assert not strays, "device code outside the kernels' symbols: %s" % strays[:8]
    names = list(tot)
    dem = subprocess.check_output(["c++filt"], input="\n".join(names), text=True).splitlines()
    return {d: tot[n] for n, d in zip(names, dem)}


def _hits(kernels, pat):
    from icem_amd import build as B
    hit = {k: v for k, v in kernels.items() if re.search(pat, k)}
    if not hit and any("ICEM_FAST_SHAPES" in f for f in B.FLAGS):
        pytest.skip("development build without the headline shape")
    assert hit, f"no built kernel matches {pat}"
    return hit


def test_exact_k_kernels_have_no_flat_access_and_no_scratch(kernels):
    hit = _hits(kernels, EXACT_K)
    assert any("merge_single_exactk_kernel<12, 10>" in k for k in hit) and any("merge_noise_exactk_kernel<30, 12, 10>" in k for k in hit)
    offenders = []
    for name, (ins, private) in hit.items():
        flat = sum(1 for l in ins if re.match(r"flat_(load|store|atomic)", l))
        scratch = sum(1 for l in ins if re.match(r"(scratch_|buffer_(load|store))", l))
        if flat or scratch or private:
            offenders.append((name, flat, scratch, private))
    assert not offenders, "FLAT accesses / scratch accesses / private segment bytes:\n%s" % "\n".join(map(str, offenders))


OLD_MEAN_STD = 2   # loads of the element's old mean and old std: in the gather's stretch in every form of the merge


def gather_loads(ins):
    """global_load_dword instructions of the gather: from the barrier that ends the selection -- the last one in front of the
    kernel's first v_div_scale, which is the refit's first division -- to that v_div_scale."""
    div = next(i for i, l in enumerate(ins) if l.startswith("v_div_scale"))
    bar = max(i for i, l in enumerate(ins[:div]) if l.startswith("s_barrier"))
    return sum(1 for l in ins[bar:div] if re.match(r"global_load_dword\s", l))


def test_exact_k_kernels_gather_ten_rows(kernels):
    counts = {name: gather_loads(ins) for name, (ins, _) in _hits(kernels, EXACT_K).items()}
    for name, n in sorted(counts.items()):
        print(f"{n:3d}  {name}")
    wrong = {k: v for k, v in counts.items() if v != 10 + OLD_MEAN_STD}
    assert not wrong, wrong
    # (what the count is measured against: the runtime-K kernels of the headline step ask for all twelve register slots)
    for pat in (HEADLINE_RUNTIME, r"merge_single_kernel<12, false>", r"merge_noise_kernel<30, 12>"):
        for name, (ins, _) in _hits(kernels, pat).items():
            assert gather_loads(ins) == 12 + OLD_MEAN_STD, (name, gather_loads(ins))


def steps_of(ins):
    """The kernel's instructions cut at every third v_mfma; without the first and the last step (test_step_slots_cpu.py)."""
    at = [i for i, l in enumerate(ins) if l.startswith("v_mfma")]
    starts = at[::3]
    return [ins[a:b] for a, b in zip(starts[:-1], starts[1:])][1:-1]


def test_exact_k_headline_rollout_fits_its_slots(kernels):
    hit = _hits(kernels, HEADLINE_EXACT)
    assert len(hit) == 1, sorted(hit)
    for name, (ins, _) in hit.items():
        steps = steps_of(ins)
        assert len(steps) >= 20, (name, len(steps))   # (h = 30, fully unrolled)
        lens = [len(s) for s in steps]
        print(f"\n{name}\n  instructions per step: {lens}  median {statistics.median(lens)}")
        for i, s in enumerate(steps):
            mf = [l for l in s if l.startswith("v_mfma")]
            assert len(mf) == 3 and s[0] is mf[0], (name, i, mf)
        nops = [(i, l) for i, s in enumerate(steps) for l in s if l.startswith("s_nop")]
        assert not nops, (name, nops[:4])
        assert statistics.median(lens) <= MAX_MEDIAN_SLOTS, (name, statistics.median(lens), lens)
