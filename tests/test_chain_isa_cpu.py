"""FLAT accesses in the kernels of the headline MPC step (c2: N = 4096, h = 30, d = 6, o = 17), read from the disassembly of
the built objects (no GPU, no recompilation).

A ``flat_load`` / ``flat_store`` counts on BOTH memory counters (vmcnt and lgkmcnt) and is waited for with
``s_waitcnt vmcnt(0) lgkmcnt(0)``: behind one, nothing that is in flight overlaps.  The step at this size is a chain of
memory round trips, so its kernels -- the single-launch iteration with and without merge prologue, the
step's last merge with and without the noise drawn ahead -- address device memory as ``global_*`` and LDS as ``ds_*`` only.
The usual ways a FLAT access gets in: a row pointer rebuilt from integer halves (``merge_rows``), a ``volatile`` re-read of
an LDS slot through a generic pointer (``lds_reread_u64``), an LDS buffer written through a pointer captured by a lambda.

Every other kernel of the three units is counted and printed (``pytest -s``), nothing asserted: a kernel there may have a
FLAT access nobody has looked at yet.

Only the objects that belong to the sources in the tree are read (their names carry the hash ``icem_amd.build`` gives them;
a stale library skips).  The count is per kernel SYMBOL: device functions here are ``__forceinline__``; the test asserts
that the units define no other function symbol in which a FLAT access could hide.
"""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
UNITS = ("k_iter_small", "k_merge", "k_rollout_ahead")

# demangled names of the headline step's kernels
HEADLINE = [
    r"sample_rollout_kernel<30, 6, 17, \d+, 10, 1, (0|12), false, \d+>",
    r"merge_noise_kernel<30, 12>",
    r"merge_single_kernel<12, false>",
]


def flat_counts(obj, tmp):
    """{mangled kernel name: number of flat_load* / flat_store* instructions} of one object's gfx950 code."""
    stem = os.path.basename(obj).split(".")[0]
    fat, co = os.path.join(tmp, stem + ".fatbin"), os.path.join(tmp, stem + ".co")
    subprocess.check_call([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj])
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
    notes = subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", co], text=True)
    kernels = set(re.findall(r"\.name:\s+(\S+)", notes))
    out, name = {}, None
    strays = out.setdefault("__not_a_kernel__", [])
    dis = subprocess.Popen([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], stdout=subprocess.PIPE, text=True)
    for line in dis.stdout:
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            name = m.group(1) if m.group(1) in kernels else None
            if name:
                out[name] = 0
            else:
                strays.append(m.group(1))
        elif name and re.search(r"\bflat_(load|store)", line):
            out[name] += 1
    assert dis.wait() == 0
    return out


@pytest.fixture(scope="module")
def flats(tmp_path_factory):
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump"):
        if not os.path.exists(os.path.join(LLVM, tool)):
            pytest.skip(f"{tool} not in this image")
    from icem_amd import build as B
    if B.build_info()["stale"]:   # no library, or one built from other sources: its objects say nothing about this tree
        pytest.skip("no objects built from the sources in the tree (python -m icem_amd.build)")
    # an object's name carries the hash of (compile command, source, headers): only the objects build() would link now count
    objs = [B.object_path(u + ".hip") for u in UNITS]
    if not os.path.isdir(B.OBJ) or not glob.glob(os.path.join(B.OBJ, "*.o")):
        pytest.skip("no built objects (icem_amd/csrc/_obj): the library was built elsewhere")
    # (the library says it was built from these sources, and objects are there: then these three must be among them)
    assert all(os.path.exists(o) for o in objs), [o for o in objs if not os.path.exists(o)]
    tmp = str(tmp_path_factory.mktemp("isa"))
    tot, strays = {}, []
    for obj in objs:
        c = flat_counts(obj, tmp)
        strays += c.pop("__not_a_kernel__")
        tot.update(c)
    assert not strays, "device code outside the kernels' symbols (a FLAT access there would not be counted): %s" % strays[:8]
    names = list(tot)
    dem = subprocess.check_output(["c++filt"], input="\n".join(names), text=True).splitlines()
    return {d: tot[n] for n, d in zip(names, dem)}


def test_headline_step_kernels_have_no_flat_access(flats):
    from icem_amd import build as B
    offenders = []
    for pat in HEADLINE:
        hit = {k: v for k, v in flats.items() if re.search(pat, k)}
        if not hit and any("ICEM_FAST_SHAPES" in f for f in B.FLAGS):
            # a development build (ICEM_DEV_SHAPES: the flag is part of the compile command, so the objects read above ARE that
            # build's) narrowed to shapes other than the headline's
            pytest.skip("development build without the headline shape")
        assert hit, f"no built kernel matches {pat}"
        offenders += [(v, k) for k, v in hit.items() if v]
    assert not offenders, "flat_load / flat_store in a kernel of the headline step:\n%s" % "\n".join(
        f"{v:4d}  {k}" for v, k in sorted(offenders, reverse=True))


def test_report_flat_access_of_the_other_kernels(flats):
    """Prints the count for every kernel of the three units that is not one of the headline step's; asserts nothing about it."""
    others = {k: v for k, v in flats.items() if not any(re.search(p, k) for p in HEADLINE)}
    print("\nFLAT accesses per kernel (k_iter_small, k_merge, k_rollout_ahead; headline kernels: none, asserted above)")
    for k, v in sorted(others.items(), key=lambda kv: (-kv[1], kv[0])):
        print(f"{v:4d}  {k}")
    print(f"{sum(1 for v in others.values() if v)} of {len(others)} other kernels have a FLAT access")
