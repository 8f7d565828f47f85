"""The section arithmetic of the batched steps' argument blobs (icem_amd/csrc/block_layout.h: BlockLayout) against its rule,
restated here: a section of n blocks takes ceil(block * n / 256) * 256 bytes and starts where the previous one ended; the room
of a slot is the same sections at the batch maximum.  A stand-alone C++17 program that includes the header alone (nothing of HIP,
nothing of the library) prints what the type computes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX = 32
NS = (1, 2, 31, 32)
# one section of each size around the rounding boundary; three sections of the sizes a step's sampler, rollout and update blocks
# have (72 bytes is CemSampleArgs<float>; the other two are of that order, multiples of 8); the boundary sizes as one blob
LAYOUTS = ((1,), (255,), (256,), (257,), (72, 344, 208), (1, 255, 256, 257))

PROGRAM = r"""
#include "block_layout.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv) {   // n max block...  ->  offset... bytes room
    icem::BlockLayout lay(std::atoi(argv[1]), std::atoi(argv[2]));
    for (int i = 3; i < argc; ++i) std::printf("%zu ", lay.add((size_t)std::atoll(argv[i])));
    std::printf("%zu %zu\n", lay.bytes(), lay.room());
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("block_layout")
    src = d / "layout.cpp"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "icem_amd", "csrc"), "-o", str(d / "layout"), str(src)])
    return str(d / "layout")


def sections(blocks, n):
    """(offset of every section, total) by the rule"""
    at, total = [], 0
    for b in blocks:
        at.append(total)
        total += -(-(b * n) // 256) * 256
    return at, total


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("blocks", LAYOUTS, ids=lambda b: "-".join(map(str, b)))
def test_offsets_bytes_and_room_follow_the_rule(exe, blocks, n):
    got = [int(x) for x in subprocess.check_output([exe, str(n), str(MAX), *map(str, blocks)]).split()]
    offsets, nbytes, room = got[:-2], got[-2], got[-1]
    want_at, want_bytes = sections(blocks, n)
    assert offsets == want_at and nbytes == want_bytes
    assert room == sections(blocks, MAX)[1]
    assert all(o % 256 == 0 for o in offsets) and nbytes % 256 == 0
    assert room >= nbytes
    if n == MAX:
        assert room == nbytes
