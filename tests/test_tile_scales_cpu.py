"""The launch scalars of the fp16-plane tiles (icem_amd/csrc/tile_scales.h) without a device: the kernels multiply by the exact
reciprocals of the model's power-of-two scales where they used to divide by the scales.  tests/units/tile_scales_host.cpp
includes the header the kernels include and compares the two forms bit for bit -- exhaustively over every (exponent of
max|obs0| incl. the +-100 clamp edges, exponent of m_scale, exponent of b_scale), and for start observations of all zeros,
subnormals, one NaN entry and magnitudes of 2^+-100."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_products_give_the_bits_of_the_divisions(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "tile_scales_host")
    # (-O2 without -ffast-math: IEEE f32 arithmetic, subnormals included, as the device computes it)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "icem_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "units", "tile_scales_host.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and " 0 failures" in out.stdout, out.stdout + out.stderr
    assert int(out.stdout.split()[0]) >= 201 * 253 * 253, out.stdout
