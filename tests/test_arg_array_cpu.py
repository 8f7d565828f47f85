"""The upload decision of the batched steps' device argument array (icem_amd/csrc/arg_array.h: DeviceArgArray, shared by
icem_plan_step_batch and icem_plan_step_learned*) without a device: tests/units/arg_array_host.hip replaces the type's four HIP
calls by counting stubs.  The same bytes upload nothing; one changed byte, a changed size and growth past the capacity each
upload once; growth synchronises the stream before it frees the old array and allocates the caller's room; slots are
independent; the destructor frees what is live."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_upload_decision_on_the_host(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "arg_array_host")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "icem_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "units", "arg_array_host.hip")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "0 failures" in out.stdout, out.stdout + out.stderr
