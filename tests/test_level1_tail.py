"""level1_tail and chunk_clear_of_tail of rustray_amd/csrc/rr_frame_plan.h (which buffers of the shadow queue the last two shadow stages of
a staged level 1 still read, and which chunks of the deeper levels may be shaded beside them) under AddressSanitizer + UBSan on the
CPU: the contract frame, the frame of tests/test_gpu_tail_overlap.py, and the invariants over a sweep of level sizes, lights, chunk
sizes, 2 or 3 buffers and chunk sizes of the serial loop."""
import os
import subprocess

from tests.helpers import ROOT


def test_level1_tail_under_asan(tmp_path):
    exe = str(tmp_path / "level1_tail_test")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", "-o", exe, os.path.join(ROOT, "tests", "native", "level1_tail_test.cpp")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "level-1 tail test OK" in out.stdout, out.stdout + out.stderr
