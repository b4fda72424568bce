"""plan_level1_stages of rustray_amd/csrc/rr_frame_plan.h (how level 1's hits are cut into stages and shadow-queue buffers for the
two-stream schedule) under AddressSanitizer + UBSan on the CPU: a table of expected plans (the contract frame, explicit 65 536-ray
chunks, 32 lights, sizes one ray either side of two stages, a partial last stage) and the invariants the frame driver relies on
over a sweep of level sizes up to 2^31 - 256, 1 to 32 lights, chunk sizes and 2 or 3 buffers."""
import os
import subprocess

from tests.helpers import ROOT


def test_level1_stages_under_asan(tmp_path):
    exe = str(tmp_path / "level1_stages_test")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", "-o", exe, os.path.join(ROOT, "tests", "native", "level1_stages_test.cpp")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "level-1 stages test OK" in out.stdout, out.stdout + out.stderr
