"""rustray_amd/csrc/rr_frame_plan.h (how a frame is cut into batches and how its ray memory is sized) under AddressSanitizer +
UBSan on the CPU: a table of expected plans (the contract frame, tiny budgets, progressive passes, forced sample groups, many
lights, a grown arena, 1x1 and lopsided frames) and the invariants the frame driver relies on over a sweep."""
import os
import subprocess

from tests.helpers import ROOT


def test_frame_plan_under_asan(tmp_path):
    exe = str(tmp_path / "frame_plan_test")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", "-o", exe, os.path.join(ROOT, "tests", "native", "frame_plan_test.cpp")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "frame plan test OK" in out.stdout, out.stdout + out.stderr
