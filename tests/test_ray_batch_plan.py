"""plan_ray_batches of rustray_amd/csrc/rr_frame_plan.h (how rr_shade_rays cuts the caller's rays into device batches and sizes
the ray arena) under AddressSanitizer + UBSan on the CPU: ray counts from 1 to beyond 2^31, budgets from nothing to 64 GB,
recursion 0 to 30 -- the batches partition the rays, none exceeds the 32-bit level size, the arena stays within the budget above
the 4096-ray floor, a tiny budget gives several batches -- and three plans worked out by hand."""
import os
import subprocess

from tests.helpers import ROOT


def test_ray_batch_plan_under_asan(tmp_path):
    exe = str(tmp_path / "ray_batch_plan_test")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", "-o", exe, os.path.join(ROOT, "tests", "native", "ray_batch_plan_test.cpp")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ray batch plan test OK" in out.stdout, out.stdout + out.stderr
