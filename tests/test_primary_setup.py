"""rustray_amd/csrc/rr_primary_setup.h (what the host sets up for the level-1 kernels' primary rays: pixel centres per slot, offsets
per sample, index constants and an exact division by a run-time constant) under AddressSanitizer + UBSan on the CPU, compiled
without contraction as the library is: the ray built from the tables equals the per-ray formula it replaced bit for bit -- origin,
direction, slot and sample -- for every (pixel, sample) of 7x5, 64x48 and 70x50 frames and of a region off the origin, cell sizes
1, 2 and 16, 1 to 128 samples, sample groups 1, 2 and 64, one batch and several, batches that start in the middle of a sample
slice, pinhole and depth of field; and the division equals the machine's for every dividend below 2^25 and, in its 32-bit form,
around every multiple of each divisor, at the top of the range and for 10^7 random pairs."""
import os
import subprocess

from tests.helpers import ROOT


def test_primary_setup_under_asan(tmp_path):
    exe = str(tmp_path / "primary_setup_test")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-pthread", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", "-o", exe, os.path.join(ROOT, "tests", "native", "primary_setup_test.cpp")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "primary setup test OK" in out.stdout, out.stdout + out.stderr
