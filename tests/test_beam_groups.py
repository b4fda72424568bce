"""The two-level candidate search of the packet top level (rustray_amd/csrc/rr_beam.h, rr_scene_build.h build_item_groups; its device
form is rr_trace.h beam_candidates) under AddressSanitizer + UBSan on the CPU: over more than 10^5 seeded (box set, interval ray)
cases the grouped search names exactly the items of the flat search with the same key bits, every group box contains its members'
boxes, no padding slot is ever named, a group test that is NaN lets the group through, and build_tlas appends records of the
documented sizes, the same on every call."""
import os
import subprocess

from tests.helpers import ROOT


def test_beam_groups_under_asan(tmp_path):
    exe = str(tmp_path / "beam_groups_test")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-pthread", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", "-o", exe,
           os.path.join(ROOT, "tests", "native", "beam_groups_test.cpp"), os.path.join(ROOT, "rustray_amd", "csrc", "rr_bvh.cpp")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "beam groups test OK" in out.stdout, out.stdout + out.stderr
