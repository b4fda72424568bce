"""rr_scene_build.h's flat_normals_bytes -- the size of the flat-normal table now that an entry holds normal, tangent and bitangent --
under AddressSanitizer + UBSan on the CPU (tests/native/flat_table_size_test.cpp)."""
import os
import subprocess

from tests.helpers import ROOT


def test_flat_table_sizes_under_asan(tmp_path):
    exe = str(tmp_path / "flat_table_size_test")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-pthread", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", "-o", exe,
           os.path.join(ROOT, "tests", "native", "flat_table_size_test.cpp"), os.path.join(ROOT, "rustray_amd", "csrc", "rr_bvh.cpp")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "flat table sizes: 0 failures" in out.stdout, out.stdout + out.stderr
