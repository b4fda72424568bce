"""The two halves of build_scene_records that rr_scene_add_meshes and rr_scene_set_items are made of (rustray_amd/csrc/rr_scene_build.h),
under AddressSanitizer + UBSan on the CPU: meshes appended at every split of a mesh list give the records of the whole list byte for
byte, item records of a permuted / shortened / lengthened item list equal a fresh build's, the keep-or-derive decision marks exactly
the items whose inputs are bitwise unchanged, every rejection, and where the stack share changes with the item count."""
import os
import subprocess

from tests.helpers import ROOT


def test_scene_items_under_asan(tmp_path):
    exe = str(tmp_path / "scene_items_test")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-pthread", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", "-o", exe,
           os.path.join(ROOT, "tests", "native", "scene_items_test.cpp"), os.path.join(ROOT, "rustray_amd", "csrc", "rr_bvh.cpp")]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "scene items test OK" in out.stdout, out.stdout + out.stderr
